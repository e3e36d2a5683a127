// k_search_generic.hip -- K2, generic variants: SAD window search for EVERY valid StereoBM configuration (numDisparities a
// multiple of 16 up to 4080, any odd blockSize 5..255, any minDisparity, any cap).  They are the fallback behind
// k_search_fast.hip and a second, structurally different device implementation that the parity suite runs against the
// same oracle.  Two kernels share one walk over the rows:
//   k_search_generic  single pass: all D reversed disparity indices at once, where that fits LDS (D <= 256, not every
//                     window at large D)
//   k_search_dslice   the rest (or everything, under rtdm_debug_disparity_slice): DT indices at a time.  Same disparity
//                     and cost planes, bit for bit.
//
// The shared walk (one workgroup = TC output columns x RS output rows of one frame):
//   LDS  V[e][j]   column sums over the w window rows, for every reversed disparity index e and
//                  every sample column j of the tile (TC + w - 1 of them)
//        Ssc[e][c] the w-wide horizontal sums = sad[e] of output column c (kept so that the
//                  uniqueness and sub-pixel steps can re-read them)
//   per output row: slide V down by one row (add row y+r, subtract row y-r-1), then every thread
//   sums w entries of V, the 256 / TC thread groups split the index range, partial (min, argmin) pairs are merged
//   in index order so that the FIRST minimum wins (= largest disparity).
// Column clamping at the image border follows the reference formulation exactly:
//   left column = clamp(lofs + j, 0, W-1), right column = clamp(rofs + j, 0, W-D) + e.
// What the kernels do not share is the selection between the horizontal sums and the final write: k_search_generic tests
// uniqueness over Ssc directly (two barriers per row); k_search_dslice keeps a per-pixel record (three barriers per row).
//
// The sliced form: V and Ssc hold only DT reversed disparity indices at a time.  The workgroup walks its rows once per
// slice [E, E + DT) of the reversed index range, in index order, and folds each slice's sums into a per-pixel record in
// LDS (RS x TC records, structure of arrays):
//   m, i     minimum so far and its FIRST index (strict <, so an earlier slice keeps a tie)
//   U        smallest sum more than one index away from i (the uniqueness set)
//   Sm, Sp   S[i-1] and S[i+1] (Sp pending while i is the last index folded so far)
//   P, last  minimum of every folded index but the last one, and the last one's sum
// A new winner i' in the slice sees the earlier indices through P (i' == E: E-1 is its neighbour) or min(P, last), and its
// left neighbour through `last`; an old winner at E-1 takes its right neighbour from the slice's first sum.  After the
// last slice the record is exactly what the oracle's selection loop computes over the whole range (DESIGN.md "K2c").
// The texture sum is accumulated during the last slice's walk only.
#include "rtdm_kernels.h"

#include <algorithm>
#include <type_traits>

namespace rtdm {

static constexpr int RS = 24;          // output rows per workgroup
static constexpr int DS_NREC = 7;      // m, i, U, Sm, Sp, P, last
static constexpr int BIG = 0x7fffffff;

// One tile's arrays in LDS and the constants of its walk.  TC = output columns per workgroup: 64 for whole frames, 8 for
// the narrow border strips that the fast kernel leaves over (work per workgroup scales with TC + w - 1 sample columns).
template <typename T>
struct Tile {
    int TCH, rb0, x_tile;          // sample columns, right base of the first one, first output column index
    const uint8_t *Lb, *Rb;        // this frame's prefiltered planes
    size_t lpitch, rpitch;
    int *Tcol, *pmin, *pidx, *flag;   // TCH texture column sums; 256 partial (min, argmin) pairs; the kernel's per-column words
    T *V, *Ssc;
    short *lidx, *ridx;            // TCH each: left column of sample j, right base of sample j (tile-relative)
    uint8_t *Ln, *Lo, *Rn, *Ro;    // the staged entering and leaving rows
};

// Carve-up from p on (all offsets multiples of 4) for DT reversed indices at a time and nflag words per output column, and
// the sample-column tables.  The caller's next barrier publishes the tables.
template <typename T, int TC>
__device__ __forceinline__ Tile<T> tile_begin(unsigned char* p, Plane8 Lp, Plane8 Rp, const BMGeom& g, int gx0, int DT, int nflag)
{
    Tile<T> t;
    t.TCH = TC + g.w - 1;
    const int LW = (t.TCH + 3) & ~3, RW = (t.TCH + DT + 3) & ~3;      // staged row bytes
    t.Tcol = (int*)p;
    t.pmin = t.Tcol + t.TCH;
    t.pidx = t.pmin + 256;
    t.flag = t.pidx + 256;
    t.V = (T*)(t.flag + nflag * TC);                                  // DT * TCH
    t.Ssc = t.V + (size_t)DT * t.TCH + ((DT * t.TCH) & 1);            // DT * TC (even)
    t.lidx = (short*)(t.Ssc + (size_t)DT * TC);
    t.ridx = t.lidx + t.TCH + (t.TCH & 1);
    t.Ln = (uint8_t*)(t.ridx + t.TCH + (t.TCH & 1));
    t.Lo = t.Ln + LW;
    t.Rn = t.Lo + LW;
    t.Ro = t.Rn + RW;
    t.x_tile = gx0 + blockIdx.x * TC;
    t.Lb = Lp.base + (size_t)blockIdx.z * Lp.frame; t.lpitch = Lp.pitch;
    t.Rb = Rp.base + (size_t)blockIdx.z * Rp.frame; t.rpitch = Rp.pitch;
    // rb0 = right base of the first sample column (clamps are monotone)
    const int Wc = g.legacy ? g.W - g.rofs - 1 : g.W - g.D;   // largest right sample base (rtdm_bm_params.legacy_right_clamp)
    t.rb0 = min(max(g.rofs + t.x_tile - g.r, 0), Wc);
    for (int jj = threadIdx.x; jj < t.TCH; jj += 256) {
        const int j = t.x_tile + jj - g.r;
        t.lidx[jj] = (short)min(max(g.lofs + j, 0), g.W - 1);
        t.ridx[jj] = (short)(min(max(g.rofs + j, 0), Wc) - t.rb0);
        t.Tcol[jj] = 0;
    }
    return t;
}

// Stage the entering row row_in and the leaving row (row_in - w once `sub`, before that the entering row again) for the
// reversed indices [E, E + DL): the right rows from sample base rb0 + E on.
template <typename T>
__device__ __forceinline__ void stage_rows(const Tile<T>& t, const BMGeom& g, int row_in, bool sub, int E, int DL)
{
    const int tid = threadIdx.x, row_o = sub ? row_in - g.w : row_in;
    const uint8_t* lrow = t.Lb + (size_t)row_in * t.lpitch;
    const uint8_t* rrow = t.Rb + (size_t)row_in * t.rpitch;
    const uint8_t* lrow_o = t.Lb + (size_t)row_o * t.lpitch;
    const uint8_t* rrow_o = t.Rb + (size_t)row_o * t.rpitch;
    for (int jj = tid; jj < t.TCH; jj += 256) { t.Ln[jj] = lrow[t.lidx[jj]]; t.Lo[jj] = lrow_o[t.lidx[jj]]; }
    // legacy clamp: base + e addresses a plane of step W -- past the row's end come the next row's first bytes
    // (base <= W - rofs - 1 and e <= D - 1 <= W - rofs - 1 keep x - W < W; the test stays as the guard)
    const int rin1 = row_in + 1, rout1 = row_o + 1;
    const uint8_t* rnext = t.Rb + (size_t)min(rin1, g.H - 1) * t.rpitch;
    const uint8_t* rnext_o = t.Rb + (size_t)min(rout1, g.H - 1) * t.rpitch;
    for (int k = tid; k < t.TCH + DL; k += 256) {
        const int x = t.rb0 + E + k;
        const bool wrap = g.legacy && x >= g.W && x - g.W < g.W;
        // (past the last row the 3.x code reads what follows the plane: zeros in the oracle = the bias here)
        t.Rn[k] = x < g.W ? rrow[x] : (wrap && rin1 < g.H) ? rnext[x - g.W] : PREFILTER_BIAS;
        t.Ro[k] = x < g.W ? rrow_o[x] : (wrap && rout1 < g.H) ? rnext_o[x - g.W] : PREFILTER_BIAS;
    }
}

// Slide the column sums of DL indices down by the staged rows.
template <typename T>
__device__ __forceinline__ void slide_sums(const Tile<T>& t, int DL, bool sub)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int e = wv; e < DL; e += 4) {
        T* v = t.V + (size_t)e * t.TCH;
        for (int jj = lane; jj < t.TCH; jj += 64) {
            const int ri = t.ridx[jj] + e;
            int a = abs((int)t.Ln[jj] - (int)t.Rn[ri]);
            if (sub) a -= abs((int)t.Lo[jj] - (int)t.Ro[ri]);
            v[jj] = (T)(v[jj] + a);
        }
    }
}

// The same slide for the texture column sums.
template <typename T>
__device__ __forceinline__ void slide_texture(const Tile<T>& t, int cap, bool sub)
{
    for (int jj = threadIdx.x; jj < t.TCH; jj += 256) {
        int a = abs((int)t.Ln[jj] - (cap + PREFILTER_BIAS));          // (the planes are biased: rtdm_kernels.h)
        if (sub) a -= abs((int)t.Lo[jj] - (cap + PREFILTER_BIAS));
        t.Tcol[jj] += a;
    }
}

// Horizontal sums of this thread's indices [e0, e1) of output column c into Ssc, and their partial FIRST minimum into
// pmin / pidx.
template <typename T, int TC>
__device__ __forceinline__ void horizontal_sums(const Tile<T>& t, int w, int e0, int e1)
{
    const int c = threadIdx.x % TC, qs = threadIdx.x / TC;
    int best = BIG, besti = -1;
    for (int e = e0; e < e1; ++e) {
        const T* v = t.V + (size_t)e * t.TCH + c;
        int sum = 0;
        for (int k = 0; k < w; ++k) sum += (int)v[k];
        t.Ssc[(size_t)e * TC + c] = (T)sum;
        if (sum < best) { best = sum; besti = e; }
    }
    t.pmin[qs * TC + c] = best; t.pidx[qs * TC + c] = besti;
}

// Column c's minimum over the partial ones, in index order.
template <typename T, int TC>
__device__ __forceinline__ void first_minimum(const Tile<T>& t, int c, int* m, int* i)
{
    *m = BIG; *i = -1;
#pragma unroll
    for (int q = 0; q < 256 / TC; ++q) {
        const int b = t.pmin[q * TC + c];
        if (b < *m) { *m = b; *i = t.pidx[q * TC + c]; }
    }
}

// Output row y of tile column c from its selection: minimum m at reversed index i, pp / nn = the sums that the sub-pixel
// formula takes for S[i+1] / S[i-1].
template <typename T, int TC>
__device__ __forceinline__ void write_pixel(const Tile<T>& t, Plane16W disp, T* cost, const BMGeom& g, int gx1, int y, int c,
                                            int m, int i, int pp, int nn, bool uniq_ok)
{
    const int x = t.x_tile + c;                 // output column index
    const int col = g.lofs + x;                 // image column
    if (x >= gx1 || col >= g.W) return;
    const int f = blockIdx.z;
    int tsum = 0;
    for (int k = 0; k < g.w; ++k) tsum += t.Tcol[c + k];
    int out = g.filtered;
    if (tsum >= g.tex && uniq_ok) {
        const int den = pp + nn - 2 * m + abs(pp - nn);
        const int v = (g.D - i - 1 + g.minD) * 256 + (den != 0 ? (pp - nn) * 256 / den : 0) + 15;
        out = v >> 4;
        if (g.want_cost) cost[((size_t)f * g.H + y) * g.Ws + col] = (T)m;
    }
    if (g.mask_cols && (col < g.vx0 || col >= g.vx1)) out = g.filtered;
    disp.base[(size_t)f * disp.frame_e + (size_t)y * disp.pitch_e + col] = (int16_t)out;
}

template <typename T, int TC>
__global__ __launch_bounds__(256) void k_search_generic(Plane8 Lp, Plane8 Rp, Plane16W disp, T* cost, BMGeom g,
                                                        int gx0, int gx1)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int D = g.D, w = g.w;
    constexpr int NQ = 256 / TC;                         // parts of the disparity range
    const int tid = threadIdx.x;
    const int c = tid % TC, qs = tid / TC;               // output column within the tile, part of the range
    const Tile<T> t = tile_begin<T, TC>(smem, Lp, Rp, g, gx0, D, 3);
    int* uflag = t.flag;                                 // TC (of 3 TC: the byte count of a launch is kept)
    const int ys0 = g.vy0 + blockIdx.y * RS;
    const int ys1 = min(ys0 + RS, g.vy1);
    for (int i = tid; i < D * t.TCH; i += 256) t.V[i] = 0;
    __syncthreads();

    const int nsteps = (ys1 - ys0) + w - 1;
    for (int s = 0; s < nsteps; ++s) {
        const int row_in = ys0 - g.r + s;
        const bool sub = s >= w;
        stage_rows(t, g, row_in, sub, 0, D);
        __syncthreads();
        slide_sums(t, D, sub);
        slide_texture(t, g.cap, sub);
        __syncthreads();
        if (s < w - 1) continue;

        const int e0 = (D * qs) / NQ, e1 = (D * (qs + 1)) / NQ;
        horizontal_sums<T, TC>(t, w, e0, e1);
        if (qs == 0) uflag[c] = 0;
        __syncthreads();
        int m1, mi;
        first_minimum<T, TC>(t, c, &m1, &mi);
        if (g.uniq > 0) {
            const int thresh = m1 + (m1 * g.uniq / 100);
            int hit = 0;
            for (int e = e0; e < e1; ++e)
                hit |= ((e < mi - 1 || e > mi + 1) && (int)t.Ssc[(size_t)e * TC + c] <= thresh);
            if (hit) atomicOr(&uflag[c], 1);
        }
        __syncthreads();
        if (qs == 0) {
            const int pp = (int)t.Ssc[(size_t)((mi + 1 < D) ? mi + 1 : D - 2) * TC + c];
            const int nn = (int)t.Ssc[(size_t)((mi > 0) ? mi - 1 : 1) * TC + c];
            write_pixel<T, TC>(t, disp, cost, g, gx1, row_in - g.r, c, m1, mi, pp, nn, !uflag[c]);
        }
        // Ssc / pmin / uflag are rewritten only after the next step's two barriers
    }
}

template <typename T, int TC>
__global__ __launch_bounds__(256) void k_search_dslice(Plane8 Lp, Plane8 Rp, Plane16W disp, T* cost, BMGeom g,
                                                       int gx0, int gx1, int DT)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int D = g.D, w = g.w;
    constexpr int NREC = RS * TC, NQ = 256 / TC;         // records; parts of a slice
    int* rec = (int*)smem;                               // DS_NREC * NREC
    int* rm = rec;  int* ri_ = rec + NREC;  int* rU = rec + 2 * NREC;  int* rSm = rec + 3 * NREC;
    int* rSp = rec + 4 * NREC;  int* rP = rec + 5 * NREC;  int* rlast = rec + 6 * NREC;
    const int tid = threadIdx.x;
    const int c = tid % TC, qs = tid / TC;               // output column within the tile, part of the slice
    const Tile<T> t = tile_begin<T, TC>(smem + DS_NREC * NREC * 4, Lp, Rp, g, gx0, DT, 2);
    int* ured = t.flag;                                  // TC
    int* pred = ured + TC;                               // TC
    const int ys0 = g.vy0 + blockIdx.y * RS;
    const int ys1 = min(ys0 + RS, g.vy1);

    const int nsteps = (ys1 - ys0) + w - 1;
    for (int E = 0; E < D; E += DT) {
        const int DL = min(DT, D - E);                   // indices in this slice (a multiple of 16)
        const bool lastslice = E + DL >= D;
        for (int i = tid; i < DL * t.TCH; i += 256) t.V[i] = 0;
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
            const int row_in = ys0 - g.r + s;
            const bool sub = s >= w;
            stage_rows(t, g, row_in, sub, E, DL);
            __syncthreads();
            slide_sums(t, DL, sub);
            if (lastslice) slide_texture(t, g.cap, sub);
            __syncthreads();
            if (s < w - 1) continue;

            const int y = row_in - g.r;
            const int k = (y - ys0) * TC + c;             // this pixel's record
            const int e0 = (DL * qs) / NQ, e1 = (DL * (qs + 1)) / NQ;   // (local indices)
            horizontal_sums<T, TC>(t, w, e0, e1);
            if (qs == 0) { ured[c] = BIG; pred[c] = BIG; }
            __syncthreads();
            // the slice's minimum in index order, and the winner after this slice
            int sm, si;
            first_minimum<T, TC>(t, c, &sm, &si);
            const int mold = E > 0 ? rm[k] : BIG;
            const bool nw = sm < mold;
            const int win = nw ? E + si : ri_[k];
            // this part's contribution to U (indices more than one away from the winner) and to P (all but the slice's last)
            int uex = BIG, pl = BIG;
            for (int e = e0; e < e1; ++e) {
                const int v = (int)t.Ssc[(size_t)e * TC + c];
                if (abs(E + e - win) > 1) uex = min(uex, v);
                if (e < DL - 1) pl = min(pl, v);
            }
            if (uex < BIG) atomicMin(&ured[c], uex);
            if (pl < BIG) atomicMin(&pred[c], pl);
            __syncthreads();
            if (qs == 0) {
                const int P = E > 0 ? rP[k] : BIG, last = E > 0 ? rlast[k] : BIG;
                int m, i, U, Sm, Sp;
                if (nw) {
                    m = sm; i = win;
                    U = min(ured[c], i == E ? P : min(P, last));
                    Sm = i == E ? last : (int)t.Ssc[(size_t)(i - E - 1) * TC + c];
                    Sp = i - E + 1 < DL ? (int)t.Ssc[(size_t)(i - E + 1) * TC + c] : BIG;   // (pending)
                } else {
                    m = mold; i = win;
                    U = min(rU[k], ured[c]);
                    Sm = rSm[k];
                    Sp = i == E - 1 ? (int)t.Ssc[c] : rSp[k];
                }
                if (!lastslice) {
                    rm[k] = m; ri_[k] = i; rU[k] = U; rSm[k] = Sm; rSp[k] = Sp;
                    rP[k] = min(min(P, last), pred[c]); rlast[k] = (int)t.Ssc[(size_t)(DL - 1) * TC + c];
                } else {
                    // S[D-2] stands in at the right end, S[1] at the left end
                    write_pixel<T, TC>(t, disp, cost, g, gx1, y, c, m, i, (i + 1 < D) ? Sp : Sm, (i > 0) ? Sm : Sp,
                                       g.uniq <= 0 || U > m + (m * g.uniq / 100));
                }
            }
            // Ssc / pmin / pidx / ured / pred are rewritten only after the next step's two barriers; V is cleared for the
            // next slice after this step's last barrier
        }
    }
}

// ---- host side ----------------------------------------------------------------------------
static constexpr size_t LDS_MAX = 160 * 1024;

// Dynamic LDS of a launch with TC output columns and DT reversed indices at a time (tile_begin's carve-up, behind the
// records of the sliced form).
static size_t search_lds_bytes(const BMGeom& g, int TC, int DT, bool sliced)
{
    const size_t ts = g.cost16 ? 2 : 4;
    const int TCH = TC + g.w - 1;
    const int RW = (TCH + DT + 3) & ~3, LW = (TCH + 3) & ~3;
    size_t b = (size_t)((sliced ? DS_NREC * RS * TC : 0) + TCH + 2 * 256 + (sliced ? 2 : 3) * TC) * 4;
    b += ((size_t)DT * TCH + ((DT * TCH) & 1)) * ts + (size_t)DT * TC * ts;
    b += (size_t)2 * (TCH + (TCH & 1)) * 2;
    b += (size_t)2 * LW + 2 * RW;
    return (b + 15) & ~(size_t)15;
}

// rtdm_debug_disparity_slice: 0 = the library's choice, > 0 = every configuration runs k_search_dslice with slices of that width
static std::atomic<int> g_forced_dt{0};
void dslice_set_width(int dt) { g_forced_dt.store(dt > 0 ? (dt + 15) & ~15 : 0, std::memory_order_relaxed); }

bool generic_search_sliced(const BMGeom& g)
{
    if (g_forced_dt.load(std::memory_order_relaxed) > 0) return true;
    return g.D > 256 || g.W > 32767 || search_lds_bytes(g, 64, g.D, false) > LDS_MAX;
}

// Slice width: the forced one (capped at D and at what fits), else the widest multiple of 16 that lets two workgroups share
// a CU (half the LDS) if that leaves slices of at least 32, else the widest that fits.  Measured at D = 512, w = 25, cap 63,
// 720p (profiles/dslice_time.txt): two workgroups per CU at DT = 32 take 0.57x the time of one at the widest DT (96);
// DT = 16 (three per CU) pays more for re-walking the rows than it gains.
static int dslice_width(const BMGeom& g, int TC)
{
    const int forced = g_forced_dt.load(std::memory_order_relaxed);
    const auto widest = [&](int dt, size_t budget) {
        while (dt > 16 && search_lds_bytes(g, TC, dt, true) > budget) dt -= 16;
        return dt;
    };
    if (forced > 0) return widest(std::min(forced, g.D), LDS_MAX);
    const int half = widest(g.D, LDS_MAX / 2);
    if (search_lds_bytes(g, TC, half, true) <= LDS_MAX / 2 && (half >= 32 || half == g.D)) return half;
    return widest(g.D, LDS_MAX);
}

// f(T{}, integral_constant<int, TC>{}) for the sum type and the tile width of a launch
template <typename F>
static void with_sum_type_and_tile(bool u16, bool narrow, F&& f)
{
    using TC8 = std::integral_constant<int, 8>;
    using TC64 = std::integral_constant<int, 64>;
    if (u16) { if (narrow) f(uint16_t{}, TC8{}); else f(uint16_t{}, TC64{}); }
    else     { if (narrow) f(uint32_t{}, TC8{}); else f(uint32_t{}, TC64{}); }
}

const char* launch_search_generic(Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g,
                                  int n, hipStream_t stream, int gx0, int gx1)
{
    const bool sliced = generic_search_sliced(g);
    const char* variant = sliced ? (g.cost16 ? "generic_dslice_u16" : "generic_dslice_u32") : (g.cost16 ? "generic_u16" : "generic_u32");
    if (gx1 < 0) gx1 = g.width1;
    if (gx1 <= gx0) return variant;
    with_sum_type_and_tile(g.cost16, gx1 - gx0 <= 16, [&](auto sum, auto tile) {
        using T = decltype(sum);
        constexpr int TC = decltype(tile)::value;
        const int dt = sliced ? dslice_width(g, TC) : g.D;
        const size_t lds = search_lds_bytes(g, TC, dt, sliced);
        const dim3 grid((gx1 - gx0 + TC - 1) / TC, (g.vy1 - g.vy0 + RS - 1) / RS, n);
        const void* kernel = sliced ? (const void*)k_search_dslice<T, TC> : (const void*)k_search_generic<T, TC>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (sliced) hipLaunchKernelGGL((k_search_dslice<T, TC>), grid, dim3(256), lds, stream, Lp, Rp, disp, (T*)cost, g, gx0, gx1, dt);
        else hipLaunchKernelGGL((k_search_generic<T, TC>), grid, dim3(256), lds, stream, Lp, Rp, disp, (T*)cost, g, gx0, gx1);
    });
    return variant;
}

}  // namespace rtdm
