// k_search_dslice.hip -- K2, disparity-sliced generic variant: SAD window search for EVERY valid StereoBM configuration
// (numDisparities a multiple of 16 up to 4080, any odd blockSize 5..255, any minDisparity, any cap).  It serves what
// k_search_generic.hip cannot hold in LDS (D > 256, or large windows at large D) and produces the same disparity and cost
// planes, bit for bit.
//
// Work decomposition: as k_search_generic (one workgroup = TC output columns x RS output rows of one frame, column sums
// V[e][j] slid down the rows, horizontal sums Ssc[e][c]), but V and Ssc hold only DT reversed disparity indices at a time.
// The workgroup walks its rows once per slice [E, E + DT) of the reversed index range, in index order, and folds each
// slice's sums into a per-pixel record in LDS (RS x TC records, structure of arrays):
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

namespace rtdm {

static constexpr int DS_RS = 24;       // output rows per workgroup
static constexpr int DS_NREC = 7;      // m, i, U, Sm, Sp, P, last
static constexpr int DS_BIG = 0x7fffffff;

template <typename T, int TC>
__global__ __launch_bounds__(256) void k_search_dslice(Plane8 Lp, Plane8 Rp, Plane16W disp, T* cost, BMGeom g,
                                                       int gx0, int gx1, int DT)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int D = g.D, w = g.w, r = g.r;
    const int TCH = TC + w - 1;               // sample columns per tile
    const int RW = (TCH + DT + 3) & ~3;       // staged right-row bytes of one slice
    const int LW = (TCH + 3) & ~3;
    constexpr int NREC = DS_RS * TC;
    // carve-up (all offsets multiples of 4)
    int* rec = (int*)smem;                               // DS_NREC * NREC
    int* Tcol = rec + DS_NREC * NREC;                    // TCH
    constexpr int NQ = 256 / TC;                         // parts of a slice
    int* pmin = Tcol + TCH;                              // NQ * TC = 256
    int* pidx = pmin + 256;                              // 256
    int* ured = pidx + 256;                              // TC
    int* pred = ured + TC;                               // TC
    T* V = (T*)(pred + TC);                              // DT * TCH
    T* Ssc = V + (size_t)DT * TCH + ((DT * TCH) & 1);    // DT * TC
    short* lidx = (short*)(Ssc + (size_t)DT * TC + ((DT * TC) & 1));   // TCH (left column of sample j)
    short* ridx = lidx + TCH + (TCH & 1);                // TCH (right base of sample j, tile-relative)
    uint8_t* Ln = (uint8_t*)(ridx + TCH + (TCH & 1));    // LW
    uint8_t* Lo = Ln + LW;
    uint8_t* Rn = Lo + LW;                               // RW
    uint8_t* Ro = Rn + RW;
    int* rm = rec;  int* ri_ = rec + NREC;  int* rU = rec + 2 * NREC;  int* rSm = rec + 3 * NREC;
    int* rSp = rec + 4 * NREC;  int* rP = rec + 5 * NREC;  int* rlast = rec + 6 * NREC;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = tid % TC, qs = tid / TC;               // output column within the tile, part of the slice
    const int x_tile = gx0 + blockIdx.x * TC;            // first output column index of the tile
    const int ys0 = g.vy0 + blockIdx.y * DS_RS;
    const int ys1 = min(ys0 + DS_RS, g.vy1);
    const int f = blockIdx.z;
    const uint8_t* Lb = Lp.base + (size_t)f * Lp.frame;
    const uint8_t* Rb = Rp.base + (size_t)f * Rp.frame;
    int16_t* db = disp.base + (size_t)f * disp.frame_e;

    const int Wc = g.legacy ? g.W - g.rofs - 1 : g.W - D;      // largest right sample base (rtdm_bm_params.legacy_right_clamp)
    const int rb0 = min(max(g.rofs + x_tile - r, 0), Wc);
    for (int jj = tid; jj < TCH; jj += 256) {
        const int j = x_tile + jj - r;
        lidx[jj] = (short)min(max(g.lofs + j, 0), g.W - 1);
        ridx[jj] = (short)(min(max(g.rofs + j, 0), Wc) - rb0);
        Tcol[jj] = 0;
    }

    const int nsteps = (ys1 - ys0) + w - 1;
    for (int E = 0; E < D; E += DT) {
        const int DL = min(DT, D - E);                   // indices in this slice (a multiple of 16)
        const bool lastslice = E + DL >= D;
        for (int i = tid; i < DL * TCH; i += 256) V[i] = 0;
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
            const int row_in = ys0 - r + s;
            const bool sub = s >= w;
            const int row_out = row_in - w;
            // stage the entering (and leaving) prefiltered rows; the right rows from sample base rb0 + E on
            {
                const uint8_t* lrow = Lb + (size_t)row_in * Lp.pitch;
                const uint8_t* rrow = Rb + (size_t)row_in * Rp.pitch;
                const uint8_t* lrow_o = Lb + (size_t)(sub ? row_out : row_in) * Lp.pitch;
                const uint8_t* rrow_o = Rb + (size_t)(sub ? row_out : row_in) * Rp.pitch;
                for (int jj = tid; jj < TCH; jj += 256) { Ln[jj] = lrow[lidx[jj]]; Lo[jj] = lrow_o[lidx[jj]]; }
                // legacy clamp: base + e addresses a plane of step W -- past the row's end come the next row's first bytes
                // (base <= W - rofs - 1 and e <= D - 1 <= W - rofs - 1 keep x - W < W; the test stays as the guard)
                const int rin1 = row_in + 1, rout1 = (sub ? row_out : row_in) + 1;
                const uint8_t* rnext = Rb + (size_t)min(rin1, g.H - 1) * Rp.pitch;
                const uint8_t* rnext_o = Rb + (size_t)min(rout1, g.H - 1) * Rp.pitch;
                for (int k = tid; k < TCH + DL; k += 256) {
                    const int x = rb0 + E + k;
                    const bool wrap = g.legacy && x >= g.W && x - g.W < g.W;
                    Rn[k] = x < g.W ? rrow[x] : (wrap && rin1 < g.H) ? rnext[x - g.W] : PREFILTER_BIAS;
                    Ro[k] = x < g.W ? rrow_o[x] : (wrap && rout1 < g.H) ? rnext_o[x - g.W] : PREFILTER_BIAS;
                }
            }
            __syncthreads();
            // slide the column sums of the slice
            for (int e = wv; e < DL; e += 4) {
                T* v = V + (size_t)e * TCH;
                for (int jj = lane; jj < TCH; jj += 64) {
                    const int ri = ridx[jj] + e;
                    int a = abs((int)Ln[jj] - (int)Rn[ri]);
                    if (sub) a -= abs((int)Lo[jj] - (int)Ro[ri]);
                    v[jj] = (T)(v[jj] + a);
                }
            }
            if (lastslice) {
                for (int jj = tid; jj < TCH; jj += 256) {
                    int a = abs((int)Ln[jj] - (g.cap + PREFILTER_BIAS));          // (the planes are biased: rtdm_kernels.h)
                    if (sub) a -= abs((int)Lo[jj] - (g.cap + PREFILTER_BIAS));
                    Tcol[jj] += a;
                }
            }
            __syncthreads();
            if (s < w - 1) continue;

            const int y = row_in - r;
            const int k = (y - ys0) * TC + c;             // this pixel's record
            // horizontal sums for this part of the slice (local indices), partial FIRST minimum
            const int e0 = (DL * qs) / NQ, e1 = (DL * (qs + 1)) / NQ;
            int best = DS_BIG, besti = -1;
            for (int e = e0; e < e1; ++e) {
                const T* v = V + (size_t)e * TCH + c;
                int sum = 0;
                for (int kk = 0; kk < w; ++kk) sum += (int)v[kk];
                Ssc[(size_t)e * TC + c] = (T)sum;
                if (sum < best) { best = sum; besti = e; }
            }
            pmin[qs * TC + c] = best; pidx[qs * TC + c] = besti;
            if (qs == 0) { ured[c] = DS_BIG; pred[c] = DS_BIG; }
            __syncthreads();
            // the slice's minimum in index order, and the winner after this slice
            int sm = DS_BIG, si = -1;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int b = pmin[q * TC + c];
                if (b < sm) { sm = b; si = pidx[q * TC + c]; }
            }
            const int mold = E > 0 ? rm[k] : DS_BIG;
            const bool nw = sm < mold;
            const int win = nw ? E + si : ri_[k];
            // this part's contribution to U (indices more than one away from the winner) and to P (all but the slice's last)
            int uex = DS_BIG, pl = DS_BIG;
            for (int e = e0; e < e1; ++e) {
                const int v = (int)Ssc[(size_t)e * TC + c];
                if (abs(E + e - win) > 1) uex = min(uex, v);
                if (e < DL - 1) pl = min(pl, v);
            }
            if (uex < DS_BIG) atomicMin(&ured[c], uex);
            if (pl < DS_BIG) atomicMin(&pred[c], pl);
            __syncthreads();
            if (qs == 0) {
                const int P = E > 0 ? rP[k] : DS_BIG, last = E > 0 ? rlast[k] : DS_BIG;
                int m, i, U, Sm, Sp;
                if (nw) {
                    m = sm; i = win;
                    U = min(ured[c], i == E ? P : min(P, last));
                    Sm = i == E ? last : (int)Ssc[(size_t)(i - E - 1) * TC + c];
                    Sp = i - E + 1 < DL ? (int)Ssc[(size_t)(i - E + 1) * TC + c] : DS_BIG;   // (pending)
                } else {
                    m = mold; i = win;
                    U = min(rU[k], ured[c]);
                    Sm = rSm[k];
                    Sp = i == E - 1 ? (int)Ssc[c] : rSp[k];
                }
                const int Pn = min(min(P, last), pred[c]);
                const int lastn = (int)Ssc[(size_t)(DL - 1) * TC + c];
                if (!lastslice) {
                    rm[k] = m; ri_[k] = i; rU[k] = U; rSm[k] = Sm; rSp[k] = Sp; rP[k] = Pn; rlast[k] = lastn;
                } else {
                    const int x = x_tile + c;                 // output column index
                    const int col = g.lofs + x;               // image column
                    if (x < gx1 && col < g.W) {
                        int tsum = 0;
                        for (int kk = 0; kk < w; ++kk) tsum += Tcol[c + kk];
                        int out = g.filtered;
                        const bool uniq_ok = g.uniq <= 0 || U > m + (m * g.uniq / 100);
                        if (tsum >= g.tex && uniq_ok) {
                            const int pp = (i + 1 < D) ? Sp : Sm;       // S[D-2] at the right end
                            const int nn = (i > 0) ? Sm : Sp;           // S[1] at the left end
                            const int den = pp + nn - 2 * m + abs(pp - nn);
                            const int v = (D - i - 1 + g.minD) * 256 + (den != 0 ? (pp - nn) * 256 / den : 0) + 15;
                            out = v >> 4;
                            if (g.want_cost) cost[((size_t)f * g.H + y) * g.Ws + col] = (T)m;
                        }
                        if (g.mask_cols && (col < g.vx0 || col >= g.vx1)) out = g.filtered;
                        db[(size_t)y * disp.pitch_e + col] = (int16_t)out;
                    }
                }
            }
            // Ssc / pmin / pidx / ured / pred are rewritten only after the next step's two barriers; V is cleared for the
            // next slice after this step's last barrier
        }
    }
}

static size_t dslice_lds_bytes(const BMGeom& g, bool use16, int TC, int DT)
{
    const size_t ts = use16 ? 2 : 4;
    const int TCH = TC + g.w - 1;
    const int RW = (TCH + DT + 3) & ~3, LW = (TCH + 3) & ~3;
    size_t b = (size_t)(DS_NREC * DS_RS * TC + TCH + 2 * 256 + 2 * TC) * 4;
    b += ((size_t)DT * TCH + ((DT * TCH) & 1)) * ts + ((size_t)DT * TC + ((DT * TC) & 1)) * ts;
    b += (size_t)2 * (TCH + (TCH & 1)) * 2;
    b += (size_t)2 * LW + 2 * RW;
    return (b + 15) & ~(size_t)15;
}

static constexpr size_t DS_LDS_MAX = 160 * 1024;

// rtdm_debug_disparity_slice: 0 = the library's choice, > 0 = every configuration runs here with slices of that width
static std::atomic<int> g_forced_dt{0};
void dslice_set_width(int dt) { g_forced_dt.store(dt > 0 ? (dt + 15) & ~15 : 0, std::memory_order_relaxed); }
bool dslice_forced() { return g_forced_dt.load(std::memory_order_relaxed) > 0; }

// Slice width: the forced one (capped at D and at what fits), else the widest multiple of 16 that lets two workgroups share
// a CU (half the LDS) if that leaves slices of at least 32, else the widest that fits.  Measured at D = 512, w = 25, cap 63,
// 720p (profiles/dslice_time.txt): two workgroups per CU at DT = 32 take 0.57x the time of one at the widest DT (96);
// DT = 16 (three per CU) pays more for re-walking the rows than it gains.
int dslice_width(const BMGeom& g, bool use16, int TC)
{
    const int forced = g_forced_dt.load(std::memory_order_relaxed);
    const auto widest = [&](int dt, size_t budget) {
        while (dt > 16 && dslice_lds_bytes(g, use16, TC, dt) > budget) dt -= 16;
        return dt;
    };
    if (forced > 0) return widest(std::min(forced, g.D), DS_LDS_MAX);
    const int half = widest(g.D, DS_LDS_MAX / 2);
    if (dslice_lds_bytes(g, use16, TC, half) <= DS_LDS_MAX / 2 && (half >= 32 || half == g.D)) return half;
    return widest(g.D, DS_LDS_MAX);
}

template <typename T, int TC>
static void launch_dslice_t(Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n,
                            hipStream_t stream, int gx0, int gx1, int dt, size_t lds)
{
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k_search_dslice<T, TC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    dim3 grid((gx1 - gx0 + TC - 1) / TC, (g.vy1 - g.vy0 + DS_RS - 1) / DS_RS, n);
    hipLaunchKernelGGL((k_search_dslice<T, TC>), grid, dim3(256), lds, stream, Lp, Rp, disp, (T*)cost, g, gx0, gx1, dt);
}

void launch_search_dslice(Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g,
                          int n, hipStream_t stream, int gx0, int gx1)
{
    if (gx1 < 0) gx1 = g.width1;
    if (gx1 <= gx0) return;
    bool u16 = false;
    generic_search_supported(g, &u16);
    const bool narrow = (gx1 - gx0) <= 16;
    const int TC = narrow ? 8 : 64;
    const int dt = dslice_width(g, u16, TC);
    const size_t lds = dslice_lds_bytes(g, u16, TC, dt);
    if (u16) {
        if (narrow) launch_dslice_t<uint16_t, 8>(Lp, Rp, disp, cost, g, n, stream, gx0, gx1, dt, lds);
        else        launch_dslice_t<uint16_t, 64>(Lp, Rp, disp, cost, g, n, stream, gx0, gx1, dt, lds);
    } else {
        if (narrow) launch_dslice_t<uint32_t, 8>(Lp, Rp, disp, cost, g, n, stream, gx0, gx1, dt, lds);
        else        launch_dslice_t<uint32_t, 64>(Lp, Rp, disp, cost, g, n, stream, gx0, gx1, dt, lds);
    }
}

}  // namespace rtdm
