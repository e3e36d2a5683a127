// k_sgm_cost.hip -- the cost stage of the device StereoSGBM (k_sgm.hip: the schedule of passes; oracle/sgm_oracle.c rules R1-R3):
// from the two frames to the block-cost volume C (u16), laid out [frame][y][x - x0][d] with d fastest on the column domain
// [x0, x1) = [minD+D, W+min(minD,0)).
//
//   k_sgm_bounds x-Sobel (vertical edge replication) clipped to +-ftzero, + ftzero, and the BT bounds of it and of the
//                intensity (border columns overwritten with ftzero, R1), per pixel and channel  (HBM bound)
//   k_sgm_pixbox Birchfield-Tomasi pixel cost (gradient + (intensity >> 2), u8, kept in LDS) and the blockSize x blockSize sum
//                with clamped coordinates -> C (u16), windows <= 7; larger windows: k_sgm_pix<F> (a volume) + k_sgm_box / _any
//                (colour frames and ftzero >= 97, where a pixel cost passes 255: the u16 forms Cost16<CN> of both)
//   k_sgm_census the other pixel cost (rtdm_sgm_set_cost, rules N1-N5 of DESIGN.md section 4.20; no library counterpart): a census
//                descriptor per pixel and image instead of the bounds, in the same 8-byte records; the pixel cost is then the
//                Hamming distance of two descriptors (CostCensus), through k_sgm_pixbox or k_sgm_pix + k_sgm_box / _any
//   k_sgm_warm3  MODE_SGBM_3WAY's warm-up block costs C'.  Which of them a call runs: plan_sgm_cost (DESIGN.md "SGM: cost routes")
#include "rtdm_sgm.h"

#include <atomic>

namespace rtdm {

// R1's ftzero = max(preFilterCap, 15) | 1 comes in at run time: 15 at the default preFilterCap 0, at most 127 (the caller
// refuses preFilterCap >= 128), so every gradient value, 0 .. 2 ftzero, and every raw value still fits a byte.
//
// Per pixel and image, once: the Birchfield-Tomasi bounds (value, min and max against the half-way points to the two
// neighbours) of the clipped x-gradient and of the raw intensity, packed as two uchar4 -- the pixel-cost kernel then
// needs one 8-byte load per (pixel, image) instead of six byte loads per (pixel, disparity, image).  CN = 3 (interleaved
// colour, CV_8UC3): one such uint2 per channel, a 24-byte record per pixel ([f][y][x][c]).
template <int CN>
__device__ __forceinline__ int sgm_grad(const uint8_t* r0, const uint8_t* r1, const uint8_t* r2, int x, int W, int ftz)
{
    if (x <= 0 || x >= W - 1) return ftz;
    const int a = (x + 1) * CN, b = (x - 1) * CN;
    const int g = ((int)r1[a] - (int)r1[b]) * 2 + ((int)r0[a] - (int)r0[b]) + ((int)r2[a] - (int)r2[b]);
    return min(max(g, -ftz), ftz) + ftz;
}

template <int CN>
__global__ __launch_bounds__(256) void k_sgm_bounds(Plane8 L, Plane8 R, uint2* bl, uint2* br, int W, int H, int n, int ftz)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int y = blockIdx.y;
    int f = blockIdx.z;
    const bool right = f >= n;
    if (right) f -= n;
    const Plane8 S = right ? R : L;
    const uint8_t* img = S.base + (size_t)f * S.frame;
    const bool hm = x > 0, hp = x < W - 1;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        const uint8_t* r1 = img + (size_t)y * S.pitch + c;
        const uint8_t* r0 = img + (size_t)(y > 0 ? y - 1 : y) * S.pitch + c;
        const uint8_t* r2 = img + (size_t)(y < H - 1 ? y + 1 : y) * S.pitch + c;
        const uint32_t gb = bt_pack(sgm_grad<CN>(r0, r1, r2, x, W, ftz), hm ? sgm_grad<CN>(r0, r1, r2, x - 1, W, ftz) : 0,
                                    hp ? sgm_grad<CN>(r0, r1, r2, x + 1, W, ftz) : 0, hm, hp);
        // R1: the library overwrites columns 0 and W-1 of the raw-intensity row with ftzero as well, before the bounds are taken
        const auto raw = [&](int i) -> int { return (i <= 0 || i >= W - 1) ? ftz : (int)r1[i * CN]; };
        const uint32_t rb = bt_pack(raw(x), hm ? raw(x - 1) : 0, hp ? raw(x + 1) : 0, hm, hp);
        (right ? br : bl)[(((size_t)f * H + y) * W + x) * CN + c] = make_uint2(gb, rb);
    }
}

// A pixel cost is at most M = CN (2 ftzero + 63): 93 for gray at preFilterCap 0, 255 for gray at ftzero 96, 279 .. 951 for colour
// (CN = 3, interleaved; the channels are summed in packed u16, <= 951 per half: no carry).  Two forms of four consecutive pixel
// costs (disparities d .. d + 3 of one column; sgm_cost4, rtdm_sgm.h), for the volume and for the fused kernel's LDS tile:
//   Cost8       four u8 in a dword: gray up to ftzero 96
//   Cost16<CN>  four u16 in a uint2: colour at any preFilterCap, gray at ftzero >= 97 (and rtdm_debug_sgm_cost16).  Its block
//               sums are checked against cost_limit (> 0 where a block cost + P2 can pass 32767); Cost8's stay below it.
struct Cost8 {
    typedef uint32_t Word;
    typedef uint8_t Elem;                                  // of a volume of such costs
    static constexpr bool CHECK = false, ROLL_P = false;
    static __device__ __forceinline__ Word cost(const uint2* bl, const uint2* br, size_t row, int x, int xr)
    { const uint2 c = sgm_cost4<1>(bl, br, row, x, xr); return __builtin_amdgcn_perm(c.y, c.x, 0x06040200u); }
    static __device__ __forceinline__ void widen(Word w, uint32_t& h0, uint32_t& h1)
    { h0 = __builtin_amdgcn_perm(0u, w, 0x0C010C00u); h1 = __builtin_amdgcn_perm(0u, w, 0x0C030C02u); }   // (d, d + 1), (d + 2, d + 3) as u16
};
template <int CN>
struct Cost16 {
    typedef uint2 Word;
    typedef uint16_t Elem;
    // (colour: the fused kernel's p loop stays rolled, or the whole body of its unrolled k loop grows past what the compiler
    // unrolls, and then ring[][k] goes to scratch)
    static constexpr bool CHECK = true, ROLL_P = CN != 1;
    static __device__ __forceinline__ Word cost(const uint2* bl, const uint2* br, size_t row, int x, int xr) { return sgm_cost4<CN>(bl, br, row, x, xr); }
    static __device__ __forceinline__ void widen(Word w, uint32_t& h0, uint32_t& h1) { h0 = w.x; h1 = w.y; }
};

// N1, the census descriptor of a (2 HW + 1) x (2 HH + 1) window: one bit per offset (i, j) != (0, 0), set where the neighbour at
// clamped coordinates is strictly darker than the centre -- at most 62 bits, the low 32 in .x (bit order: row by row, the
// centre skipped; only Hamming distances leave the cost stage, so the order is nobody else's business).  A workgroup owns a
// tile of 64 x 16 pixels of one image of one frame: the tile and its halo go to LDS once (clamped coordinates, a byte per
// lane and load), then every lane builds the words of four pixels of its column and stores them, 8 bytes each, where
// k_sgm_bounds<1> stores its records.  1 byte read and 8 written per pixel and image, as there -- but it runs at 2 x that
// kernel's time (9 x 7, 720p): up to 62 LDS byte reads and compares per pixel bind it, not HBM.
template <int HW, int HH>
__global__ __launch_bounds__(256) void k_sgm_census(Plane8 L, Plane8 R, uint2* cl, uint2* cr, int W, int H, int n)
{
    constexpr int TX = 64, TY = 16, LW = TX + 2 * HW, LH = TY + 2 * HH;
    __shared__ uint8_t tile[LH][LW];
    int f = blockIdx.z;
    const bool right = f >= n;
    if (right) f -= n;
    const Plane8 S = right ? R : L;
    const uint8_t* img = S.base + (size_t)f * S.frame;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    for (int i = threadIdx.x; i < LW * LH; i += 256) {
        const int ty = i / LW, tx = i - ty * LW;
        const int ys = min(max(y0 + ty - HH, 0), H - 1), xs = min(max(x0 + tx - HW, 0), W - 1);
        tile[ty][tx] = img[(size_t)ys * S.pitch + xs];
    }
    __syncthreads();
    const int tx = threadIdx.x % TX, x = x0 + tx;
    if (x >= W) return;
    uint2* out = (right ? cr : cl) + (size_t)f * H * W;
#pragma unroll
    for (int q = 0; q < TY / 4; ++q) {
        const int ty = threadIdx.x / TX + 4 * q, y = y0 + ty;
        if (y >= H) break;
        const uint32_t c = tile[ty + HH][tx + HW];
        uint32_t lo = 0u, hi = 0u;
        int bit = 0;
#pragma unroll
        for (int j = 0; j <= 2 * HH; ++j) {
#pragma unroll
            for (int i = 0; i <= 2 * HW; ++i) {
                if (i == HW && j == HH) continue;
                const uint32_t b = (uint32_t)tile[ty + j][tx + i] < c ? 1u : 0u;
                if (bit < 32) lo |= b << bit; else hi |= b << (bit - 32);
                ++bit;
            }
        }
        out[(size_t)y * W + x] = make_uint2(lo, hi);
    }
}

// N2: the pixel cost of census descriptors, popcount(left xor right) <= M = cw ch - 1 <= 62, four consecutive disparities as
// four u8 in a dword like Cost8 (whose widen it shares); block sums of the fused kernel's windows stay below 49 * 62: no check
struct CostCensus : Cost8 {
    static __device__ __forceinline__ Word cost(const uint2* cl, const uint2* cr, size_t row, int x, int xr) { return sgm_census_cost4(cl, cr, row, x, xr); }
};

// The item of a thread of the kernels below whose grid.x covers W1 * D/4: column xi of the domain and the four consecutive
// disparities d .. d + 3 (d fastest).  false: the thread is past the last item.
__device__ __forceinline__ bool sgm_item(const SGMGeom& g, int& xi, int& d)
{
    const int dq = g.D >> 2;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)g.W1 * dq) return false;
    d = (int)(idx % dq) * 4; xi = (int)(idx / dq);
    return true;
}

// pixel cost -> the volume pix [n][H][W1][D] of F::Elem (u8: b.pix; u16: it lives in S, dead until the first path pass writes it)
template <typename F>
__global__ __launch_bounds__(256) void k_sgm_pix(const uint2* bl, const uint2* br, typename F::Elem* pix, SGMGeom g)
{
    int xi, d;
    if (!sgm_item(g, xi, d)) return;
    const int y = blockIdx.y, f = blockIdx.z;
    const int x = g.x0 + xi, xr = x - (d + g.minD);                     // element j pairs x with xr - j (N2: xr - 3 >= 1 on the domain)
    const size_t row = ((size_t)f * g.H + y) * g.W;
    *(typename F::Word*)(pix + (((size_t)f * g.H + y) * g.W1 + xi) * g.D + d) = F::cost(bl, br, row, x, xr);
}

// four consecutive pixel costs (u8 volume: one dword, u16 volume: one qword) added to s[0..3]
__device__ __forceinline__ void sgm_acc4(const uint8_t* p, int* s)
{ const uint32_t w = *(const uint32_t*)p; s[0] += w & 0xff; s[1] += (w >> 8) & 0xff; s[2] += (w >> 16) & 0xff; s[3] += w >> 24; }
__device__ __forceinline__ void sgm_acc4(const uint16_t* p, int* s)
{ const uint2 w = *(const uint2*)p; s[0] += w.x & 0xffff; s[1] += w.x >> 16; s[2] += w.y & 0xffff; s[3] += w.y >> 16; }

// The four 32-bit sums of an item.  (Packing, storing and checking them stays written out in k_sgm_box, which stores them
// unmasked, and in k_sgm_box_any and k_sgm_warm3, which truncate: a shared helper changes the instruction streams of all three.)
struct Sum4 { int v[4]; };

// block cost: thread = (x, four consecutive d); walks down a strip of rows keeping the last 2R+1 horizontal sums in
// registers, so every pixel-cost element is read (2R+1) times instead of (2R+1)^2 times.  T: the pixel-cost volume's type
// (uint8_t, or uint16_t where a pixel cost can pass 255: colour, preFilterCap >= 96)
template <int R, typename T>
__global__ __launch_bounds__(256) void k_sgm_box(const T* pix, uint16_t* C, SGMGeom g, int rows_per_strip, int cost_limit, int32_t* ovf)
{
    int xi, d;
    if (!sgm_item(g, xi, d)) return;
    const int f = blockIdx.z;
    const int y0 = blockIdx.y * rows_per_strip, y1 = min(y0 + rows_per_strip, g.H);
    const T* base = pix + (size_t)f * g.H * g.W1 * g.D + d;
    int xs[2 * R + 1];
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) xs[k] = min(max(xi + k - R, 0), g.W1 - 1) * g.D;
    const auto hsum = [&](int y) -> Sum4 {
        const T* row = base + (size_t)min(max(y, 0), g.H - 1) * g.W1 * g.D;
        Sum4 s = {{0, 0, 0, 0}};
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) sgm_acc4(row + xs[k], s.v);
        return s;
    };
    Sum4 ring[2 * R + 1];
    int sum[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) {
        ring[k] = hsum(y0 - R + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) sum[j] += ring[k].v[j];
    }
    uint16_t* out = C + (((size_t)f * g.H) * g.W1 + xi) * g.D + d;
    for (int y = y0; y < y1; y += 2 * R + 1) {
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
            if (y + k < y1) {
                *(uint2*)(out + (size_t)(y + k) * g.W1 * g.D) =
                    make_uint2((uint32_t)sum[0] | ((uint32_t)sum[1] << 16), (uint32_t)sum[2] | ((uint32_t)sum[3] << 16));
                if (cost_limit > 0 && max(max(sum[0], sum[1]), max(sum[2], sum[3])) > cost_limit) *ovf = 1;
                const Sum4 h = hsum(y + k + R + 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) { sum[j] += h.v[j] - ring[k].v[j]; }
                ring[k] = h;
            }
        }
    }
}

// Pixel cost and block sum in ONE kernel for the small windows (R <= 3; D = 16, 32, 64, 128, 256): a workgroup owns a tile of
// TX = 4 * CG output columns (CG = 256 / (D / 4) columns per pass of its threads) and walks a strip of rows; per source row every
// thread computes the Birchfield-Tomasi costs of ~4.5 (column, four disparities) items of the tile + halo into LDS (k_sgm_pix's
// arithmetic, in the form F: Cost8 or Cost16<CN>), and after one barrier (the tile is double-buffered) sums 2R + 1 of them from
// LDS for each of its four output columns and slides the vertical window in registers (k_sgm_box's ring, packed u16: block sums
// stay below 49 * 951 < 65536).  The pixel-cost volume is neither written nor read: 280 MB of HBM traffic per 720p D = 128
// pair, and k_sgm_box's 2R + 1 trips to L2 per output are LDS reads.  F::CHECK: block sums above cost_limit (> 0) set *ovf.
template <typename F, int R, int DQ>
__global__ __launch_bounds__(256) void k_sgm_pixbox(const uint2* bl, const uint2* br, uint16_t* C, SGMGeom g, int rows_per_strip,
                                                    int cost_limit, int32_t* ovf)
{
    constexpr int CG = 256 / DQ, TX = 4 * CG, TW = TX + 2 * R, NP = (TW + CG - 1) / CG, W1R = 2 * R + 1, PU = F::ROLL_P ? 1 : NP;
    __shared__ typename F::Word tile[2][TW][DQ];            // [row parity][tile column][disparity quad]: four pixel costs
    const int dqi = threadIdx.x % DQ, cg = threadIdx.x / DQ, d = dqi * 4;
    const int xt0 = blockIdx.x * TX;                        // first output column of the tile (W1 domain)
    const int f = blockIdx.z;
    const int y0 = blockIdx.y * rows_per_strip, y1 = min(y0 + rows_per_strip, g.H);
    uint32_t ring[4][W1R][2], sum[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { sum[i][0] = sum[i][1] = 0u; for (int k = 0; k < W1R; ++k) ring[i][k][0] = ring[i][k][1] = 0u; }
    bool over = false;
    const int nsrc = (y1 - y0) + 2 * R;                     // source rows y0 - R .. y1 - 1 + R (clamped into the frame)
    for (int base = 0; base < nsrc; base += W1R) {
#pragma unroll
        for (int k = 0; k < W1R; ++k) {
            const int t = base + k;
            if (t < nsrc) {                                 // workgroup-uniform
                const int par = t & 1;
                const int ysrc = min(max(y0 - R + t, 0), g.H - 1);
                const size_t row = ((size_t)f * g.H + ysrc) * g.W;
                // pixel costs of this row's tile columns (+ halo), clamped into [0, W1)
#pragma unroll PU
                for (int p = 0; p < NP; ++p) {
                    const int tc = cg + p * CG;
                    if (tc < TW) {
                        const int xi = min(max(xt0 - R + tc, 0), g.W1 - 1);
                        const int x = g.x0 + xi;
                        tile[par][tc][dqi] = F::cost(bl, br, row, x, x - (d + g.minD));
                    }
                }
                __syncthreads();
                const int yo = y0 - 2 * R + t;               // the output row whose window this source row completes
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int tcol = cg + i * CG;            // output column xt0 + tcol: tile columns tcol .. tcol + 2R
                    uint32_t h0 = 0u, h1 = 0u;
#pragma unroll
                    for (int q = 0; q < W1R; ++q) {
                        uint32_t w0, w1;
                        F::widen(tile[par][tcol + q][dqi], w0, w1);
                        h0 = pk_add(h0, w0);
                        h1 = pk_add(h1, w1);
                    }
                    sum[i][0] = pk_sub(pk_add(sum[i][0], h0), ring[i][k][0]);
                    sum[i][1] = pk_sub(pk_add(sum[i][1], h1), ring[i][k][1]);
                    ring[i][k][0] = h0; ring[i][k][1] = h1;
                    const int xo = xt0 + tcol;
                    if (yo >= y0 && xo < g.W1) {
                        *(uint2*)(C + (((size_t)f * g.H + yo) * g.W1 + xo) * g.D + d) = make_uint2(sum[i][0], sum[i][1]);
                        if constexpr (F::CHECK) {
                            const uint32_t m = pk_max_u(sum[i][0], sum[i][1]);
                            over |= (int)max(m & 0xffffu, m >> 16) > cost_limit;
                        }
                    }
                }
            }
        }
    }
    if (F::CHECK && cost_limit > 0 && over) *ovf = 1;
}

// Any window (R > 8: the register ring of k_sgm_box<R> would not fit): the running vertical sum gains the entering row's
// horizontal sum and loses the leaving row's, both recomputed -- 2 (2R + 1) loads per output instead of 2R + 1.  Sums are
// 32-bit; a block cost above cost_limit (> 0) sets *ovf and is stored truncated (the caller refuses the frame).
template <typename T>
__global__ __launch_bounds__(256) void k_sgm_box_any(const T* pix, uint16_t* C, SGMGeom g, int R, int rows_per_strip, int cost_limit, int32_t* ovf)
{
    int xi, d;
    if (!sgm_item(g, xi, d)) return;
    const int f = blockIdx.z;
    const int y0 = blockIdx.y * rows_per_strip, y1 = min(y0 + rows_per_strip, g.H);
    const T* base = pix + (size_t)f * g.H * g.W1 * g.D + d;
    const auto hsum = [&](int y) -> Sum4 {
        const T* row = base + (size_t)min(max(y, 0), g.H - 1) * g.W1 * g.D;
        Sum4 s = {{0, 0, 0, 0}};
        for (int k = -R; k <= R; ++k) sgm_acc4(row + (size_t)min(max(xi + k, 0), g.W1 - 1) * g.D, s.v);
        return s;
    };
    int sum[4] = {0, 0, 0, 0};
    for (int k = -R; k <= R; ++k) { const Sum4 h = hsum(y0 + k); for (int j = 0; j < 4; ++j) sum[j] += h.v[j]; }
    uint16_t* out = C + (((size_t)f * g.H) * g.W1 + xi) * g.D + d;
    for (int y = y0; y < y1; ++y) {
        *(uint2*)(out + (size_t)y * g.W1 * g.D) =
            make_uint2((uint32_t)(sum[0] & 0xffff) | ((uint32_t)sum[1] << 16), (uint32_t)(sum[2] & 0xffff) | ((uint32_t)sum[3] << 16));
        if (cost_limit > 0 && max(max(sum[0], sum[1]), max(sum[2], sum[3])) > cost_limit) *ovf = 1;
        const Sum4 a = hsum(y + R + 1), b = hsum(y - R);
        for (int j = 0; j < 4; ++j) sum[j] += a.v[j] - b.v[j];
    }
}

// MODE_SGBM_3WAY's warm-up block costs (rule T3): for stripe s = 1 .. 3 with first source row a > 0 the
// rows y in [a, min(a + R, e)) get C'(y) = sum over j = -R .. R of h(clamp(y + j, a, H - 1)) -- R3's window with its top clamped to
// the stripe's first source row instead of the frame's.  thread = (x, four consecutive d) of one stripe of one frame, as in
// k_sgm_box; h(r), the horizontal sum of row r's pixel costs (first and last column of the domain replicated), comes straight
// from F::cost, so no cost volume is read and none of the kernels above changes.  C'(a) = (R + 1) h(a) + h(a + 1) + .. + h(a + R);
// a row further down the window gains h(y + 1 + R) and loses one h(a).  At most 2 R rows of h per thread.  Sums are 32-bit; a
// C' above cost_limit (> 0) sets *ovf and is stored truncated (T8: the caller refuses the frame).
// Cw: [frame][stripe - 1][row - a, wrows of them][x - x0][d].
template <typename F>
__global__ __launch_bounds__(256) void k_sgm_warm3(const uint2* bl, const uint2* br, uint16_t* Cw, SGMGeom g, Sgm3Stripes st, int R,
                                                   int wrows, int cost_limit, int32_t* ovf)
{
    int xi, d;
    if (!sgm_item(g, xi, d)) return;
    const int f = blockIdx.z;
    const Sgm3Stripe s = st.s[1 + blockIdx.y];
    if (s.a <= 0 || s.o >= s.e) return;                                 // C' = C (T3), or an empty stripe
    const auto hsum = [&](int y) -> Sum4 {
        const size_t row = ((size_t)f * g.H + min(y, g.H - 1)) * g.W;
        Sum4 h = {{0, 0, 0, 0}};
        for (int k = -R; k <= R; ++k) {
            const int x = g.x0 + min(max(xi + k, 0), g.W1 - 1);
            uint32_t w0, w1;
            F::widen(F::cost(bl, br, row, x, x - (d + g.minD)), w0, w1);
            h.v[0] += (int)(w0 & 0xffffu); h.v[1] += (int)(w0 >> 16); h.v[2] += (int)(w1 & 0xffffu); h.v[3] += (int)(w1 >> 16);
        }
        return h;
    };
    const Sum4 ha = hsum(s.a);
    int sum[4];
    for (int j = 0; j < 4; ++j) sum[j] = (R + 1) * ha.v[j];
    for (int k = 1; k <= R; ++k) { const Sum4 h = hsum(s.a + k); for (int j = 0; j < 4; ++j) sum[j] += h.v[j]; }
    const int rows = min(wrows, s.e - s.a);
    uint16_t* out = Cw + ((((size_t)f * (SGM3_STRIPES - 1) + blockIdx.y) * wrows) * g.W1 + xi) * g.D + d;
    for (int k = 0; k < rows; ++k) {
        *(uint2*)(out + (size_t)k * g.W1 * g.D) =
            make_uint2((uint32_t)(sum[0] & 0xffff) | ((uint32_t)sum[1] << 16), (uint32_t)(sum[2] & 0xffff) | ((uint32_t)sum[3] << 16));
        if (cost_limit > 0 && max(max(sum[0], sum[1]), max(sum[2], sum[3])) > cost_limit) *ovf = 1;
        if (k + 1 < rows) { const Sum4 h = hsum(s.a + k + 1 + R); for (int j = 0; j < 4; ++j) sum[j] += h.v[j] - ha.v[j]; }
    }
}

// rtdm_debug_sgm_cost16: the u16 cost forms for gray frames as well (they must give what the u8 forms give)
static std::atomic<int> g_cost16{0};
void sgm_cost16_set(int on) { g_cost16.store(on ? 1 : 0, std::memory_order_relaxed); }
bool sgm_cost16_forced() { return g_cost16.load(std::memory_order_relaxed) != 0; }

// The one step from a plan's form to its type: fn is called with a value of Cost8, Cost16<1>, Cost16<3> or CostCensus
template <typename Fn>
static void with_cost_form(SgmCostForm form, Fn&& fn)
{
    switch (form) {
        case SgmCostForm::BT8: return fn(Cost8{});
        case SgmCostForm::BT16_GRAY: return fn(Cost16<1>{});
        case SgmCostForm::BT16_COLOUR: return fn(Cost16<3>{});
        case SgmCostForm::CENSUS: return fn(CostCensus{});
    }
}
// ... and from a run-time value to a template argument: fn(std::integral_constant<int, V>) for the V of the list that v equals,
// for the last one if it equals none (the plan sends no such value)
template <int V0, int... V, typename Fn>
static void with_int(int v, Fn&& fn)
{
    if (sizeof...(V) == 0 || v == V0) fn(std::integral_constant<int, V0>{});
    else if constexpr (sizeof...(V) != 0) with_int<V...>(v, fn);
}

// The whole cost stage as plan_sgm_cost planned it ("SGM: cost routes"): the bounds or the descriptors, the pixel-cost
// volume where the plan has one, the block sum -> b.C, and last MODE_SGBM_3WAY's warm-up costs -> b.Cw: they read the records
// before the caller reuses b.gr for the winners, and b.Cw may alias b.pix, which is dead only once C exists.
void launch_sgm_cost(const SgmCostPlan& p, Plane8 L, Plane8 R, const SGMGeom& g, const SGMBuffers& b, int n, hipStream_t stream)
{
    const dim3 blk(256);
    const int rps = 48, strips = (g.H + rps - 1) / rps, tx = 4 * (256 / (g.D / 4));     // rows per strip, columns per tile, of the block sums
    const auto items = [&](int rows) { return dim3((unsigned)(((size_t)g.W1 * (g.D / 4) + 255) / 256), rows, n); };   // a thread per sgm_item
    uint2 *bl = (uint2*)(p.colour_records ? b.cl : b.gl), *br = (uint2*)(p.colour_records ? b.cr : b.gr);
    if (p.form == SgmCostForm::CENSUS) {                     // the window (cw, ch) in {3, 5, 7, 9} x {3, 5, 7}: the caller has checked it
        const dim3 grid((g.W + 63) / 64, (g.H + 15) / 16, 2 * n);
        with_int<3, 5, 7, 9>(p.cw, [&](auto cw) { with_int<3, 5, 7>(p.ch, [&](auto ch) {
            hipLaunchKernelGGL((k_sgm_census<decltype(cw)::value / 2, decltype(ch)::value / 2>), grid, blk, 0, stream, L, R, bl, br, g.W, g.H, n);
        }); });
    } else {
        const dim3 grid((g.W + 255) / 256, g.H, 2 * n);
        if (p.colour_records) hipLaunchKernelGGL(k_sgm_bounds<3>, grid, blk, 0, stream, L, R, bl, br, g.W, g.H, n, p.ftz);
        else hipLaunchKernelGGL(k_sgm_bounds<1>, grid, blk, 0, stream, L, R, bl, br, g.W, g.H, n, p.ftz);
    }
    with_cost_form(p.form, [&](auto form) {
        using F = decltype(form); using T = typename F::Elem;
        T* vol = p.volume == SgmCostVolume::PIX ? (T*)b.pix : (T*)b.S;
        if (p.volume != SgmCostVolume::NONE) hipLaunchKernelGGL(k_sgm_pix<F>, items(g.H), blk, 0, stream, bl, br, vol, g);
        switch (p.sum) {
            case SgmCostSum::FUSED:                          // R <= 3 and D / 4 in {4, 8, 16, 32, 64}
                with_int<0, 1, 2, 3>(p.R, [&](auto r) { with_int<4, 8, 16, 32, 64>(g.D / 4, [&](auto dq) {
                    hipLaunchKernelGGL((k_sgm_pixbox<F, decltype(r)::value, decltype(dq)::value>), dim3((g.W1 + tx - 1) / tx, strips, n), blk, 0,
                                       stream, bl, br, b.C, g, rps, p.cost_limit, b.ovf);
                }); });
                break;
            case SgmCostSum::BOX:                            // R <= 8 on a u8 volume, <= 6 on a u16 one: above, the register ring would spill
                with_int<0, 1, 2, 3, 4, 5, 6, 7, 8>(p.R, [&](auto r) {
                    if constexpr (decltype(r)::value <= (sizeof(T) == 1 ? 8 : 6))
                        hipLaunchKernelGGL((k_sgm_box<decltype(r)::value, T>), items(strips), blk, 0, stream, vol, b.C, g, rps, p.cost_limit, b.ovf);
                });
                break;
            case SgmCostSum::BOX_ANY:
                hipLaunchKernelGGL(k_sgm_box_any<T>, items(strips), blk, 0, stream, vol, b.C, g, p.R, rps, p.cost_limit, b.ovf);
                break;
        }
        if (p.warm)
            hipLaunchKernelGGL(k_sgm_warm3<F>, items(SGM3_STRIPES - 1), blk, 0, stream, bl, br, b.Cw, g, sgm3_stripes(g.H, 2 * p.R + 1), p.R,
                               p.wrows, p.cost_limit, b.ovf);
    });
}

}  // namespace rtdm
