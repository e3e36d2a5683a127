// rtdm_sgm.h -- device-side pieces shared by the StereoSGBM units (k_sgm_cost.hip, k_sgm_paths.hip, k_sgm_wide.hip):
// the vector loads and stores of a lane's disparities, the DPP minima, the Birchfield-Tomasi pixel
// cost and the path recurrence.  One copy of each: a fix to the recurrence, to R5 or to R6 is made here.
#pragma once

#include "rtdm_kernels.h"
#include "rtdm_device.h"
#include "rtdm_pk16.h"
#include "rtdm_sgm_stripes.h"

namespace rtdm {

// Two u16 in a dword (the pk_* helpers of rtdm_pk16.h): max(0, u - v1, v0 - u) is max(u -sat v1, v0 -sat u), so a
// Birchfield-Tomasi cost is 11 VALU per two disparities; the path recurrence and the block sums use the wrapping /
// saturating sums and differences.

// The 2 * NP2 consecutive disparities of a lane as NP2 u16 pairs (NP2 = 1, 2, 4, 8), loaded and stored in the widest pieces
template <int NP2> struct PackW { uint32_t w[NP2]; };
template <int NP2>
__device__ __forceinline__ PackW<NP2> ld_w(const uint16_t* p)
{
    PackW<NP2> r;
    if constexpr (NP2 == 1) { r.w[0] = *(const uint32_t*)p; }
    else if constexpr (NP2 == 2) { const uint2 v = *(const uint2*)p; r.w[0] = v.x; r.w[1] = v.y; }
    else {
#pragma unroll
        for (int q = 0; q < NP2 / 4; ++q) {
            const uint4 v = *(const uint4*)(p + 8 * q);
            r.w[4 * q] = v.x; r.w[4 * q + 1] = v.y; r.w[4 * q + 2] = v.z; r.w[4 * q + 3] = v.w;
        }
    }
    return r;
}
template <int NP2>
__device__ __forceinline__ void st_w(uint16_t* p, const uint32_t* o)
{
    if constexpr (NP2 == 1) { *(uint32_t*)p = o[0]; }
    else if constexpr (NP2 == 2) { *(uint2*)p = make_uint2(o[0], o[1]); }
    else {
#pragma unroll
        for (int q = 0; q < NP2 / 4; ++q) *(uint4*)(p + 8 * q) = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
}

// minimum over the lane's row of 16, in every lane of that row (values < 2^31): four DPP steps
__device__ __forceinline__ int row_min_i32(int v)
{
#define RTDM_DPP_MIN(ctrl) v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, ctrl, 0xf, 0xf, false))
    RTDM_DPP_MIN(0xB1); RTDM_DPP_MIN(0x4E); RTDM_DPP_MIN(0x141); RTDM_DPP_MIN(0x140);
#undef RTDM_DPP_MIN
    return v;
}
// ... over the lane's half-wave, in every lane of that half: the two rows of a half by v_permlane16_swap
__device__ __forceinline__ int half_min_i32(int v)
{
    v = row_min_i32(v);
    const auto s = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);   // {rows 0 0 2 2, rows 1 1 3 3}
    return min((int)s[0], (int)s[1]);
}
// ... over the whole wave, in every lane: the two halves by v_permlane32_swap
__device__ __forceinline__ int wave_min_i32(int v)
{
    v = half_min_i32(v);
    const auto t = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return min((int)t[0], (int)t[1]);
}

// Birchfield-Tomasi bounds of a value against the half-way points to its two neighbours: value | min << 8 | max << 16
__device__ __forceinline__ uint32_t bt_pack(int v, int m, int p, bool has_m, bool has_p)
{
    const int l = has_m ? (v + m) / 2 : v, r = has_p ? (v + p) / 2 : v;
    return (uint32_t)v | ((uint32_t)min(min(l, r), v) << 8) | ((uint32_t)max(max(l, r), v) << 16);
}
// the cost of one left pixel (u, u0, u1 replicated into both halves) against two right pixels (low / high half)
__device__ __forceinline__ uint32_t bt_cost2(uint32_t U, uint32_t U0, uint32_t U1, uint32_t V, uint32_t V0, uint32_t V1)
{ return pk_min_u(pk_max_u(pk_subsat_u(U, V1), pk_subsat_u(V0, U)), pk_max_u(pk_subsat_u(V, U1), pk_subsat_u(U0, V))); }

// packed u16 pixel cost (gradient + (intensity >> 2)) of one left record a against two right records (low half: lo, high half: hi)
__device__ __forceinline__ uint32_t sgm_cost2(uint2 a, uint2 lo, uint2 hi)
{
    const auto rep = [](uint32_t w, int k) -> uint32_t { return ((w >> (8 * k)) & 0xffu) * 0x00010001u; };
    const uint32_t cg = bt_cost2(rep(a.x, 0), rep(a.x, 1), rep(a.x, 2), __builtin_amdgcn_perm(hi.x, lo.x, 0x0C040C00u),
                                 __builtin_amdgcn_perm(hi.x, lo.x, 0x0C050C01u), __builtin_amdgcn_perm(hi.x, lo.x, 0x0C060C02u));
    const uint32_t cr = bt_cost2(rep(a.y, 0), rep(a.y, 1), rep(a.y, 2), __builtin_amdgcn_perm(hi.y, lo.y, 0x0C040C00u),
                                 __builtin_amdgcn_perm(hi.y, lo.y, 0x0C050C01u), __builtin_amdgcn_perm(hi.y, lo.y, 0x0C060C02u));
    return cg + ((cr >> 2) & 0x003f003fu);                              // both <= 63 + 30 per channel: no carry between the halves
}

// pixel costs of left column x against right columns xr, xr - 1, xr - 2, xr - 3 (disparities d .. d + 3), summed over the CN
// channels: {(d, d + 1), (d + 2, d + 3)} as packed u16.  row = (f * H + y) * W.
template <int CN>
__device__ __forceinline__ uint2 sgm_cost4(const uint2* bl, const uint2* br, size_t row, int x, int xr)
{
    uint32_t c0 = 0u, c1 = 0u;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        const uint2 a = bl[(row + x) * CN + c];
        uint2 b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = br[(row + xr - j) * CN + c];
        c0 += sgm_cost2(a, b[0], b[1]);
        c1 += sgm_cost2(a, b[2], b[3]);
    }
    return make_uint2(c0, c1);
}

// The census pixel cost (N2): Hamming distances of the 64-bit descriptor of left column x to those of right
// columns xr, xr - 1, xr - 2, xr - 3 (disparities d .. d + 3), each <= 62, as four u8 in a dword, d in the low byte.  Two
// popcounts per disparity, the second accumulating onto the first (v_bcnt_u32_b32).  row = (f * H + y) * W.
__device__ __forceinline__ uint32_t sgm_census_cost4(const uint2* cl, const uint2* cr, size_t row, int x, int xr)
{
    const uint2 a = cl[row + x];
    uint32_t w = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint2 b = cr[row + xr - j];
        w |= (uint32_t)(__builtin_popcount(a.x ^ b.x) + __builtin_popcount(a.y ^ b.y)) << (8 * j);
    }
    return w;
}

// The path recurrence (R4) for one u16 pair of a line: L <- C + min(Lp[d], Lp[d -+ 1] + P1, min Lp + P2) - min Lp, with the
// previous pixel's (previous, own, next) pairs, its line minimum mps and mpP2 = that + P2 in both halves of a dword
__device__ __forceinline__ uint32_t sgm_pair_step(uint32_t prev, uint32_t own, uint32_t next, uint32_t c, uint32_t mps, uint32_t mpP2,
                                                  uint32_t P1s)
{
    const uint32_t dn = __builtin_amdgcn_alignbit(own, prev, 16);       // {prev.hi, own.lo}: d - 1 of both elements
    const uint32_t up = __builtin_amdgcn_alignbit(next, own, 16);       // {own.hi, next.lo}: d + 1
    const uint32_t best = pk_min_u(pk_min_u(own, mpP2), pk_addsat_u(pk_min_u(dn, up), P1s));
    return pk_sub(pk_add(c, best), mps);
}

// one step of one line for both half-waves of the wave: sgm_pair_step on every pair, or C where the line starts; the pairs at
// the lane's ends come from the neighbouring lanes by DPP wave shifts (none outside the half-wave); mps <- the new line
// minimum in both halves of a dword.  L may alias Lp.
template <int NP2, bool MAY_START>
__device__ __forceinline__ void sgm_line_step(uint32_t* L, uint32_t& mps, const uint32_t* Lp, uint32_t mpsp, const uint32_t* c,
                                              bool start, bool live, int hl, uint32_t P1s, uint32_t P2s)
{
    const uint32_t NONE = 0xffffffffu;
    uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)NONE, (int)Lp[NP2 - 1], 0x138, 0xf, 0xf, false);   // wave_shr:1
    uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)NONE, (int)Lp[0], 0x130, 0xf, 0xf, false);         // wave_shl:1
    lo = hl == 0 ? NONE : lo;
    hi = hl == 31 ? NONE : hi;
    const uint32_t mpP2 = pk_add(mpsp, P2s);
    uint32_t nl[NP2];
#pragma unroll
    for (int r = 0; r < NP2; ++r) {
        nl[r] = sgm_pair_step(r ? Lp[r - 1] : lo, Lp[r], r + 1 < NP2 ? Lp[r + 1] : hi, c[r], mpsp, mpP2, P1s);
        if (MAY_START) nl[r] = start ? c[r] : nl[r];
    }
    uint32_t mm = NONE;
#pragma unroll
    for (int r = 0; r < NP2; ++r) { L[r] = live ? nl[r] : NONE; mm = pk_min_u(mm, L[r]); }
    mps = (uint32_t)half_min_i32((int)min(mm & 0xffffu, mm >> 16)) * 0x10001u;
}

// Path line `line` of direction (dx, dy) on the W1 x H cost domain: its first pixel (sx, sy); returns its number of steps.
// Lines [0, H) for dy = 0, [0, W1) for dx = 0, else the W1 that start in the first row and then the H - 1 that start in the
// first column below it (sgm_line_count of them).
__device__ __forceinline__ int sgm_line_start(int line, int dx, int dy, int W1, int H, int& sx, int& sy)
{
    if (dy == 0) { sy = line; sx = dx > 0 ? 0 : W1 - 1; }
    else if (dx == 0) { sx = line; sy = dy > 0 ? 0 : H - 1; }
    else if (line < W1) { sx = line; sy = dy > 0 ? 0 : H - 1; }
    else { const int k = line - W1 + 1; sx = dx > 0 ? 0 : W1 - 1; sy = dy > 0 ? k : H - 1 - k; }
    const int nx = dx > 0 ? W1 - sx : (dx < 0 ? sx + 1 : 0x7fffffff);
    const int ny = dy > 0 ? H - sy : (dy < 0 ? sy + 1 : 0x7fffffff);
    return min(nx, ny);
}
inline int sgm_line_count(const SGMGeom& g, int dx, int dy) { return dy == 0 ? g.H : (dx == 0 ? g.W1 : g.W1 + g.H - 1); }

// The end of the winner-take-all step: the record of a pixel whose first minimum is mins at disparity bd, with the aggregated
// costs s_p / s_n at bd + 1 / bd - 1 (quadratic sub-pixel, x16).  rejected (uniqueness, or every cost saturated): the invalid value.
__device__ __forceinline__ SgmWin sgm_win_record(int bd, int mins, int s_p, int s_n, bool rejected, int D, int minD)
{
    int d16 = bd * 16;
    if (bd > 0 && bd < D - 1) {
        const int den = max(s_n + s_p - 2 * mins, 1);
        d16 += div_trunc_rcp((s_n - s_p) * 16 + den, den * 2);            // |numerator| < 2^21
    }
    SgmWin w;
    w.d16 = (int16_t)((minD - 1) * 16); w.bd = (int16_t)(minD - 1); w.mins = 0; w.pad = 0;
    if (!rejected) { w.d16 = (int16_t)(d16 + minD * 16); w.bd = (int16_t)(bd + minD); w.mins = (uint16_t)mins; }
    return w;
}

// Host side, between launch_sgm (k_sgm.hip) and the units that own the kernels: one launcher per step kind of a plan.  Each
// issues the planned pass and decides nothing.
static constexpr int SWEEP_RING = 4;                      // rows of edge data kept per (strip, side) of a k_sgm_sweep launch
inline int sgm_np2(int D) { return D <= 64 ? 1 : (D <= 128 ? 2 : 4); }   // u16 pairs per lane of the half-wave forms
struct SgmCall { const SGMGeom& g; const SGMBuffers& b; int P1, P2, uniq, n; SgmWin* win; hipStream_t stream; int blockSize; };   // (blockSize: VERT3 only)
void launch_sgm_wide(const SgmPass& p, const SgmCall& c);
void launch_path_h(const SgmPass& p, const SgmCall& c);
void launch_vert(const SgmPass& p, const SgmCall& c);
// MODE_SGBM_3WAY (T1-T8): the striped vertical pass that reads the warm-up block costs C' of stripes
// 1 .. 3 (b.Cw: the cost stage's last kernel) and decides the winners.  Rows of C' kept per stripe: sgm3_warm_rows (rtdm_sgm_stripes.h).
void launch_vert3(const SgmPass& p, const SgmCall& c);
// false: the runtime refused (device, sweep stream or event record) before anything was launched
bool launch_sweep(const SgmPass& p, const SgmCall& c);
void launch_sgm_add_s2(const SgmCall& c);

}  // namespace rtdm
