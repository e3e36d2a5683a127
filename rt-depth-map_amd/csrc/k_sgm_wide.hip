// k_sgm_wide.hip -- the StereoSGBM path pass for wide lines: every numDisparities from 16 to 4080 in steps of 16 (the narrow
// forms in k_sgm_paths.hip hold at most 256 disparities per line).  Same recurrence as k_sgm_path_h (oracle/sgm_oracle.c R4, R5),
// same packed u16 arithmetic, same 0xffff "no neighbour" sentinel; what changes is how a line is spread over lanes:
//
//   NW = 1  one WAVE per line (four lines per workgroup), lane l holds the 2 * NP2 consecutive disparities 2 NP2 l .. as NP2
//           u16 pairs (NP2 <= 8: D <= 1024).  d - 1 / d + 1 across lanes by DPP wave shifts, the line minimum by a DPP
//           reduction inside the rows of 16 and the v_permlane16_swap / v_permlane32_swap exchanges -- no LDS, no barrier.
//   NW = 4  one WORKGROUP per line: 256 lanes, NP2 <= 8 (D <= 4096).  Inside a wave as above; what crosses a wave boundary
//           -- the wave's line minimum and its two edge pairs -- goes through LDS, double-buffered by step parity, so one
//           barrier per step suffices ("wide lines").
//
// D is a multiple of 16 and a lane holds 2, 4, 8 or 16 disparities, so padding is whole lanes: a dead lane holds 0xffff in
// every element, which never wins a minimum against a live value (<= 32767) and acts as the missing d + 1 of d = D - 1.
// LAST (the frame's last direction) decides the winners with the 12-bit key (S << 12) | d < 2^27 and writes the SgmWin record
// k_sgm_lrfinal reads, as k_sgm_path_h<.., true> does.
#include "rtdm_sgm.h"

#include <atomic>

namespace rtdm {

// One line of direction (dx, dy) per wave (NW = 1) or per workgroup (NW = 4); S (+)= L_r, or (LAST) the winners.
template <int NP2, int NW, int PF, bool LAST>
__global__ __launch_bounds__(256) void k_sgm_wide(const uint16_t* C, uint16_t* S, SGMGeom g, int dx, int dy, int P1, int P2,
                                                  int first_dir, int nlines, SgmWin* win, int uniq)
{
    constexpr int LPD = 2 * NP2;                                  // disparities per lane
    // NW > 1: what crosses a wave boundary, by step parity: each wave's line minimum, first and last pair (and, LAST, its
    // minimum key); the winner's second round (uniqueness votes, S[d* -+ 1]) is single-buffered
    __shared__ uint32_t xmin[2][NW], xlo[2][NW], xhi[2][NW];
    __shared__ int xkey[2][NW], xhit[NW], xsp, xsn;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int line = NW == 1 ? blockIdx.x * 4 + wv : blockIdx.x;
    if (line >= nlines) return;                                   // whole waves (NW = 1) / whole workgroups (NW = 4)
    const int D = g.D, W1 = g.W1, H = g.H;
    int sx, sy;
    const int nsteps = sgm_line_start(line, dx, dy, W1, H, sx, sy);   // uniform over the line's lanes
    const int li = NW == 1 ? lane : wv * 64 + lane;               // lane of the line
    const int d0 = li * LPD;
    const bool live = d0 < D;                                     // whole lanes: D is a multiple of 16 >= LPD
    const uint32_t NONE = 0xffffffffu;
    const long stride = ((long)dy * W1 + dx) * D;
    const size_t off0 = (size_t)blockIdx.y * H * W1 * D + ((size_t)sy * W1 + sx) * D + (live ? d0 : 0);
    const uint16_t* cp = C + off0;
    uint16_t* sp = S + off0;
    const uint32_t P1s = (uint32_t)P1 * 0x10001u, P2s = (uint32_t)P2 * 0x10001u;
    PackW<NP2> cr[PF], sr[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
#pragma unroll
        for (int r = 0; r < NP2; ++r) cr[k].w[r] = sr[k].w[r] = 0u;
        if (live && k < nsteps) {
            cr[k] = ld_w<NP2>(cp + (long)k * stride);
            if (!first_dir) sr[k] = ld_w<NP2>(sp + (long)k * stride);
        }
    }
    uint32_t l[NP2];
    uint32_t mps = 0, mpP2 = 0;                                   // previous pixel's line minimum, and that + P2
    uint32_t elo = NONE, ehi = NONE;                              // NW > 1: the previous step's pair next to lane 0 / lane 63
    for (int base = 0; base < nsteps; base += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int step = base + k;
            if (step >= nsteps) break;
            const PackW<NP2> c = cr[k], sv = sr[k];
            if (live && step + PF < nsteps) {
                cr[k] = ld_w<NP2>(cp + (long)(step + PF) * stride);
                if (!first_dir) sr[k] = ld_w<NP2>(sp + (long)(step + PF) * stride);
            }
            if (step == 0) {
#pragma unroll
                for (int r = 0; r < NP2; ++r) l[r] = live ? c.w[r] : NONE;
            } else {
                // the pairs next to the lane's own: lane - 1's last, lane + 1's first; at a wave's ends the neighbouring wave's
                // (LDS) or none
                uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)NONE, (int)l[NP2 - 1], 0x138, 0xf, 0xf, false);   // wave_shr:1
                uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)NONE, (int)l[0], 0x130, 0xf, 0xf, false);         // wave_shl:1
                lo = lane == 0 ? elo : lo;
                hi = lane == 63 ? ehi : hi;
                uint32_t nl[NP2];
#pragma unroll
                for (int r = 0; r < NP2; ++r) nl[r] = sgm_pair_step(r ? l[r - 1] : lo, l[r], r + 1 < NP2 ? l[r + 1] : hi, c.w[r], mps, mpP2, P1s);
#pragma unroll
                for (int r = 0; r < NP2; ++r) l[r] = live ? nl[r] : NONE;
            }
            uint32_t o[NP2];
#pragma unroll
            for (int r = 0; r < NP2; ++r) o[r] = first_dir ? l[r] : pk_min_u(pk_add(sv.w[r], l[r]), 0x7fff7fffu);   // R5
            if constexpr (!LAST) {
                if (live) st_w<NP2>(sp + (long)step * stride, o);
            }
            uint32_t mm = l[0];
#pragma unroll
            for (int r = 1; r < NP2; ++r) mm = pk_min_u(mm, l[r]);
            int m = wave_min_i32((int)min(mm & 0xffffu, mm >> 16));
            int key = 0x7fffffff;
            if constexpr (LAST) {
                // R6: the first minimum -- key (S << 12) | d, d < 4096, S <= 32767
#pragma unroll
                for (int r = 0; r < NP2; ++r) {
                    key = min(key, (int)(((o[r] & 0xffffu) << 12) | (unsigned)(d0 + 2 * r)));
                    key = min(key, (int)(((o[r] >> 16) << 12) | (unsigned)(d0 + 2 * r + 1)));
                }
                key = wave_min_i32(live ? key : 0x7fffffff);
            }
            if constexpr (NW > 1) {
                const int p = step & 1;
                if (lane == 0) { xmin[p][wv] = (uint32_t)m; xlo[p][wv] = l[0]; if (LAST) xkey[p][wv] = key; }
                if (lane == 63) xhi[p][wv] = l[NP2 - 1];
                __syncthreads();      // (the other parity was last read before the previous step's barrier: no second one)
#pragma unroll
                for (int q = 0; q < NW; ++q) {
                    m = min(m, (int)xmin[p][q]);
                    if (LAST) key = min(key, xkey[p][q]);
                }
                elo = wv > 0 ? xhi[p][wv - 1] : NONE;
                ehi = wv < NW - 1 ? xlo[p][wv + 1] : NONE;
            }
            mps = (uint32_t)m * 0x10001u;
            mpP2 = pk_add(mps, P2s);
            if constexpr (LAST) {
                const int mins = key >> 12, bd = key & 0xfff;
                bool hit = false;
                const int lim = mins * 100;
#pragma unroll
                for (int r = 0; r < NP2; ++r) {
                    hit |= (unsigned)(d0 + 2 * r - bd + 1) > 2u && (int)(o[r] & 0xffffu) * (100 - uniq) < lim;
                    hit |= (unsigned)(d0 + 2 * r + 1 - bd + 1) > 2u && (int)(o[r] >> 16) * (100 - uniq) < lim;
                }
                // S[d* +- 1]: the pair that holds it (the same r in every lane), from the lane that holds it (ds_bpermute)
                const int ip = min(bd + 1, D - 1), in = max(bd - 1, 0);
                const int rp = (ip >> 1) & (NP2 - 1), rn = (in >> 1) & (NP2 - 1);
                uint32_t wp = o[0], wn = o[0];
#pragma unroll
                for (int r = 1; r < NP2; ++r) { wp = rp == r ? o[r] : wp; wn = rn == r ? o[r] : wn; }
                wp = (uint32_t)__builtin_amdgcn_ds_bpermute(((ip / LPD) & 63) << 2, (int)wp);
                wn = (uint32_t)__builtin_amdgcn_ds_bpermute(((in / LPD) & 63) << 2, (int)wn);
                int s_p = (int)((wp >> ((ip & 1) << 4)) & 0xffffu), s_n = (int)((wn >> ((in & 1) << 4)) & 0xffffu);
                bool rejected = __any(hit && live);
                if constexpr (NW > 1) {
                    // second round: every wave's uniqueness vote, S[d* -+ 1] from the waves that hold them
                    if (lane == 0) {
                        xhit[wv] = rejected ? 1 : 0;
                        if ((ip / LPD) >> 6 == wv) xsp = s_p;
                        if ((in / LPD) >> 6 == wv) xsn = s_n;
                    }
                    __syncthreads();  // (rewritten only after the next step's first barrier, which wave 0 passes after reading)
                    if (wv == 0) {
#pragma unroll
                        for (int q = 0; q < NW; ++q) rejected |= xhit[q] != 0;
                        s_p = xsp; s_n = xsn;
                    }
                }
                // every aggregated cost saturated at 32767: the library finds no winner (sgm_wta_half)
                rejected |= mins >= 32767;
                if (wv == 0 || NW == 1) {
                    const SgmWin w = sgm_win_record(bd, mins, s_p, s_n, rejected, D, g.minD);
                    if (lane == 0) {
                        const int xi = sx + step * dx, yy = sy + step * dy;
                        win[((size_t)blockIdx.y * H + yy) * W1 + xi] = w;
                    }
                }
            }
        }
    }
}

// rtdm_debug_sgm_wide_paths: 0 = the library's choice, 1 = the one-wave form wherever it holds the line (D <= 1024), 4 = the
// four-wave form; either forces the wide pass for every D
static std::atomic<int> g_wide_mode{0};
void sgm_wide_set_mode(int m) { g_wide_mode.store(m == 1 || m == 4 ? m : 0, std::memory_order_relaxed); }
int sgm_wide_mode() { return g_wide_mode.load(std::memory_order_relaxed); }

// Prefetch depth per pair count: C and S of PF steps are in flight per lane (2 PF NP2 VGPRs); PF shrinks as the lane widens so
// that no instantiation spills (profiles/sgm_wide_vgpr_scratch.txt).
template <int NP2> struct WidePF { static constexpr int v = NP2 >= 8 ? 4 : (NP2 == 4 ? 6 : 8); };

template <int NP2, int NW>
static void launch_wide_t(const SGMGeom& g, const uint16_t* C, uint16_t* S, int dx, int dy, int P1, int P2, int first, bool last,
                          int lines, int n, SgmWin* win, int uniq, hipStream_t stream)
{
    constexpr int PF = WidePF<NP2>::v;
    const dim3 grid(NW == 1 ? (lines + 3) / 4 : lines, n);
    if (last) hipLaunchKernelGGL((k_sgm_wide<NP2, NW, PF, true>), grid, dim3(256), 0, stream, C, S, g, dx, dy, P1, P2, first, lines, win, uniq);
    else      hipLaunchKernelGGL((k_sgm_wide<NP2, NW, PF, false>), grid, dim3(256), 0, stream, C, S, g, dx, dy, P1, P2, first, lines, win, uniq);
}

void launch_sgm_wide(const SgmPass& p, const SgmCall& c)
{
    const SGMGeom& g = c.g;
    int np2 = 1;
    while (p.waves * 128 * np2 < g.D) np2 *= 2;                   // D <= 4080 < 4 * 128 * 8
    const int lines = sgm_line_count(g, p.dx, p.dy);
#define RTDM_WIDE(N, W) launch_wide_t<N, W>(g, c.b.C, c.b.S, p.dx, p.dy, c.P1, c.P2, p.first, p.last, lines, c.n, c.win, c.uniq, c.stream)
    if (p.waves == 1) {
        switch (np2) { case 1: RTDM_WIDE(1, 1); break; case 2: RTDM_WIDE(2, 1); break; case 4: RTDM_WIDE(4, 1); break; default: RTDM_WIDE(8, 1); break; }
    } else {
        switch (np2) { case 1: RTDM_WIDE(1, 4); break; case 2: RTDM_WIDE(2, 4); break; case 4: RTDM_WIDE(4, 4); break; default: RTDM_WIDE(8, 4); break; }
    }
#undef RTDM_WIDE
}

}  // namespace rtdm
