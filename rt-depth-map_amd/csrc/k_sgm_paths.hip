// k_sgm_paths.hip -- the path passes of the device StereoSGBM for lines of at most 256 disparities (k_sgm.hip: the schedule
// of passes; wider lines: k_sgm_wide.hip; oracle/sgm_oracle.c rules R4-R6).  A wavefront's lanes = consecutive disparities =
// one coalesced line of C and S per pixel.
//
//   k_sgm_path_h one HALF-WAVE per path line, packed u16 recurrence: L_r, S = min(S + L_r, 32767) (R5); the two horizontal
//                directions in one launch (-> S, <- S2)
//   k_sgm_sweep  the three directions that advance a row per step in one row-synchronous pass (adds S2; the last sweep decides
//                the winners: wave minimum, uniqueness, quadratic sub-pixel) -> 8 bytes per pixel
//   k_sgm_vert   MODE_HH4's two vertical directions, one pass each: a line per half-wave, neighbouring columns in neighbouring
//                half-waves, no LDS, no barrier, no wait on another workgroup (the upward pass decides the winners)
//   k_sgm_vert3  MODE_SGBM_3WAY's downward direction in four row stripes, k_sgm_vert's layout over (columns, frame, stripe);
//                always the last pass
#include "rtdm_sgm.h"

#include <cstdlib>
#include <mutex>

namespace rtdm {

// Half-wave form of the path pass (round 3, second half): one HALF-WAVE per path line, two neighbouring lines per wave, and
// the whole recurrence in packed 16-bit arithmetic.  A lane holds 2 * NP2 consecutive disparities as NP2 u16 pairs
// (D = 64 * NP2 fills the 32 lanes; a smaller D leaves the upper lanes dead), so
//   * a step is v_pk_min/add/sub_u16 on pairs -- L_r <= block cost + P2 <= 32767 (rtdm_sgm_create) and the "no neighbour"
//     value is 0xffff under a saturating + P1 --, d - 1 / d + 1 of a pair are two v_alignbit over (previous, own, next)
//     pair, the pairs at the lane's ends come from the neighbouring lanes by DPP wave shifts (replaced by 0xffff at the
//     half-wave's ends), and S is added as it was loaded: no unpacking, no packing;
//   * the line minimum is four DPP steps inside the rows of 16 and one v_permlane16_swap between the two rows of a half, for
//     both lines at once;
//   * the two lines of a wave are neighbours in memory for every direction but the horizontal ones (columns x and x + 1 of
//     one row: 2 * 2 D bytes in one piece), which halves the number of separate pieces the pass asks HBM for.
// LAST (the last direction of a frame): the aggregated costs min(S + L_r, 32767) of a pixel are complete the moment this
// wave has them in its lanes, so the winner-take-all step runs right here (sgm_wta_half) and S is neither written back nor
// read again.  What leaves is 8 bytes per pixel (SgmWin, rtdm_kernels.h) for k_sgm_lrfinal.
// (Tests: every D, both modes, against the oracle.)

// Winner-take-all on the finished pixels of a wave's two half-waves: wave minimum of S << 8 | d, uniqueness vote, S[d* +- 1],
// quadratic sub-pixel -- every quantity a per-half VECTOR value: both pixels are decided by the same instructions.  o = the aggregated
// costs of the lane's 2 * NP2 disparities d0 .. as u16 pairs.  Every lane of a half returns that half's record.
template <int NP2>
__device__ __forceinline__ SgmWin sgm_wta_half(const uint32_t* o, bool live, int lane, int d0, int D, int uniq, int minD)
{
    int v[2 * NP2];
    unsigned key = 0x7fffffffu;
#pragma unroll
    for (int r = 0; r < NP2; ++r) {
        v[2 * r] = (int)(o[r] & 0xffffu); v[2 * r + 1] = (int)(o[r] >> 16);
        key = min(key, ((unsigned)v[2 * r] << 8) | (unsigned)(d0 + 2 * r));
        key = min(key, ((unsigned)v[2 * r + 1] << 8) | (unsigned)(d0 + 2 * r + 1));
    }
    key = (unsigned)half_min_i32(live ? (int)key : 0x7fffffff);     // keys are < 2^24
    const int mins = (int)(key >> 8), bd = (int)(key & 0xffu);
    bool hit = false;
    const int lim = mins * 100;
#pragma unroll
    for (int j = 0; j < 2 * NP2; ++j) hit |= (unsigned)(d0 + j - bd + 1) > 2u && v[j] * (100 - uniq) < lim;
    const unsigned long long hits = __ballot(hit && live);
    // every aggregated cost saturated (R5) at 32767: the library's search for a cost BELOW its initial SHRT_MAX finds none, its
    // bestDisp stays -1 and what it writes is the invalid value -- no winner, no vote (reachable with a large P2 and 8 paths)
    const bool rejected = ((lane & 32) ? (uint32_t)(hits >> 32) : (uint32_t)hits) != 0u || mins >= 32767;
    // S[d* +- 1]: the pair that holds it, from the lane that holds it (ds_bpermute, no LDS memory involved)
    const int ip = min(bd + 1, D - 1), in = max(bd - 1, 0);
    constexpr int LG = NP2 == 1 ? 1 : (NP2 == 2 ? 2 : 3);         // log2 of the disparities per lane
    const int ap = ((lane & 32) + (ip >> LG)) << 2, an = ((lane & 32) + (in >> LG)) << 2;
    uint32_t wp = 0, wn = 0;
#pragma unroll
    for (int r = 0; r < NP2; ++r) {
        const uint32_t tp = (uint32_t)__builtin_amdgcn_ds_bpermute(ap, (int)o[r]);
        const uint32_t tn = (uint32_t)__builtin_amdgcn_ds_bpermute(an, (int)o[r]);
        if (((ip >> 1) & (NP2 - 1)) == r) wp = tp;
        if (((in >> 1) & (NP2 - 1)) == r) wn = tn;
    }
    const int s_p = (int)((wp >> ((ip & 1) << 4)) & 0xffffu), s_n = (int)((wn >> ((in & 1) << 4)) & 0xffffu);
    return sgm_win_record(bd, mins, s_p, s_n, rejected, D, minD);
}

template <int NP2, int PF, bool LAST>
__global__ __launch_bounds__(256) void k_sgm_path_h(const uint16_t* C, uint16_t* S, SGMGeom g, int dx_, int dy, int P1, int P2,
                                                    int first_dir, int nlines, SgmWin* win, int uniq, uint16_t* S2)
{
    // S2 != null (the two horizontal directions side by side, first_dir = 1): lines [0, nlines) run (dx, 0) and write S, lines
    // [nlines, 2 nlines) run (-dx, 0) and write S2 -- the first sweep adds the two up.  Same bytes moved as one pass after the
    // other (the second one's read of S against the sweep's read of S2), but twice the lines in flight: a single pair's 720 rows
    // are 360 waves on 1024 SIMDs, each a serial chain of W1 steps.
    const int lane = threadIdx.x & 63, hl = lane & 31, half = lane >> 5;
    const int line0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;
    const int nall = S2 ? 2 * nlines : nlines;
    if (line0 >= nall) return;                                    // whole waves only
    const int gline = min(line0 + half, nall - 1);
    const bool line_ok = line0 + half < nall;
    const bool second = gline >= nlines;                          // (only with S2)
    const int line = second ? gline - nlines : gline;
    const int dx = second ? -dx_ : dx_;
    const int D = g.D, W1 = g.W1, H = g.H;
    int sx, sy;
    const int nline = sgm_line_start(line, dx, dy, W1, H, sx, sy);
    const int nsteps = line_ok ? nline : 0;                       // of this half's line
    const int nmax = max(__builtin_amdgcn_readlane(nsteps, 0), __builtin_amdgcn_readlane(nsteps, 32));
    const int d0 = hl * 2 * NP2;
    const bool live = d0 < D;                                     // D is a multiple of 16 = of 2 * NP2
    const long stride = ((long)dy * W1 + dx) * D;
    const size_t off0 = (size_t)blockIdx.y * H * W1 * D + ((size_t)sy * W1 + sx) * D + (live ? d0 : 0);
    const uint16_t* cp = C + off0;
    uint16_t* sp = (second ? S2 : S) + off0;
    const uint32_t P1s = (uint32_t)P1 * 0x10001u, P2s = (uint32_t)P2 * 0x10001u;
    PackW<NP2> cr[PF], sr[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        if (k < nsteps) {
            cr[k] = ld_w<NP2>(cp + (long)k * stride);
            if (!first_dir) sr[k] = ld_w<NP2>(sp + (long)k * stride);
        }
    }
    uint32_t l[NP2], mps = 0;                                     // the previous pixel's L_r and its line minimum in both halves
#pragma unroll
    for (int r = 0; r < NP2; ++r) l[r] = 0xffffffffu;
    for (int base = 0; base < nmax; base += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int step = base + k;
            if (step >= nmax) break;
            const PackW<NP2> c = cr[k], sv = sr[k];
            if (step + PF < nsteps) {
                cr[k] = ld_w<NP2>(cp + (long)(step + PF) * stride);
                if (!first_dir) sr[k] = ld_w<NP2>(sp + (long)(step + PF) * stride);
            }
            sgm_line_step<NP2, true>(l, mps, l, mps, c.w, step == 0, live, hl, P1s, P2s);
            uint32_t o[NP2];
#pragma unroll
            for (int r = 0; r < NP2; ++r) o[r] = first_dir ? l[r] : pk_min_u(pk_add(sv.w[r], l[r]), 0x7fff7fffu);   // R5
            if constexpr (!LAST) {
                if (live && step < nsteps) st_w<NP2>(sp + (long)step * stride, o);
            } else {
                const SgmWin wv = sgm_wta_half<NP2>(o, live, lane, d0, D, uniq, g.minD);
                if (hl == 0 && step < nsteps) {
                    const int xi = sx + step * dx, yy = sy + step * dy;
                    win[((size_t)blockIdx.y * H + yy) * W1 + xi] = wv;
                }
            }
        }
    }
}

// Row-synchronous sweep (round 3): the three directions that advance one row per step -- (0, dy), (+1, dy), (-1, dy) -- in ONE
// pass, so C is read once and S read-modified-written once for the three of them (separate passes: three reads of C, three
// read-modify-writes of S; with the last sweep deciding the winners, S is not written at all).  A workgroup owns a strip of
// 8 * CPH columns of one frame and walks its rows; a half-wave owns CPH (4, 2 or 1) neighbouring columns and keeps the previous
// row's L_r of its 3 * CPH (column, direction) lines in registers.  A diagonal line changes column every row: inside a half-wave that is a
// register rename (the columns are processed in the order that makes the update in-place), between the half-waves of a
// workgroup the edge line goes through LDS (double-buffered, one barrier per row), and between neighbouring STRIPS through a
// small ring in global memory whose 64-bit words carry their own tag (epoch << 16 | row + 1 in the high half, the u16 pair in
// the low half: single-copy atomic, so a word that shows the expected tag is the expected data -- no fence, no L2 write-back).
// Every strip needs its neighbours' edge of the PREVIOUS row, which they publish at the start of that row: the strips of a
// frame advance in lockstep within a row of each other, and a wait is normally already satisfied.  All workgroups of the
// launch must be resident at once (grid <= what the device holds, one sweep at a time per process: launch_sweep); as a second
// line of defence a wait gives up after ~1 s, sets *abortf and the pass runs to its end without waiting (the host then
// reports the call as failed and the handle falls back to one pass per direction).
__device__ __forceinline__ unsigned long long ld_u64_relaxed(const unsigned long long* p)
{ return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_u64_relaxed(unsigned long long* p, unsigned long long v)
{ __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int NP2, bool LAST, int CPH, bool ADD2>
__global__ __launch_bounds__(256) void k_sgm_sweep(const uint16_t* C, uint16_t* S, SGMGeom g, int dy, int P1, int P2, int strips,
                                                   int items, unsigned long long* ring, int32_t* abortf, uint32_t epoch, SgmWin* win,
                                                   int uniq, int mute_strip, const uint16_t* S2)
{
    __shared__ uint32_t xch[2][8][2][NP2 + 1][32];             // [row parity][half-wave][0: (+1, dy) edge, 1: (-1, dy) edge][pairs, minimum][lane]
    const int lane = threadIdx.x & 63, hl = lane & 31, hw = threadIdx.x >> 5;
    const int D = g.D, W1 = g.W1, H = g.H;
    const int d0 = hl * 2 * NP2;
    const bool live = d0 < D;
    const uint32_t NONE = 0xffffffffu;
    const uint32_t P1s = (uint32_t)P1 * 0x10001u, P2s = (uint32_t)P2 * 0x10001u;
    const size_t rowstride = (size_t)W1 * D;                   // elements
    bool gave_up = false;                                      // (per lane; only the polling lanes ever set it)
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int f = item / strips, s = item - f * strips;
        const int xb = s * (8 * CPH) + hw * CPH;               // the half-wave's first column
        int xc[CPH]; bool okc[CPH];
#pragma unroll
        for (int c = 0; c < CPH; ++c) { okc[c] = xb + c < W1; xc[c] = min(xb + c, W1 - 1); }
        const size_t fbase = (size_t)f * H * rowstride + (live ? d0 : 0);
        const bool has_left = s > 0, has_right = (s + 1) * (8 * CPH) < W1;
        unsigned long long* ring_me = ring + (size_t)(f * strips + s) * 2 * SWEEP_RING * 32 * NP2;
        const unsigned long long* ring_l = ring_me - (size_t)2 * SWEEP_RING * 32 * NP2;                                  // strip s - 1, side 0
        const unsigned long long* ring_r = ring_me + (size_t)2 * SWEEP_RING * 32 * NP2 + (size_t)SWEEP_RING * 32 * NP2;  // strip s + 1, side 1
        uint32_t L0[CPH][NP2], L1[CPH][NP2], L2[CPH][NP2], m0[CPH], m1[CPH], m2[CPH];
#pragma unroll
        for (int c = 0; c < CPH; ++c) { m0[c] = m1[c] = m2[c] = 0; for (int r = 0; r < NP2; ++r) L0[c][r] = L1[c][r] = L2[c][r] = NONE; }
        // this row's and the next row's costs: C and S of the half-wave's four columns, requested a row ahead
        PackW<NP2> cn[CPH], sn[CPH], tn[ADD2 ? CPH : 1];                // (two rows ahead measured slower: 1.16 -> 1.25 ms per pair at 4 pairs per call)
        {
            const int y = dy > 0 ? 0 : H - 1;
#pragma unroll
            for (int c = 0; c < CPH; ++c) {
                cn[c] = ld_w<NP2>(C + fbase + (size_t)y * rowstride + (size_t)xc[c] * D);
                sn[c] = ld_w<NP2>(S + fbase + (size_t)y * rowstride + (size_t)xc[c] * D);
                if constexpr (ADD2) tn[c] = ld_w<NP2>(S2 + fbase + (size_t)y * rowstride + (size_t)xc[c] * D);   // the other horizontal direction's L_r (k_sgm_path_h)
            }
        }
        for (int t = 0; t < H; ++t) {
            const int y = dy > 0 ? t : H - 1 - t, par = t & 1;
            PackW<NP2> cc[CPH], sc[CPH];
#pragma unroll
            for (int c = 0; c < CPH; ++c) {
                cc[c] = cn[c]; sc[c] = sn[c];
                if constexpr (ADD2) { for (int r = 0; r < NP2; ++r) sc[c].w[r] = pk_min_u(pk_add(sc[c].w[r], tn[c].w[r]), 0x7fff7fffu); }   // R5
            }
            if (t + 1 < H) {
                const int yn = y + dy;
#pragma unroll
                for (int c = 0; c < CPH; ++c) {
                    cn[c] = ld_w<NP2>(C + fbase + (size_t)yn * rowstride + (size_t)xc[c] * D);
                    sn[c] = ld_w<NP2>(S + fbase + (size_t)yn * rowstride + (size_t)xc[c] * D);
                    if constexpr (ADD2) tn[c] = ld_w<NP2>(S2 + fbase + (size_t)yn * rowstride + (size_t)xc[c] * D);
                }
            }
            const bool first_row = t == 0;
            uint32_t acc[CPH][NP2];
            const auto add_to = [&](int c, const uint32_t* L) {
#pragma unroll
                for (int r = 0; r < NP2; ++r) acc[c][r] = pk_min_u(pk_add(acc[c][r], L[r]), 0x7fff7fffu);   // R5
            };
#pragma unroll
            for (int c = 0; c < CPH; ++c) for (int r = 0; r < NP2; ++r) acc[c][r] = sc[c].w[r];
            // the neighbouring strip's edge of the previous row was published a row ago: ask for it now, look at it after the
            // row's other lines (a load from the ring is a round trip to memory, ~1 us: as long as a whole row of a lone wave)
            const bool poll_l = hw == 0 && has_left && !first_row, poll_r = hw == 7 && has_right && !first_row;
            const unsigned long long* ring_src = (poll_l ? ring_l : ring_r) + ((size_t)((t - 1) & (SWEEP_RING - 1)) * 32 + hl) * NP2;
            unsigned long long w[NP2];
#pragma unroll
            for (int r = 0; r < NP2; ++r) w[r] = 0ull;
            if (poll_l || poll_r) {
#pragma unroll
                for (int r = 0; r < NP2; ++r) w[r] = ld_u64_relaxed(ring_src + r);
            }
            // (+1, dy): columns CPH - 1 ... 1 take the line of their left neighbour's previous row -- in place in that order
#pragma unroll
            for (int c = CPH - 1; c >= 1; --c) { sgm_line_step<NP2, true>(L1[c], m1[c], L1[c - 1], m1[c - 1], cc[c].w, first_row, live, hl, P1s, P2s); add_to(c, L1[c]); }
            // (-1, dy): columns 0 ... CPH - 2 take their right neighbour's; a line starts at the frame's last column
#pragma unroll
            for (int c = 0; c <= CPH - 2; ++c) { sgm_line_step<NP2, true>(L2[c], m2[c], L2[c + 1], m2[c + 1], cc[c].w, first_row || xb + c == W1 - 1, live, hl, P1s, P2s); add_to(c, L2[c]); }
            // the two lines that enter the half-wave's columns from outside: from the neighbouring half-wave (LDS, written in the
            // previous row) or, at the strip's ends, from the neighbouring strip (the ring)
            uint32_t inL[NP2], inR[NP2], inLm = 0, inRm = 0;
#pragma unroll
            for (int r = 0; r < NP2; ++r) { inL[r] = NONE; inR[r] = NONE; }
            if (!first_row) {
                if (hw > 0) { for (int r = 0; r < NP2; ++r) inL[r] = xch[par ^ 1][hw - 1][0][r][hl]; inLm = xch[par ^ 1][hw - 1][0][NP2][hl]; }
                if (hw < 7) { for (int r = 0; r < NP2; ++r) inR[r] = xch[par ^ 1][hw + 1][1][r][hl]; inRm = xch[par ^ 1][hw + 1][1][NP2][hl]; }
            }
            const int wv = threadIdx.x >> 6;
            const bool ring_l_wave = wv == 0 && has_left && !first_row, ring_r_wave = wv == 3 && has_right && !first_row;   // wave-uniform
            // the entering lines that do not come through the ring, now: what a strip hands to its neighbours (the (+1, dy) line of
            // its last column, the (-1, dy) line of its first) never depends on what it is still waiting for from them
            if (!ring_l_wave) { sgm_line_step<NP2, true>(L1[0], m1[0], inL, inLm, cc[0].w, first_row || xb == 0, live, hl, P1s, P2s); add_to(0, L1[0]); }
            if (!ring_r_wave) {
                sgm_line_step<NP2, true>(L2[CPH - 1], m2[CPH - 1], inR, inRm, cc[CPH - 1].w, first_row || xb + CPH - 1 >= W1 - 1, live, hl, P1s, P2s);
                add_to(CPH - 1, L2[CPH - 1]);
            }
            const unsigned long long tag = ((unsigned long long)((epoch << 16) | (uint32_t)(t + 1))) << 32;
            if (hw == 7 && has_right && s != mute_strip) {          // (mute_strip >= 0: the test of the give-up path -- that strip never publishes)
#pragma unroll
                for (int r = 0; r < NP2; ++r) st_u64_relaxed(ring_me + ((size_t)(t & (SWEEP_RING - 1)) * 32 + hl) * NP2 + r, tag | L1[CPH - 1][r]);
            }
            if (hw == 0 && has_left) {
#pragma unroll
                for (int r = 0; r < NP2; ++r)
                    st_u64_relaxed(ring_me + (size_t)SWEEP_RING * 32 * NP2 + ((size_t)(t & (SWEEP_RING - 1)) * 32 + hl) * NP2 + r, tag | L2[0][r]);
            }
            // (0, dy)
#pragma unroll
            for (int c = 0; c < CPH; ++c) { sgm_line_step<NP2, true>(L0[c], m0[c], L0[c], m0[c], cc[c].w, first_row, live, hl, P1s, P2s); add_to(c, L0[c]); }
            if (ring_l_wave || ring_r_wave) {
                const uint32_t want = (epoch << 16) | (uint32_t)t;                  // the previous row's tag
                bool done = !(poll_l || poll_r) || gave_up;
                for (int spin = 0;; ++spin) {
                    if (!done) {
                        bool all = true;
#pragma unroll
                        for (int r = 0; r < NP2; ++r) { if (spin) w[r] = ld_u64_relaxed(ring_src + r); all &= (uint32_t)(w[r] >> 32) == want; }
                        done = all;
                    }
                    if (__all(done)) break;
                    if ((spin & 63) == 63 && (spin > (1 << 20) || __hip_atomic_load(abortf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                        if (!done) { gave_up = true; __hip_atomic_store(abortf, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (poll_l) { for (int r = 0; r < NP2; ++r) inL[r] = (uint32_t)w[r]; }
                if (poll_r) { for (int r = 0; r < NP2; ++r) inR[r] = (uint32_t)w[r]; }
                // the minimum of a line that came through the ring is not sent along: take it here (both halves do, one needs it)
                uint32_t mmL = NONE, mmR = NONE;
#pragma unroll
                for (int r = 0; r < NP2; ++r) { mmL = pk_min_u(mmL, live ? inL[r] : NONE); mmR = pk_min_u(mmR, live ? inR[r] : NONE); }
                const uint32_t hmL = (uint32_t)half_min_i32((int)min(mmL & 0xffffu, mmL >> 16)) * 0x10001u;
                const uint32_t hmR = (uint32_t)half_min_i32((int)min(mmR & 0xffffu, mmR >> 16)) * 0x10001u;
                if (poll_l) inLm = hmL;
                if (poll_r) inRm = hmR;
                if (ring_l_wave) { sgm_line_step<NP2, true>(L1[0], m1[0], inL, inLm, cc[0].w, xb == 0, live, hl, P1s, P2s); add_to(0, L1[0]); }
                if (ring_r_wave) {
                    sgm_line_step<NP2, true>(L2[CPH - 1], m2[CPH - 1], inR, inRm, cc[CPH - 1].w, xb + CPH - 1 >= W1 - 1, live, hl, P1s, P2s);
                    add_to(CPH - 1, L2[CPH - 1]);
                }
            }
            // the edge lines for the neighbouring half-waves' next row (final only now when one of them came through the ring)
#pragma unroll
            for (int r = 0; r < NP2; ++r) { xch[par][hw][0][r][hl] = L1[CPH - 1][r]; xch[par][hw][1][r][hl] = L2[0][r]; }
            xch[par][hw][0][NP2][hl] = m1[CPH - 1]; xch[par][hw][1][NP2][hl] = m2[0];
            // S (or the winners)
#pragma unroll
            for (int c = 0; c < CPH; ++c) {
                if constexpr (!LAST) {
                    if (live && okc[c]) st_w<NP2>(S + fbase + (size_t)y * rowstride + (size_t)xc[c] * D, acc[c]);
                } else {
                    const SgmWin wv = sgm_wta_half<NP2>(acc[c], live, lane, d0, D, uniq, g.minD);
                    if (hl == 0 && okc[c]) win[((size_t)f * H + y) * W1 + xc[c]] = wv;
                }
            }
            __syncthreads();
        }
    }
}

// Column-parallel vertical pass (MODE_HH4, rule R4'): the direction (0, dy) alone.  A vertical line never changes column, so
// nothing crosses a half-wave: no LDS edge, no barrier, no ring, no wait on another workgroup in any form -- the grid may be of
// any size and run in any order.  One line per half-wave (k_sgm_path_h's layout, sgm_line_step's recurrence with the previous
// row's L_r in registers); neighbouring half-waves take neighbouring columns, so a workgroup's row step is one contiguous piece
// of C and of S (columns per workgroup = blockDim.x / 32).  A lone line is a serial chain of H steps: C and S (and S2) are
// requested PF rows ahead.  ADD2 (the downward pass after the side-by-side horizontal directions): S2, the (-1, 0) direction's
// L_r, is added as it is loaded.  LAST (the upward pass): the winners are decided in the lanes (sgm_wta_half), S is not written.
template <int NP2, bool LAST, bool ADD2, int PF>
__global__ __launch_bounds__(256) void k_sgm_vert(const uint16_t* C, uint16_t* S, const uint16_t* S2, SGMGeom g, int dy, int P1, int P2,
                                                  SgmWin* win, int uniq)
{
    const int lane = threadIdx.x & 63, hl = lane & 31;
    const int D = g.D, W1 = g.W1, H = g.H;
    const int col = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    if ((col & ~1) >= W1) return;                                 // whole waves only
    const bool ok = col < W1;                                     // (an odd W1's last wave: its second half repeats the last column)
    const int xc = min(col, W1 - 1), f = blockIdx.y;
    const int d0 = hl * 2 * NP2;
    const bool live = d0 < D;                                     // D is a multiple of 16 = of 2 * NP2
    const uint32_t P1s = (uint32_t)P1 * 0x10001u, P2s = (uint32_t)P2 * 0x10001u;
    const long stride = (long)dy * W1 * D;                        // one row, elements
    const size_t off0 = ((size_t)f * H + (dy > 0 ? 0 : H - 1)) * W1 * D + (size_t)xc * D + (live ? d0 : 0);
    const uint16_t* cp = C + off0;
    uint16_t* sp = S + off0;
    const uint16_t* tp = ADD2 ? S2 + off0 : nullptr;
    PackW<NP2> cr[PF], sr[PF], tr[ADD2 ? PF : 1];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        if (k < H) {
            cr[k] = ld_w<NP2>(cp + (long)k * stride);
            sr[k] = ld_w<NP2>(sp + (long)k * stride);
            if constexpr (ADD2) tr[k] = ld_w<NP2>(tp + (long)k * stride);
        }
    }
    uint32_t l[NP2], mps = 0;
#pragma unroll
    for (int r = 0; r < NP2; ++r) l[r] = 0xffffffffu;
    for (int base = 0; base < H; base += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int step = base + k;
            if (step >= H) break;
            const PackW<NP2> c = cr[k];
            uint32_t o[NP2];
#pragma unroll
            for (int r = 0; r < NP2; ++r) o[r] = sr[k].w[r];
            if constexpr (ADD2) {
#pragma unroll
                for (int r = 0; r < NP2; ++r) o[r] = pk_min_u(pk_add(o[r], tr[k].w[r]), 0x7fff7fffu);       // R5
            }
            if (step + PF < H) {
                cr[k] = ld_w<NP2>(cp + (long)(step + PF) * stride);
                sr[k] = ld_w<NP2>(sp + (long)(step + PF) * stride);
                if constexpr (ADD2) tr[k] = ld_w<NP2>(tp + (long)(step + PF) * stride);
            }
            sgm_line_step<NP2, true>(l, mps, l, mps, c.w, step == 0, live, hl, P1s, P2s);
#pragma unroll
            for (int r = 0; r < NP2; ++r) o[r] = pk_min_u(pk_add(o[r], l[r]), 0x7fff7fffu);                  // R5
            if constexpr (!LAST) {
                if (live && ok) st_w<NP2>(sp + (long)step * stride, o);
            } else {
                const SgmWin wv = sgm_wta_half<NP2>(o, live, lane, d0, D, uniq, g.minD);
                if (hl == 0 && ok) win[((size_t)f * H + (dy > 0 ? step : H - 1 - step)) * W1 + xc] = wv;
            }
        }
    }
}

// MODE_SGBM_3WAY's vertical direction (rules T1, T4-T6): (0, 1) in four row stripes, each a chain of its
// own that starts at the stripe's first source row a with L = C'(a).  k_sgm_vert's layout -- a line per half-wave, neighbouring
// columns in neighbouring half-waves, sgm_line_step, PF rows requested ahead -- over a grid of (columns, frame, stripe); like
// k_sgm_vert it has no LDS, no barrier and no wait on another workgroup in any form: the grid may be of any size and run in any
// order.  Rows [a, o) serve the recurrence only: their block cost alone is loaded, C' (Cw, k_sgm_warm3) for the first ncw rows of
// a stripe with a > 0 and C below them.  Rows [o, e) load C and S (ADD2: and S2, the other horizontal direction's L_r), form
// min(S + L, 32767) (T5) and decide the winner in the lanes (sgm_wta_half): this is always the last pass, S is never written.
template <int NP2, bool ADD2, int PF>
__global__ __launch_bounds__(256) void k_sgm_vert3(const uint16_t* C, const uint16_t* Cw, const uint16_t* S, const uint16_t* S2, SGMGeom g,
                                                   Sgm3Stripes st, int wrows, int P1, int P2, SgmWin* win, int uniq)
{
    const int lane = threadIdx.x & 63, hl = lane & 31;
    const int D = g.D, W1 = g.W1, H = g.H;
    const int col = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    if ((col & ~1) >= W1) return;                                 // whole waves only
    const bool ok = col < W1;                                     // (an odd W1's last wave: its second half repeats the last column)
    const int xc = min(col, W1 - 1), f = blockIdx.y, si = blockIdx.z;
    const Sgm3Stripe s = st.s[si];
    if (s.o >= s.e) return;                                       // an empty stripe
    const int a = s.a, nrows = s.e - a, nwarm = s.o - a;          // steps of the chain; those before the first output row
    const int ncw = a > 0 ? min(wrows, nrows) : 0;                // steps whose block cost is C' (T3; a = 0: C' = C)
    const int d0 = hl * 2 * NP2;
    const bool live = d0 < D;                                     // D is a multiple of 16 = of 2 * NP2
    const uint32_t P1s = (uint32_t)P1 * 0x10001u, P2s = (uint32_t)P2 * 0x10001u;
    const size_t stride = (size_t)W1 * D;                         // one row, elements
    const size_t loff = (size_t)xc * D + (live ? d0 : 0);
    const size_t off0 = ((size_t)f * H + a) * stride + loff;
    const uint16_t* cp = C + off0;
    const uint16_t* wp = ncw ? Cw + ((size_t)f * (SGM3_STRIPES - 1) + (si - 1)) * wrows * stride + loff : cp;   // (a > 0: si >= 1)
    const uint16_t* sp = S + off0;
    const uint16_t* tp = ADD2 ? S2 + off0 : nullptr;
    const auto ld_c = [&](int t) { return ld_w<NP2>((t < ncw ? wp : cp) + (size_t)t * stride); };
    PackW<NP2> cr[PF], sr[PF], tr[ADD2 ? PF : 1];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        sr[k] = PackW<NP2>{};                                     // (a warm-up row's S is never loaded and never used)
        if (ADD2 || k == 0) tr[ADD2 ? k : 0] = PackW<NP2>{};
        if (k < nrows) {
            cr[k] = ld_c(k);
            if (k >= nwarm) {
                sr[k] = ld_w<NP2>(sp + (size_t)k * stride);
                if constexpr (ADD2) tr[k] = ld_w<NP2>(tp + (size_t)k * stride);
            }
        }
    }
    uint32_t l[NP2], mps = 0;
#pragma unroll
    for (int r = 0; r < NP2; ++r) l[r] = 0xffffffffu;
    for (int base = 0; base < nrows; base += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int step = base + k;
            if (step >= nrows) break;
            const PackW<NP2> c = cr[k];
            uint32_t o[NP2];
#pragma unroll
            for (int r = 0; r < NP2; ++r) o[r] = sr[k].w[r];
            if constexpr (ADD2) {
#pragma unroll
                for (int r = 0; r < NP2; ++r) o[r] = pk_min_u(pk_add(o[r], tr[k].w[r]), 0x7fff7fffu);       // R5
            }
            if (step + PF < nrows) {
                cr[k] = ld_c(step + PF);
                if (step + PF >= nwarm) {
                    sr[k] = ld_w<NP2>(sp + (size_t)(step + PF) * stride);
                    if constexpr (ADD2) tr[k] = ld_w<NP2>(tp + (size_t)(step + PF) * stride);
                }
            }
            sgm_line_step<NP2, true>(l, mps, l, mps, c.w, step == 0, live, hl, P1s, P2s);
            if (step >= nwarm) {                                  // (grid-uniform per stripe: o is S only from here on)
#pragma unroll
                for (int r = 0; r < NP2; ++r) o[r] = pk_min_u(pk_add(o[r], l[r]), 0x7fff7fffu);              // T5
                const SgmWin wv = sgm_wta_half<NP2>(o, live, lane, d0, D, uniq, g.minD);
                if (hl == 0 && ok) win[((size_t)f * H + a + step) * W1 + xc] = wv;
            }
        }
    }
}

// S = min(S + S2, 32767) (R5), two elements per thread: only where the two horizontal directions ran side by side into S and S2
// and the sweep that was to add them up could not be launched after all
__global__ __launch_bounds__(256) void k_sgm_add_s2(uint32_t* S, const uint32_t* S2, size_t npairs)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npairs) S[i] = pk_min_u(pk_add(S[i], S2[i]), 0x7fff7fffu);
}

size_t sgm_ring_words(int maxW, int D, int max_batch)                  // sized for the narrowest strips (8 columns)
{ return (size_t)max_batch * ((size_t)(maxW + 7) / 8) * 2 * SWEEP_RING * 32 * sgm_np2(D); }

// The k_sgm_sweep instantiation of a form: the one table the capacities and the launch go through.  (ADD2, the instantiation
// that also adds S2 -- the first sweep after the side-by-side horizontal directions -- holds one more volume's row in
// registers: a template parameter, so that the other sweep keeps its occupancy.)
using SweepKernel = decltype(&k_sgm_sweep<1, false, 1, false>);
template <int NP2, bool LAST>
static SweepKernel sweep_kernel_t(int cols, bool add2)
{
    switch (cols * 2 + (add2 ? 1 : 0)) {
        case 2: return k_sgm_sweep<NP2, LAST, 1, false>;
        case 3: return k_sgm_sweep<NP2, LAST, 1, true>;
        case 4: return k_sgm_sweep<NP2, LAST, 2, false>;
        case 5: return k_sgm_sweep<NP2, LAST, 2, true>;
        case 8: return k_sgm_sweep<NP2, LAST, 4, false>;
        default: return k_sgm_sweep<NP2, LAST, 4, true>;
    }
}
static SweepKernel sweep_kernel(int np2, bool last, int cols, bool add2)
{
    switch (np2 * 2 + (last ? 1 : 0)) {
        case 2: return sweep_kernel_t<1, false>(cols, add2);
        case 3: return sweep_kernel_t<1, true>(cols, add2);
        case 4: return sweep_kernel_t<2, false>(cols, add2);
        case 5: return sweep_kernel_t<2, true>(cols, add2);
        case 8: return sweep_kernel_t<4, false>(cols, add2);
        default: return sweep_kernel_t<4, true>(cols, add2);
    }
}
static int sweep_capacity(SweepKernel k)
{
    int dev = 0, cus = 0, per_cu = 0, cap = -1;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 256, 0) == hipSuccess && per_cu > 0)
        cap = per_cu * cus;
    (void)hipGetLastError();
    return cap;
}
// The capacities of every sweep form a handle of this mode can launch, three column widths each: the down form (LAST in
// MODE_SGBM) without ADD2 and, where there is an S2, with it; MODE_HH's up form.  MODE_HH4 and wide lines: none (all 0).
void sgm_sweep_caps(int D, int paths, bool s2, int cap[2][3][2])
{
    for (int i = 0; i < 12; ++i) (&cap[0][0][0])[i] = 0;
    if (paths == 4 || paths == 3 || D > 256) return;              // (MODE_SGBM_3WAY runs no sweep either)
    for (int c = 0; c < 3; ++c) {
        for (int add2 = 0; add2 <= (s2 ? 1 : 0); ++add2) cap[paths == 5][c][add2] = sweep_capacity(sweep_kernel(sgm_np2(D), paths == 5, 1 << c, add2));
        if (paths == 8) cap[1][c][0] = sweep_capacity(sweep_kernel(sgm_np2(D), true, 1 << c, false));
    }
}
// The workgroups of a sweep wait for each other, so all of them must be resident at once: the grid is no larger than what the
// device holds (plan_sgm), and the sweeps of ONE PROCESS never run side by side -- they all go through one stream per device (two sweeps
// half resident each would wait for workgroups that cannot start).  The caller's stream and the sweep stream are tied
// together by the handle's two events; kernels of other streams may share the device with a sweep (they do not wait for it,
// so they finish and make room).  (hipLaunchCooperativeKernel would promise the residency, but a process that has used it
// from a thread other than its main one dies in the runtime's exit handlers on ROCm 7.2: tools/sgm_two_threads.py.)
struct SweepLane { std::mutex mu; hipStream_t s = nullptr; };
static SweepLane& sweep_lane(int dev) { static SweepLane lanes[64]; return lanes[dev & 63]; }

// One row-synchronous pass over (0, dy), (+1, dy), (-1, dy).
bool launch_sweep(const SgmPass& p, const SgmCall& c)
{
    const SGMBuffers& b = c.b;
    const uint32_t epoch = (*b.epoch + 1) & 0xffffu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return false; }
    SweepLane& lane = sweep_lane(dev);
    std::lock_guard<std::mutex> lk(lane.mu);
    if (!lane.s && hipStreamCreateWithFlags(&lane.s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); lane.s = nullptr; return false; }
    if (hipEventRecord((hipEvent_t)b.ev_in, c.stream) != hipSuccess || hipStreamWaitEvent(lane.s, (hipEvent_t)b.ev_in, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
    // RTDM_SGM_SWEEP_TEST_GIVEUP=1 (tests only): strip 0 never publishes its edge, so its neighbour's wait must run into its bound
    static const int mute = env_int("RTDM_SGM_SWEEP_TEST_GIVEUP", 0) ? 0 : -1;
    const SweepKernel kernel = sweep_kernel(sgm_np2(c.g.D), p.last, p.cols, p.s2);
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(256), 0, lane.s, b.C, b.S, c.g, p.dy, c.P1, c.P2, p.strips, p.items, b.ring, b.abortf,
                       epoch, c.win, c.uniq, mute, p.s2 ? (const uint16_t*)b.S2 : nullptr);
    // (from here on the caller's stream has to wait for the sweep stream whatever happens, or it would run ahead of it)
    (void)hipEventRecord((hipEvent_t)b.ev_out, lane.s);
    (void)hipStreamWaitEvent(c.stream, (hipEvent_t)b.ev_out, 0);
    ++*b.epoch;
    return true;
}

// One k_sgm_path_h launch: half-wave lines, packed arithmetic, eight lines per workgroup.  p.s2: the two horizontal
// directions side by side, (dx, 0) -> S and (-dx, 0) -> S2 (first).
void launch_path_h(const SgmPass& p, const SgmCall& c)
{
    const SGMGeom& g = c.g;
    uint16_t* S2 = p.s2 ? c.b.S2 : nullptr;
    const int lines = sgm_line_count(g, p.dx, p.dy), first = p.first;
    const dim3 hgrid(((S2 ? 2 : 1) * lines + 7) / 8, c.n), blk(256);
#define RTDM_PATHH(N) do { if (p.last) hipLaunchKernelGGL((k_sgm_path_h<N, 8, true>), hgrid, blk, 0, c.stream, c.b.C, c.b.S, g, p.dx, p.dy, c.P1, c.P2, first, lines, c.win, c.uniq, S2); \
                           else hipLaunchKernelGGL((k_sgm_path_h<N, 8, false>), hgrid, blk, 0, c.stream, c.b.C, c.b.S, g, p.dx, p.dy, c.P1, c.P2, first, lines, c.win, c.uniq, S2); } while (0)
    switch (sgm_np2(g.D)) { case 1: RTDM_PATHH(1); break; case 2: RTDM_PATHH(2); break; default: RTDM_PATHH(4); break; }
#undef RTDM_PATHH
}

// One k_sgm_vert launch over (0, dy).  p.last: the winners instead of S; p.s2 (never with last): S2 is added to S on the way.
void launch_vert(const SgmPass& p, const SgmCall& c)
{
    // columns per workgroup and rows of prefetch, by measurement (profiles/sgm_hh4_time.txt: 720p, D = 128, 1 / 4 / 16 pairs per
    // call): 2 columns -- one wave per workgroup, so that a lone pair's 576 waves spread over all compute units -- and 8 rows
    // (2 / 4 / 16 rows: 14 % / 6 % / 3 % slower at one pair per call; 4 or 8 columns: 2 % to 15 % slower there; all within 4 %
    // of each other at 16 pairs); D = 64 and D = 256 agree
    constexpr int cols = 2, PF = 8;
    const SGMGeom& g = c.g;
    const uint16_t* S2 = p.s2 ? c.b.S2 : nullptr;
    const dim3 vgrid((g.W1 + cols - 1) / cols, c.n), blk(32 * cols);
#define RTDM_VERT(N) do { if (p.last) hipLaunchKernelGGL((k_sgm_vert<N, true, false, PF>), vgrid, blk, 0, c.stream, c.b.C, c.b.S, S2, g, p.dy, c.P1, c.P2, c.win, c.uniq); \
                          else if (S2) hipLaunchKernelGGL((k_sgm_vert<N, false, true, PF>), vgrid, blk, 0, c.stream, c.b.C, c.b.S, S2, g, p.dy, c.P1, c.P2, c.win, c.uniq); \
                          else hipLaunchKernelGGL((k_sgm_vert<N, false, false, PF>), vgrid, blk, 0, c.stream, c.b.C, c.b.S, S2, g, p.dy, c.P1, c.P2, c.win, c.uniq); } while (0)
    switch (sgm_np2(g.D)) { case 1: RTDM_VERT(1); break; case 2: RTDM_VERT(2); break; default: RTDM_VERT(4); break; }
#undef RTDM_VERT
}

// One k_sgm_vert3 launch: MODE_SGBM_3WAY's striped (0, 1), always last.  p.s2: S2 is added to S on the way.  Columns per
// workgroup and rows of prefetch as launch_vert has them.
void launch_vert3(const SgmPass& p, const SgmCall& c)
{
    constexpr int cols = 2, PF = 8;
    const SGMGeom& g = c.g;
    const Sgm3Stripes st = sgm3_stripes(g.H, c.blockSize);
    const int wrows = sgm3_warm_rows(c.blockSize, g.H);
    const dim3 vgrid((g.W1 + cols - 1) / cols, c.n, SGM3_STRIPES), blk(32 * cols);
#define RTDM_VERT3(N) do { if (p.s2) hipLaunchKernelGGL((k_sgm_vert3<N, true, PF>), vgrid, blk, 0, c.stream, c.b.C, c.b.Cw, c.b.S, c.b.S2, g, st, wrows, c.P1, c.P2, c.win, c.uniq); \
                           else hipLaunchKernelGGL((k_sgm_vert3<N, false, PF>), vgrid, blk, 0, c.stream, c.b.C, c.b.Cw, c.b.S, c.b.S2, g, st, wrows, c.P1, c.P2, c.win, c.uniq); } while (0)
    switch (sgm_np2(g.D)) { case 1: RTDM_VERT3(1); break; case 2: RTDM_VERT3(2); break; default: RTDM_VERT3(4); break; }
#undef RTDM_VERT3
}

void launch_sgm_add_s2(const SgmCall& c)
{
    const size_t npairs = (size_t)c.n * c.g.H * c.g.W1 * c.g.D / 2;
    hipLaunchKernelGGL(k_sgm_add_s2, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, c.stream, (uint32_t*)c.b.S, (const uint32_t*)c.b.S2, npairs);
}

}  // namespace rtdm
