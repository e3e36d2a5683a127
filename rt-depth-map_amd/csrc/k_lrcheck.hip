// k_lrcheck.hip -- K3, the left-right check of the block matcher for gfx950, in three forms (scalar, eight columns per
// thread, packed) with the speckle filter's per-row init fused in, and the entry that launches the form plan_lrcheck
// (k_rows.hip) has chosen.  Semantics: SURVEY.md Appendix A.4; oracle: oracle/bm_oracle.c.
#include "rtdm_kernels.h"
#include "rtdm_device.h"
#include "rtdm_pk16.h"

namespace rtdm {

// ---------------------------------------------------------------------------------------------
// K3 left-right check (cv::validateDisparity): one workgroup per (valid
// row, frame).  LDS holds a snapshot of the row and one 64-bit key per column: (cost << 32 | x);
// ds_min_u64 reproduces pass 1 ("strictly smaller cost wins, first x wins ties").  Pass 2 reads the
// snapshot, so the in-place update cannot race.  Columns outside the valid rectangle are masked in
// the same pass.  With SPK the final row is handed straight to the speckle filter's init step.
// ---------------------------------------------------------------------------------------------
// KT = key type: 32-bit keys (cost << 16 | x) when the cost plane is 16-bit, else 64-bit (cost << 32 | x).
// One row per workgroup (the multi-row form, which merged the row pairs inside a block from head maps it kept in LDS, was
// measured and retired: DESIGN.md section 6).
template <bool SPK, typename CT, typename KT>
__global__ __launch_bounds__(256) void k_lrcheck(Plane16W disp, const CT* cost, BMGeom g, int maxDiff16,
                                                 int32_t* label, int32_t* size, uint32_t* runs, int32_t* rowcnt,
                                                 int16_t* headmap, int spkDiff)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int KSH = sizeof(KT) * 4;                               // bit position of the cost inside a key
    constexpr KT NONE = (KT)~(KT)0, XMASK = ((KT)1 << KSH) - 1;
    constexpr int KB = sizeof(KT) > 4 ? 8 : 4;
    const int W = g.W, INV = g.filtered;
    int* sc = (int*)smem;                                             // W ints: keys first, then scan scratch
    KT* key = (KT*)smem;                                              // (64-bit keys need 2W ints)
    int16_t* snap = (int16_t*)(smem + (size_t)W * KB);                // W
    int16_t* fin = snap + W;                                          // W: the final row (SPK only)
    __shared__ int wsum[4];
    const int nt = blockDim.x;
    const int f = blockIdx.z;
    const int y = g.vy0 + blockIdx.y;
    const int minX1 = max(g.minD + g.D, 0), maxX1 = W + min(g.minD, 0);
    int16_t* row = disp.base + (size_t)f * disp.frame_e + (size_t)y * disp.pitch_e;
    const CT* crow = cost + ((size_t)f * g.H + y) * g.Ws;
    for (int x = threadIdx.x; x < W; x += nt) { key[x] = NONE; snap[x] = row[x]; }
    __syncthreads();
    for (int x = minX1 + threadIdx.x; x < maxX1; x += nt) {
        const int d = snap[x];
        if (d == INV) continue;
        const int x2 = x - ((d + 8) >> 4);
        if (x2 < 0 || x2 >= W) continue;
        atomicMin(&key[x2], ((KT)(unsigned)crow[x] << KSH) | (KT)(unsigned)x);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += nt) {
        int d = snap[x];
        bool kill = (x < g.vx0 || x >= g.vx1);
        if (!kill && d != INV && x >= minX1 && x < maxX1) {
            const int x0 = x - (d >> 4), x1 = x - ((d + 15) >> 4);
            bool bad0 = false, bad1 = false;
            if (x0 >= 0 && x0 < W && key[x0] != NONE) bad0 = abs((int)snap[(unsigned)(key[x0] & XMASK)] - d) > maxDiff16;
            if (x1 >= 0 && x1 < W && key[x1] != NONE) bad1 = abs((int)snap[(unsigned)(key[x1] & XMASK)] - d) > maxDiff16;
            kill = bad0 && bad1;
        }
        if (kill && d != INV) { row[x] = (int16_t)INV; d = INV; }
        if (SPK) fin[x] = (int16_t)d;
    }
    if (!SPK) return;
    __syncthreads();
    // the keys are no longer needed: scan scratch
    spk_row_init(fin, sc, wsum, W, (f * g.H + y) * g.Ws, label, size, runs, rowcnt + (f * g.H + y), headmap, INV, spkDiff);
}

// ---------------------------------------------------------------------------------------------
// The tail of the speckle init fused into k_lrcheck_vec and k_lrcheck_pk (what spk_row_init does, on per-thread aggregates):
// every thread brings the run heads of its 8-column chunk as agg = OpHead element (heads << 16 | x of the last head + 1, or
// 0), the row's chunks lie in consecutive lanes of whole waves or of half-waves (HALF: two rows per workgroup).  In order:
// spk_agg_scan, a barrier of the caller's kind, spk_agg_carry, spk_register_runs.
// ---------------------------------------------------------------------------------------------
template <int CTRL, int RMASK>
__device__ __forceinline__ int spk_scan_step(int t) { return OpHead::f(t, __builtin_amdgcn_update_dpp(0, t, CTRL, RMASK, 0xf, false)); }

// Inclusive scan of agg over the (half-)wave with DPP row shifts / row broadcasts (a __shfl_up chain is six dependent
// LDS-crossbar round trips); lanes without a source get the identity 0.  The (half-)wave's total goes to *wtotal.
template <bool HALF>
__device__ __forceinline__ int spk_agg_scan(int agg, int hl, int* wtotal)
{
    int t = agg;
    t = spk_scan_step<0x111, 0xf>(t); t = spk_scan_step<0x112, 0xf>(t);             // row_shr:1,2
    t = spk_scan_step<0x114, 0xf>(t); t = spk_scan_step<0x118, 0xf>(t);             // row_shr:4,8
    t = spk_scan_step<0x142, 0xa>(t);                                               // row_bcast:15
    if constexpr (!HALF) t = spk_scan_step<0x143, 0xc>(t);                          // row_bcast:31 (whole waves only)
    if (hl == (HALF ? 31 : 63)) *wtotal = t;
    return t;
}

// What the row carries into this thread's chunk from the left, after the barrier behind spk_agg_scan: the scan of the lane
// before it and the totals of the wv (half-)waves before its own.
__device__ __forceinline__ int spk_agg_carry(int t, int hl, const int* wtotals, int wv)
{
    int run = __builtin_amdgcn_update_dpp(0, t, 0x138, 0xf, 0xf, false);            // wave_shr:1
    if (hl == 0) run = 0;
    for (int q = 0; q < wv; ++q) run = OpHead::f(run, wtotals[q]);
    return run;
}

// Registers the runs of one chunk of row `rowi` (= f * H + y): hm / lm = the chunk's run heads / run ends, run = spk_agg_carry.
// Head record of the chunk, one dword instead of eight head columns: (runs that start left of the chunk) | starts << 16
// | cand << 24 (cand: the contacts with the row above that k_lrcheck_vec<.., NIT > 1> has found, else 0).  The union-find node
// of a run is its INDEX in the row (dense: a row's labels, sizes and run list are a few contiguous lines instead of one
// touched sector per run head -- the count / apply passes and this kernel's own stores used to scatter over the whole
// plane): the pixel at bit k belongs to run cin + popcount(starts at or left of k), 1-based; the merge kernels rebuild the
// few nodes they need from that.
__device__ __forceinline__ void spk_register_runs(int run, unsigned hm, unsigned lm, unsigned cand, int x0, int chunk, int W, int Ws, int rowi,
                                                  int32_t* label, int32_t* size, uint32_t* runs, int32_t* rowcnt, int16_t* headmap)
{
    const int base = rowi * Ws;
    const int hin = (run & 0xffff) - 1, cin = run >> 16;             // head and run count carried in from the left
    ((uint32_t*)headmap)[(size_t)rowi * (Ws >> 3) + chunk] = (uint32_t)cin | (hm << 16) | (cand << 24);
    while (lm) {                                                      // one trip per run that ends in this chunk
        const int k = __builtin_ctz(lm);
        lm &= lm - 1;
        const unsigned hb = hm & ((2u << k) - 1u);                    // heads at or left of the end
        const int h = hb ? x0 + (31 - __builtin_clz(hb)) : hin;
        const int node = base + cin + __builtin_popcount(hb) - 1;     // (1-based index of this run in the row) - 1
        const int len = x0 + k - h + 1;
        label[node] = node;
        size[node] = len;
        runs[node] = (uint32_t)h | ((uint32_t)len << 16);
    }
    if (x0 + 8 >= W) rowcnt[rowi] = cin + __builtin_popcount(hm);
}

// Vector form of k_lrcheck<SPK, uint16_t, uint32_t> for 16-byte-aligned rows with W % 8 == 0: one thread owns
// 8 consecutive columns, so the row, its costs, the write-back and the head map each move as ONE 128-bit access
// per thread (the scalar kernel spends its time issuing 2-byte accesses), and the run scan works on one
// aggregate per thread instead of one LDS element per column.  Same results as the scalar kernel.
// TWO (round 3): two rows per workgroup, one per HALF-wave -- lanes 0..31 of every wave take 32 chunks of row y, lanes 32..63
// the same chunks of row y + 1.  A 1280-wide row is 160 chunks = five half-waves: five full waves per row pair instead of
// three waves of which one is half empty per row (17 % of the lanes idle in a VALU-saturated kernel), and half the
// barriers per row.  Scans stop at the half-wave boundary (no row_bcast:31 step), everything else is per thread.
// NIT > 1 (SPK and TWO only): the workgroup walks NIT row pairs, 2 NIT consecutive rows, and finds the speckle filter's
// vertical contacts on the way -- while a row and the row above it are both in LDS -- for every pair of rows inside the block:
// the chunk's head record gets 8 more bits, `cand`: bit k = "the pixel at column x0 + k touches the pixel above it, and that
// contact is not the continuation of the contact to its left" (one union per contact segment).  k_spk_merge_rec then reads
// the 4-byte records only (0.5 bytes per pixel; k_spk_merge_strip read the disparity plane again and was HBM bound at
// 0.75 ms per 1024 720p pairs) and k_spk_merge_strip<1> is left with the one pair in 2 NIT that crosses two blocks.
// A thread compares ITS row (registers) with the row above: the other half-wave's current row (upper half) or the upper
// half's row of the previous trip (lower half) -- one 16-byte LDS read; the partner lane's run starts come by v_permlane32_swap.
template <bool SPK, bool TWO, int NIT>
__global__ __launch_bounds__(512) void k_lrcheck_vec(Plane16W disp, const uint16_t* cost, BMGeom g, int maxDiff16,
                                                     int32_t* label, int32_t* size, uint32_t* runs, int32_t* rowcnt,
                                                     int16_t* headmap, int spkDiff)
{
    static_assert(NIT == 1 || (SPK && TWO), "merging walks row pairs");
    constexpr bool MERGE = NIT > 1;
    constexpr int NB = MERGE ? 2 : 1;                                 // buffers of the final rows
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int W = g.W, INV = g.filtered;
    const int Wp = (W + 7) & ~7;                                      // LDS rows hold whole 8-column chunks
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int half = TWO ? lane >> 5 : 0;                             // which of the workgroup's rows this lane works on
    const int hl = TWO ? lane & 31 : lane;                            // lane inside the (half-)wave
    const int chunk = TWO ? wv * 32 + hl : tid;
    // per row: Wp keys: cost << 16 | (d + 0x8000); key[W] stays "none", key[W+1] takes the votes nobody uses; then the row
    // after the check (SPK; NB of them)
    const size_t per_half = (size_t)Wp * 4 + 16 + (size_t)NB * Wp * 2;
    uint32_t* key = (uint32_t*)(smem + (size_t)half * per_half);
    int16_t* fin0 = (int16_t*)(key + Wp + 4);                         // NB x Wp
    // the other half's rows: the row above an upper-half row is the lower half's current row, the row above a lower-half
    // row is the upper half's row of the previous trip
    const int16_t* ofin0 = (const int16_t*)((uint32_t*)(smem + (size_t)(half ^ 1) * per_half) + Wp + 4);
    __shared__ int wsum[2][8];
    const int x0 = chunk * 8;
    const int f = blockIdx.z;
    const int minX1 = max(g.minD + g.D, 0), maxX1 = W + min(g.minD, 0);
    // per-thread column masks (bit k = column x0 + k): inside the image / allowed to vote / inside the valid rectangle
    const auto span = [&](int lo, int hi) -> unsigned {
        const int a = min(max(lo - x0, 0), 8), b = min(max(hi - x0, 0), 8);
        return b > a ? ((1u << b) - 1u) & ~((1u << a) - 1u) : 0u;
    };
    const unsigned inimg = span(0, W), votem = span(minX1, maxX1), keepm = span(g.vx0, g.vx1);
    if (chunk == 0) { key[Wp] = ~0u; key[Wp + 1] = ~0u; }            // (W == Wp: the two extra slots lie behind the chunks)
    uint32_t prev_mine = 0;                                           // MERGE: run starts | disparity mask << 8 of the previous trip's row
#pragma unroll 1
    for (int it = 0; it < NIT; ++it) {
        const int ypair = TWO ? 2 * ((int)blockIdx.y * NIT + it) : (int)blockIdx.y;   // first row of this trip, from vy0
        if (MERGE && g.vy0 + ypair >= g.vy1) break;                   // (uniform) the frame's rows end inside this block
        const int yu = g.vy0 + ypair + half;
        const bool active = x0 < W && yu < g.vy1;                     // (an odd row count leaves the last trip's second half idle)
        const int y = min(yu, g.vy1 - 1);
        const int cur = MERGE ? it & 1 : 0;
        int16_t* fin = fin0 + (size_t)cur * Wp;
        int16_t* row = disp.base + (size_t)f * disp.frame_e + (size_t)y * disp.pitch_e;
        const uint16_t* crow = cost + ((size_t)f * g.H + y) * g.Ws;
        Short8 d8, c8;
        unsigned im = 0;                                              // bit k: d8.v[k] is a disparity (not INV)
        if (active) {
            d8 = *(const Short8*)(row + x0);
            c8 = *(const Short8*)(crow + x0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!((inimg >> k) & 1)) d8.v[k] = (int16_t)INV;      // ragged last chunk: padding columns do not exist
                im |= (unsigned)(d8.v[k] != INV) << k;
            }
            const uint4 none = make_uint4(~0u, ~0u, ~0u, ~0u);
            ((uint4*)(key + x0))[0] = none; ((uint4*)(key + x0))[1] = none;
        }
        __syncthreads();
        // Votes and look-ups are straight-line code for all eight columns (per-column branches cost more in exec-mask
        // bookkeeping than the work they skip).  The key of a vote carries the voter's DISPARITY, not its column: among the
        // voters of one right column a smaller x means a smaller disparity (x - x2 is its rounded integer part), so the
        // minimum still prefers the lower cost and then the first voter, and a look-up has the winner's disparity without a
        // second read.  A column that may not vote, or whose target lies outside the row, votes into key[W+1]; a look-up
        // outside the row reads key[W], which nobody writes: "no vote".
        if (active) {
            const unsigned vm = im & votem;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int x = x0 + k, d = d8.v[k];
                const int x2 = x - ((d + 8) >> 4);
                const bool ok = ((vm >> k) & 1) && (unsigned)x2 < (unsigned)W;
                atomicMin(&key[ok ? x2 : W + 1], ((uint32_t)(uint16_t)c8.v[k] << 16) | ((uint32_t)(d + 0x8000) & 0xffffu));
            }
        }
        __syncthreads();
        if (active) {
            const unsigned chk = im & votem & keepm;                  // columns whose two matches are looked up
            unsigned kill = im & ~keepm;                              // outside the valid rectangle: always dropped
            // |d2 - d| > M  <=>  (unsigned)(d2 - d + M) > 2 M; unchecked columns are masked once, at the end
            const unsigned M2 = 2u * (unsigned)maxDiff16;
            const int dofs = maxDiff16 - 0x8000;
            unsigned bad0m = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int x = x0 + k, d = d8.v[k];
                const uint32_t q = key[min((unsigned)(x - (d >> 4)), (unsigned)W)];
                bad0m |= ((unsigned)(q != ~0u) & (unsigned)((unsigned)((int)(q & 0xffffu) - d + dofs) > M2)) << k;
            }
            bad0m &= chk;
            // a pixel dies only if BOTH matches disagree: the second look-ups are needed only where the first ones did
            // (consistent regions: by none of the wave's lanes)
            if (__builtin_amdgcn_ballot_w64(bad0m != 0) != 0) {
                unsigned bad1m = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int x = x0 + k, d = d8.v[k];
                    const uint32_t q = key[min((unsigned)(x - ((d + 15) >> 4)), (unsigned)W)];
                    bad1m |= ((unsigned)(q != ~0u) & (unsigned)((unsigned)((int)(q & 0xffffu) - d + dofs) > M2)) << k;
                }
                kill |= bad0m & bad1m;
            }
            if (kill) {
#pragma unroll
                for (int k = 0; k < 8; ++k) if ((kill >> k) & 1) d8.v[k] = (int16_t)INV;
                *(Short8*)(row + x0) = d8;
                im &= ~kill;
            }
            if (SPK) *(Short8*)(fin + x0) = d8;
        }
        if (!SPK) return;                                             // (NIT == 1)
        __syncthreads();
        // ---- speckle init of the finished row (what spk_row_init does, on per-thread aggregates) ----
        int left = INV, right = INV;
        if (active) { if (x0 > 0) left = fin[x0 - 1]; if (x0 + 8 < W) right = fin[x0 + 8]; }
        // cb bit k (k = 0..8): columns x0+k-1 and x0+k are connected (both disparities, close enough)
        unsigned cb = 0;
        if (active) {
            cb |= (unsigned)conn(left, d8.v[0], INV, spkDiff);
#pragma unroll
            for (int k = 1; k < 8; ++k) cb |= (unsigned)(abs((int)d8.v[k] - (int)d8.v[k - 1]) <= spkDiff) << k;
            cb &= (im & (im << 1)) | 1u;                              // bits 1..7 need both columns to be disparities
            cb |= (unsigned)conn(d8.v[7], right, INV, spkDiff) << 8;
        }
        const unsigned hm = im & ~cb & 0xffu;                         // run heads
        const unsigned lm = im & ~(cb >> 1) & 0xffu;                  // run ends
        // ---- contacts between this thread's row (B, registers) and the row above it (A, LDS) ----
        unsigned cand = 0;
        if constexpr (MERGE) {
            const uint32_t mine = active ? (hm | (im << 8)) : 0u;
            const uint32_t give = half ? prev_mine : mine;            // what the partner lane (same chunk, other half) wants to see
            const auto sw = __builtin_amdgcn_permlane32_swap(give, give, false, false);   // {lower lanes' value, upper lanes' value}, in every lane
            const uint32_t above = half ? sw[0] : sw[1];              // upper half: the lower half's row; lower half: the upper half's previous row
            prev_mine = mine;
            if (active && (half == 1 || it > 0)) {
                const int16_t* afin = ofin0 + (size_t)(half == 1 ? cur : cur ^ 1) * Wp;
                const Short8 a8 = *(const Short8*)(afin + x0);
                const unsigned startA = above & 0xffu, ima = (above >> 8) & 0xffu;
                unsigned cm = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) cm |= (unsigned)(abs((int)a8.v[k] - (int)d8.v[k]) <= spkDiff) << k;
                cm &= ima & im;
                // a contact repeats the union of the contact to its left iff neither pixel of the pair starts a run
                const unsigned leftc = (cm & 1u) && x0 > 0 ? (unsigned)conn(afin[x0 - 1], left, INV, spkDiff) : 0u;
                cand = cm & ~(((cm << 1) | leftc) & ~startA & ~hm);
            }
        }
        const int agg = hm ? ((__builtin_popcount(hm) << 16) | (x0 + (31 - __builtin_clz(hm)) + 1)) : 0;
        const int t = spk_agg_scan<TWO>(agg, hl, &wsum[half][wv]);
        __syncthreads();
        const int run = spk_agg_carry(t, hl, wsum[half], wv);
        if (!active) { if (MERGE) continue; else return; }
        spk_register_runs(run, hm, lm, cand, x0, chunk, W, g.Ws, f * g.H + y, label, size, runs, rowcnt, headmap);
    }
}

// ---------------------------------------------------------------------------------------------
// k_lrcheck_pk (round 3): k_lrcheck_vec<SPK, true, 1> with TWO COLUMNS PER INSTRUCTION.  k_lrcheck_vec unpacks its eight
// columns and spends ~73 VALU instructions per pixel on per-column arithmetic and on building bit masks out of compares
// (v_cmp + v_cndmask + v_or per column and test) -- it is VALU bound.  Here the row stays packed as it arrives (four dwords
// of two int16 columns): key-slot ADDRESSES are formed in packed u16 arithmetic (LDS byte addresses fit 16 bits), votes and
// look-ups take one v_perm / one shift per column to split them, the two-sided consistency test is a packed subtraction whose
// SIGN bits are the verdict, the kill is a v_bfi on the packed row, and only what the run scan needs as bit masks (the
// validity of the final row, the connected-to-the-left flags) is extracted -- eight flags at a time with two v_perm and two
// v_dot4_u32_u8.  Measured: 354 instead of 509 VALU instructions on the always-taken path, but packed ops and v_perm issue at
// 4.4 cycles where most of k_lrcheck_vec's v_and / v_or / v_add / v_sub issue at 2.6: 1.39 -> 1.32 ms per 1024 720p pairs,
// 0.527 -> 0.487 at 640x480.  Timing-only ablations (profiles/r03_lrcheck_ablation.txt): loading the two planes and
// resetting the keys alone takes 0.59 ms -- 3.8 GB at 6.4 TB/s, the HBM floor; the speckle init costs 0.25 ms, the votes 0.09.  Key slots: key[W] takes the votes nobody may see, key[W + 1] is never written
// ("no vote").  Needs: costs < 32768 (a slot's cost half is negative only in the empty slot), minD .. minD + D inside
// int16 / 16, the workgroup's LDS below 64 KB.  Same bytes as k_lrcheck_vec.
// ---------------------------------------------------------------------------------------------
template <bool SPK>
__global__ __launch_bounds__(512) void k_lrcheck_pk(Plane16W disp, const uint16_t* cost, BMGeom g, int maxDiff16,
                                                    int32_t* label, int32_t* size, uint32_t* runs, int32_t* rowcnt,
                                                    int16_t* headmap, int spkDiff)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int W = g.W, INV = g.filtered;
    const int Wp = (W + 7) & ~7;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int half = lane >> 5, hl = lane & 31;                       // half-wave = row of the pair (see k_lrcheck_vec<.., TWO>)
    const int chunk = wv * 32 + hl;
    const size_t per_half = (size_t)Wp * 4 + 16 + (size_t)Wp * 2;
    uint32_t* key = (uint32_t*)(smem + (size_t)half * per_half);      // Wp + 4 keys (two used behind the row)
    int16_t* fin = (int16_t*)(key + Wp + 4);                          // the row after the check (SPK)
    __shared__ int wsum[2][8];
    const int x0 = chunk * 8;
    const int f = blockIdx.z;
    const int minX1 = max(g.minD + g.D, 0), maxX1 = W + min(g.minD, 0);
    const uint32_t INVpk = (uint32_t)(INV & 0xffff) * 0x00010001u;
    // ---- thread constants ----
    const uint32_t KB = (uint32_t)(uintptr_t)(lr_lds_u32*)key * 0x00010001u;   // LDS byte address of key[0], in both halves
    const uint32_t TRASH = (uint32_t)W * 0x00010001u, NONE = TRASH + 0x00010001u;   // slot indices
    uint32_t X[4], VOTEM[4], KEEPM[4];                                // the columns; halves masks (0xffff / 0)
    const auto in_range = [](int x, int lo, int hi) -> uint32_t { return (x >= lo && x < hi) ? 0xffffu : 0u; };
    // lo <= x < hi  <=>  (u16)(x - lo) < hi - lo  <=>  (hi - lo) -sat (u16)(x - lo) != 0: four packed instructions per pair of
    // columns (as scalar compares and selects the masks were a third of the kernel's prologue -- which a thread pays per row)
    const uint32_t vlo = (uint32_t)(minX1 & 0xffff) * 0x00010001u, vhl = (uint32_t)max(maxX1 - minX1, 0) * 0x00010001u;
    const uint32_t klo = (uint32_t)(g.vx0 & 0xffff) * 0x00010001u, khl = (uint32_t)max(g.vx1 - g.vx0, 0) * 0x00010001u;
    const uint32_t X0 = (uint32_t)x0 * 0x00010001u + 0x00010000u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        X[k] = X0 + (uint32_t)k * 0x00020002u;
        VOTEM[k] = pk_sub(pk_is_zero(pk_subsat_u(vhl, pk_sub(X[k], vlo))), 0x00010001u);
        KEEPM[k] = pk_sub(pk_is_zero(pk_subsat_u(khl, pk_sub(X[k], klo))), 0x00010001u);
    }
    // slot index (a negative one wraps to a large u16) -> LDS byte address, anything outside the row -> the slot `lim`
    const auto slot_addr = [&](uint32_t idx, uint32_t lim) -> uint32_t { return pk_add(pk_shl<2>(pk_min_u(idx, lim)), KB); };
    const uint32_t Mpk = (uint32_t)maxDiff16 * 0x00010001u;
    const uint32_t Spk = (uint32_t)spkDiff * 0x00010001u, S2pk = Spk + Spk;
    if (chunk == 0) { key[Wp] = ~0u; key[Wp + 1] = ~0u; }            // (W == Wp: the two slots lie behind the chunks)
    // One trip.  The loop statement is what is left of the retired form that walked several row pairs.  It stays: as straight-line
    // code the same body compiles to 45 VGPRs / 838 instructions instead of 46 / 830, with two s_waitcnt vmcnt(0) behind the row's
    // write-back -- the wait lr_lds_barrier() exists to avoid -- and the stage is 1.8 % slower (profiles/basic_split_resources.txt,
    // profiles/rows_plan_resources.txt).
#pragma unroll 1
    for (int it = 0; it < 1; ++it) {
        const int ypair = 2 * (int)blockIdx.y;                        // first row of the pair, from vy0
        const int y0 = g.vy0 + ypair, y = y0 + half;                  // (row addresses: wave-uniform part + the half's row step)
        const bool active = x0 < W && y < g.vy1;
        int16_t* row = disp.base + ((size_t)f * disp.frame_e + (size_t)y0 * disp.pitch_e) + (half ? (uint32_t)disp.pitch_e : 0u);
        [[maybe_unused]] const uint16_t* crow = cost + ((size_t)f * g.H + y0) * g.Ws + (half ? (uint32_t)g.Ws : 0u);
        uint32_t D[4] = {INVpk, INVpk, INVpk, INVpk}, C[4] = {0, 0, 0, 0};
        if (active) {
            const uint4 dq = *(const uint4*)(row + x0), cq = *(const uint4*)(crow + x0);
            D[0] = dq.x; D[1] = dq.y; D[2] = dq.z; D[3] = dq.w; C[0] = cq.x; C[1] = cq.y; C[2] = cq.z; C[3] = cq.w;
            if (x0 + 8 > W) {                                         // ragged last chunk: padding columns do not exist
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t m = in_range(x0 + 2 * k, 0, W) | (in_range(x0 + 2 * k + 1, 0, W) << 16);
                    D[k] = lr_bfi(m, D[k], INVpk);
                }
            }
            const uint4 none = make_uint4(~0u, ~0u, ~0u, ~0u);
            ((uint4*)(key + x0))[0] = none; ((uint4*)(key + x0))[1] = none;
        }
        lr_lds_barrier();
        uint32_t V[4], Dx[4];                                        // halves: is a disparity (0xffff / 0); d + 0x8000
        if (active) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                V[k] = pk_sub(pk_is_zero(D[k] ^ INVpk), 0x00010001u);
                Dx[k] = D[k] ^ 0x80008000u;
                // vote into the slot of x2 = x - ((d + 8) >> 4) with the key cost << 16 | d + 0x8000 (see k_lrcheck_vec).  A column
                // that may not vote votes with the cost 0xffff: such a key only ever replaces the empty slot's, and reads as empty
                // (negative cost half) -- no address select; targets outside the row (none inside the vote range) go to key[W]
                const uint32_t cv = C[k] | ~(V[k] & VOTEM[k]);
                const uint32_t a = slot_addr(pk_sub(X[k], pk_ashr<4>(pk_add(D[k], 0x00080008u))), TRASH);
                lr_lds_min(a & 0xffffu, __builtin_amdgcn_perm(cv, Dx[k], 0x05040100u));
                lr_lds_min(a >> 16, __builtin_amdgcn_perm(cv, Dx[k], 0x07060302u));
            }
        }
        lr_lds_barrier();
        if (active) {
            // look-up at x - (d >> 4) (and, where that disagrees, at x - ((d + 15) >> 4)): the slot's voter disagrees iff
            // |its d - d| > M: the sign of M - |difference|; an empty slot (cost half 0xffff: negative) never disagrees
            uint32_t bad0[4], any0 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t a = slot_addr(pk_sub(X[k], pk_ashr<4>(D[k])), NONE);
                const uint32_t qe = lr_lds_ld(a & 0xffffu), qo = lr_lds_ld(a >> 16);
                const uint32_t df = pk_sub(__builtin_amdgcn_perm(qo, qe, 0x05040100u), Dx[k]);
                const uint32_t r = pk_sub(Mpk, pk_max_i(df, pk_sub(0u, df)));
                bad0[k] = r & ~__builtin_amdgcn_perm(qo, qe, 0x07060302u) & V[k] & VOTEM[k] & KEEPM[k];
                any0 |= bad0[k];
            }
            uint32_t Dn[4] = {D[0], D[1], D[2], D[3]};
            if (__builtin_amdgcn_ballot_w64((any0 & 0x80008000u) != 0) != 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t a = slot_addr(pk_sub(X[k], pk_ashr<4>(pk_add(D[k], 0x000f000fu))), NONE);
                    const uint32_t qe = lr_lds_ld(a & 0xffffu), qo = lr_lds_ld(a >> 16);
                    const uint32_t df = pk_sub(__builtin_amdgcn_perm(qo, qe, 0x05040100u), Dx[k]);
                    const uint32_t r = pk_sub(Mpk, pk_max_i(df, pk_sub(0u, df)));
                    const uint32_t killed = pk_ashr<15>(bad0[k] & r & ~__builtin_amdgcn_perm(qo, qe, 0x07060302u));   // 0xffff where both disagree
                    Dn[k] = lr_bfi(killed, INVpk, D[k]);
                }
            }
            uint32_t chg = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                Dn[k] = lr_bfi(KEEPM[k], Dn[k], INVpk);               // outside the valid rectangle: always dropped
                chg |= Dn[k] ^ D[k];
                D[k] = Dn[k];
            }
            if (chg) *(uint4*)(row + x0) = make_uint4(D[0], D[1], D[2], D[3]);
            if (SPK) *(uint4*)(fin + x0) = make_uint4(D[0], D[1], D[2], D[3]);
        }
        if (!SPK) return;
        lr_lds_barrier();
        // ---- speckle init of the finished row (as in k_lrcheck_vec) ----
        unsigned im = 0, cb = 0;
        if (active) {
            const int left = x0 > 0 ? (int)fin[x0 - 1] : INV, right = x0 + 8 < W ? (int)fin[x0 + 8] : INV;
            uint32_t iz[4], cl[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                iz[k] = pk_is_zero(D[k] ^ INVpk);                     // 1 = NOT a disparity
                // columns (2k - 1, 2k) and (2k, 2k + 1): |a - b| <= S  <=>  (u16)(a - b + S) <= 2 S
                const uint32_t prev = __builtin_amdgcn_alignbit(D[k], k ? D[k - 1] : ((uint32_t)left << 16), 16);
                cl[k] = pk_is_zero(pk_subsat_u(pk_add(pk_sub(D[k], prev), Spk), S2pk));   // 1 = close
            }
            im = ~lr_bits8(iz) & 0xffu;
            // cb bit k (k = 0..8): columns x0+k-1 and x0+k are connected (both disparities, close enough)
            cb = lr_bits8(cl) & (im & ((im << 1) | (unsigned)(left != INV)));
            cb |= (unsigned)conn((int)(int16_t)(D[3] >> 16), right, INV, spkDiff) << 8;
        }
        const unsigned hm = im & ~cb & 0xffu;                         // run heads
        const unsigned lm = im & ~(cb >> 1) & 0xffu;                  // run ends
        const int agg = hm ? ((__builtin_popcount(hm) << 16) | (x0 + (31 - __builtin_clz(hm)) + 1)) : 0;
        const int t = spk_agg_scan<true>(agg, hl, &wsum[half][wv]);
        lr_lds_barrier();
        const int run = spk_agg_carry(t, hl, wsum[half], wv);
        if (active) spk_register_runs(run, hm, lm, 0u, x0, chunk, W, g.Ws, f * g.H + y, label, size, runs, rowcnt, headmap);
    }
}

// The plan's form -> its kernel; SPK: the speckle init runs in the same pass (plan.heads != NONE).
template <bool SPK>
static void lr_issue(const LrPlan& p, Plane16W disp, const void* cost, const BMGeom& g, const SpkBuffers& wk, hipStream_t stream)
{
    const auto go = [&](auto kernel, auto* c) {
        hipLaunchKernelGGL(kernel, dim3(1, p.gy, p.n), dim3(p.threads), p.lds, stream, disp, c, g, p.maxDiff16, wk.label, wk.size,
                           wk.runs, wk.rowcnt, wk.headmap, p.spkDiff);
    };
    const uint16_t* c16 = (const uint16_t*)cost;
    switch (p.form) {
        case LrForm::SCALAR_U16: go(k_lrcheck<SPK, uint16_t, uint32_t>, c16); break;
        case LrForm::SCALAR_I32: go(k_lrcheck<SPK, int32_t, unsigned long long>, (const int32_t*)cost); break;
        case LrForm::VEC_WAVE:   go(k_lrcheck_vec<SPK, false, 1>, c16); break;
        case LrForm::VEC_HALF:   go(k_lrcheck_vec<SPK, true, 1>, c16); break;
        case LrForm::VEC_HALF2:  go(k_lrcheck_vec<true, true, 2>, c16); break;   // (planned with the speckle init only)
        case LrForm::PACKED:     go(k_lrcheck_pk<SPK>, c16); break;
    }
}

void launch_lrcheck(const LrPlan& plan, Plane16W disp, const void* cost, const BMGeom& g, const SpkBuffers& wk, hipStream_t stream)
{
    if (plan.heads != SpkHeads::NONE) lr_issue<true>(plan, disp, cost, g, wk, stream);
    else lr_issue<false>(plan, disp, cost, g, wk, stream);
}

}  // namespace rtdm
