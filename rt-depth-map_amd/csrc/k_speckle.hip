// k_speckle.hip -- K4, the speckle filter of the block matcher for gfx950: init, the merge kernels, count, apply and the entry
// that launches what plan_speckle (k_rows.hip) has chosen.  Semantics: SURVEY.md Appendix A.5; oracle: oracle/bm_oracle.c.
#include "rtdm_kernels.h"
#include "rtdm_device.h"
#include "rtdm_pk16.h"

namespace rtdm {

// ---------------------------------------------------------------------------------------------
// K4 speckle filter (cv::filterSpeckles as called by cv::StereoBM::compute, SURVEY.md Appendix
// A.5): 4-connected components of pixels != newVal under |a-b| <= maxDiff; components with
// size <= maxSize become newVal.  Run-based union-find:
//   init   (fused into k_lrcheck, or k_spk_init when the left-right check is off) per row: a
//          max-scan turns the "connected to my left neighbour" flags into run heads; every pixel of
//          a horizontal run is represented by its head, which starts as its own parent and carries
//          the run length; the row's runs are also listed compactly (x | len << 16).
//   merge  one workgroup per block of rows: ONE union per vertical contact segment between two
//          runs (a pixel is skipped when its left neighbour already linked the same two runs).
//   count  one wave per row, lanes over its runs: every non-root head adds its run length to its
//          root (skipped once the root is known to be large: only "<= maxSize" matters).
//   apply  one wave per row, lanes over its runs: a run whose root is small is overwritten.
// Parent pointers only ever move to smaller indices of the same component and every hook is a
// device-scope atomicMin on a root, so stale reads are still ancestors and the set of small
// components is independent of scheduling.  Components never span frames.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_spk_init(Plane16W disp, int32_t* label, int32_t* size, uint32_t* runs,
                                                  int32_t* rowcnt, int16_t* headmap, int W, int Ws, int H, int newVal, int maxDiff)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* sc = (int*)smem;                 // W
    int16_t* d = (int16_t*)(sc + W);      // W
    __shared__ int wsum[4];
    const int y = blockIdx.y, f = blockIdx.z;
    const int16_t* row = disp.base + (size_t)f * disp.frame_e + (size_t)y * disp.pitch_e;
    for (int x = threadIdx.x; x < W; x += 256) d[x] = row[x];
    __syncthreads();
    spk_row_init(d, sc, wsum, W, (f * H + y) * Ws, label, size, runs, rowcnt + (f * H + y), headmap, newVal, maxDiff);
}

// merge: one thread = 8 consecutive pixels of a row pair (y, y+1); no LDS, no scans: the heads come
// from the head map.  A pixel is skipped when its left neighbour already linked the same two runs.
// For rows that are not 16-byte aligned (aligned rows go to k_spk_merge_strip); reached only without compact heads, where
// no pair was merged before: the pairs are consecutive.
__global__ __launch_bounds__(256) void k_spk_merge(Plane16W disp, int32_t* label, const int16_t* headmap, int W, int Ws, int H,
                                                   int y_lo, int npairs, int newVal, int maxDiff)
{
    // pairs (y, y+1) for y = y_lo + k, k < npairs.  The kernel is bound by the number of load instructions
    // (a 2-byte-per-lane load costs the address unit as much as a 16-byte one), so the left-neighbour state comes
    // from lane-1's registers; only lane 0 of a wave fetches it from memory.
    const int nxb = (W + 7) / 8;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const bool inb = idx < nxb * npairs;
    const int cidx = inb ? idx : 0;
    const int y = y_lo + cidx / nxb, x0 = (cidx % nxb) * 8;
    const int f = blockIdx.y;
    const int16_t* d0 = disp.base + (size_t)f * disp.frame_e + (size_t)y * disp.pitch_e;
    const int16_t* d1 = d0 + disp.pitch_e;
    const int base0 = (f * H + y) * Ws, base1 = base0 + Ws;
    const int16_t* h0 = headmap + base0;
    const int16_t* h1 = headmap + base1;
    Short8 a8, b8, ha8, hb8;
    unsigned cm = 0;
    if (inb) {
        for (int k = 0; k < 8; ++k) { const int x = min(x0 + k, W - 1); a8.v[k] = d0[x]; b8.v[k] = d1[x]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) cm |= (unsigned)((x0 + k < W) && conn(a8.v[k], b8.v[k], newVal, maxDiff)) << k;
    }
    ha8.v[7] = hb8.v[7] = 0;
    if (cm) {
        for (int k = 0; k < 8; ++k) { const int x = min(x0 + k, W - 1); ha8.v[k] = h0[x]; hb8.v[k] = h1[x]; }
    }
    // state of the pixel left of x0: lane-1 holds it in element 7 (same row whenever x0 > 0)
    const int packed = (int)(cm >> 7) | ((int)(uint16_t)ha8.v[7] << 1) | ((int)(uint16_t)hb8.v[7] << 17);
    const int fromLeft = __shfl_up(packed, 1);
    if (!cm) return;
    bool pc = false;
    int ph0 = -1, ph1 = -1;
    if (x0 > 0) {
        if ((threadIdx.x & 63) != 0) {
            pc = fromLeft & 1; ph0 = (fromLeft >> 1) & 0xffff; ph1 = (fromLeft >> 17) & 0x7fff;
        } else {
            pc = conn(d0[x0 - 1], d1[x0 - 1], newVal, maxDiff);
            if (pc) { ph0 = h0[x0 - 1]; ph1 = h1[x0 - 1]; }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool c = (cm >> k) & 1;
        const int ha = ha8.v[k], hb = hb8.v[k];
        if (c && !(pc && ph0 == ha && ph1 == hb)) uf_union(label, base0 + ha, base1 + hb);
        pc = c; ph0 = ha; ph1 = hb;
    }
}

// The contact queue of the merge kernels: the contacts found by a workgroup's 256 threads are queued in LDS and united
// afterwards by the first threads, one union per lane: a union is a chain of dependent global accesses, and a wave with a
// single busy lane stalls as long as a full one.  A contact that finds the queue full is united at once.
constexpr int SPK_QCAP = 1024;
__device__ __forceinline__ void spk_queue_push(int2* queue, int& qn, int32_t* label, int a, int b)
{
    const int slot = atomicAdd(&qn, 1);
    if (slot < SPK_QCAP) queue[slot] = make_int2(a, b);
    else uf_union(label, a, b);
}
// whole workgroup, behind its last push
__device__ __forceinline__ void spk_queue_drain(const int2* queue, const int& qn, int32_t* label, int32_t* size, int maxSize)
{
    __syncthreads();
    const int total = min(qn, SPK_QCAP);
    for (int i = threadIdx.x; i < total; i += 256) uf_union_contact(label, size, queue[i].x, queue[i].y, maxSize);
}

// The contacts k_lrcheck_vec<.., NIT > 1> has found (MergeRecArgs, rtdm_kernels.h).
// Item idx = one chunk of a row y of frame f: all it reads is the row's head records -- most have cand == 0 -- and, for the
// others, the record of the chunk above; every contact goes to the queue.
__device__ __forceinline__ void spk_rec_collect(int2* queue, int& qn, int32_t* label, const uint32_t* heads, int Ws, int H,
                                                const MergeRecArgs& ra, int idx, int f)
{
    // rows r = 1 .. nrows-1 from vy0 with r % blk != 0, numbered densely: j -> r = j + j / (blk - 1) + 1
    const int inblk = ra.blk - 1, npairs = (ra.nrows / ra.blk) * inblk + max(ra.nrows % ra.blk - 1, 0);
    if (idx >= npairs * ra.nch) return;
    const int j = idx / ra.nch, chunk = idx - j * ra.nch;
    const int y = ra.vy0 + j + j / inblk + 1;
    const size_t rrow = (size_t)(f * H + y) * (Ws >> 3);
    const uint32_t cb = heads[rrow + chunk];
    unsigned cand = cb >> 24;
    if (!cand) return;
    const uint32_t ca = heads[rrow - (Ws >> 3) + chunk];
    const unsigned startA = (ca >> 16) & 0xffu, startB = (cb >> 16) & 0xffu;
    const int base = (f * H + y) * Ws;
    while (cand) {
        const int k = __builtin_ctz(cand);
        cand &= cand - 1;
        const unsigned msk = (2u << k) - 1u;
        const int na = base - Ws + (int)(ca & 0xffffu) + __builtin_popcount(startA & msk) - 1;
        const int nb = base + (int)(cb & 0xffffu) + __builtin_popcount(startB & msk) - 1;
        spk_queue_push(queue, qn, label, na, nb);
    }
}

// The unions for those contacts as a launch of its own (k_spk_merge_strip<.., REC> carries them in its grid).
__global__ __launch_bounds__(256) void k_spk_merge_rec(int32_t* label, const uint32_t* heads, int Ws, int H, MergeRecArgs ra,
                                                       int32_t* size, int maxSize)
{
    __shared__ int2 queue[SPK_QCAP];
    __shared__ int qn;
    if (threadIdx.x == 0) qn = 0;
    __syncthreads();
    spk_rec_collect(queue, qn, label, heads, Ws, H, ra, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
    spk_queue_drain(queue, qn, label, size, maxSize);
}

// Strip form of the merge for aligned rows: one thread walks RS consecutive row pairs of its 8 columns, so every
// row of disparities / heads is loaded once instead of twice (as the lower row of one pair and the upper row of the
// next).  Same unions as k_spk_merge.
// size / maxSize: a contact between two runs that are EACH longer than maxSize needs no union -- both components are
// "large" whatever else they touch, and only "size <= maxSize" is ever asked (exact; it removes most unions: disparity
// maps are made of long runs).  size[] still holds the run lengths here (k_spk_count runs afterwards).
// COMPACT: the heads come as one record per 8-column chunk and row (k_lrcheck_vec: carried head + 1 | run starts << 16)
// instead of one int16 per pixel: a quarter of the head bytes, and "same two runs as the pixel to the left" becomes bit
// arithmetic (neither pixel of the pair starts a run).
// COMPACT forms settle most (chunk, row pair) items from the head records and one entry of the row's run list (`runs`)
// and read the disparity rows only for the others -- see "SETTLED PAIRS" in the kernel: 3.06 -> 1.43 MB per 720p pair.
// RS == 1: the pairs are (y, y + 1) for y = y_lo + k * ystep -- what is left when k_lrcheck_vec has merged the pairs inside
// blocks of ystep rows itself.
// REC: the first ra.blocks workgroups do k_spk_merge_rec's work instead (the contacts k_lrcheck_vec<.., NIT > 1> left in the head
// records: spk_rec_collect) -- same queue, same drain, one launch less for a single frame.
// Packed forms of the contact test (helpers of k_lrcheck_pk): bit k = column k of the chunk.
__device__ __forceinline__ unsigned spk_invalid_pk(const Short8& r, uint32_t INVpk)          // the column holds newVal
{
    const uint4 q = __builtin_bit_cast(uint4, r);
    const uint32_t z[4] = {pk_is_zero(q.x ^ INVpk), pk_is_zero(q.y ^ INVpk), pk_is_zero(q.z ^ INVpk), pk_is_zero(q.w ^ INVpk)};
    return lr_bits8(z);
}
__device__ __forceinline__ unsigned spk_close_pk(const Short8& a, const Short8& b, uint32_t Spk)   // |a - b| <= S, S < 32767
{
    const uint4 qa = __builtin_bit_cast(uint4, a), qb = __builtin_bit_cast(uint4, b);
    const uint32_t A[4] = {qa.x, qa.y, qa.z, qa.w}, B[4] = {qb.x, qb.y, qb.z, qb.w};
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const lr_s2 df = __builtin_elementwise_sub_sat(lr_s(A[k]), lr_s(B[k]));                  // saturating: no wrap-around
        const uint32_t ad = lr_w(__builtin_elementwise_max(df, __builtin_elementwise_sub_sat(lr_s(0u), df)));   // 0 .. 32767
        c[k] = pk_is_zero(pk_subsat_u(ad, Spk));
    }
    return lr_bits8(c);
}

template <int RS, bool COMPACT, bool REC = false>
__global__ __launch_bounds__(256) void k_spk_merge_strip(Plane16W disp, int32_t* label, const int16_t* headmap, int W, int Ws, int H,
                                                         int y_lo, int npairs, int newVal, int maxDiff, int32_t* size, int maxSize,
                                                         int ystep, MergeRecArgs ra, const uint32_t* runs)
{
    __shared__ int2 queue[SPK_QCAP];                      // (spk_queue_push)
    __shared__ int qn;
    if (threadIdx.x == 0) qn = 0;
    __syncthreads();
    const bool rec_block = REC && (int)blockIdx.x < ra.blocks;            // workgroup-uniform
    if (rec_block) spk_rec_collect(queue, qn, label, (const uint32_t*)headmap, Ws, H, ra, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
    const int nxb = (W + 7) >> 3;                         // a ragged last chunk reads the plane's padding columns and masks them
    const int nstrips = (npairs + RS - 1) / RS;
    const int idx = ((int)blockIdx.x - (REC ? ra.blocks : 0)) * 256 + threadIdx.x;
    const bool inb = !rec_block && idx < nxb * nstrips;
    const int cidx = inb ? idx : 0;
    const int strip = cidx / nxb, x0 = (cidx % nxb) * 8;
    const int y = y_lo + strip * (RS == 1 ? ystep : RS);
    const int nr = inb ? min(RS, npairs - strip * RS) : 0;
    const int f = blockIdx.y;
    const int16_t* d = disp.base + (size_t)f * disp.frame_e + (size_t)y * disp.pitch_e + x0;
    int base = (f * H + y) * Ws;
    const int16_t* h = headmap + base + x0;
    const unsigned colmask = x0 + 8 <= W ? 0xffu : (0xffu >> (x0 + 8 - W));
    Short8 a8{}, b8{}, ha8, hb8;
    if (!COMPACT && inb) a8 = *(const Short8*)d;
    bool ha_loaded = false;
    const uint32_t* hc = (const uint32_t*)headmap + (size_t)(f * H + y) * (Ws >> 3) + (x0 >> 3);   // COMPACT: this chunk's records
    uint32_t ca = (COMPACT && inb) ? hc[0] : 0u;
    // COMPACT: the strip's RS + 1 head records are requested up front, then one run-list entry per chunk-row, then the rows
    // that are needed (with a load, a wait and the union queue's atomics per row, a wave kept one row in flight); records
    // past the strip's end repeat its last one and are not used.
    // SETTLED PAIRS.  A chunk-row is classified from its record before any disparity is read: no run start in the chunk and
    // none left of it -- EMPTY (no valid pixel); no run start in the chunk, cnt > 0 runs started left of it -- every valid
    // pixel of the chunk belongs to run cnt - 1 of the row, whose (x, len) is in the row's run list: x + len <= x0 -- EMPTY,
    // else LONG iff len > maxSize (the run list's length, not size[]: a marked short run is not long); a chunk with a run
    // start stays undecided.  The pair (r, r + 1) is settled when either chunk-row is empty or both are long: its contact mask
    // is taken as 0 and a row is loaded only if an unsettled pair touches it -- disparity maps are made of long runs, and the
    // second read of the plane was what this kernel spent its time on.  Exact: a settled pair has no contact or only contacts
    // between two long runs, which uf_union_contact drops without a union or a mark (only "size <= maxSize" is ever asked; the
    // overflow path's plain uf_union of two long runs joins two components that are both large, which changes no such answer
    // either -- so nothing here assumes that a long run is a root).  A long run over a short one is never settled, so the mark
    // still arrives.  The left-neighbour bit reads 0 behind a settled neighbour (and is fetched from memory by the first lane
    // of a wave): a contact at this thread's first pixel may then be queued although it continues the neighbour's contact --
    // only when neither pixel starts a run, so both runs are the neighbour's, hence long, and the duplicate is dropped as
    // long-long.
    Short8 rows[COMPACT ? RS : 1];
    uint32_t heads[COMPACT ? RS : 1];
    unsigned unsettled = 0, need = 0;                     // bit r: the pair (r, r + 1) has to be compared; bit j: row j is loaded
    // The contact mask in packed 16-bit arithmetic, two columns per instruction (the settled pairs took the kernel off the HBM
    // limit and left it bound by its VALU instructions, most of them this mask's per-column compares): one mask of invalid
    // columns per loaded row, |a - b| <= maxDiff per pair.  Differences saturate at 32767, so maxDiff must stay below that,
    // and newVal must be an int16 to be met at all (uniform; the per-column compares serve everything else).
    const bool pk = COMPACT && maxDiff >= 0 && maxDiff < 32767 && newVal == (int)(int16_t)newVal;
    const uint32_t INVpk = (uint32_t)(newVal & 0xffff) * 0x00010001u, Spk = (uint32_t)(maxDiff & 0xffff) * 0x00010001u;
    unsigned inva = 0, invb = 0;                          // bit k: column k of the upper / lower row is newVal
    if constexpr (COMPACT) {
        const int hp = Ws >> 3;
#pragma unroll
        for (int r = 0; r < RS; ++r) heads[r] = inb ? hc[(size_t)(r < nr ? r + 1 : nr) * hp] : 0u;
        // one look-up per chunk-row, all in flight together and without a branch: where cnt == 0 or the chunk has run
        // starts, entry 0 / cnt - 1 of the row is read (inside the row's part of the list) and not used
        uint32_t look[RS + 1];
#pragma unroll
        for (int j = 0; j <= RS; ++j) {
            const uint32_t rec = j ? heads[j - 1] : ca;
            look[j] = runs[(size_t)base + (size_t)(j <= nr ? j : nr) * Ws + (max((int)(rec & 0xffffu), 1) - 1)];
        }
        unsigned empty = 0, lng = 0;
#pragma unroll
        for (int j = 0; j <= RS; ++j) {
            const uint32_t rec = j ? heads[j - 1] : ca;
            const int cnt = (int)(rec & 0xffffu), rx = (int)(look[j] & 0xffffu), rlen = (int)(look[j] >> 16);
            const bool nostart = (rec & 0xff0000u) == 0u;
            const bool e = nostart && (cnt == 0 || rx + rlen <= x0);
            empty |= (unsigned)e << j;
            lng |= (unsigned)(nostart && !e && rlen > maxSize) << j;
        }
        unsettled = ~(empty | (empty >> 1) | (lng & (lng >> 1))) & ((1u << nr) - 1u);
        need = unsettled | (unsettled << 1);
        if (need & 1u) a8 = *(const Short8*)d;
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            rows[r] = Short8{};
            if ((need >> (r + 1)) & 1u) rows[r] = *(const Short8*)(d + (size_t)(r + 1) * disp.pitch_e);
        }
        if (pk && (need & 1u)) inva = spk_invalid_pk(a8, INVpk);
    }
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        unsigned cm = 0;
        if constexpr (COMPACT) b8 = rows[r];              // (zeros where no unsettled pair touches the row)
        if constexpr (COMPACT) if (pk && ((need >> (r + 1)) & 1u)) invb = spk_invalid_pk(b8, INVpk);
        if (COMPACT ? ((unsettled >> r) & 1u) != 0 : r < nr) {
            if constexpr (!COMPACT) b8 = *(const Short8*)(d + disp.pitch_e);
            if (COMPACT && pk) cm = spk_close_pk(a8, b8, Spk) & ~(inva | invb);
            else {
#pragma unroll
                for (int k = 0; k < 8; ++k) cm |= (unsigned)conn(a8.v[k], b8.v[k], newVal, maxDiff) << k;
            }
            cm &= colmask;
        }
        inva = invb;
        if constexpr (COMPACT) {
            const uint32_t cb = r < nr ? heads[r] : 0u;
            // contact bit of the pixel left of the chunk: lane-1's bit 7, or (first lane of a wave) from memory
            unsigned leftc = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(cm >> 7), 0x138, 0xf, 0xf, false);   // wave_shr:1
            if ((threadIdx.x & 63) == 0) leftc = (cm && x0 > 0) ? (unsigned)conn(d[-1], d[disp.pitch_e - 1], newVal, maxDiff) : 0u;
            if (x0 == 0) leftc = 0;                             // (lane-1 belongs to another strip there)
            const unsigned startA = (ca >> 16) & 0xffu, startB = (cb >> 16) & 0xffu;
            // a contact repeats the union of the contact to its left iff neither pixel of the pair starts a run
            unsigned cand = cm & ~(((cm << 1) | (leftc & 1u)) & ~startA & ~startB);
            while (cand) {
                const int k = __builtin_ctz(cand);
                cand &= cand - 1;
                // nodes = run indices (k_lrcheck_vec): runs that start left of the chunk + starts at or left of the pixel, - 1
                const unsigned ma = startA & ((2u << k) - 1u), mb = startB & ((2u << k) - 1u);
                const int ha = (int)(ca & 0xffffu) + __builtin_popcount(ma) - 1;
                const int hb = (int)(cb & 0xffffu) + __builtin_popcount(mb) - 1;
                spk_queue_push(queue, qn, label, base + ha, base + Ws + hb);
            }
            ca = cb;
        } else {
        hb8.v[7] = 0;
        if (cm) {
            if (!ha_loaded) ha8 = *(const Short8*)h;
            hb8 = *(const Short8*)(h + Ws);
        } else ha8.v[7] = 0;
        const int packed = (int)(cm >> 7) | ((int)(uint16_t)ha8.v[7] << 1) | ((int)(uint16_t)hb8.v[7] << 17);
        const int fromLeft = __shfl_up(packed, 1);
        if (cm) {
            bool pc = false;
            int ph0 = -1, ph1 = -1;
            if (x0 > 0) {
                if ((threadIdx.x & 63) != 0) {
                    pc = fromLeft & 1; ph0 = (fromLeft >> 1) & 0xffff; ph1 = (fromLeft >> 17) & 0x7fff;
                } else {
                    pc = conn(d[-1], d[disp.pitch_e - 1], newVal, maxDiff);
                    if (pc) { ph0 = h[-1]; ph1 = h[Ws - 1]; }
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bool c = (cm >> k) & 1;
                const int ha = ha8.v[k], hb = hb8.v[k];
                if (c && !(pc && ph0 == ha && ph1 == hb)) {
                    spk_queue_push(queue, qn, label, base + ha, base + Ws + hb);
                }
                pc = c; ph0 = ha; ph1 = hb;
            }
        }
        ha8 = hb8; ha_loaded = cm != 0;
        }
        a8 = b8;
        d += disp.pitch_e; h += Ws; base += Ws;
    }
    spk_queue_drain(queue, qn, label, size, maxSize);
}

// DENSE: the node of a run is base + its index in the row (k_lrcheck_vec), else base + the x of its head (spk_row_init).
template <bool DENSE>
__global__ __launch_bounds__(256) void k_spk_count(int32_t* label, int32_t* size, const uint32_t* runs,
                                                   const int32_t* rowcnt, int Ws, int nrows, int maxSize)
{
    const int row = blockIdx.x * 16 + (threadIdx.x >> 4);        // 16 lanes per row of the batch: rows have a few dozen runs
    if (row >= nrows) return;                                   // and every lane's work is a chain of dependent loads
    const int cnt = rowcnt[row], base = row * Ws;
    for (int i = threadIdx.x & 15; i < cnt; i += 16) {
        const uint32_t rn = runs[base + i];
        const int idx = base + (DENSE ? i : (int)(rn & 0xffffu));
        const int root = uf_find(label, idx);
        if (root == idx) continue;
        st_relaxed(&label[idx], root);             // roots are final in this launch
        // a non-root's size is its run length, or maxSize + 1 if the merge marked it (uf_union_contact): nobody adds to it
        if (ld_relaxed(&size[root]) <= maxSize) atomicAdd(&size[root], ld_relaxed(&size[idx]));
    }
}

template <bool DENSE>
__global__ __launch_bounds__(256) void k_spk_apply(Plane16W disp, const int32_t* label, const int32_t* size,
                                                   const uint32_t* runs, const int32_t* rowcnt, int Ws, int H, int nrows,
                                                   int newVal, int maxSize)
{
    const int row = blockIdx.x * 16 + (threadIdx.x >> 4);        // 16 lanes per row, as in k_spk_count
    if (row >= nrows) return;
    const int cnt = rowcnt[row], base = row * Ws;
    const int f = row / H, y = row - f * H;
    int16_t* drow = disp.base + (size_t)f * disp.frame_e + (size_t)y * disp.pitch_e;
    for (int i = threadIdx.x & 15; i < cnt; i += 16) {
        const uint32_t rn = runs[base + i];
        const int x = (int)(rn & 0xffffu), len = (int)(rn >> 16);
        if (len > maxSize) continue;               // a run longer than the limit is in a large component by itself
        // after k_spk_count a head is at most a couple of hops from its root (a late path-halving
        // store of another thread may have left an ancestor instead of the root), so chase it
        int root = base + (DENSE ? i : x);
        for (int p = label[root]; p != root; p = label[root]) root = p;
        if (size[root] <= maxSize)
            for (int k = 0; k < len; ++k) drow[x + k] = (int16_t)newVal;
    }
}

void launch_speckle(const SpkPlan& p, Plane16W disp, const SpkBuffers& wk, int newVal, int maxSize, int maxDiff, hipStream_t stream)
{
    const dim3 block(256);
    if (p.init_lds)
        hipLaunchKernelGGL(k_spk_init, dim3(1, p.H, p.n), block, p.init_lds, stream, disp, wk.label, wk.size, wk.runs, wk.rowcnt,
                           wk.headmap, p.W, p.Ws, p.H, newVal, maxDiff);
    if (p.rec_own.blocks)
        hipLaunchKernelGGL(k_spk_merge_rec, dim3(p.rec_own.blocks, p.n), block, 0, stream, wk.label, (const uint32_t*)wk.headmap, p.Ws,
                           p.H, p.rec_own, wk.size, maxSize);
    const auto strip = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(p.merge_gx, p.n), block, 0, stream, disp, wk.label, wk.headmap, p.W, p.Ws, p.H, p.first, p.npairs,
                           newVal, maxDiff, wk.size, maxSize, p.ystep, p.rec_fused, wk.runs);
    };
    switch (p.merge) {
        case SpkMerge::NONE: break;
        case SpkMerge::ROWS:
            hipLaunchKernelGGL(k_spk_merge, dim3(p.merge_gx, p.n), block, 0, stream, disp, wk.label, wk.headmap, p.W, p.Ws, p.H, p.first,
                               p.npairs, newVal, maxDiff);
            break;
        case SpkMerge::STRIP4_PIXEL:     strip(k_spk_merge_strip<4, false, false>); break;
        case SpkMerge::STRIP1_CHUNK:     strip(k_spk_merge_strip<1, true, false>); break;
        case SpkMerge::STRIP2_CHUNK:     strip(k_spk_merge_strip<2, true, false>); break;
        case SpkMerge::STRIP4_CHUNK:     strip(k_spk_merge_strip<4, true, false>); break;
        case SpkMerge::STRIP1_CHUNK_REC: strip(k_spk_merge_strip<1, true, true>); break;
    }
    const int nrows = p.n * p.H;
    const auto count_apply = [&](auto count, auto apply) {   // DENSE (chunk records): nodes are run indices
        hipLaunchKernelGGL(count, dim3(p.rows_gx), block, 0, stream, wk.label, wk.size, wk.runs, wk.rowcnt, p.Ws, nrows, maxSize);
        hipLaunchKernelGGL(apply, dim3(p.rows_gx), block, 0, stream, disp, wk.label, wk.size, wk.runs, wk.rowcnt, p.Ws, p.H, nrows, newVal, maxSize);
    };
    if (p.heads == SpkHeads::CHUNK) count_apply(k_spk_count<true>, k_spk_apply<true>);
    else count_apply(k_spk_count<false>, k_spk_apply<false>);
}

}  // namespace rtdm

