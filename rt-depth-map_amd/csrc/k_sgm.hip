// k_sgm.hip -- the device counterpart of the reference's SWSemiGlobalMatcher (stereo-matcher/
// sgbm-sw.cpp:12-37 -> cv::StereoSGBM, P1 = 600, P2 = 2400): paths = 5 is the library's MODE_SGBM (what sgbm-sw.cpp:15
// creates), paths = 8 its MODE_HH (BASELINE config 5, "8-path"), paths = 4 its MODE_HH4 (left, right, down, up).  The algorithm is the restatement in
// oracle/sgm_oracle.c (rules R1-R12 there; integer arithmetic, tolerance 0 against that oracle; parity against a real
// cv::StereoSGBM is unpinned).  Cost volumes live on the column domain [x0, x1) = [minD+D, W+min(minD,0)) and are laid
// out [frame][y][x - x0][d] with d fastest, so a wavefront's lanes = consecutive disparities = one coalesced line per pixel.
//
//   k_sgm_cost.hip   the two frames -> the block costs C (plan_sgm_cost / launch_sgm_cost)
//   k_sgm_paths.hip  the path passes over lines of at most 256 disparities: C -> S, the last pass -> the winners
//   k_sgm_wide.hip   the path pass for wider lines
//   here             the schedule of the passes (plan_sgm / launch_sgm) and what follows the winners:
//
//   k_sgm_lrfinal one workgroup per row: the votes of the integer winners (LDS, right-most voter wins ties: R7) and the
//                always-on left-right check (R9)
//   k_sgm_final3 MODE_SGBM_3WAY's final stage: neither of the two (T6)
//   k_sgm_median 3x3 median with clamped coordinates (R10) + the speckle filter's per-row init
#include "rtdm_sgm.h"

namespace rtdm {

// The winners that were found inside the last path pass (k_sgm_path_h / k_sgm_sweep / k_sgm_vert / k_sgm_wide, LAST): the votes
// of a row (R7), the always-on left-right check (R9) and the row's x16 disparities.  One workgroup per row.
__global__ __launch_bounds__(256) void k_sgm_lrfinal(const SgmWin* win, Plane16W disp, SGMGeom g, int disp12MaxDiff)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* key = (unsigned long long*)smem;     // W : (minS << 32 | 0xffff - x) votes per right column
    int16_t* bdv = (int16_t*)(key + g.W);                    // W : integer winner + minD of column x (or minD-1)
    int16_t* row = bdv + g.W;                                // W : disparity row
    const int y = blockIdx.y, f = blockIdx.z;
    const int W = g.W, minD = g.minD, INV = (minD - 1) * 16;
    for (int x = threadIdx.x; x < W; x += 256) { key[x] = ~0ull; bdv[x] = (int16_t)(minD - 1); row[x] = (int16_t)INV; }
    __syncthreads();
    const SgmWin* wrow = win + ((size_t)f * g.H + y) * g.W1;
    for (int xi = threadIdx.x; xi < g.W1; xi += 256) {
        const SgmWin w = wrow[xi];
        if (w.bd < minD) continue;                            // rejected by the uniqueness test: no vote, INV
        const int x = g.x0 + xi, x2 = x - (int)w.bd;
        if (x2 >= 0 && x2 < W) atomicMin(&key[x2], ((unsigned long long)w.mins << 32) | (unsigned)(0xffff - x));
        bdv[x] = w.bd;
        row[x] = w.d16;
    }
    __syncthreads();
    int16_t* out = disp.base + (size_t)f * disp.frame_e + (size_t)y * disp.pitch_e;
    for (int x = threadIdx.x; x < W; x += 256) {
        int d1 = row[x];
        if (d1 != INV) {                                      // R9: always on (the host passes disp12MaxDiff > 0 ? it : 1)
            const int da = d1 >> 4, db = (d1 + 15) >> 4;
            const int xa = x - da, xb = x - db;
            const auto vote = [&](int xv) -> int { return key[xv] != ~0ull ? (int)bdv[0xffff - (unsigned)(key[xv] & 0xffffu)] : INV; };
            bool ba = false, bb = false;
            if (xa >= 0 && xa < W) { const int v = vote(xa); ba = v >= minD && abs(v - da) > disp12MaxDiff; }
            if (xb >= 0 && xb < W) { const int v = vote(xb); bb = v >= minD && abs(v - db) > disp12MaxDiff; }
            if (ba && bb) d1 = INV;
        }
        out[x] = (int16_t)d1;
    }
}

// MODE_SGBM_3WAY's final stage (T6): the winners' x16 disparities as they are -- no votes (R7) and no left-right check (R9)
__global__ __launch_bounds__(256) void k_sgm_final3(const SgmWin* win, Plane16W disp, SGMGeom g)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= g.W) return;
    const int xi = x - g.x0;
    int d1 = (g.minD - 1) * 16;
    if (xi >= 0 && xi < g.W1) {
        const SgmWin w = win[((size_t)f * g.H + y) * g.W1 + xi];
        if (w.bd >= g.minD) d1 = w.d16;                       // (rejected by the uniqueness test or saturated: INV)
    }
    disp.base[(size_t)f * disp.frame_e + (size_t)y * disp.pitch_e + x] = (int16_t)d1;
}

// R10: medianBlur(disp, disp, 3) -- 3x3 median of the int16 map with clamped coordinates -- followed by the speckle
// filter's per-row init on the filtered row.  One workgroup per row; the three source rows stream through L2.
__device__ __forceinline__ void mnmx(int& a, int& b) { const int t = min(a, b); b = max(a, b); a = t; }
template <bool SPK>
__global__ __launch_bounds__(256) void k_sgm_median(const int16_t* src, Plane16W disp, int W, int H, int INV, int32_t* label,
                                                    int32_t* size, uint32_t* runs, int32_t* rowcnt, int16_t* headmap, int spkDiff)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* sc = (int*)smem;                                   // W : scan scratch of the speckle init
    int16_t* fin = (int16_t*)(sc + W);                      // W : the filtered row
    __shared__ int wsum[4];
    const int y = blockIdx.y, f = blockIdx.z;
    const int16_t* base = src + (size_t)f * H * W;
    const int16_t* r0 = base + (size_t)max(y - 1, 0) * W;
    const int16_t* r1 = base + (size_t)y * W;
    const int16_t* r2 = base + (size_t)min(y + 1, H - 1) * W;
    int16_t* out = disp.base + (size_t)f * disp.frame_e + (size_t)y * disp.pitch_e;
    for (int x = threadIdx.x; x < W; x += 256) {
        const int xm = max(x - 1, 0), xp = min(x + 1, W - 1);
        int p0 = r0[xm], p1 = r0[x], p2 = r0[xp], p3 = r1[xm], p4 = r1[x], p5 = r1[xp], p6 = r2[xm], p7 = r2[x], p8 = r2[xp];
        // median-of-nine exchange network (19 exchanges)
        mnmx(p1, p2); mnmx(p4, p5); mnmx(p7, p8); mnmx(p0, p1); mnmx(p3, p4); mnmx(p6, p7); mnmx(p1, p2); mnmx(p4, p5);
        mnmx(p7, p8); mnmx(p0, p3); mnmx(p5, p8); mnmx(p4, p7); mnmx(p3, p6); mnmx(p1, p4); mnmx(p2, p5); mnmx(p4, p7);
        mnmx(p4, p2); mnmx(p6, p4); mnmx(p4, p2);
        out[x] = (int16_t)p4;
        if (SPK) fin[x] = (int16_t)p4;
    }
    if (SPK) {
        __syncthreads();
        spk_row_init(fin, sc, wsum, W, (f * H + y) * W, label, size, runs, rowcnt + (f * H + y), headmap, INV, spkDiff);
    }
}

// the winners' votes and left-right check (k_sgm_lrfinal: the last path pass decided them; !votes, MODE_SGBM_3WAY: neither,
// k_sgm_final3), the median and the speckle filter
static void sgm_finish(Plane16W disp, const SGMGeom& g, const SGMBuffers& b, int disp12MaxDiff, int speckleWindowSize,
                       int speckleRange, int n, hipStream_t stream, const SgmWin* win, bool votes)
{
    dim3 blk(256);
    const bool speckle = speckleWindowSize > 0;                           // R11
    const size_t lds = (size_t)g.W * (8 + 2 + 2 + 2);
    // select -> a temporary plane (the bounds buffer of the left image is free again), median -> the caller's plane
    int16_t* tmp = (int16_t*)b.gl;
    const Plane16W tplane{tmp, (size_t)g.W, (size_t)g.W * g.H};
    if (votes) hipLaunchKernelGGL(k_sgm_lrfinal, dim3(1, g.H, n), blk, lds, stream, win, tplane, g, disp12MaxDiff);
    else hipLaunchKernelGGL(k_sgm_final3, dim3((g.W + 255) / 256, g.H, n), blk, 0, stream, win, tplane, g);
    const size_t mlds = (size_t)g.W * 6;
    const int INV = (g.minD - 1) * 16;
    if (speckle) {
        hipLaunchKernelGGL((k_sgm_median<true>), dim3(1, g.H, n), blk, mlds, stream, tmp, disp, g.W, g.H, INV, b.label, b.size, b.runs,
                           b.rowcnt, b.headmap, 16 * speckleRange);
        // k_sgm_median has initialised every row with per-pixel heads (workspace rows of W elements) and merged nothing
        const SpkPlan sp = plan_speckle(g.W, g.W, g.H, n, SpkHeads::PIXEL, 1, 0, g.H, rows_aligned(disp, nullptr, nullptr, g.W));
        launch_speckle(sp, disp, SpkBuffers{b.label, b.size, b.runs, b.rowcnt, b.headmap}, INV, speckleWindowSize, 16 * speckleRange, stream);
    } else {
        hipLaunchKernelGGL((k_sgm_median<false>), dim3(1, g.H, n), blk, mlds, stream, tmp, disp, g.W, g.H, INV, b.label, b.size, b.runs,
                           b.rowcnt, b.headmap, 0);
    }
}

// Whether a sweep of the form (LAST, ADD2) fits, and in which shape: the narrowest strips whose workgroups all fit the device at
// once -- 8 columns (one per half-wave), 16, 32: a frame's rows are a serial chain, so the pass is latency bound until every
// SIMD holds several waves, and the fewer lines a wave carries the shorter its row; wider strips pay the per-row overhead
// (barrier, edges, addresses) less often -- and whose edges fit the ring.  cols == 0: none does.
struct SweepFit { int cols, strips, items, grid; };
static SweepFit sweep_fit(const SGMGeom& g, int n, const SgmLimits& lim, bool last, bool add2)
{
    // RTDM_SGM_SWEEP_COLS=1 / 2 / 4 (test hook): fixes the first width tried, as a capacity miss does
    static const int cols_env = env_int("RTDM_SGM_SWEEP_COLS", 0);
    const auto cap = [&](int c) { return lim.cap[last][c == 4 ? 2 : c - 1][add2]; };
    const int pick = cols_env ? cols_env : (n * ((g.W1 + 7) / 8) <= cap(1) ? 1 : (n * ((g.W1 + 15) / 16) <= cap(2) ? 2 : 4));
    for (int c = pick == 1 || pick == 2 ? pick : 4; c <= 4; c *= 2) {
        const int strips = (g.W1 + 8 * c - 1) / (8 * c), items = n * strips;
        if (cap(c) >= strips && (size_t)items * 2 * SWEEP_RING * 32 * sgm_np2(g.D) <= lim.ring_words)
            return SweepFit{c, strips, items, items <= cap(c) ? items : cap(c) / strips * strips};   // the strips of a frame run in the same round
    }
    return SweepFit{0, 0, 0, 0};
}

SgmPlan plan_sgm(const SGMGeom& g, int paths, int n, const SgmLimits& lim, SgmDone done)
{
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
    const int last_dir = paths == 4 ? 3 : (paths == 5 ? 5 : 7);   // MODE_HH4 (R4'): the first four directions and no others
    SgmPlan plan{};
    const auto add = [&](SgmStep step, int k, bool s2) -> SgmPass& {
        SgmPass& p = plan.pass[plan.npasses++];
        p = SgmPass{step, k, k < 0 ? 0 : dirs[k][0], k < 0 ? 0 : dirs[k][1], k == 0, k == last_dir, s2, 0, 0, 0, 0, 0};
        return p;
    };
    // MODE_SGBM_3WAY (T4, T5; D <= 256: rtdm_sgm_set_mode has refused the others): -> and <- over the whole frame as for
    // MODE_HH4, then the striped downward pass, which decides the winners.  No sweep, no wide form: RTDM_SGM_SWEEP and
    // rtdm_debug_sgm_wide_paths are not consulted; RTDM_SGM_DUAL = 0 keeps its meaning.
    // RTDM_SGM_DUAL=0 (test hook): the two horizontal directions one after the other (the second adds to S) instead of side by
    // side -- what runs without S2
    static const int dual_env = env_int("RTDM_SGM_DUAL", 1);
    if (paths == 3) {
        const bool dual = dual_env && lim.s2;
        add(SgmStep::PATH_H, 0, dual);
        if (!dual) add(SgmStep::PATH_H, 1, false);
        add(SgmStep::VERT3, 2, dual).last = true;
        plan.variant = "vert3";
        return plan;
    }
    // D > 256 (or rtdm_debug_sgm_wide_paths): one wide pass per direction (k_sgm_wide.hip), the last one deciding the winners;
    // none of the forms below -- they hold at most 256 disparities per line -- and none of their hooks
    const int wide = sgm_wide_mode();
    if (g.D > 256 || wide) {
        const int waves = wide == 4 || g.D > 1024 ? 4 : 1;
        for (int k = 0; k <= last_dir; ++k)
            if (paths != 5 || dirs[k][1] >= 0) add(SgmStep::WIDE, k, false).waves = waves;
        plan.variant = waves == 1 ? "wide_w1" : "wide_w4";
        return plan;
    }
    // RTDM_SGM_SWEEP=0 (test hook): one k_sgm_path_h pass per direction for those that advance a row per step as well -- what
    // runs after a sweep gave up or did not fit, and what k_sgm_vert is timed against
    static const int sweep_env = env_int("RTDM_SGM_SWEEP", 1);
    if (paths == 4 && sweep_env) {
        // MODE_HH4: -> and <- (side by side into S and S2 where there is an S2), then the two vertical directions on the
        // column-parallel pass, the upward one deciding the winners -- no sweep, no ring, no epoch, no sweep stream
        const bool dual = dual_env && lim.s2;
        add(SgmStep::PATH_H, 0, dual);
        if (!dual) add(SgmStep::PATH_H, 1, false);
        add(SgmStep::VERT, 2, dual);
        add(SgmStep::VERT, 3, false);
        plan.variant = "vert";
        return plan;
    }
    bool sweeping = sweep_env && lim.sweep;
    for (int k = 0; k <= last_dir; ++k) {
        if ((done.dirs >> k & 1) || (paths == 5 && dirs[k][1] < 0)) continue;   // MODE_SGBM's five directions: nothing runs upwards
        if (k == 0) {
            // both horizontal directions in one launch, (1, 0) -> S and (-1, 0) -> S2, where the downward sweep will add the two up
            done.s2_pending = sweeping && dual_env && lim.s2 && sweep_fit(g, n, lim, paths == 5, true).cols;
            add(SgmStep::PATH_H, 0, done.s2_pending);
            if (done.s2_pending) done.dirs |= 1u << 1;
            continue;
        }
        if (k == 2 || k == 3) {
            // (0, dy), (+1, dy), (-1, dy) in one row-synchronous pass: -> <- down [up]; the last sweep decides the winners.  One
            // that does not fit: this and the remaining directions run as passes of their own
            const bool last = paths == 5 || k == 3;
            const SweepFit f = sweeping ? sweep_fit(g, n, lim, last, done.s2_pending) : SweepFit{0, 0, 0, 0};
            sweeping = f.cols != 0;
            if (sweeping) {
                SgmPass& p = add(SgmStep::SWEEP, k, done.s2_pending);
                p.last = last; p.cols = f.cols; p.strips = f.strips; p.items = f.items; p.grid = f.grid;
                done.dirs |= k == 2 ? 0x30u : 0xc0u;   // the two diagonals of that dy are covered
                done.s2_pending = false; done.swept = true;
                continue;
            }
        }
        if (done.s2_pending) { add(SgmStep::ADD_S2, -1, false); done.s2_pending = false; }   // (no sweep adds S2 after all)
        add(SgmStep::PATH_H, k, false);
    }
    plan.variant = done.swept ? "sweep" : "half";
    return plan;
}

// What is done once the first `count` passes of a plan have been issued
static SgmDone sgm_done(const SgmPlan& plan, int count)
{
    SgmDone d{0, false, false};
    for (int i = 0; i < count; ++i) {
        const SgmPass& p = plan.pass[i];
        if (p.dir >= 0) d.dirs |= 1u << p.dir;
        if (p.step == SgmStep::PATH_H && p.s2) { d.dirs |= 1u << 1; d.s2_pending = true; }
        if (p.step == SgmStep::SWEEP) { d.dirs |= p.dy > 0 ? 0x30u : 0xc0u; d.swept = true; }
        if (p.step == SgmStep::SWEEP || p.step == SgmStep::ADD_S2) d.s2_pending = false;
    }
    return d;
}

// Issues the passes in order; returns how many were issued: less than all where the next one is a sweep the runtime refused
static int sgm_issue(const SgmPlan& plan, const SgmCall& c)
{
    for (int i = 0; i < plan.npasses; ++i) {
        const SgmPass& p = plan.pass[i];
        switch (p.step) {
            case SgmStep::WIDE: launch_sgm_wide(p, c); break;
            case SgmStep::PATH_H: launch_path_h(p, c); break;
            case SgmStep::VERT: launch_vert(p, c); break;
            case SgmStep::ADD_S2: launch_sgm_add_s2(c); break;
            case SgmStep::VERT3: launch_vert3(p, c); break;
            case SgmStep::SWEEP: if (!launch_sweep(p, c)) return i; break;
        }
    }
    return plan.npasses;
}

const char* launch_sgm(Plane8 L, Plane8 R, Plane16W disp, const SGMGeom& g, const SGMBuffers& b, const SgmLimits& lim, int paths,
                       int n, hipStream_t stream, SgmParams p)
{
    launch_sgm_cost(plan_sgm_cost(g.D, g.H, p.blockSize, p.P2, p.cn, p.ftz, p.cost, paths, sgm_cost16_forced()), L, R, g, b, n, stream);
    // (the right image's bounds are dead once the cost stage is through: 8 bytes per pixel for the winners; C, S and S2 are whole
    // allocations: 16-byte aligned, as the packed loads and stores of the path passes need)
    const SgmCall c{g, b, p.P1, p.P2, p.uniq, n, (SgmWin*)b.gr, stream, p.blockSize};
    SgmPlan plan = plan_sgm(g, paths, n, lim);
    const int issued = sgm_issue(plan, c);
    if (issued < plan.npasses) {                     // a refused sweep: the remainder without sweeps, which nothing can refuse
        SgmLimits rest = lim;
        rest.sweep = false;
        plan = plan_sgm(g, paths, n, rest, sgm_done(plan, issued));
        sgm_issue(plan, c);
    }
    sgm_finish(disp, g, b, p.disp12MaxDiff, p.speckleWindowSize, p.speckleRange, n, stream, c.win, paths != 3);
    return plan.variant;
}

}  // namespace rtdm
