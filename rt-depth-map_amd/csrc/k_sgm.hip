// k_sgm.hip -- the device counterpart of the reference's SWSemiGlobalMatcher (stereo-matcher/
// sgbm-sw.cpp:12-37 -> cv::StereoSGBM, P1 = 600, P2 = 2400): paths = 5 is the library's MODE_SGBM (what sgbm-sw.cpp:15
// creates), paths = 8 its MODE_HH (BASELINE config 5, "8-path"), paths = 4 its MODE_HH4 (left, right, down, up).  The algorithm is the restatement in
// oracle/sgm_oracle.c (rules R1-R12 there; integer arithmetic, tolerance 0 against that oracle; parity against a real
// cv::StereoSGBM is unpinned).  Cost volumes live on the column domain [x0, x1) = [minD+D, W+min(minD,0)) and are laid
// out [frame][y][x - x0][d] with d fastest, so a wavefront's lanes = consecutive disparities = one coalesced line per pixel.
//
//   k_sgm_cost.hip   the two frames -> the block costs C (launch_sgm_cost)
//   k_sgm_paths.hip  the path passes over lines of at most 256 disparities: C -> S, the last pass -> the winners
//   k_sgm_wide.hip   the path pass for wider lines
//   here             the schedule of the passes (launch_sgm) and what follows the winners:
//
//   k_sgm_lrfinal one workgroup per row: the votes of the integer winners (LDS, right-most voter wins ties: R7) and the
//                always-on left-right check (R9)
//   k_sgm_median 3x3 median with clamped coordinates (R10) + the speckle filter's per-row init
#include "rtdm_kernels.h"
#include "rtdm_device.h"

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

// the winners' votes and left-right check (k_sgm_lrfinal: the last path pass decided them), the median and the speckle filter
static void sgm_finish(Plane16W disp, const SGMGeom& g, const SGMBuffers& b, int disp12MaxDiff, int speckleWindowSize,
                       int speckleRange, int n, hipStream_t stream, const SgmWin* win)
{
    dim3 blk(256);
    const bool speckle = speckleWindowSize > 0;                           // R11
    const size_t lds = (size_t)g.W * (8 + 2 + 2 + 2);
    // select -> a temporary plane (the bounds buffer of the left image is free again), median -> the caller's plane
    int16_t* tmp = (int16_t*)b.gl;
    const Plane16W tplane{tmp, (size_t)g.W, (size_t)g.W * g.H};
    hipLaunchKernelGGL(k_sgm_lrfinal, dim3(1, g.H, n), blk, lds, stream, win, tplane, g, disp12MaxDiff);
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

const char* launch_sgm(Plane8 L, Plane8 R, Plane16W disp, const SGMGeom& g, const SGMBuffers& b, int blockSize, int P1, int P2,
                       int uniq, int disp12MaxDiff, int speckleWindowSize, int speckleRange, int paths, int n, hipStream_t stream,
                       int cost_limit, int cn, int ftz)
{
    launch_sgm_cost(L, R, g, b, blockSize, cost_limit, cn, ftz, n, stream);
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
    const int last_dir = paths == 4 ? 3 : (paths == 5 ? 5 : 7);   // MODE_HH4 (R4'): the first four directions and no others
    SgmWin* win = (SgmWin*)b.gr;                     // the right image's bounds are dead once the pixel costs exist: 8 bytes per pixel
    // D > 256 (or rtdm_debug_sgm_wide_paths): one wide pass per direction (k_sgm_wide.hip), the last one deciding the winners;
    // none of the forms below -- they hold at most 256 disparities per line
    if (g.D > 256 || sgm_wide_mode()) {
        for (int k = 0; k <= last_dir; ++k) {
            if (paths == 5 && dirs[k][1] < 0) continue;
            launch_sgm_wide(g, b.C, b.S, dirs[k][0], dirs[k][1], P1, P2, k == 0 ? 1 : 0, k == last_dir, n, win, uniq, stream);
        }
        sgm_finish(disp, g, b, disp12MaxDiff, speckleWindowSize, speckleRange, n, stream, win);
        return sgm_wide_waves(g.D) == 1 ? "wide_w1" : "wide_w4";
    }
    // (C, S and S2 are whole allocations: 16-byte aligned, as the packed loads and stores of the path passes need)
    // RTDM_SGM_SWEEP=0 (test hook): one pass per direction for the six that advance a row per step as well -- what runs after
    // a sweep gave up or did not fit
    static const int sweep_env = env_int("RTDM_SGM_SWEEP", 1);
    bool sweep = sweep_env && b.ring && b.abortf && *b.abortf == 0;
    bool swept_down = false, swept_up = false;
    // RTDM_SGM_DUAL=0 (test hook): the two horizontal directions one after the other (the second adds to S) instead of side by
    // side -- what runs without S2
    static const int dual_env = env_int("RTDM_SGM_DUAL", 1);
    if (paths == 4) {
        // MODE_HH4: -> and <- (side by side into S and S2 where there is an S2), then the two vertical directions on the
        // column-parallel pass, the upward one deciding the winners -- no sweep, no ring, no epoch, no sweep stream.
        // RTDM_SGM_SWEEP=0: one k_sgm_path_h pass per direction instead (what k_sgm_vert is timed against)
        if (!sweep_env) {
            for (int k = 0; k < 4; ++k) launch_path_h(g, b, dirs[k][0], dirs[k][1], P1, P2, k == 0, k == 3, n, win, uniq, stream);
            sgm_finish(disp, g, b, disp12MaxDiff, speckleWindowSize, speckleRange, n, stream, win);
            return "half";
        }
        const bool dual = dual_env && b.S2;
        launch_path_h(g, b, 1, 0, P1, P2, 1, false, n, win, uniq, stream, dual ? b.S2 : nullptr);
        if (!dual) launch_path_h(g, b, -1, 0, P1, P2, 0, false, n, win, uniq, stream);
        launch_vert(g, b, 1, P1, P2, false, n, win, uniq, stream, dual ? b.S2 : nullptr);
        launch_vert(g, b, -1, P1, P2, true, n, win, uniq, stream, nullptr);
        sgm_finish(disp, g, b, disp12MaxDiff, speckleWindowSize, speckleRange, n, stream, win);
        return "vert";
    }
    bool s2_pending = false;                         // S2 holds the (-1, 0) direction's L_r and has not been added to S yet
    bool swept = false;                              // a row-synchronous sweep ran (the variant this call reports)
    for (int k = 0; k < 8; ++k) {
        const int dx = dirs[k][0], dy = dirs[k][1];
        if (paths == 5 && dy < 0) continue;          // MODE_SGBM's five directions: nothing runs upwards
        if (k == 0 && sweep && dual_env && b.S2 &&
            launch_sweep(paths == 5, g, b, 1, P1, P2, n, win, uniq, stream, nullptr, true)) {
            // both horizontal directions in one launch: (1, 0) -> S, (-1, 0) -> S2; the downward sweep adds the two up
            launch_path_h(g, b, 1, 0, P1, P2, 1, false, n, win, uniq, stream, b.S2);
            s2_pending = true;
            continue;
        }
        if (k == 1 && s2_pending) continue;
        if (dy != 0) {
            // (0, dy), (+1, dy), (-1, dy) in one row-synchronous pass: -> <- down [up]; the last sweep decides the winners
            bool& done = dy > 0 ? swept_down : swept_up;
            if (done) continue;
            if (sweep && (k == 2 || k == 3)) {
                const bool last_sweep = paths == 5 || dy < 0;
                if (launch_sweep(last_sweep, g, b, dy, P1, P2, n, win, uniq, stream, s2_pending ? b.S2 : nullptr)) { done = true; s2_pending = false; swept = true; continue; }
                sweep = false;                       // not launched: this and the remaining directions run as passes of their own
            }
            if (s2_pending) { launch_sgm_add_s2(g, b, n, stream); s2_pending = false; }   // (the sweep that was to add S2 could not be launched)
        }
        launch_path_h(g, b, dx, dy, P1, P2, k == 0, k == last_dir, n, win, uniq, stream);
    }
    sgm_finish(disp, g, b, disp12MaxDiff, speckleWindowSize, speckleRange, n, stream, win);
    return swept ? "sweep" : "half";
}

}  // namespace rtdm
