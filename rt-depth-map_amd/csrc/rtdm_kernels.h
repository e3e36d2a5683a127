// rtdm_kernels.h -- internal launch interface between the C-ABI layer (api_*.hip) and the
// gfx950 kernels.  Everything here is device-pointer based and asynchronous on `stream`.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>
#include <vector>

#include "rtdm_sgm_cost_plan.h"

namespace rtdm {

// Process-wide state shared BETWEEN handles (two handles may be driven from two host threads): environment switches (test
// hooks that force a form the library also runs on its own, and measurement knobs) are read through
// env_int() into a function-local `static const` (C++11 initialises those exactly once, thread-safely), and "once per
// device" actions go through OncePerDevice.  Nothing else in the launch paths is static and mutable.
inline int env_int(const char* name, int dflt)
{
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
// first(dev) is true for exactly one caller per device; the others may run concurrently with that caller's action, so the
// action must be idempotent (hipFuncSetAttribute with a fixed value is).  Devices >= 64: always true.
struct OncePerDevice {
    std::atomic<unsigned long long> mask{0};
    bool first()
    {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev < 0 || dev >= 64) return true;
        const unsigned long long bit = 1ull << dev;
        if (mask.load(std::memory_order_acquire) & bit) return false;
        return !(mask.fetch_or(bit, std::memory_order_acq_rel) & bit);
    }
};

// Geometry of one StereoBM search, derived once per call on the host.
struct BMGeom {
    int W, H;            // frame size
    int Ws;              // row stride (elements) of the per-pixel workspace planes (cost, labels, sizes, run lists,
                         // head map): W rounded up to 8 so that their rows start 16-byte aligned
    int D, minD;         // numDisparities, minDisparity
    int w, r;            // blockSize, blockSize/2
    int cap, tex, uniq;  // preFilterCap, textureThreshold, uniquenessRatio
    int lofs, rofs, width1;
    int vx0, vx1, vy0, vy1;  // valid-disparity rectangle [vx0,vx1) x [vy0,vy1)
    int cx0, cx1;            // image columns that have to be searched: the valid columns plus, when the
                             // left-right check is on, every column that can vote for them (setROI1 skips the rest)
    int filtered;            // (minD-1)*16
    int mask_cols;           // 1: the search kernel masks columns outside [vx0,vx1) itself
    int want_cost;           // 1: a cost plane is written for the left-right check
    int cost16;              // 1: the cost plane is uint16 (all SADs < 65536), else int32
    int legacy;              // rtdm_bm_params.legacy_right_clamp: right sample base clamped to W-rofs-1, base + d wraps into the next row
};

struct Plane8 {  // batch of 8-bit images: frame f, row y at base + f*frame + y*pitch
    const uint8_t* base; size_t pitch, frame;
};
struct Plane8W { uint8_t* base; size_t pitch, frame; };
struct Plane16W { int16_t* base; size_t pitch_e, frame_e; };  // strides in elements

// The internal prefiltered planes hold clamp(sobel) + cap + PREFILTER_BIAS: every byte is >= 1.  The packed search kernels
// need that (v_mqsad_pk_u16_u8 skips ZERO reference bytes: that is how a window's unused tail bytes are masked), absolute
// differences do not see a common offset, and the texture term becomes |p - (cap + PREFILTER_BIAS)|.  (Until round 3 every
// search wave added the bias to each staged dword itself.)  cap <= 63: the bytes stay <= 127.
static constexpr int PREFILTER_BIAS = 1;

// K1: prefilter of n left and n right frames in one launch (writes biased values, see above).  type: RTDM_PREFILTER_XSOBEL
// (k_prefilter.hip; ws is not read) or RTDM_PREFILTER_NORMALIZED_RESPONSE with window ws (k_prefilter_norm.hip).
// fill != null: launch_fill_frame's job (below) for the same n frames rides in the same launch where the strip form runs
// (a single frame is bound by the number of its launches), and is launched by itself before the other forms.
struct FillJob { Plane16W disp; int cx0, cx1, vy0, vy1, value; int32_t* rowcnt; };
void launch_prefilter(Plane8 L, Plane8 R, Plane8W Lp, Plane8W Rp, int W, int H, int cap, int n,
                      hipStream_t stream, const FillJob* fill = nullptr, int type = 1, int ws = 9);
// The NORMALIZED_RESPONSE form by itself (rules N1-N5); every alignment class of L / R, the planes Lp / Rp 16-byte aligned.
void launch_prefilter_norm(Plane8 L, Plane8 R, Plane8W Lp, Plane8W Rp, int W, int H, int cap, int ws, int n, hipStream_t stream);

// Fill the rectangle [x0,x1) x [y0,y1) of every disparity frame with `value`.
void launch_fill16(Plane16W disp, int x0, int x1, int y0, int y1, int n, int value, hipStream_t stream);
// The complement of [cx0, cx1) x [vy0, vy1) in every frame, plus (rowcnt != null) rowcnt[n][H] = 0, in one launch.
void launch_fill_frame(Plane16W disp, int W, int H, int cx0, int cx1, int vy0, int vy1, int n, int value, int32_t* rowcnt,
                       hipStream_t stream);

// K2: the SAD search (k_search.hip): writes disp (+ the cost plane, uint16 or int32 by g.cost16) for every valid configuration
// (D a multiple of 16 up to 4080, any odd w).  plan_search decides, once per call and without touching the runtime, what
// launch_search then issues: the kernel of the interior columns (whose windows need no border clamping), the form of the
// border columns and where they run.  The route table is in DESIGN.md ("K2: routes").
struct BorderGeom { int lx0, lx1, rx0, rx1, rs, rsp; };   // kernel arguments of the two border forms: output-column ranges,
struct Border2Geom { int lx0, lx1, rx0, rx1, ro; };       // rows per workgroup / output rows per wave
enum class SearchTiles { GENERIC, FAST, RING };           // k_search_generic / k_search_dslice, k_search_fast, k_search_ring
enum class BorderForm { NONE, ROWS, DISP, GENERIC };      // no border columns, border2_body, border_body, launch_search_generic
enum class BorderPlace { FUSED, SIDE, AFTER };            // in the tile kernel's grid, own launch on the side stream, own launch behind
struct BorderPlan {
    BorderForm form;
    Border2Geom rows; BorderGeom disp;     // the geometry of form ROWS / DISP (DISP + g.legacy: the LEGACY instantiation)
    int gx, gy;                            // its grid per frame
    size_t lds;                            // its dynamic LDS
};
struct SearchPlan {
    SearchTiles tiles; int lanes;          // RING: lanes per pixel (2 / 4 / 8 / 16), else 0
    int x0, nx;                            // output columns [x0, x0 + nx) of the tile kernel (GENERIC: every searched column)
    int lx0, lx1, rx0, rx1;                // the border columns [lx0, lx1) and [rx0, rx1)
    BorderPlan border; BorderPlace place;
    const char* variant;                   // "generic_u16", "generic_u32", "generic_dslice_u16", "generic_dslice_u32", "fast_qsad",
};                                         // "fast_ring_qsad", "fast_ring4_qsad", "fast_ring8_qsad", "fast_ring16_qsad"
// planes_contiguous: the right prefiltered planes lie behind the left ones in one allocation, less than 4 GB - 1 MB apart and
// with the same strides (k_search_ring addresses both from the left plane's rows with 32-bit offsets).
SearchPlan plan_search(const BMGeom& g, int n, bool planes_contiguous);
struct SearchSide { hipStream_t stream; hipEvent_t fork, join; };   // where BorderPlace::SIDE runs, and how it leaves and rejoins
// Row strips per frame for the packed search of a batch, chosen by measurement and remembered: the models are right on average,
// but neighbouring strip counts differ by up to 5 % through scheduling effects they cannot see
// (profiles/r01_xcd_mapping_sweep.txt).  The search only writes its own outputs, so timing it a few times on the caller's data
// is harmless.  The key is the SHAPE of the work (frame size, batch, searched columns and rows as counts, not positions): a
// caller that moves a same-sized ROI around (estimator.cpp:53-54) keeps its entry.  A shape is measured the SECOND time it is
// seen -- a caller whose ROI changes size every call never pays the ~30 extra launches and the stream synchronisation -- and
// the table is a 16-entry LRU.  Small batches keep the model.  RTDM_AUTOTUNE=0: off.
struct StripTuner {
    struct Key {
        int W, H, n, ncols, nrows, fuse;
        bool operator==(const Key& o) const { return W == o.W && H == o.H && n == o.n && ncols == o.ncols && nrows == o.nrows && fuse == o.fuse; }
    };
    struct Entry { Key key; int strips; };   // strips: 0 = seen once, not measured yet; -1 = measuring failed
    std::vector<Entry> tuned;                // least recently used first
    long shapes = 0, launches = 0;           // rtdm_bm_get_tuner_stats
    // the strip count to launch the plan's tile kernel with (0: its model's), after timing it on stream s where that is due
    int tune_strips(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n, hipStream_t s);
};
// Issues the plan on `stream` (BorderPlace::SIDE: the border launch on side.stream between side.fork and side.join).
hipError_t launch_search(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n,
                         hipStream_t stream, const SearchSide& side, StripTuner* tuner);
void ring_set_mode(int mode);      // rtdm_debug_search_kernel
void dslice_set_width(int dt);     // rtdm_debug_disparity_slice

// K3 / K4: the row stages behind the search -- the row-local left-right consistency check (+ column masking to the valid
// rectangle; k_lrcheck.hip) and the speckle filter (connected components under |a-b| <= maxDiff, size <= maxSize removed;
// k_speckle.hip).  plan_lrcheck / plan_speckle (k_rows.hip) decide, once per call and without touching the runtime, what
// launch_lrcheck / launch_speckle then issue.  The route table is in DESIGN.md ("K3 / K4: routes").
// The speckle filter's workspace: label / size / runs / headmap n * Ws * H elements each, rowcnt n * H.
struct SpkBuffers { int32_t *label, *size; uint32_t* runs; int32_t* rowcnt; int16_t* headmap; };
// What a row kernel (k_lrcheck*, k_sgm_median) has left in that workspace for the filter: nothing; the rows initialised with
// one int16 head column per pixel (union-find nodes = head positions); the rows initialised with one record per 8-column
// chunk (nodes = run indices).
enum class SpkHeads { NONE, PIXEL, CHUNK };
// k_lrcheck<SPK, uint16_t, uint32_t> / <SPK, int32_t, unsigned long long>, k_lrcheck_vec<SPK, false, 1> / <SPK, true, 1> /
// <true, true, 2>, k_lrcheck_pk<SPK>
enum class LrForm { SCALAR_U16, SCALAR_I32, VEC_WAVE, VEC_HALF, VEC_HALF2, PACKED };
struct LrPlan {
    LrForm form;
    unsigned threads, gy, n;               // block; grid (1, gy, n)
    size_t lds;                            // dynamic LDS
    int maxDiff16, spkDiff;                // kernel arguments: 16 disp12MaxDiff, speckleRange
    SpkHeads heads;                        // what the launch leaves for the speckle filter (NONE: the SPK = false instantiation)
    int block_rows;                        // CHUNK: the pairs inside blocks of that many rows, from g.vy0, are merged (1: none)
};
// The contacts k_lrcheck_vec<.., NIT > 1> has found: row pairs (y - 1, y) inside its blocks of `blk` rows, `nrows` rows counted
// from vy0, `nch` chunks per row; `blocks` workgroups of 256 items cover them.
struct MergeRecArgs { int blocks, vy0, nrows, blk, nch; };
// k_spk_merge (rows that are not aligned); k_spk_merge_strip<4, false>, <1 | 2 | 4, true>, <1, true, true>
enum class SpkMerge { NONE, ROWS, STRIP4_PIXEL, STRIP1_CHUNK, STRIP2_CHUNK, STRIP4_CHUNK, STRIP1_CHUNK_REC };
struct SpkPlan {
    int W, Ws, H, n;                       // Ws: row stride of label / size / runs / headmap (>= W)
    size_t init_lds;                       // k_spk_init's dynamic LDS; 0: the caller's row kernel has initialised the rows
    SpkHeads heads;                        // PIXEL or CHUNK (count / apply: DENSE)
    MergeRecArgs rec_own, rec_fused;       // k_spk_merge_rec as a launch of its own / in the first workgroups of the strip form
                                           // (blocks == 0: not there)
    SpkMerge merge;
    int merge_gx;                          // its grid (merge_gx, n)
    int first, npairs, ystep;              // row pairs (y, y + 1), y = first + k * ystep, k < npairs
    int rows_gx;                           // grid of count and apply
};
// The pointer-dependent conditions of the 128-bit row kernels, evaluated by the callers so that the plans stay pure: base,
// pitch and frame stride of the plane 16-byte aligned, its rows at least W rounded up to 8 long (a ragged last chunk is
// masked in registers; it needs padding columns that belong to the plane), and the cost plane and head map, where the kernel
// at hand moves them in 128-bit accesses too (K3; the merge kernels of K4 pass null), 16-byte aligned.
inline bool rows_aligned(Plane16W disp, const void* cost, const void* headmap, int W)
{
    return (((size_t)disp.base | (disp.pitch_e * 2) | (disp.frame_e * 2) | (size_t)cost | (size_t)headmap) & 15) == 0 &&
           disp.pitch_e >= (size_t)((W + 7) & ~7);
}
// speckle: the speckle filter's per-row init runs on the checked row in the same pass (the launch needs the workspace).
LrPlan plan_lrcheck(const BMGeom& g, int disp12MaxDiff, int spkDiff, int n, bool speckle, bool aligned);
void launch_lrcheck(const LrPlan& plan, Plane16W disp, const void* cost, const BMGeom& g, const SpkBuffers& wk, hipStream_t stream);
// heads != NONE: the rows [y_lo, y_hi) were initialised by the caller's row kernel (rowcnt zeroed beforehand), every other row
// is entirely newVal, and (CHUNK) the pairs inside blocks of block_rows rows are merged.  NONE: k_spk_init does every row.
SpkPlan plan_speckle(int W, int Ws, int H, int n, SpkHeads heads, int block_rows, int y_lo, int y_hi, bool aligned);
void launch_speckle(const SpkPlan& plan, Plane16W disp, const SpkBuffers& wk, int newVal, int maxSize, int maxDiff, hipStream_t stream);
// n frames of W x H int16: src -> dst (any pitches)
void launch_copy16(Plane16W src, Plane16W dst, int W, int H, int n, hipStream_t stream);

// The row stage under per-frame ROIs from device memory (k_bm_rois.hip, rules B1-B6 in DESIGN.md section 4.19).  d_rois: n x
// (x, y, w, h) ints on the device; a frame with w <= 0 or h <= 0 is skipped: neither kernel touches it.  G: rtdm_bm_geom.h.
// launch_roi_mask: every element of `disp` (the handle's internal plane: 16-byte aligned rows of W rounded up to 8 elements)
// outside the frame's own rectangle becomes `filtered` -- SEARCHED: [cx0, cx1) x [vy0, vy1), what the frame's own restricted
// search would have written; VALID: its valid rectangle; BOTH: their intersection (the left-right check is off).
struct BMRoiGeom;
enum class RoiMask { SEARCHED, VALID, BOTH };
void launch_roi_mask(RoiMask what, Plane16W disp, const BMRoiGeom& G, const int* d_rois, int n, int filtered, hipStream_t stream);
// launch_copy16 for the frames that are not skipped
void launch_copy16_rois(Plane16W src, Plane16W dst, int W, int H, int n, const int* d_rois, hipStream_t stream);

// K5: erode / dilate / dilate / erode with the 10x10 ellipse; tmp = n*W*H bytes scratch.
void launch_morph_open_close(Plane8 in, Plane8W out, uint8_t* tmp0, uint8_t* tmp1, int W, int H,
                             int n, hipStream_t stream);
// The general morphology path (k_morph_general.hip, rules M1-M7 in DESIGN.md section 4.14): any element up to 63 x 63, the
// operations of cv::morphologyEx plus OPEN_CLOSE, 1..16 iterations; one launch per erosion / dilation.  The element travels
// BY VALUE in the kernel arguments as one 64-bit word of members per row (a launch in flight never sees a later setting);
// the workgroup expands it into its run table.  nruns, kmax: what morph_element_bits counted (runs of all rows; log2 of the
// longest run, rounded down).
#define MORPH_MAX_SIZE 63
struct MorphBits { unsigned long long rows[MORPH_MAX_SIZE]; int w, h, ax, ay, nruns, kmax; };
// mask: w x h bytes with pitch w, 1 <= w, h <= MORPH_MAX_SIZE; false = no member at all.  (Plain host code, inline so that
// tests/morph_bits_host.cpp can run it under the sanitizers.)
inline bool morph_element_bits(const uint8_t* mask, int w, int h, int ax, int ay, MorphBits* out)
{
    MorphBits b{};
    b.w = w; b.h = h; b.ax = ax; b.ay = ay;
    int longest = 0;
    for (int i = 0; i < h; ++i) {
        int run = 0;
        for (int j = 0; j < w; ++j) {
            if (mask[i * w + j]) {
                b.rows[i] |= 1ull << j;
                if (!run) ++b.nruns;
                if (++run > longest) longest = run;
            } else run = 0;
        }
    }
    while (longest >> (b.kmax + 1)) ++b.kmax;
    *out = b;
    return b.nruns > 0;
}
// tmp0 / tmp1: n * W * H bytes each.  in.base == out.base (with equal strides) is served; other overlaps are not.
hipError_t launch_morph_general(int op, int iterations, const MorphBits& el, Plane8 in, Plane8W out, uint8_t* tmp0, uint8_t* tmp1,
                                int W, int H, int n, hipStream_t stream);

// SGM-8 (BASELINE config 5).  Cost volumes live on the column domain [x0, x0+W1).
struct SGMGeom { int W, H, D, minD, x0, W1; };
struct SGMBuffers {
    uint8_t *gl, *gr;        // Birchfield-Tomasi bounds of gradient and intensity, 2 x uchar4 per pixel  [n][H][W]
    uint8_t *cl, *cr;        // the same for colour frames, one uint2 per channel: 24 bytes per pixel [n][H][W][3] (or null:
                             // allocated by the first colour call)
    uint8_t* pix;            // pixel cost                 [n][H][W1][D]
    uint16_t *C, *S;         // block cost, aggregated     [n][H][W1][D]
    uint16_t* S2;            // the (-1, 0) direction's path costs where the two horizontal directions run side by side (or null)
    uint16_t* Cw;            // MODE_SGBM_3WAY: the warm-up block costs C' (T3)  [n][3][min(blockSize / 2, H)][W1][D], set per call
    int32_t *label, *size, *rowcnt; uint32_t* runs; int16_t* headmap;   // speckle filter workspace
    int32_t* ovf;            // set to 1 by the block-cost kernel where a block cost + P2 passes 32767 (windows > 17 only)
    // row-synchronous sweep (k_sgm_sweep): edge ring between neighbouring strips, give-up flag (page-locked, host readable),
    // the handle's launch counter (tags of the ring words)
    unsigned long long* ring; size_t ring_words;
    int32_t* abortf; uint32_t* epoch;
    void *ev_in, *ev_out;    // hipEvent_t: the caller's stream -> the process's sweep stream -> the caller's stream
};
size_t sgm_ring_words(int maxW, int D, int max_batch);
// What the last path pass leaves per pixel for k_sgm_lrfinal: {x16 disparity or INV, integer winner + minD or minD - 1,
// minimum cost, 0}
struct SgmWin { int16_t d16, bd; uint16_t mins, pad; };
void sgm_wide_set_mode(int m);     // rtdm_debug_sgm_wide_paths
int sgm_wide_mode();
// The cost stage (k_sgm_cost.hip) of n pairs as plan_sgm_cost (rtdm_sgm_cost_plan.h; DESIGN.md "SGM: cost routes") planned it:
// bounds or census descriptors, pixel cost and block sum -> b.C, under MODE_SGBM_3WAY the warm-up costs -> b.Cw as well
void launch_sgm_cost(const SgmCostPlan& p, Plane8 L, Plane8 R, const SGMGeom& g, const SGMBuffers& b, int n, hipStream_t stream);
// The path passes between the cost stage and the winners' left-right check.  plan_sgm (k_sgm.hip) decides, once per call and
// without touching the runtime, what launch_sgm then issues; the route table is in DESIGN.md ("SGM: routes").  Directions are
// indexed 0..7 = (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,1) (1,-1) (-1,-1): paths 4 runs 0..3, paths 5 those with dy >= 0, paths 8 all,
// paths 3 (MODE_SGBM_3WAY, through rtdm_sgm_set_mode only) 0..2 with (0,1) cut into stripes.
//   WIDE    k_sgm_wide, one direction, `waves` (1 / 4) waves per line: D > 256 or rtdm_debug_sgm_wide_paths
//   PATH_H  k_sgm_path_h, one direction; s2: (dx, 0) -> S and (-dx, 0) -> S2 side by side
//   VERT    k_sgm_vert over (0, dy); s2: S2 is added to S on the way
//   SWEEP   k_sgm_sweep over (0, dy), (+1, dy), (-1, dy), `cols` (1 / 2 / 4) columns per half-wave, `strips` strips per frame,
//           `items` = n strips on `grid` workgroups; s2: S2 is added to S on the way
//   ADD_S2  k_sgm_add_s2: S = min(S + S2, 32767)
//   VERT3   k_sgm_vert3 over (0, 1) in the four row stripes of MODE_SGBM_3WAY (paths 3, rules T1-T8 of DESIGN.md section 4.21),
//           always the last pass; s2: S2 is added to S on the way
// first: S is written, not added to; last: the pass decides the winners instead of writing S.
enum class SgmStep { WIDE, PATH_H, VERT, SWEEP, ADD_S2, VERT3 };
struct SgmPass {
    SgmStep step;
    int dir, dx, dy;                       // direction index and vector (ADD_S2: -1, 0, 0)
    bool first, last, s2;
    int cols, strips, items, grid;         // SWEEP
    int waves;                             // WIDE
};
struct SgmPlan {
    SgmPass pass[8]; int npasses;
    const char* variant;                   // "sweep", "half", "vert", "wide_w1", "wide_w4", "vert3"
};
// What a plan may use of the handle and the device, filled by the caller: sweep -- the handle may run k_sgm_sweep (edge ring
// and both events there, give-up flag clear); s2 -- S2 exists; cap -- the workgroups the device holds at once of the
// k_sgm_sweep instantiations of the handle's numDisparities class, [LAST][columns 1 / 2 / 4][ADD2] (sgm_sweep_caps; <= 0: unusable).
struct SgmLimits { bool sweep, s2; size_t ring_words; int cap[2][3][2]; };
void sgm_sweep_caps(int D, int paths, bool s2, int cap[2][3][2]);   // asks the runtime: once per handle
// What of a call has been issued already: bit k of dirs -- direction k is in S (or S2); s2_pending -- S2 holds (-1, 0) and has
// not been added to S; swept -- a sweep ran.
struct SgmDone { unsigned dirs; bool s2_pending, swept; };
SgmPlan plan_sgm(const SGMGeom& g, int paths, int n, const SgmLimits& lim, SgmDone done = SgmDone{0, false, false});
// cn: 1 (gray) or 3 (interleaved colour, reads b.cl / b.cr); ftz: R1's ftzero = max(preFilterCap, 15) | 1, at most 127; cost: the pixel
// cost; under SGM_COST_CENSUS ftz is not read and cn is 1.  What the cost stage makes of them, its limit included: plan_sgm_cost.
struct SgmParams { int blockSize, P1, P2, uniq, disp12MaxDiff, speckleWindowSize, speckleRange, cn, ftz; SgmCostKind cost; };
// The cost stage of plan_sgm_cost, the passes of plan_sgm, sgm_finish.  Returns the plan's variant.  A sweep that the runtime refuses before
// anything was launched: the remainder runs as plan_sgm plans it without sweeps.
const char* launch_sgm(Plane8 L, Plane8 R, Plane16W disp, const SGMGeom& g, const SGMBuffers& b, const SgmLimits& lim, int paths,
                       int n, hipStream_t stream, SgmParams p);
void sgm_cost16_set(int on);       // rtdm_debug_sgm_cost16
bool sgm_cost16_forced();

// Depth statistics after the matcher (estimator.cpp:75-77, 206-263).  q = the 4x4 reprojection matrix Q, row major.
struct DepthQ { double q[16]; };
size_t depth_scratch_bytes(int max_regions, int maxH);
// h_regions: n x (x, y, w, h) on the host, inside the image; rows of a region are summed by one workgroup each
// (maxH >= the tallest region).  Results arrive in h_mean / h_counts after the stream is synchronised.  reuse_min: the
// map's minimum is still in `scratch` from the call before on the same stream, map and scratch (another mask, other regions).
void launch_depth_stats(const int16_t* disp, size_t pitch_e, int W, int H, const DepthQ& q, const uint8_t* mask, size_t mpitch,
                        const int* h_regions, int n, int maxH, double unit, void* scratch, double* h_mean, int* h_counts,
                        hipStream_t stream, bool reuse_min = false);

// The same statistics for n frames whose object lists lie on the device (k_depth_objects.hip, rules D1-D6 in DESIGN.md section
// 4.16).  Travels BY VALUE in the kernel arguments.  disp: frame f at disp + f * dframe_e (elements); mask: plane f * K + c at
// mask + (f * K + c) * mplane (bytes); obj: frame f's list at obj + f * cap; counts: n * K.  nb is set by the launcher.
struct CcObject;
struct DepthObjects {
    const int16_t* disp; size_t dpitch_e, dframe_e;
    const uint8_t* mask; size_t mpitch, mplane;
    const CcObject* obj; const int* counts;
    int n, W, H, K, cap, nb;
};
size_t depth_objects_bytes(int n, int cap, int H);
// mean / npix: n * cap entries on the device, written for the stored objects only.  Three kernels and one memset on `stream`,
// nothing else: no allocation, no synchronisation, no copy.  labels (rule L5): `mask` holds the detector's int32 label planes
// (mpitch / mplane in bytes, multiples of 4) and object i counts the pixels whose label is i + 1; the walk and the sums are the same.
void launch_depth_objects(DepthObjects a, const DepthQ& q, double unit, void* workspace, double* mean, int* npix, hipStream_t stream,
                          bool labels = false);

// Rectification in front of the matcher (estimator.cpp:29-39).  RectifySrc: n RGB frames, pitch/frame in bytes.
struct RectifySrc { const uint8_t* base; size_t pitch, frame; };
void launch_rectify_gray(RectifySrc L, RectifySrc R, const int16_t* map1L, const uint16_t* map2L, const int16_t* map1R,
                         const uint16_t* map2R, int sW, int sH, int rw, int rh, Plane8W outL, Plane8W outR, int n,
                         hipStream_t stream);
void launch_rectify_rgb(RectifySrc S, const int16_t* map1, const uint16_t* map2, int sW, int sH, int rw, int rh, Plane8W out,
                        int n, hipStream_t stream);

// initUndistortRectifyMap (k_rectmap.hip): the entries of the rectangle (rx, ry, rw, rh) of the maps of
// a frame, rh x rw, map1 4-byte aligned.  ir: (P[:3,:3] R)^-1 (calib_rectmap_inverse); k: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4.
// ckpt: rectmap_scratch_bytes(rx, rw, rh) bytes, in use until the launch has finished.
struct RectMapParams { double ir[9]; double fx, fy, u0, v0; double k[12]; };
size_t rectmap_scratch_bytes(int rx, int rw, int rh);
void launch_rectmap(const RectMapParams& P, int rx, int ry, int rw, int rh, double* ckpt, int16_t* map1, uint16_t* map2,
                    hipStream_t stream);

// Object detection that produces the matcher's ROI (estimator.cpp:40-53).  rgb: H x W x 3, R first.
void launch_hsv_inrange(const uint8_t* rgb, size_t pitch, int W, int H, const int lo[3], const int hi[3], uint8_t* mask,
                        size_t mpitch, hipStream_t stream);
size_t cc_scratch_bytes(int W, int H, int max_records);
// records: (first pixel index, x, y, w, h, external) per 8-connected foreground component, in no particular order
void launch_cc_boxes(const uint8_t* mask, size_t mpitch, int W, int H, int zero_border, void* scratch, int max_records,
                     int** d_count, int** d_records, hipStream_t stream);
// Frame batches and colour classes (rules O1-O6).  HsvClasses travels BY VALUE in the kernel
// arguments: nranges ranges (H, S, V inclusive), each owned by class cls[i] < nclasses.
#define HSV_MAX_RANGES 16
#define HSV_MAX_CLASSES 8
struct HsvClasses { int lo[HSV_MAX_RANGES][3], hi[HSV_MAX_RANGES][3], cls[HSV_MAX_RANGES], nranges, nclasses; };
void hsv_tables_ready(hipStream_t stream);   // the conversion's tables of this device are filled (synchronises the first time)
// n frames -> n * nclasses raw class masks, plane f * nclasses + c at mask + (f * nclasses + c) * mplane
void launch_hsv_classes(const uint8_t* rgb, size_t pitch, size_t frame, int n, int W, int H, const HsvClasses& C, uint8_t* mask,
                        size_t mpitch, size_t mplane, hipStream_t stream);
struct CcObject { int x, y, w, h, cls, first_pixel, reserved[2]; };          // rtdm_object
size_t cc_plane_bytes(int W, int H, int max_records);                        // cc_scratch_bytes, rounded up to 64
// Labels the n * nclasses planes (scratch: cc_plane_bytes each) and selects on the device: frame f's kept boxes, class
// ascending and first pixel descending inside a class, at objects + f * capacity (positions >= capacity are not written);
// counts[f * nclasses + c]: kept boxes of the plane; rois: 4 ints per frame, the union box (x, y, w, h) of all of them.
// out (rules L1-L4), both parts optional: labels -- plane f * nclasses + c at labels + plane * lplane
// bytes, rows of lpitch bytes (multiples of 4), 1 + list index on the pixels of the stored objects and 0 elsewhere; stats -- the
// raw moments of those pixels at stats + f * capacity.  With neither the launches are the ones without `out`.
struct CcStats { long long m00, m10, m01, m20, m11, m02; };                  // rtdm_object_stats
struct CcLabelsOut { int32_t* labels; size_t lpitch, lplane; CcStats* stats; };
void launch_cc_objects(const uint8_t* mask, size_t mpitch, size_t mplane, int n, int nclasses, int W, int H, int zero_border,
                       int min_area, void* scratch, int max_records, CcObject* objects, int capacity, int* counts, int* rois,
                       hipStream_t stream, const CcLabelsOut& out = CcLabelsOut{nullptr, 0, 0, nullptr});

// Disparity WLS post-filter (k_wls.hip, rules W1-W8 in DESIGN.md section 4.9).  Internal planes (F, weights, confidence,
// window statistics) share one layout: element (f, y, x) at f * frame + y * pitch + x.
struct WlsDisp { const int16_t* base; size_t pitch_e, frame_e; };
struct WlsGuide { const uint8_t* base; size_t pitch, frame; int cn; };     // bytes
struct WlsGeom { int x0, x1, y0, y1; };                                      // valid ROI [x0,x1) x [y0,y1)
struct __align__(8) WlsMM { int16_t mn, mx, cnt, pad; };                     // W3 row window: min, max, valid count
struct WlsOut {                                                              // strides in elements; filt / conf may be null
    int16_t* out; size_t out_pitch, out_frame;
    float* filt; size_t filt_pitch, filt_frame;
    float* conf; size_t conf_pitch, conf_frame;
};
#define RTDM_WLS_MAX_ITER 16
struct WlsLaunch {
    WlsDisp dl, dr;                // dr unused when use_conf == 0
    WlsGuide guide;
    WlsOut out;
    WlsGeom g;
    int W, H, r, T, invL, invR, use_conf, num_iter;
    float lambda[RTDM_WLS_MAX_ITER];
    const float* lut;
    size_t pitch, frame;
    float2* F; float *wh, *wv; uint8_t* conf; WlsMM *mmL, *mmR;
};
void launch_wls(const WlsLaunch& L, int n, hipStream_t stream);

// reprojectImageTo3D and the point cloud (k_xyz.hip, rules X1-X8 in DESIGN.md section 4.11).  A frame is cut into tiles of
// XYZ_TILE consecutive pixels of its row-major order; minkey holds one int per frame of the launch, tile_cnt
// xyz_tiles(W, H) ints per frame.  Strides are in elements unless the name says bytes.
#define XYZ_TILE 1024
struct XyzParams { double q[16]; double max_z; int mode, hmv, invalid16; };  // invalid16 = (min_disparity - 1) * 16
#define XYZ_MODE_ROUNDED 1       // XyzParams::mode = RTDM_XYZ_ROUNDED: d is the rounded quotient, calc_depth's (0: RTDM_XYZ_FIXED16)
struct XyzDisp { const int16_t* base; size_t pitch_e, frame_e; };
struct XyzMap { float* xyz; size_t xyz_pitch, xyz_frame; float* z; size_t z_pitch, z_frame; };   // either may be null
struct XyzCloudIn {
    XyzDisp disp;
    const uint8_t* guide; size_t gpitch, gframe; int cn;                     // bytes; cn 0: no guide
    const uint8_t* mask; size_t mpitch, mframe;                              // null: every pixel passes
};
struct XyzRec { float x, y, z; uint32_t rgba; };                             // rtdm_point: r in the lowest byte
int xyz_tiles(int W, int H);
// X4: minkey[f] = the smallest key (xyz_key of `mode`) of frame f, for any n and any frame size: one memset and one kernel
// (one more for every further 32768 frames).  The one frame minimum: of the map and the cloud, of calc_depth and the
// per-object depth (ROUNDED keys: the rounded disparity) and of the measurements.
void launch_xyz_min(XyzDisp D, int n, int W, int H, int mode, int* minkey, hipStream_t stream);
// (the map and the cloud: n <= 65535, W * H < 2^31)
void launch_xyz_map(XyzDisp D, int n, int W, int H, const XyzParams& P, int* minkey, XyzMap O, hipStream_t stream);
// counts: n ints (device), the kept pixels of every frame; records at or beyond `capacity` are not written
void launch_xyz_cloud(const XyzCloudIn& I, int n, int W, int H, const XyzParams& P, int* minkey, int* tile_cnt, XyzRec* points,
                      size_t points_frame_b, int capacity, int* counts, hipStream_t stream);

// Per-object measurements (k_measure.hip, rules G1-G10 in DESIGN.md section 4.18): Z quantiles, extent and centre of every
// stored object of the detector's device lists.  `a` as for launch_depth_objects (a.mask: mask bytes, or with `labels` the
// int32 label planes); P: Q, max_z and mode are used, X4 is always on.  out: n * cap records, written for the stored objects
// only.  One memset and the launches of launch_xyz_min, k_meas_bands, k_meas_final and -- with quantiles -- k_meas_select on
// `stream`, nothing else: no allocation, no synchronisation, no copy, and every grid is sized from n, cap, H and nquant.
struct MeasRecord { int32_t npix, nplane; float zq[8]; float lo[3], hi[3]; double mean[3]; };   // rtdm_object_measure
struct MeasQuant { int nquant; int permille[8]; };
size_t measure_bytes(int n, int cap, int H, int nquant);
void launch_measure(DepthObjects a, const XyzParams& P, const MeasQuant& mq, void* workspace, MeasRecord* out, hipStream_t stream,
                    bool labels);

// Baseline MJPEG frames (k_mjpeg.hip, rules J1-J5 in DESIGN.md section 4.12): m frames of one geometry and sampling (`shape`:
// any of their descriptors), descriptors, segment table and stream bytes on the device.  d_coef: m * blocks * 64 int16,
// ZEROED by the caller; d_planes: m * blocks * 64 bytes; d_status: m ints, zeroed by the caller, MJ_BAD_STREAM where the
// entropy data of a frame is damaged.  max_nseg: the largest segment count among the frames.  (Types: rtdm_mjpeg.h.)
// split: which frames k_mjpeg_huff_split decodes -- those of ONE segment that `bytes` per subsequence (mjpeg_split_plan) cut into
// two subsequences or more; the caller has counted them (`frames` of the m, the most subsequences of one: max_nsub).  totals
// (two counters: frames, subsequences) and max_rounds (device) are added to by that kernel.
struct MjpegDesc;
struct MjpegSeg;
struct MjpegSplitCall { uint32_t bytes; int frames; uint32_t max_nsub; unsigned long long* totals; int* max_rounds; };
void launch_mjpeg(const uint8_t* d_streams, const MjpegDesc* d_desc, const MjpegSeg* d_segs, int m, const MjpegDesc& shape,
                  unsigned max_nseg, const MjpegSplitCall& split, int16_t* d_coef, uint8_t* d_planes, uint8_t* d_rgb, size_t pitch,
                  size_t frame_stride, int* d_status, hipStream_t stream);

// Synthetic stream generator (bit-identical to synth.py).
void launch_synth(uint64_t seed, int first_frame, int n, int W, int H, int D, Plane8W L, Plane8W R,
                  void* param_scratch, hipStream_t stream);
size_t synth_scratch_bytes(int n);

}  // namespace rtdm
