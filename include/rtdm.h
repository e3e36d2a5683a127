/*
 * rtdm.h -- C ABI of the MI355X stereo block-matching module (librtdm_hip.so).
 *
 * This is the drop-in boundary for the hot path of wafgo/rt-depth-map: a HIPMatcher class that
 * derives from the reference's BlockMatcher (include/stereo-matcher/stereo-matcher.h:13-19) and
 * sits next to SWMatcherKonolige / HWMatcherDisparityCoprocessor calls exactly these entry points
 * (the adapter is rt-depth-map_amd/host/bm-hip.{h,cpp}; INTEGRATION.md shows the three-line
 * change to main.cpp:134 and the Makefile.build rule).  Plain C types only: no OpenCV, no torch.
 *
 * Every function returns RTDM_OK (0) or a negative rtdm_status; nothing throws or aborts.  The
 * library has NO CPU fallback: without a usable HIP device every create call fails with
 * RTDM_ERR_NO_DEVICE.
 */
#ifndef RTDM_H_
#define RTDM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTDM_ABI_VERSION 3   /* 2: rtdm_bm_params.legacy_right_clamp, rtdm_bm_get_tuner_stats; 3: rtdm_sgm_get_pass_stats;
                                * additions that only add entry points and types (rtdm_xyz_*, rtdm_mjpeg_*, rtdm_calib_load ..
                                * rtdm_rectify_create_calib) change nothing for an existing caller and keep the number */

typedef enum rtdm_status {
    RTDM_OK = 0,
    RTDM_ERR_BAD_PARAM = -1,   /* what cv::StereoBM::compute rejects with cv::Exception */
    RTDM_ERR_BAD_SIZE = -2,    /* frame larger than the handle was created for, bad pitch ... */
    RTDM_ERR_NO_DEVICE = -3,
    RTDM_ERR_HIP = -4,         /* a HIP runtime call failed; see rtdm_last_hip_error() */
    RTDM_ERR_NOMEM = -5,
    RTDM_ERR_UNSUPPORTED = -6, /* valid for OpenCV but outside what this build implements */
    RTDM_ERR_NULL = -7,
    RTDM_ERR_BAD_STREAM = -8   /* a JPEG stream that is damaged or incomplete (rtdm_mjpeg_*); a calibration file that
                                * cannot be read or breaks the syntax (rtdm_calib_load) */
} rtdm_status;

/* Same nine knobs SWMatcherKonolige's constructor forwards to cv::StereoBM
 * (stereo-matcher/bm-sw.cpp:16-25; literals at main.cpp:134-135).  preFilterType and preFilterSize,
 * which the reference leaves at cv::StereoBM's defaults (XSOBEL, 9), are set with rtdm_bm_set_prefilter. */
typedef struct rtdm_bm_params {
    int preFilterCap;      /* 1..63 */
    int blockSize;         /* odd, 5..255, smaller than min(width,height) */
    int minDisparity;      /* >= -2047 and minDisparity + numDisparities <= 2047: the x16 output is 16 bits wide */
    int numDisparities;    /* > 0, multiple of 16, minDisparity + numDisparities <= 2047 (so up to 4080); every such value is
                            * served -- the only RTDM_ERR_UNSUPPORTED left for BlockMatcher is max_width > 4096 */
    int textureThreshold;  /* >= 0 */
    int uniquenessRatio;   /* >= 0 */
    int speckleWindowSize; /* <= 0 disables the speckle filter */
    int speckleRange;      /* compared unscaled against the x16 fixed-point disparities */
    int disp12MaxDiff;     /* < 0 disables the left-right check */
    /* 0 (default): the right image's window samples are clamped as in OpenCV 4.x (column <= W - numDisparities, so
     * base + d stays inside the row).  1: the rule of the 3.1-3.2 era the reference links (Makefile.include:18-23):
     * the base is clamped to W - rofs - 1 and base + d runs on into the following bytes of a step == W plane, i.e. into
     * the next row (zeros after the last row).  Only the last blockSize/2 searched columns differ, and they reach the
     * result only as voters of the left-right check (oracle/rtdm_oracle.h, hazard H1).  Still unpinned: no OpenCV here. */
    int legacy_right_clamp;
} rtdm_bm_params;

typedef struct rtdm_bm rtdm_bm;       /* one matcher = one GPU + one HIP stream + its workspace */
typedef struct rtdm_morph rtdm_morph; /* one morphological filter device */

const char* rtdm_strerror(int status);
const char* rtdm_last_hip_error(void);   /* text of the last failing HIP call on this thread */
int rtdm_abi_version(void);
int rtdm_device_count(int* count);
/* Fills the reference's literals: cap 31, block 13, minD 0, texture 10, uniqueness 10,
 * speckle 100/32, disp12MaxDiff 1 (main.cpp:134-135); numDisparities as given. */
void rtdm_bm_default_params(rtdm_bm_params* p, int numDisparities);

/* ---- BlockMatcher ------------------------------------------------------------------------
 * rtdm_bm_create   <- SWMatcherKonolige::SWMatcherKonolige (bm-sw.cpp:12-26); like the FPGA
 *                     matcher (bm-hw-ip.h:74) it is told the frame size up front and owns
 *                     device buffers for max_batch frames of max_width x max_height.
 * rtdm_bm_set_roi  <- SWMatcherKonolige::setROI1 / setROI2 (bm-sw.cpp:40-48); which = 1 | 2;
 *                     a zero-area rectangle means "whole image", as in cv::StereoBM.
 * rtdm_bm_compute  <- SWMatcherKonolige::compute (bm-sw.cpp:33-38): host 8UC1 left/right with
 *                     arbitrary row pitch (the caller passes ROI views, estimator.cpp:33,36),
 *                     host 16SC1 output, fixed point x16, invalid = (minDisparity-1)*16.
 *                     Synchronous.  Pageable planes are gathered through a page-locked staging area;
 *                     planes that are themselves page-locked (hipHostMalloc, hipHostRegister) are
 *                     read and written by DMA in place.
 */
int rtdm_bm_create(const rtdm_bm_params* params, int max_width, int max_height, int max_batch,
                   int device, rtdm_bm** out);
void rtdm_bm_destroy(rtdm_bm* bm);
int rtdm_bm_set_roi(rtdm_bm* bm, int which, int x, int y, int width, int height);
int rtdm_bm_get_params(const rtdm_bm* bm, rtdm_bm_params* out);
/* cv::StereoBM::setPreFilterType / setPreFilterSize, from the next compute call on (every entry point that runs the matcher).
 * A new handle reports (RTDM_PREFILTER_XSOBEL, 9), the library's defaults.  NORMALIZED_RESPONSE is the Konolige prefilter:
 * (4 c + l + r + u + d) * scale_g - (box sum over preFilterSize^2) * scale_s, >> 10, clipped to +-preFilterCap (rules N1-N6,
 * DESIGN.md section 4.10; restated from memory, parity with the library unpinned).  preFilterSize is read by that type only,
 * but checked for both, as cv::StereoBM::compute does: RTDM_ERR_BAD_PARAM for a type other than 0 / 1 and for a size that is
 * even or outside 5 .. 255.  No device synchronisation, no reallocation. */
#define RTDM_PREFILTER_NORMALIZED_RESPONSE 0   /* cv::StereoBM::PREFILTER_NORMALIZED_RESPONSE */
#define RTDM_PREFILTER_XSOBEL 1                /* cv::StereoBM::PREFILTER_XSOBEL, the default */
int rtdm_bm_set_prefilter(rtdm_bm* bm, int preFilterType, int preFilterSize);
int rtdm_bm_get_prefilter(const rtdm_bm* bm, int* preFilterType, int* preFilterSize);
int rtdm_bm_compute(rtdm_bm* bm, const uint8_t* left, size_t left_pitch, const uint8_t* right,
                    size_t right_pitch, int width, int height, int16_t* disp, size_t disp_pitch);

/* Batched stream of independent pairs (BASELINE config 4).  Device-resident variant: frame i
 * of an image lives at base + i*frame_stride, rows `pitch` bytes apart; the work is enqueued on
 * `hip_stream` (a hipStream_t; NULL = the HIP null stream, which is also torch's default stream) and NOT synchronised.  n may
 * exceed max_batch; it is processed in chunks. */
int rtdm_bm_compute_device(rtdm_bm* bm, int n, const uint8_t* d_left, const uint8_t* d_right,
                           size_t pitch, size_t frame_stride, int width, int height,
                           int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                           void* hip_stream);
/* The same with one ROI1 PER FRAME, read from device memory (rules B1-B6): d_roi1 holds n x 4 ints
 * (x, y, w, h).  Frame f's output plane holds, byte for byte, what rtdm_bm_set_roi(bm, 1, roi f) followed by
 * rtdm_bm_compute_device on frame f alone writes -- except that a frame whose rectangle has w <= 0 or h <= 0 is SKIPPED: no
 * byte of its plane is written (deliberately not rtdm_bm_set_roi's meaning of an empty rectangle, "no ROI").  ROI2 is the
 * handle's; the handle's own ROI1 is neither read nor changed.  The rectangles are device data and untrusted: they become the
 * frame's geometry on the device in 64-bit arithmetic, and whatever they hold, nothing is read or written outside the n
 * frames and the handle's workspaces.  The work is enqueued on hip_stream; the call adds no synchronisation, allocation or
 * host copy of its own, and its grids depend on n, width, height and the handle's parameters only.  What it shares with
 * rtdm_bm_compute_device stays what it is there: the strip tuner's one measured (synchronising) call per work shape with 16
 * pairs or more per chunk, the chunks of max_batch, rtdm_bm_search_variant, the stage times (the per-frame masks count as
 * the left-right stage).  Refusals, before any device use: those of rtdm_bm_compute_device in its order, d_roi1 among the
 * pointers of RTDM_ERR_NULL. */
int rtdm_bm_compute_device_rois(rtdm_bm* bm, int n, const uint8_t* d_left, const uint8_t* d_right, size_t pitch,
                                size_t frame_stride, int width, int height, const int* d_roi1 /* n x 4: x, y, w, h */,
                                int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride, void* hip_stream);
/* Host variant: frames in host memory, processed in chunks; returns when `disp` is complete.  If left, right and disp are
 * page-locked (hipHostMalloc / hipHostRegister) the copies are DMA on streams of their own: chunk k+1 comes in and chunk
 * k-1 goes out while chunk k is computed (needs max_batch >= 2).  Pageable memory is staged by the HIP runtime, chunk by
 * chunk. */
int rtdm_bm_compute_batch(rtdm_bm* bm, int n, const uint8_t* left, const uint8_t* right,
                          size_t pitch, size_t frame_stride, int width, int height,
                          int16_t* disp, size_t disp_pitch, size_t disp_frame_stride);
int rtdm_bm_synchronize(rtdm_bm* bm);

/* Per-stage device timing with HIP events on the launching stream (bench.py's roofline leg).
 * Stages: 0 prefilter, 1 SAD search, 2 left-right check, 3 speckle filter. */
#define RTDM_STAGE_PREFILTER 0
#define RTDM_STAGE_SEARCH 1
#define RTDM_STAGE_LRCHECK 2
#define RTDM_STAGE_SPECKLE 3
#define RTDM_NUM_STAGES 4
int rtdm_bm_set_profiling(rtdm_bm* bm, int enabled);
int rtdm_bm_get_stage_time(rtdm_bm* bm, int stage, double* total_ms, long* launches, long* frames);
int rtdm_bm_reset_stage_times(rtdm_bm* bm);
/* Name of the SAD-search kernel variant the current parameters select ("generic_u16", ...). */
const char* rtdm_bm_search_variant(const rtdm_bm* bm);
/* Diagnostic counters of the strip-count tuner inside rtdm_bm_compute_device (it times a few search launches the second
 * time a batch shape is seen): shapes measured so far and the extra search launches that took.  Either pointer may be NULL. */
int rtdm_bm_get_tuner_stats(const rtdm_bm* bm, long* shapes_measured, long* timing_launches);
/* Diagnostic switch, process wide: which of the hand-written search kernels may be chosen for configurations that
 * several cover.  0: k_search_fast only; 1: k_search_ring where it is instantiated; 2 / 4 / 8: as 1, with two / four / eight
 * lanes per pixel where that form of the ring kernel exists; -1 (default): the library's choice.  Results never depend on it. */
void rtdm_debug_search_kernel(int mode);
/* Diagnostic switch, process wide: 0 (default): the library picks the SAD-search kernel and, for the disparity-sliced one
 * ("generic_dslice_*": configurations whose column sums do not fit the generic kernel's LDS, numDisparities > 256 among
 * them), its slice width.  dt > 0: EVERY configuration is searched by the disparity-sliced kernel with slices of dt
 * reversed disparity indices (rounded up to a multiple of 16, capped by numDisparities and by what fits in LDS).  Results
 * never depend on it; it exists so that tests can put slice boundaries anywhere. */
void rtdm_debug_disparity_slice(int dt);

/* ---- VideoFilterDevice (morphological filter; default: open + close, 10x10 ellipse) -------
 * rtdm_morph_create      <- SWMorphologicalFilter::SWMorphologicalFilter (filter/mf-sw.cpp:10-17)
 * rtdm_morph_in_buffer / _out_buffer
 *                        <- VideoFilterDevice::getVideoInBuffer / getVideoOutBuffer
 *                           (filter/filter.cpp:45-53): width*height bytes each, owned by the
 *                           device object, here page-locked host memory.
 * rtdm_morph_run         <- SWMorphologicalFilter::run (filter/mf-sw.cpp:19-28): erode, dilate,
 *                           dilate, erode with MORPH_ELLIPSE 10x10 (mf-sw.h:11-12) unless rtdm_morph_set_op
 *                           chose another operation, element or iteration count.  Synchronous.
 * rtdm_morph_make_element <- cv::getStructuringElement(shape, Size(width, height)) with the default anchor
 *                           (width/2, height/2).  Host only: no device is touched.
 * rtdm_morph_set_op      <- what the reference fixes with MORPH_FILTER_DX / MORPH_FILTER_DY and the four calls of run():
 *                           cv::morphologyEx(src, dst, op, element, anchor, iterations) with the default constant border
 *                           (out-of-image samples never win), plus RTDM_MORPH_OPEN_CLOSE, the reference's own sequence.
 *                           Rules M1-M7, DESIGN.md section 4.14 (restated from memory: parity with the library unpinned).
 *                           Takes effect from the next call on; no reallocation, no device synchronisation; work already
 *                           enqueued keeps the setting it was enqueued with.  A new handle reports
 *                           (RTDM_MORPH_OPEN_CLOSE, 1, ELLIPSE 10x10).  d_out == d_in is served for every operation.
 *                           Every setting but the default passes its intermediate results through the handle's two scratch
 *                           planes: calls of rtdm_morph_run_device on ONE handle must then be ordered by their streams (the
 *                           same stream, or events between them); calls that overlap on different streams race on those
 *                           planes.  The default setting touches no scratch plane and has no such rule.
 *                           Refusals are decided before the handle is looked at: RTDM_ERR_NULL for a NULL element (then
 *                           for a NULL handle); RTDM_ERR_BAD_PARAM for an unknown op (cv::MORPH_HITMISS = 7 included),
 *                           iterations outside 1..16, a side below 1, an anchor outside the element, an all-zero mask;
 *                           RTDM_ERR_UNSUPPORTED for a side above RTDM_MORPH_MAX_SIZE, which the library would take.
 * rtdm_debug_morph_general  Diagnostic switch, process wide: 1 = even the default setting runs the general kernel
 *                           (k_morph_general.hip) instead of the fused 10x10 one; 0 (default) = the library's choice.
 *                           Results never depend on it.
 */
#define RTDM_MORPH_RECT 0      /* cv::MorphShapes */
#define RTDM_MORPH_CROSS 1
#define RTDM_MORPH_ELLIPSE 2
#define RTDM_MORPH_ERODE 0     /* cv::MorphTypes 0..6 */
#define RTDM_MORPH_DILATE 1
#define RTDM_MORPH_OPEN 2
#define RTDM_MORPH_CLOSE 3
#define RTDM_MORPH_GRADIENT 4
#define RTDM_MORPH_TOPHAT 5
#define RTDM_MORPH_BLACKHAT 6
#define RTDM_MORPH_OPEN_CLOSE 100   /* SWMorphologicalFilter::run: open, then close; the default */
#define RTDM_MORPH_MAX_SIZE 63
#define RTDM_MORPH_MAX_ITERATIONS 16
/* mask: width x height bytes, row major with pitch `width`; nonzero = member.  Any mask is legal (several runs per row,
 * empty rows and columns), with the anchor anywhere inside the element. */
typedef struct rtdm_morph_element {
    int width, height, anchor_x, anchor_y;
    uint8_t mask[RTDM_MORPH_MAX_SIZE * RTDM_MORPH_MAX_SIZE];
} rtdm_morph_element;
int rtdm_morph_make_element(int shape, int width, int height, rtdm_morph_element* out);
int rtdm_morph_set_op(rtdm_morph* mf, int op, int iterations, const rtdm_morph_element* el);
int rtdm_morph_get_op(const rtdm_morph* mf, int* op, int* iterations, rtdm_morph_element* el);   /* any pointer may be NULL */
void rtdm_debug_morph_general(int on);
int rtdm_morph_create(int width, int height, int max_batch, int device, rtdm_morph** out);
void rtdm_morph_destroy(rtdm_morph* mf);
uint8_t* rtdm_morph_in_buffer(rtdm_morph* mf);
uint8_t* rtdm_morph_out_buffer(rtdm_morph* mf);
int rtdm_morph_run(rtdm_morph* mf, const uint8_t* in, size_t in_pitch, uint8_t* out,
                   size_t out_pitch, int width, int height);
int rtdm_morph_run_device(rtdm_morph* mf, int n, const uint8_t* d_in, size_t in_pitch,
                          size_t in_frame_stride, uint8_t* d_out, size_t out_pitch,
                          size_t out_frame_stride, int width, int height, void* hip_stream);

/* ---- SWSemiGlobalMatcher counterpart: cv::StereoSGBM (rows S / f4, BASELINE config 5) -------------------
 * rtdm_sgm_create   <- SWSemiGlobalMatcher::SWSemiGlobalMatcher (stereo-matcher/sgbm-sw.cpp:12-25):
 *                      StereoSGBM::create(0, numDisparities, blockSize), P1 = 600, P2 = 2400 (:17-18),
 *                      then the five setters (:19-24).  preFilterCap starts at 0 (=> clip at +-15; rtdm_sgm_set_prefilter_cap
 *                      changes it), mode MODE_SGBM.
 * rtdm_sgm_compute  <- SWSemiGlobalMatcher::compute (sgbm-sw.cpp:32-37); setROI1/2 are no-ops in the
 *                      reference (sgbm-sw.h:32-33), so there is no ROI entry point.  rtdm_sgm_compute_cn also takes
 *                      interleaved three-channel pairs (CV_8UC3), as cv::StereoSGBM::compute does.
 * The algorithm is the restatement of cv::StereoSGBM::compute in oracle/sgm_oracle.c (rules R1-R12 there: pixel cost,
 * block sum, 5 or 8 path directions, saturating sum, winner / uniqueness / sub-pixel, the always-on left-right check,
 * 3x3 median, speckle filter), integer arithmetic, bit-exact against that oracle; parity against the library itself is
 * unpinned (OpenCV is not available where this was built). */
typedef struct rtdm_sgm_params {
    int blockSize;         /* 1..255; an even size runs as the next odd one, as in the library (window = blockSize / 2 either
                            * side).  A pixel cost is at most M = channels * (2 ftzero + 63), ftzero = max(preFilterCap, 15) | 1
                            * (93 for gray at preFilterCap 0).  Where M * window^2 + P2 > 32767 (gray at preFilterCap 0: window
                            * > 17 at P2 = 2400) a block cost + P2 CAN pass
                            * 32767, where the library's 16-bit costs wrap around -- which is not reproduced: a frame in which
                            * it does is refused by the compute call (RTDM_ERR_UNSUPPORTED; it takes nearly every pixel of a
                            * window at the maximum pixel cost), and rtdm_sgm_compute_device synchronises its stream to tell */
    int minDisparity;
    int numDisparities;    /* multiple of 16 (any: above 256 the path passes run on the wide-line kernel, k_sgm_wide.hip, and
                            * the cost volumes cover the column domain only, max_width + min(minD, 0) - max(minD + D, 0)) */
    int P1, P2;            /* as the library: P1 <= 0 -> 2, P2 <= 0 -> 5, P2 >= P1 + 1 */
    int uniquenessRatio;   /* <= 100; < 0 -> 10 */
    int speckleWindowSize; /* <= 0 disables the speckle filter */
    int speckleRange;      /* multiplied by 16, as cv::StereoSGBM does */
    int disp12MaxDiff;     /* <= 0 -> 1: the library's left-right check cannot be switched off */
    int paths;             /* cv::StereoSGBM::setMode by its direction count.  5: MODE_SGBM, the mode sgbm-sw.cpp:15 creates (left,
                            * right, down, down-right, down-left); 8: MODE_HH, all eight neighbours (BASELINE config 5);
                            * 4: MODE_HH4 (OpenCV 3.4 / 4.x), left, right, down, up and no others (rule R4', DESIGN.md section 4
                            * "K6 for MODE_HH4"; restated from memory, parity with the library unpinned like R1-R12).
                            * 3 (MODE_SGBM_3WAY): RTDM_ERR_UNSUPPORTED at creation; the mode is served through
                            * rtdm_sgm_set_mode on a live handle (below).  Any other
                            * value: RTDM_ERR_BAD_PARAM */
} rtdm_sgm_params;
typedef struct rtdm_sgm rtdm_sgm;
/* blockSize as given, minD 0, P1 600, P2 2400 (sgbm-sw.cpp:17-18), uniqueness 10, speckle 100/32,
 * disp12MaxDiff 1 (the literals main.cpp:134-135 passes to the BM matcher), 8 paths. */
void rtdm_sgm_default_params(rtdm_sgm_params* p, int numDisparities, int blockSize);
int rtdm_sgm_create(const rtdm_sgm_params* params, int max_width, int max_height, int max_batch,
                    int device, rtdm_sgm** out);
void rtdm_sgm_destroy(rtdm_sgm* sg);
int rtdm_sgm_compute(rtdm_sgm* sg, const uint8_t* left, size_t left_pitch, const uint8_t* right,
                     size_t right_pitch, int width, int height, int16_t* disp, size_t disp_pitch);
int rtdm_sgm_compute_device(rtdm_sgm* sg, int n, const uint8_t* d_left, const uint8_t* d_right,
                            size_t pitch, size_t frame_stride, int width, int height,
                            int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride, void* hip_stream);
/* How the path directions of this handle's calls have run so far: *sweeps = row-synchronous passes launched (three directions
 * each: k_sgm_sweep), *gave_up = 1 once such a pass has given up waiting for a neighbouring strip (the call that finds this
 * returns RTDM_ERR_HIP once; from then on the handle runs one pass per direction).  Either pointer may be NULL.  A MODE_HH4
 * handle (paths = 4) never runs such a pass -- its vertical directions wait for no other workgroup -- and stays at 0 / 0. */
int rtdm_sgm_get_pass_stats(const rtdm_sgm* sg, long* sweeps, int* gave_up);
/* Name of the path-pass form this handle's last call ran: "sweep" (row-synchronous sweeps), "vert" (MODE_HH4: the two
 * horizontal directions and the column-parallel vertical pass, k_sgm_vert), "half" (half-wave lines, one pass per direction),
 * "wide_w1" / "wide_w4" (the wide-line pass, one wave / four waves per line: numDisparities > 256 or forced); "" before the
 * first call. */
const char* rtdm_sgm_path_variant(const rtdm_sgm* sg);
/* Diagnostic switch, process wide: 0 (default): the library's choice (numDisparities > 256 runs the wide-line pass, one wave
 * per line up to 1024 disparities, four above).  1: EVERY numDisparities runs the wide-line pass, one wave per line where that
 * holds the line (<= 1024), four waves above.  4: every numDisparities runs the wide-line pass with four waves per line.
 * Other values mean 0.  Results never depend on it; it exists so that tests can put lane and wave boundaries anywhere. */
void rtdm_debug_sgm_wide_paths(int lines_per_wave_or_waves);
/* cv::StereoSGBM::setPreFilterCap, from the next compute call on: R1's gradient clip ftzero = max(preFilterCap, 15) | 1
 * (0 and 15 -> 15, 16 -> 17, 63 -> 63).  preFilterCap >= 128: RTDM_ERR_UNSUPPORTED (the library's 8-bit clip table wraps
 * there).  Where a pixel cost can pass 255 (ftzero >= 97, or colour) the cost stage runs on 16-bit pixel costs. */
int rtdm_sgm_set_prefilter_cap(rtdm_sgm* sg, int preFilterCap);
/* rtdm_sgm_compute / rtdm_sgm_compute_device for channels = 1 (exactly those) or 3: interleaved colour, a row holds
 * channels * width bytes, pitches in bytes.  The pixel cost is summed over the channels (R1 generalised: for every channel the
 * clipped x-gradient and the raw value, Birchfield-Tomasi each; cost = sum BT(gradient) + sum (BT(raw) >> 2)), which restates
 * the library's calcPixelCostBT from memory -- parity with the library itself is unpinned.  Other channel counts:
 * RTDM_ERR_BAD_PARAM.  The first colour call of a handle allocates its colour buffers (24 bytes per pixel and image of
 * max_width x max_height x max_batch, plus the host entry point's staging). */
int rtdm_sgm_compute_cn(rtdm_sgm* sg, int channels, const uint8_t* left, size_t left_pitch, const uint8_t* right,
                        size_t right_pitch, int width, int height, int16_t* disp, size_t disp_pitch);
int rtdm_sgm_compute_device_cn(rtdm_sgm* sg, int channels, int n, const uint8_t* d_left, const uint8_t* d_right,
                               size_t pitch, size_t frame_stride, int width, int height,
                               int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride, void* hip_stream);
/* Diagnostic switch, process wide: 1 runs the 16-bit pixel-cost forms on gray frames as well (0, the default: only where a
 * pixel cost can pass 255).  Results never depend on it; it exists so that tests can hold the 16-bit forms against the 8-bit
 * ones.  There is no 16-bit census form: under RTDM_SGM_COST_CENSUS (below) the switch changes nothing. */
void rtdm_debug_sgm_cost16(int on);
/* The pixel cost of a handle, from the next compute call on (like rtdm_sgm_set_prefilter_cap; no allocation, no
 * synchronisation).  RTDM_SGM_COST_BT, the default, is R1.  RTDM_SGM_COST_CENSUS is this project's own and has NO counterpart
 * in cv::StereoSGBM (nothing to be at parity with): the census transform with a Hamming-distance cost, for pairs whose two
 * cameras expose differently -- the result does not change under any strictly increasing intensity mapping of either image.
 * How much a brightness difference costs the BT maps, and what census gains on real pairs, is unmeasured.  Rules (DESIGN.md
 * section 4.20):
 *   N1  descriptor of pixel (x, y) of a gray image I over an odd window census_width x census_height, width in {3, 5, 7, 9},
 *       height in {3, 5, 7}: one bit per offset (i, j) != (0, 0), |i| <= width / 2, |j| <= height / 2, set where
 *       I[clamp(y + j)][clamp(x + i)] < I[y][x] (strict; coordinates clamped into the frame): at most 62 bits
 *   N2  cost(x, y, d) = popcount(descL(x, y) xor descR(x - d - minDisparity, y)) <= M = width * height - 1
 *   N3  R1 is not used: no ftzero, no overwritten border columns; preFilterCap stays stored, has no effect while census is
 *       selected and applies again once the cost is RTDM_SGM_COST_BT
 *   N4  everything after the pixel cost (R3-R12: block sum, paths, saturating sum, winners, left-right check, median, speckle
 *       filter, coerced knobs) is unchanged; where M * window^2 + P2 > 32767 the block costs are checked against 32767 - P2
 *       and a frame that passes it is refused with RTDM_ERR_UNSUPPORTED, as under R1 with its own M
 *   N5  gray only: a compute call with channels = 3 on a census handle returns RTDM_ERR_UNSUPPORTED before any device use
 * sg NULL: RTDM_ERR_NULL; cost neither value, or census with a size outside the sets above: RTDM_ERR_BAD_PARAM (the handle
 * keeps its setting); RTDM_SGM_COST_BT ignores the two sizes.  rtdm_sgm_get_cost: any out pointer may be NULL; the sizes are
 * those of the last accepted census setting (9 x 7 before the first).  The setting is not part of rtdm_sgm_params: a caller
 * that builds a right matcher (rtdm_sgm_right_params) copies it to the right handle, as the adapters do. */
#define RTDM_SGM_COST_BT     0   /* R1, the default */
#define RTDM_SGM_COST_CENSUS 1
int rtdm_sgm_set_cost(rtdm_sgm* sg, int cost, int census_width, int census_height);
int rtdm_sgm_get_cost(const rtdm_sgm* sg, int* cost, int* census_width, int* census_height);
/* cv::StereoSGBM::setMode / getMode on a live handle, with the library's values.  The mode holds from the next compute call on;
 * the call allocates nothing and does not use the device, and a handle that never calls it launches what it launched before.
 * MODE_SGBM, MODE_HH and MODE_HH4 plan exactly as a handle created with paths = 5, 8 or 4 plans with the buffers THIS handle
 * owns: one created with paths = 4 has no edge ring, so its MODE_SGBM and MODE_HH calls run one pass per direction ("half").
 * MODE_SGBM_3WAY is served through this call only -- rtdm_sgm_create with paths = 3 keeps returning RTDM_ERR_UNSUPPORTED -- by
 * rules T1-T8, restated from memory of the library's computeDisparity3WAY (OpenCV 3.4 / 4.x); parity
 * with the library is unpinned, as for R1-R12:
 *   T1  always 4 row stripes, sz = (H + 3) / 4 rows each, ovl = (blockSize / 2 + 1) + (sz + 9) / 10; stripe s = 0 .. 3 has the
 *       output rows [o, e) = [min(s sz, H), min((s + 1) sz, H)) and the first source row a = max(min(s sz - ovl, H), 0)
 *   T2  R1-R3 unchanged except for T3's rows
 *   T3  for y in [a, min(a + blockSize / 2, e)) the vertical window of R3 clamps at the top to row a, not to row 0 (C'); a = 0: C' = C
 *   T4  (1, 0) and (-1, 0) over the whole frame (R4); (0, 1) per stripe, started at row a with L = C'(a); rows [a, o) serve the
 *       recurrence only
 *   T5  S = min(L-> + L<- + Ldown, 32767) on the output rows
 *   T6  R6 and R8 unchanged (min S = 32767 is no winner); no votes (R7) and no left-right check (R9): disp12MaxDiff is
 *       accepted and ignored
 *   T7  R10-R12 unchanged
 *   T8  where M window^2 + P2 > 32767 every block cost the mode reads, every C' included, is checked against 32767 - P2; a frame
 *       that passes it is refused (RTDM_ERR_UNSUPPORTED)
 * Under MODE_SGBM_3WAY rtdm_sgm_path_variant says "vert3" and rtdm_sgm_get_pass_stats does not move; RTDM_SGM_DUAL = 0 keeps its
 * meaning (the second horizontal direction adds into S), RTDM_SGM_SWEEP and rtdm_debug_sgm_wide_paths are ignored.  A frame
 * lower than about 6 (blockSize / 2) rows makes the first such call allocate a buffer for the C' (the call fails if that does).
 * sg NULL (get: or mode NULL): RTDM_ERR_NULL; a value outside 0 .. 3: RTDM_ERR_BAD_PARAM; MODE_SGBM_3WAY on a handle whose
 * numDisparities > 256: RTDM_ERR_UNSUPPORTED; a refused call leaves the mode as it was.  rtdm_sgm_right_params does not carry
 * the mode: the caller copies it to the right handle, as with the cost setting (the adapters do). */
#define RTDM_SGM_MODE_SGBM      0
#define RTDM_SGM_MODE_HH        1
#define RTDM_SGM_MODE_SGBM_3WAY 2
#define RTDM_SGM_MODE_HH4       3
int rtdm_sgm_set_mode(rtdm_sgm* sg, int mode);
int rtdm_sgm_get_mode(const rtdm_sgm* sg, int* mode);

/* ---- the step after the matcher, kept on the device ------------
 * rtdm_bm_compute_depth <- estimator.cpp:56 + 75-77: bm->compute(...); left_disp /= 16.;
 *                          reprojectImageTo3D(left_disp, xyz, Q, true, CV_32F); calc_depth(...) (206-263).
 *                          The disparity map stays in HBM; only mean Z [cm = Z * unit / 10] and the pixel
 *                          count of every region come back (disp may be NULL; if given it also receives the
 *                          x16 map, like rtdm_bm_compute).  Q: 4x4 row major (stereoRectify's Q, main.cpp:92).
 *                          mask: 8UC1 host image (filter_out, estimator.cpp:45); regions: obj_boundings.
 * rtdm_depth_stats_device  the same reduction on a device-resident x16 disparity map and mask. */
typedef struct rtdm_region { int x, y, width, height; } rtdm_region;
#define RTDM_MAX_REGIONS 64
int rtdm_bm_compute_depth(rtdm_bm* bm, const uint8_t* left, size_t left_pitch, const uint8_t* right, size_t right_pitch,
                          int width, int height, const double* Q, const uint8_t* mask, size_t mask_pitch,
                          const rtdm_region* regions, int nregions, double calibration_unit,
                          double* mean_cm, int* counts, int16_t* disp, size_t disp_pitch);
int rtdm_depth_stats_device(int device, const int16_t* d_disp, size_t disp_pitch, int width, int height, const double* Q,
                            const uint8_t* d_mask, size_t mask_pitch, const rtdm_region* regions, int nregions,
                            double calibration_unit, double* mean_cm, int* counts, void* hip_stream);
/* rtdm_depth_objects_device: the same reduction for n frames whose object lists lie in device memory as
 *                          rtdm_objects_detect_device leaves them (rules D1-D6).  Frame f has total_f =
 *                          sum over c of max(d_counts[f * nclasses + c], 0) objects, the first min(total_f, capacity) of them at
 *                          d_objects + f * capacity; object i is measured over its box (intersected with the frame) where mask
 *                          plane f * nclasses + cls (at d_masks + plane * mask_plane_stride) is non-zero, against disparity map
 *                          f (at d_disp + f * disp_frame_stride bytes) and that map's own minimum.  d_mean_cm[f * capacity + i]
 *                          and d_npix[f * capacity + i] receive the result; entries at or beyond min(total_f, capacity) are
 *                          left untouched.  There is no limit on the number of objects.  An object whose cls lies outside
 *                          [0, nclasses) or whose clipped box is empty gets npix 0 and mean 0.0; no list content makes the
 *                          kernels read outside the maps, planes and lists.  Bit-identical run to run and independent of n,
 *                          of the frame's position, of capacity and of the other objects.  Enqueued on hip_stream: the call
 *                          never synchronises, allocates or copies to the host; Q is read before it returns.  d_workspace: at
 *                          least rtdm_depth_objects_workspace_bytes(n, capacity, height) bytes of device memory, the call's own
 *                          until its work has finished (that function needs no device and grows with each argument).
 *                          n = 0 is RTDM_OK.  Refusals, before any device use: RTDM_ERR_NULL (d_disp, Q, d_masks, d_counts,
 *                          d_mean_cm, d_npix, d_workspace; d_objects with capacity > 0), RTDM_ERR_BAD_SIZE (n < 0, capacity < 0,
 *                          width or height <= 0, an odd disp_pitch or disp_frame_stride, disp_pitch < 2 * width, mask_pitch <
 *                          width, a frame stride below disp_pitch * height or a plane stride below mask_pitch * height where
 *                          a second frame or plane follows), RTDM_ERR_BAD_PARAM (nclasses outside 1 .. RTDM_MAX_CLASSES),
 *                          RTDM_ERR_BAD_SIZE (workspace_bytes too small). */
struct rtdm_object;
size_t rtdm_depth_objects_workspace_bytes(int n, int capacity, int height);
int rtdm_depth_objects_device(int device, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                              int width, int height, const double* Q, const uint8_t* d_masks, size_t mask_pitch,
                              size_t mask_plane_stride, int nclasses, const struct rtdm_object* d_objects, int capacity,
                              const int* d_counts, double calibration_unit, double* d_mean_cm, int* d_npix,
                              void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* ---- the step in front of the matcher, on the device --------------
 * rtdm_rectify_create  <- the maps the reference builds once (main.cpp:95-96, initUndistortRectifyMap(..., CV_16SC2,
 *                         map1, map2)): map1 = H x W x 2 int16 (source x, y), map2 = H x W uint16 (fy*32 + fx);
 *                         roi = the crop `roif` applied to every remapped frame (main.cpp:80-85, estimator.cpp:33,36).
 *                         Only the roi part of the maps is kept on the device.
 * rtdm_rectify_gray    <- estimator.cpp:29-36: cvtColor(img[i], gray, CV_RGB2GRAY); remap(gray, rect, map1, map2,
 *                         INTER_LINEAR); rect = rect(roif) for both cameras.  rgb: H x W x 3 bytes, first channel R;
 *                         outputs: roi_h x roi_w bytes.
 * rtdm_rectify_rgb     <- estimator.cpp:38-39: remap(img[0], img_rectified, ...)(roif); out: roi_h x roi_w x 3.
 * rtdm_bm_compute_rgb  <- estimator.cpp:29-36 + 56 in one call: the rectified gray pair never leaves HBM; the
 *                         matcher must have been created for at least roi_w x roi_h.
 * The *_device forms take n contiguous device frames (n x H x W x 3 in, n x roi_h x roi_w out). */
typedef struct rtdm_rectify rtdm_rectify;
int rtdm_rectify_create(const int16_t* map1_left, const uint16_t* map2_left, const int16_t* map1_right,
                        const uint16_t* map2_right, int width, int height, int roi_x, int roi_y, int roi_width,
                        int roi_height, int max_batch, int device, rtdm_rectify** out);
void rtdm_rectify_destroy(rtdm_rectify* rc);
int rtdm_rectify_gray(rtdm_rectify* rc, const uint8_t* rgb_left, size_t left_pitch, const uint8_t* rgb_right,
                      size_t right_pitch, uint8_t* left_rect, size_t left_rect_pitch, uint8_t* right_rect,
                      size_t right_rect_pitch);
int rtdm_rectify_rgb(rtdm_rectify* rc, int which /* 0 = left maps, 1 = right maps */, const uint8_t* rgb, size_t pitch,
                     uint8_t* out, size_t out_pitch);
int rtdm_rectify_gray_device(rtdm_rectify* rc, int n, const uint8_t* d_rgb_left, const uint8_t* d_rgb_right,
                             uint8_t* d_left_rect, uint8_t* d_right_rect, void* hip_stream);
int rtdm_bm_compute_rgb(rtdm_bm* bm, rtdm_rectify* rc, const uint8_t* rgb_left, size_t left_pitch,
                        const uint8_t* rgb_right, size_t right_pitch, int16_t* disp, size_t disp_pitch);
int rtdm_bm_compute_rgb_device(rtdm_bm* bm, rtdm_rectify* rc, int n, const uint8_t* d_rgb_left,
                               const uint8_t* d_rgb_right, int16_t* d_disp, void* hip_stream);

/* ---- rectification from the calibration files (main.cpp:53-98, get_rectified_remap_matrices) ---------------------------------
 * rtdm_calib_load            <- FileStorage(intrinsics.yml / extrinsics.yml): the subset of OpenCV's YAML 1.0 those files use
 *                               (`name: !!opencv-matrix` with rows / cols / dt: d / data, `name: [ a, b, c, d ]`, `name: scalar`;
 *                               unknown keys are skipped).  Required: M1 D1 M2 D2 R T; a D of 4, 5, 8, 12 or 14 entries is
 *                               zero-padded to 14.  Optional: Width Height ROI1 ROI2 R1 R2 P1 P2 Q -- what the calibration tool
 *                               stored; *stored_mask says which were there (RTDM_CALIB_HAS_*; the others are zero; width /
 *                               height are 0 when absent).  stored and stored_mask may be NULL.  RTDM_ERR_BAD_STREAM: a file
 *                               that cannot be read, is longer than 1 MiB or breaks the syntax; RTDM_ERR_BAD_PARAM: a missing
 *                               required key, a matrix of another shape or element type, rows * cols unlike the data count.
 * rtdm_stereo_rectify        <- cv::stereoRectify(M1, D1, M2, D2, size, R, T, R1, R2, P1, P2, Q, flags, alpha, new_size, &roi1,
 *                               &roi2), rules C1-C9 of DESIGN.md section 4.13.  With alpha = 1 and RTDM_CALIB_ZERO_DISPARITY the
 *                               result is pinned to what the library itself returned for the reference's three calibrations
 *                               (recorded in their extrinsics.yml: ROIs and P1 exact, the rest within 1e-12); every other alpha,
 *                               the reference's own -1 (main.cpp:92) among them, rests on the same restated rules.  flags: 0 or
 *                               RTDM_CALIB_ZERO_DISPARITY, otherwise RTDM_ERR_BAD_PARAM, as is an R that is no rotation
 *                               (|R^T R - I| > 1e-6) and a zero baseline.  RTDM_ERR_UNSUPPORTED: a new size other than 0 x 0 or
 *                               the image size, tilt coefficients (D[12], D[13]), a rotation by pi between the cameras.
 * Both are host code: they work with no device present.
 * rtdm_undistort_rectify_map <- initUndistortRectifyMap(M, D, R, P, size, CV_16SC2, map1, map2) on the device: map1 = height x
 *                               width x 2 int16, map2 = height x width uint16, the maps rtdm_rectify_create takes; M, R: 3 x 3,
 *                               D: 14, P: 3 x 4, row major.  The ray is accumulated along the row as the library's scalar loop
 *                               does; bit-identical run to run.  Checked before any device use: RTDM_ERR_BAD_SIZE outside 1 ..
 *                               32767, RTDM_ERR_BAD_PARAM for a singular P[:3,:3] R or a non-finite entry, RTDM_ERR_UNSUPPORTED
 *                               for tilt.  The _device form writes device maps (d_map1 4-byte aligned) through hip_stream; both
 *                               forms return when the maps are complete.
 * rtdm_rectify_create_calib  <- main.cpp:95-96 + 80-85: both cameras' maps are built in device memory (only their roi part) and
 *                               never exist on the host; the handle is what rtdm_rectify_create gives for the same maps. */
typedef struct rtdm_calib { double M1[9], D1[14], M2[9], D2[14], R[9], T[3]; int width, height; } rtdm_calib;
typedef struct rtdm_rectification { double R1[9], R2[9], P1[12], P2[12], Q[16]; rtdm_region roi1, roi2; } rtdm_rectification;
#define RTDM_CALIB_ZERO_DISPARITY 1024   /* cv::CALIB_ZERO_DISPARITY */
#define RTDM_CALIB_HAS_WIDTH 1
#define RTDM_CALIB_HAS_HEIGHT 2
#define RTDM_CALIB_HAS_ROI1 4
#define RTDM_CALIB_HAS_ROI2 8
#define RTDM_CALIB_HAS_R1 16
#define RTDM_CALIB_HAS_R2 32
#define RTDM_CALIB_HAS_P1 64
#define RTDM_CALIB_HAS_P2 128
#define RTDM_CALIB_HAS_Q 256
int rtdm_calib_load(const char* intrinsics_path, const char* extrinsics_path, rtdm_calib* calib, rtdm_rectification* stored,
                    unsigned* stored_mask);
int rtdm_stereo_rectify(const rtdm_calib* calib, int flags, double alpha, int new_width, int new_height,
                        rtdm_rectification* out);
int rtdm_undistort_rectify_map(const double* M, const double* D, const double* R, const double* P, int width, int height,
                               int device, int16_t* map1, uint16_t* map2);
int rtdm_undistort_rectify_map_device(const double* M, const double* D, const double* R, const double* P, int width, int height,
                                      int device, int16_t* d_map1, uint16_t* d_map2, void* hip_stream);
int rtdm_rectify_create_calib(const rtdm_calib* calib, const rtdm_rectification* rect, int roi_x, int roi_y, int roi_width,
                              int roi_height, int max_batch, int device, rtdm_rectify** out);

/* ---- the object detection that yields the matcher's ROI ---------------
 * rtdm_objects_detect <- estimator.cpp:40-53: cvtColor(RGB2BGR) + cvtColor(BGR2HSV) + inRange(low, high) -> filter_in;
 *                        morphFilter->run(filter_in, filter_out); findContours(RETR_EXTERNAL) + boundingRect per contour,
 *                        boxes below min_area dropped (fill_bounding_rects_of_contours, estimator.cpp:167-174); roi = union
 *                        of the boxes (find_relevant_matching_region, estimator.cpp:176-204).  rgb = the rectified colour
 *                        crop (height x width x 3, R first).  boxes come in the order of the reference's obj_boundings;
 *                        *nboxes = how many there are (only max_boxes are stored).  zero_border = 1 restates
 *                        OpenCV <= 3.1's findContours, which clears the outermost rows/columns first; 0 = OpenCV >= 3.2.
 * rtdm_objects_set_morph / _get_morph: the detector's morphFilter setting, exactly as rtdm_morph_set_op / _get_op (same
 *                        values, refusals and default); rtdm_objects_detect and rtdm_estimate_frame filter with it.
 * rtdm_estimate_frame <- one iteration of Estimator::run without capture, decode and drawing (estimator.cpp:29-77):
 *                        raw RGB frames in, per object the box, mean Z [cm] and pixel count out.  Everything between
 *                        stays in HBM; one small read-back (the boxes) decides the matcher's ROI1.  If no box survives
 *                        the matcher is skipped (*nboxes = 0).  At most RTDM_MAX_REGIONS objects get a depth. */
typedef struct rtdm_objects rtdm_objects;
typedef struct rtdm_hsv_range { int low[3], high[3]; } rtdm_hsv_range;   /* H, S, V inclusive; estimator.cpp:110-115: {0,150,0}..{9,255,255} */
int rtdm_objects_create(int width, int height, int device, rtdm_objects** out);
void rtdm_objects_destroy(rtdm_objects* ob);
int rtdm_objects_set_morph(rtdm_objects* ob, int op, int iterations, const rtdm_morph_element* el);
int rtdm_objects_get_morph(const rtdm_objects* ob, int* op, int* iterations, rtdm_morph_element* el);
int rtdm_objects_detect(rtdm_objects* ob, const uint8_t* rgb, size_t pitch, const rtdm_hsv_range* range, int min_area,
                        int zero_border, uint8_t* mask_out, size_t mask_pitch, rtdm_region* boxes, int max_boxes,
                        int* nboxes, rtdm_region* roi);
int rtdm_estimate_frame(rtdm_bm* bm, rtdm_rectify* rc, rtdm_objects* ob, const uint8_t* rgb_left, size_t left_pitch,
                        const uint8_t* rgb_right, size_t right_pitch, const double* Q, const rtdm_hsv_range* range,
                        int min_area, int zero_border, double calibration_unit, rtdm_region* boxes, double* mean_cm,
                        int* counts, int max_boxes, int* nboxes, int16_t* disp, size_t disp_pitch);

/* ---- the same detector on frame batches and for several colour classes per call (rules O1-O6) ----
 * A call names nranges HSV ranges (1 .. RTDM_MAX_HSV_RANGES) and a class range_class[r] in [0, nclasses) for each; every
 * class owns at least one range.  The raw mask of a class is 255 where at least one of its ranges holds (each range by the
 * rule of rtdm_objects_detect: inclusive, no hue wrap-around inside a range -- red is {0..9} OR {170..179}), each class mask
 * is filtered with the handle's morphological setting and labelled like the single mask of rtdm_objects_detect.
 * rtdm_object:           one kept box, its class and first_pixel = y * width + x of the first pixel of its component in
 *                        raster order (what orders a class's list: descending); reserved is written as 0.
 * rtdm_objects_create_batch: a handle that takes up to max_batch (1 .. 64) frames x max_classes (1 .. 8) class planes per
 *                        launch; rtdm_objects_create is create_batch(width, height, 1, 1, ...).  Device memory grows with
 *                        max_batch * max_classes planes of about 30 bytes per pixel.
 * rtdm_objects_detect_device: n device-resident frames (frame f at d_rgb + f * frame_stride, rows of pitch bytes) ->
 *                        frame f's object list at d_objects + f * capacity: the per-class lists, class ascending; the first
 *                        min(total, capacity) entries are stored and the rest of the array is left untouched (d_objects
 *                        needs no more than the alignment of an int).
 *                        d_counts[f * nclasses + c] = kept objects of class c (never clipped to capacity); d_rois[f] = union
 *                        box of all kept objects of the frame (with none: x = y = 1000000, width = height = -2000000, as
 *                        rtdm_objects_detect reports an empty frame).  d_masks (optional): the filtered masks (filter_out),
 *                        plane f * nclasses + c at d_masks + (f * nclasses + c) * mask_plane_stride; only width bytes of a
 *                        row are written.  Enqueued on hip_stream and never synchronised; ranges and range_class are host
 *                        arrays that are read before the call returns.  n may exceed max_batch (chunks); n = 0 is RTDM_OK.
 *                        The work planes belong to the handle: calls that share a handle must be ordered on one stream.
 *                        All outputs are bit-identical from run to run and do not depend on n, on the frame's position, on
 *                        max_batch or on the chunking.  Refusals, before any device use and in this order: RTDM_ERR_NULL
 *                        (ranges, range_class, d_rgb, d_counts, d_rois; d_objects with capacity > 0), RTDM_ERR_BAD_PARAM
 *                        (nranges outside 1 .. 16, nclasses outside 1 .. 8, a class id outside [0, nclasses), a class without a range),
 *                        RTDM_ERR_BAD_SIZE (n < 0, capacity < 0), RTDM_ERR_NULL (the handle), RTDM_ERR_BAD_PARAM (nclasses
 *                        above the handle's max_classes), RTDM_ERR_BAD_SIZE (pitch < 3 * width, mask_pitch < width, a frame
 *                        stride below pitch * height or a plane stride below mask_pitch * height where a second frame or
 *                        plane follows).
 * rtdm_objects_detect_batch: the same with host pointers; synchronous.
 * rtdm_estimate_frame_classes: rtdm_estimate_frame for several classes: ROI1 is the union box over all classes; object i is
 *                        measured over its box where the filtered mask of its own class is non-zero.  *nobjects = how many
 *                        there are; the first min(*nobjects, max_objects) are stored and the first min(*nobjects,
 *                        max_objects, RTDM_MAX_REGIONS) get mean_cm[i] / counts[i].  With one class and one range the boxes,
 *                        means, counts and disparity map are rtdm_estimate_frame's. */
#define RTDM_MAX_HSV_RANGES 16
#define RTDM_MAX_CLASSES 8
typedef struct rtdm_object { int x, y, width, height, cls, first_pixel, reserved[2]; } rtdm_object;
int rtdm_objects_create_batch(int width, int height, int max_batch, int max_classes, int device, rtdm_objects** out);
int rtdm_objects_detect_device(rtdm_objects* ob, int n, const uint8_t* d_rgb, size_t pitch, size_t frame_stride,
                               const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, int min_area,
                               int zero_border, uint8_t* d_masks, size_t mask_pitch, size_t mask_plane_stride,
                               rtdm_object* d_objects, int capacity, int* d_counts, rtdm_region* d_rois, void* hip_stream);
int rtdm_objects_detect_batch(rtdm_objects* ob, int n, const uint8_t* rgb, size_t pitch, size_t frame_stride,
                              const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, int min_area,
                              int zero_border, uint8_t* masks, size_t mask_pitch, size_t mask_plane_stride,
                              rtdm_object* objects, int capacity, int* counts, rtdm_region* rois);
int rtdm_estimate_frame_classes(rtdm_bm* bm, rtdm_rectify* rc, rtdm_objects* ob, const uint8_t* rgb_left, size_t left_pitch,
                                const uint8_t* rgb_right, size_t right_pitch, const double* Q, const rtdm_hsv_range* ranges,
                                const int* range_class, int nranges, int nclasses, int min_area, int zero_border,
                                double calibration_unit, rtdm_object* objects, double* mean_cm, int* counts, int max_objects,
                                int* nobjects, int16_t* disp, size_t disp_pitch);

/* ---- which pixels belong to which object: label planes, pixel moments, own-pixel depth (rules L1-L8) ----
 * rtdm_objects_detect_labels_device: rtdm_objects_detect_device with two more outputs, each optional.
 *                        d_labels: one int32 plane per (frame, class), plane f * nclasses + c at d_labels + plane *
 *                        label_plane_stride bytes, rows of label_pitch bytes.  A pixel holds 1 + i where i is the index, in frame
 *                        f's stored list, of the kept object whose component (8-connected foreground of the filtered class
 *                        plane) contains it; every other pixel holds 0: background, the outermost rows and columns under
 *                        zero_border, components that are enclosed, below min_area or beyond capacity.  Only width ints of a
 *                        row are written.
 *                        d_stats[f * capacity + i]: the raw moments of exactly the pixels that carry object i's label (x, y in
 *                        frame coordinates, exact integers); its centroid is (m10 / m00, m01 / m00).  Entries at or beyond
 *                        min(total_f, capacity) are left untouched.
 *                        Labels and stats are bit-identical from run to run and independent of n, of the frame's position, of
 *                        max_batch and of the chunking.  With both absent the call enqueues what rtdm_objects_detect_device
 *                        enqueues and writes the same bytes.  Refusals: those of rtdm_objects_detect_device in its order, then
 *                        RTDM_ERR_BAD_SIZE (label_pitch < 4 * width or no multiple of 4; a label_plane_stride that is no
 *                        multiple of 4, or below label_pitch * height where a second plane follows; a d_labels that is not
 *                        4-byte aligned; a d_stats that is not 8-byte aligned), then RTDM_ERR_UNSUPPORTED (a handle whose
 *                        width * height * max(width, height)^2 does not fit int64: none that can be created today).
 * rtdm_objects_detect_labels_batch: the same with host pointers; synchronous.
 * rtdm_depth_objects_labels_device: rtdm_depth_objects_device with label planes in place of mask planes: object i of frame f
 *                        is measured over its clipped box where label == i + 1 on plane f * nclasses + cls, so same-class
 *                        pixels of OTHER objects inside its box stay out of its mean.  Everything else is that call's: the
 *                        summation order (an object whose box holds no foreign foreground of its class gets the same bits
 *                        from both), the untouched entries, the workspace (rtdm_depth_objects_workspace_bytes serves both).
 *                        A label is only ever compared, never used as an index: no plane content makes the kernels read
 *                        or write outside.  Refusals: that call's with "mask" read as "label": label_pitch < 4 * width or no
 *                        multiple of 4, a stride that is no multiple of 4, d_labels not 4-byte aligned.
 * rtdm_estimator_set_own_pixels: on != 0: rtdm_estimate_batch and rtdm_estimate_batch_device run the labels form of the
 *                        detector and of the depth call, so every object is measured over its own pixels; objects, counts,
 *                        ROIs and maps are unaffected.  The chunk's label planes (4 bytes per pixel and class plane of the
 *                        detector) are allocated by this call, not per estimate, and freed when it is switched off.  The
 *                        default is 0: nothing changes, allocations included.  Waits for the device. */
typedef struct rtdm_object_stats { int64_t m00, m10, m01, m20, m11, m02; } rtdm_object_stats;
int rtdm_objects_detect_labels_device(rtdm_objects* ob, int n, const uint8_t* d_rgb, size_t pitch, size_t frame_stride,
                                      const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses,
                                      int min_area, int zero_border, uint8_t* d_masks, size_t mask_pitch,
                                      size_t mask_plane_stride, rtdm_object* d_objects, int capacity, int* d_counts,
                                      rtdm_region* d_rois, int32_t* d_labels, size_t label_pitch, size_t label_plane_stride,
                                      rtdm_object_stats* d_stats, void* hip_stream);
int rtdm_objects_detect_labels_batch(rtdm_objects* ob, int n, const uint8_t* rgb, size_t pitch, size_t frame_stride,
                                     const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses,
                                     int min_area, int zero_border, uint8_t* masks, size_t mask_pitch, size_t mask_plane_stride,
                                     rtdm_object* objects, int capacity, int* counts, rtdm_region* rois, int32_t* labels,
                                     size_t label_pitch, size_t label_plane_stride, rtdm_object_stats* stats);
int rtdm_depth_objects_labels_device(int device, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                                     int width, int height, const double* Q, const int32_t* d_labels, size_t label_pitch,
                                     size_t label_plane_stride, int nclasses, const rtdm_object* d_objects, int capacity,
                                     const int* d_counts, double calibration_unit, double* d_mean_cm, int* d_npix,
                                     void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* ---- the whole loop body on frame batches -------------------------------------------------------
 * rtdm_estimator_create: a handle for rtdm_estimate_batch.  It BORROWS the three handles: they must outlive it, live on one
 *                        device and fit together as rtdm_estimate_frame_classes asks (detector and matcher serve the
 *                        rectifier's crop).  It owns the raw frames, the rectified gray pairs and the colour crops of one
 *                        chunk, the object lists and results of a chunk, the depth workspace and page-locked read-back space.
 *                        A chunk is min(max_batch, the matcher's max_batch, the detector's max_batch) frames; capacity: the
 *                        objects of a frame that are stored and measured.  Refusals: RTDM_ERR_NULL (out), RTDM_ERR_BAD_SIZE
 *                        (max_batch < 1, capacity < 1), RTDM_ERR_NULL (a handle), RTDM_ERR_BAD_PARAM (handles of different
 *                        devices), RTDM_ERR_BAD_SIZE (a detector of another size than the crop, a matcher too small for it).
 * rtdm_estimate_batch:   rtdm_estimate_frame_classes for n frame pairs (frame f at rgb + f * frame_stride; n may exceed the
 *                        chunk).  Per chunk: one batched rectification, one detector launch set, ONE read-back of the chunk's
 *                        counts and union boxes, the matcher (consecutive frames with equal union boxes share a launch set
 *                        under that ROI1, every other frame runs under its own), one rtdm_depth_objects_device launch set and
 *                        one download.  objects: frame f's list at objects + f * capacity (the first min(total, capacity)
 *                        entries, every one of them measured: there is no RTDM_MAX_REGIONS limit here); counts[f * nclasses +
 *                        c]: kept objects of class c, never clipped; mean_cm / npix[f * capacity + i]: object i of frame f;
 *                        disp (may be NULL): frame f's x16 map at disp + f * disp_frame_stride bytes.  A frame without objects
 *                        skips the matcher: its counts are 0 and its disp frame and mean_cm / npix entries are left
 *                        untouched, as are the entries past the stored ones, as rtdm_estimate_frame leaves them.  ROI1 of the
 *                        matcher is left at the last frame that had objects, as a loop of single calls leaves it.  Objects,
 *                        counts, npix and maps are those of rtdm_estimate_frame_classes on each frame alone; the means are
 *                        the same sums in another fixed order (rule D3).  Refusals, in the order of
 *                        rtdm_estimate_frame_classes: RTDM_ERR_NULL (frames, Q, outputs), the ranges' and classes' refusals
 *                        of rtdm_objects_detect_device, RTDM_ERR_BAD_SIZE (n < 0), RTDM_ERR_NULL (the handle),
 *                        RTDM_ERR_BAD_PARAM (nclasses above the detector's max_classes), RTDM_ERR_BAD_SIZE (a pitch below 3 *
 *                        width, disp_pitch below 2 * crop width or odd, an odd disp_frame_stride, with n > 1 a frame stride
 *                        below pitch * height).  n = 0 is RTDM_OK.
 * rtdm_estimate_batch_device: the same with device frames and device outputs, enqueued on hip_stream, which is synchronised
 *                        ONCE PER CHUNK (the read-back that decides the matcher's ROI1); the results are complete on the stream
 *                        when the call returns, not synchronised.  Calls that share handles must be ordered on one stream.
 * rtdm_estimator_set_device_roi: on != 0: the matcher takes every frame's union box from device memory
 *                        (rtdm_bm_compute_device_rois' route: one launch set per chunk, frames without objects skipped on the
 *                        device), so the read-back in front of the matcher is gone.  The device forms then NEVER synchronise:
 *                        the results are complete on the stream.  The host forms synchronise once per chunk, at its end.
 *                        Every output is that of the default mode, byte for byte, and frames without objects still leave the
 *                        caller's entries and maps untouched.  The one difference: the matcher's ROI1 is left as the caller
 *                        set it, not at the last frame that had objects.  The default is 0: everything as before.  No
 *                        allocation, no synchronisation. */
typedef struct rtdm_estimator rtdm_estimator;
int rtdm_estimator_create(rtdm_bm* bm, rtdm_rectify* rc, rtdm_objects* ob, int max_batch, int capacity, rtdm_estimator** out);
void rtdm_estimator_destroy(rtdm_estimator* est);
int rtdm_estimator_set_own_pixels(rtdm_estimator* est, int on);
int rtdm_estimator_get_own_pixels(const rtdm_estimator* est, int* on);
int rtdm_estimator_set_device_roi(rtdm_estimator* est, int on);
int rtdm_estimator_get_device_roi(const rtdm_estimator* est, int* on);
int rtdm_estimate_batch(rtdm_estimator* est, int n, const uint8_t* rgb_left, size_t left_pitch, size_t left_frame_stride,
                        const uint8_t* rgb_right, size_t right_pitch, size_t right_frame_stride, const double* Q,
                        const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, int min_area,
                        int zero_border, double calibration_unit, rtdm_object* objects, int* counts, double* mean_cm, int* npix,
                        int16_t* disp, size_t disp_pitch, size_t disp_frame_stride);
int rtdm_estimate_batch_device(rtdm_estimator* est, int n, const uint8_t* d_rgb_left, size_t left_pitch,
                               size_t left_frame_stride, const uint8_t* d_rgb_right, size_t right_pitch,
                               size_t right_frame_stride, const double* Q, const rtdm_hsv_range* ranges, const int* range_class,
                               int nranges, int nclasses, int min_area, int zero_border, double calibration_unit,
                               rtdm_object* d_objects, int* d_counts, double* d_mean_cm, int* d_npix, int16_t* d_disp,
                               size_t disp_pitch, size_t disp_frame_stride, void* hip_stream);

/* ---- object measurements: Z quantiles, 3-D position and extent per object (rules G1-G10) -------------
 * What calc_depth gives an object is one number: the mean of Z over its kept pixels, at integer disparity.  These calls
 * reduce the same pixels of the same device lists to a record per object, in camera coordinates (Q's unit; distance_cm =
 * value * calibration_unit / 10):
 *   npix, nplane   kept pixels; pixels of the clipped box that pass the plane predicate
 *   zq[k]          k < nquant: the Z of rank ((npix - 1) * permille[k]) / 1000 (64-bit integer arithmetic) among the kept Z in
 *                  ascending order -- 0 the minimum, 1000 the maximum, 500 the lower median; nothing is interpolated, the float
 *                  comes back bit for bit; duplicated and unsorted permille values are fine.  k >= nquant: +0.0.
 *   lo[j], hi[j]   minimum / maximum of X, Y, Z (j = 0, 1, 2) over the kept pixels.  Exact.
 *   mean[j]        sum of the component, widened to double, / npix: the centre.  The order of the sum is a function of the
 *                  clipped box alone (rule D3's) and no atomic takes part, so the bits are the same run to run and independent
 *                  of n, of the frame's position, of capacity and of the other objects.
 * The order of floats is that of the key (sign bit set -> ~bits, else bits | 0x80000000), so -0.0 lies below +0.0.
 * The point (X, Y, Z) of a pixel is exactly rtdm_xyz_map's for Q, disparity_mode and handle_missing_values = 1 (the minimum
 * is the frame's, over the whole frame, in the key of the mode).  A pixel is kept iff it passes the plane predicate -- mask
 * byte != 0, or with planes_are_labels the int32 label == i + 1 for object i (compared, never used as an index) -- and
 * fabs((double)Z - 10000.0) >= FLT_EPSILON and fabs((double)Z) <= max_z (NaN fails): calc_depth's test with max_z a parameter.
 * There is NO matcher-marker clause: a pixel whose disparity is the matcher's invalid value is kept unless it is the frame's
 * minimum (which it is in a map that has any) or fails the Z tests.  An object with nothing kept, an empty clipped box or a
 * cls outside [0, nclasses) gets npix 0 and +0.0 in zq, lo, hi and mean; nplane is what was counted (0 without a box).
 * rtdm_objects_measure_device: addressing as rtdm_depth_objects_device: object i of frame f writes d_measures[f * capacity + i],
 *                        entries at or beyond min(total_f, capacity) are left untouched; no list or plane content makes the
 *                        kernels read or write outside.  Enqueued on hip_stream: the call never synchronises, allocates or
 *                        copies to the host; Q and params are read before it returns; no kernel waits for another workgroup
 *                        and every grid is sized from n, capacity, height and nquant.  d_workspace: at least
 *                        rtdm_objects_measure_workspace_bytes(n, capacity, height, nquant) bytes, the call's own until its
 *                        work has finished (that function needs no device, is never 0 and does not shrink when an argument
 *                        grows).  n = 0 is RTDM_OK.  Refusals, before any device use: those of rtdm_depth_objects_device in
 *                        its order up to nclasses, with "mask" read as "plane" (and rtdm_depth_objects_labels_device's pitch,
 *                        stride and alignment rules with planes_are_labels), then RTDM_ERR_NULL (params, d_measures),
 *                        RTDM_ERR_BAD_PARAM (disparity_mode other than 0 / 1, max_z not finite or <= 0, nquant outside 0 .. 8,
 *                        a permille outside 0 .. 1000), RTDM_ERR_BAD_SIZE (d_measures not 8-byte aligned, workspace_bytes too
 *                        small), RTDM_ERR_UNSUPPORTED (width * height >= 2^31).
 * rtdm_estimate_batch_measured / _device: rtdm_estimate_batch / _device, which ARE these calls with mp = measures = NULL (the
 *                        same launches, the same bytes).  With both given, every chunk's objects are also measured against
 *                        the chunk's maps -- over their labels when own pixels are on, under their class masks otherwise --
 *                        and the records travel with mean_cm / npix: measures[f * capacity + i], downloaded in the host form,
 *                        complete on the stream in the device form; frames without objects and entries past the stored ones
 *                        are left untouched.  mean_cm / npix mean what they always meant.  The measurement's workspace is
 *                        allocated by the first measured call.  Refusals on top: RTDM_ERR_NULL first (one of mp / measures
 *                        NULL and the other not), and after all of rtdm_estimate_batch's RTDM_ERR_BAD_PARAM (params, as
 *                        above) and RTDM_ERR_BAD_SIZE (measures not 8-byte aligned). */
typedef struct rtdm_measure_params {
    int disparity_mode;         /* RTDM_XYZ_FIXED16 (0) | RTDM_XYZ_ROUNDED (1) */
    double max_z;               /* finite, > 0; 1e4 (calc_depth's literal) */
    int nquant;                 /* 0 .. 8 */
    int permille[8];            /* 0 .. 1000 each */
} rtdm_measure_params;
typedef struct rtdm_object_measure {           /* 88 bytes, 8-byte aligned */
    int32_t npix, nplane; float zq[8]; float lo[3], hi[3]; double mean[3];
} rtdm_object_measure;
void rtdm_measure_default_params(rtdm_measure_params* p);   /* ROUNDED, 1e4, nquant 3: 500, 250, 750 */
size_t rtdm_objects_measure_workspace_bytes(int n, int capacity, int height, int nquant);
int rtdm_objects_measure_device(int device, const rtdm_measure_params* params, int n, const int16_t* d_disp, size_t disp_pitch,
                                size_t disp_frame_stride, int width, int height, const double* Q, const void* d_planes,
                                size_t plane_pitch, size_t plane_stride, int planes_are_labels, int nclasses,
                                const struct rtdm_object* d_objects, int capacity, const int* d_counts,
                                rtdm_object_measure* d_measures, void* d_workspace, size_t workspace_bytes, void* hip_stream);
int rtdm_estimate_batch_measured(rtdm_estimator* est, int n, const uint8_t* rgb_left, size_t left_pitch, size_t left_frame_stride,
                                 const uint8_t* rgb_right, size_t right_pitch, size_t right_frame_stride, const double* Q,
                                 const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, int min_area,
                                 int zero_border, double calibration_unit, rtdm_object* objects, int* counts, double* mean_cm,
                                 int* npix, int16_t* disp, size_t disp_pitch, size_t disp_frame_stride,
                                 const rtdm_measure_params* mp, rtdm_object_measure* measures);
int rtdm_estimate_batch_measured_device(rtdm_estimator* est, int n, const uint8_t* d_rgb_left, size_t left_pitch,
                                        size_t left_frame_stride, const uint8_t* d_rgb_right, size_t right_pitch,
                                        size_t right_frame_stride, const double* Q, const rtdm_hsv_range* ranges,
                                        const int* range_class, int nranges, int nclasses, int min_area, int zero_border,
                                        double calibration_unit, rtdm_object* d_objects, int* d_counts, double* d_mean_cm,
                                        int* d_npix, int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                                        void* hip_stream, const rtdm_measure_params* mp, rtdm_object_measure* d_measures);

/* ---- the step after the matcher that the reference keeps switched off: the disparity WLS post-filter -------------------
 * ENABLE_POST_FILTER (estimator.cpp:57-70, 106-109; include/estimator.h:32,116) -- cv::ximgproc's createRightMatcher,
 * createDisparityWLSFilter, setLambda(8000), setSigmaColor(1.5) and filter(left_disp, left_rect, filtered, right_disp).
 * The rules W1-W8 it follows are restated in DESIGN.md section 4.9 (from memory: parity with the library is unpinned).
 * The result is FGS(C dL) / FGS(C): C is a confidence in {0, 255} from a left-right check and two discontinuity maps, FGS
 * a fast global smoother guided by the left view (three horizontal + vertical passes of tridiagonal solves, fp32). */
typedef struct rtdm_wls_params {
    double lambda;              /* >= 0; 8000 (setLambda) */
    double sigma_color;         /* > 0; 1.5 (setSigmaColor) */
    int lrc_thresh;             /* T >= 0, x16 units; 24 */
    int depth_discontinuity_radius;   /* r >= 0; ceil(0.33 w) from a StereoBM, ceil(0.5 w) from a StereoSGBM */
    int min_disparity;          /* of the LEFT matcher: its invalid value is (min_disparity - 1) * 16 */
    int num_disparities;        /* of the left matcher: the right matcher's minD is -(min_disparity + num_disparities) + 1 */
    int roi_left, roi_right, roi_top, roi_bottom;   /* >= 0: the valid ROI is the frame minus these (W2) */
    int num_iter;               /* 1 .. 16; 3 */
    double attenuation;         /* (0, 1]; 0.25: lambda of pass t + 1 = lambda of pass t * attenuation */
    int use_confidence;         /* 1: the filter above; 0: ximgproc's generic filter, FGS(dL) alone (no right map) */
} rtdm_wls_params;
typedef struct rtdm_wls rtdm_wls;
/* W2: the parameters createDisparityWLSFilter derives from a left StereoBM / StereoSGBM (common: lambda 8000, sigma 1.5,
 * T 24, 3 iterations, attenuation 0.25, use_confidence 1).  RTDM_ERR_NULL / RTDM_OK; nothing is validated here. */
int rtdm_wls_params_for_bm(const rtdm_bm_params* left, rtdm_wls_params* out);
int rtdm_wls_params_for_sgm(const rtdm_sgm_params* left, rtdm_wls_params* out);
/* W1: the parameters of createRightMatcher: the same matcher with minDisparity -(minD + numD) + 1, no texture / uniqueness /
 * speckle filtering and disp12MaxDiff 1000000; it is called as compute(right, left).  The StereoSGBM's preFilterCap is not part
 * of rtdm_sgm_params (rtdm_sgm_set_prefilter_cap sets it): the caller copies it to the right handle (the adapters do).
 * Likewise the StereoBM's preFilterType and preFilterSize (rtdm_bm_set_prefilter), which createRightMatcher copies too. */
int rtdm_bm_right_params(const rtdm_bm_params* left, rtdm_bm_params* right);
int rtdm_sgm_right_params(const rtdm_sgm_params* left, rtdm_sgm_params* right);
/* Parameters are validated before any device use: RTDM_ERR_BAD_PARAM for lambda < 0, sigma <= 0, T < 0, r < 0, a negative
 * offset, num_iter outside 1..16 or attenuation outside (0, 1].  max_width > 4096 or max_height > 4096: RTDM_ERR_UNSUPPORTED
 * (a row or column segment is solved by one wave).  set_params synchronises the device when sigma changes (the weight table
 * is rebuilt). */
int rtdm_wls_create(const rtdm_wls_params* params, int max_width, int max_height, int max_batch, int device, rtdm_wls** out);
void rtdm_wls_destroy(rtdm_wls* wls);
int rtdm_wls_set_params(rtdm_wls* wls, const rtdm_wls_params* params);
int rtdm_wls_get_params(const rtdm_wls* wls, rtdm_wls_params* out);
/* Host planes, pitches in bytes.  disp_left / disp_right: the x16 maps of the left and the right matcher (disp_right may be
 * NULL when use_confidence is 0); guide: the left view, 8-bit, channels 1 or 3 (interleaved).  out: int16 x16 map, invalid
 * value (min_disparity - 1) * 16 outside the valid ROI and where FGS(C) is 0.  conf (optional): the confidence C as float
 * (0 outside the ROI, and everywhere when use_confidence is 0).  filtered (optional): FGS(C dL) / FGS(C) as float before
 * rounding (the invalid value where out has it).  Synchronous. */
int rtdm_wls_filter(rtdm_wls* wls, const int16_t* disp_left, size_t left_pitch, const int16_t* disp_right, size_t right_pitch,
                    const uint8_t* guide, size_t guide_pitch, int channels, int width, int height, int16_t* out,
                    size_t out_pitch, float* conf, size_t conf_pitch, float* filtered, size_t filtered_pitch);
/* n device frames (frame i of a plane at base + i * frame_stride bytes), enqueued on hip_stream, NOT synchronised; n may
 * exceed max_batch (chunks). */
int rtdm_wls_filter_device(rtdm_wls* wls, int n, const int16_t* d_left, size_t left_pitch, size_t left_frame_stride,
                           const int16_t* d_right, size_t right_pitch, size_t right_frame_stride, const uint8_t* d_guide,
                           size_t guide_pitch, size_t guide_frame_stride, int channels, int width, int height,
                           int16_t* d_out, size_t out_pitch, size_t out_frame_stride, float* d_conf, size_t conf_pitch,
                           size_t conf_frame_stride, float* d_filtered, size_t filtered_pitch, size_t filtered_frame_stride,
                           void* hip_stream);
/* estimator.cpp:56-61 in one call: left_bm->compute(left, right), right_bm->compute(right, left) and the filter guided by the
 * left view.  The raw maps and the confidence stay in HBM; raw_left (optional) receives the left matcher's map.  right_bm is
 * a handle made with rtdm_bm_right_params; all three handles live on the same device.  Synchronous. */
int rtdm_bm_compute_filtered(rtdm_bm* left_bm, rtdm_bm* right_bm, rtdm_wls* wls, const uint8_t* left, size_t left_pitch,
                             const uint8_t* right, size_t right_pitch, int width, int height, int16_t* out, size_t out_pitch,
                             int16_t* raw_left, size_t raw_left_pitch);

/* ---- the depth map and the point cloud: reprojectImageTo3D on the device ----------------------------------------------------
 * rtdm_xyz_map    <- estimator.cpp:75-77: left_disp /= 16.; reprojectImageTo3D(left_disp, xyz, Q, true, CV_32F): the xyz image
 *                    (height x width x 3 interleaved floats, CV_32FC3) that the reference hands to calc_depth, and / or its Z
 *                    plane (height x width floats), from an x16 disparity map.
 * rtdm_xyz_cloud  <- the pixels calc_depth keeps (estimator.cpp:235), compacted in row-major order into 16-byte records with
 *                    the colour of an optional guide image (the rectified colour crop rtdm_rectify_rgb gives, or a gray view).
 * The rules X1-X8 are restated in DESIGN.md section 4.11 (from memory of OpenCV: parity with the library is unpinned).  The
 * homogeneous point is computed in double without fused multiply-adds, h_r = ((Q[4r] x + Q[4r+1] y) + Q[4r+2] d) + Q[4r+3], a
 * component is (float)(h_r / h_3); where h_3 is 0, inf and NaN are stored as the library stores them.  A pixel is kept iff its
 * disparity is not (min_disparity - 1) * 16, fabs((double)Z - 10000.0) >= FLT_EPSILON, fabs((double)Z) <= max_z (so NaN is
 * dropped) and its mask byte, where a mask is given, is non-zero.  Results are bit-identical run to run. */
#define RTDM_XYZ_FIXED16 0   /* d = disp / 16.0, exact: the sub-pixel value convertTo(CV_32F, 1/16.) gives */
#define RTDM_XYZ_ROUNDED 1   /* d = disp / 16 rounded half to even: the reference's `left_disp /= 16.` on CV_16S, and the rule of
                              * rtdm_depth_stats_device */
typedef struct rtdm_xyz_params {
    double Q[16];               /* 4x4 row major (stereoRectify's Q, main.cpp:92); every entry finite */
    int disparity_mode;         /* RTDM_XYZ_FIXED16 | RTDM_XYZ_ROUNDED */
    int handle_missing_values;  /* 0 | 1: a pixel whose d equals the minimum of d over its own frame gets Z = 10000.0f (X, Y stay) */
    int min_disparity;          /* of the matcher: the cloud drops its invalid value (min_disparity - 1) * 16 */
    double max_z;               /* > 0; 10000.0: calc_depth's bound */
} rtdm_xyz_params;
typedef struct rtdm_point { float x, y, z; uint8_t r, g, b, a; } rtdm_point;   /* 16 bytes; a = 255; r = g = b = 0 without a guide */
typedef struct rtdm_xyz rtdm_xyz;
/* The reference's call: ROUNDED, handle_missing_values 1, max_z 10000.  Q NULL: the identity. */
void rtdm_xyz_default_params(rtdm_xyz_params* p, const double* Q, int min_disparity);
/* Parameters are validated before any device use: RTDM_ERR_BAD_PARAM for a mode or a flag other than 0 / 1, a non-finite Q
 * entry or max_z that is not > 0.  There is no row limit (no 4096 cap): RTDM_ERR_UNSUPPORTED only where max_width *
 * max_height does not fit an int.  The handle owns its scratch -- frame minima, tile counts, counts, and the single-frame
 * staging of the host entries (40 bytes per pixel of max_width x max_height) -- so no entry allocates anything per call. */
int rtdm_xyz_create(const rtdm_xyz_params* params, int max_width, int max_height, int max_batch, int device, rtdm_xyz** out);
void rtdm_xyz_destroy(rtdm_xyz* xyz);
int rtdm_xyz_set_params(rtdm_xyz* xyz, const rtdm_xyz_params* params);   /* from the next call on; no synchronisation */
int rtdm_xyz_get_params(const rtdm_xyz* xyz, rtdm_xyz_params* out);
/* Host planes, pitches in bytes.  disp: the x16 map; xyz (optional): 3 floats per pixel; z (optional): the Z plane.
 * RTDM_ERR_BAD_SIZE when both outputs are absent.  Synchronous. */
int rtdm_xyz_map(rtdm_xyz* xyz, const int16_t* disp, size_t disp_pitch, int width, int height, float* xyz_out, size_t xyz_pitch,
                 float* z, size_t z_pitch);
/* n device frames (frame i of a plane at base + i * frame_stride bytes), enqueued on hip_stream, NOT synchronised; n may
 * exceed max_batch (chunks).  Calls that share a handle must be ordered on one stream: they share its scratch. */
int rtdm_xyz_map_device(rtdm_xyz* xyz, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride, int width,
                        int height, float* d_xyz, size_t xyz_pitch, size_t xyz_frame_stride, float* d_z, size_t z_pitch,
                        size_t z_frame_stride, void* hip_stream);
/* Host planes.  guide: channels 0 (none; guide may be NULL), 1 (copied to r, g and b) or 3 (interleaved, R first); other
 * counts: RTDM_ERR_BAD_PARAM, as is a negative capacity.  mask (optional): 8-bit.  *count = the number of kept pixels, even
 * when it exceeds capacity; only the first min(*count, capacity) records are written and nothing beyond them is touched
 * (points may be NULL when capacity is 0).  Synchronous. */
int rtdm_xyz_cloud(rtdm_xyz* xyz, const int16_t* disp, size_t disp_pitch, const uint8_t* guide, size_t guide_pitch, int channels,
                   const uint8_t* mask, size_t mask_pitch, int width, int height, rtdm_point* points, int capacity, int* count);
/* n device frames: the records of frame i start at d_points + i * points_frame_stride bytes (4-byte aligned, at least
 * capacity records apart), capacity holds per frame, d_counts receives n ints.  Enqueued on hip_stream, NOT synchronised. */
int rtdm_xyz_cloud_device(rtdm_xyz* xyz, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                          const uint8_t* d_guide, size_t guide_pitch, size_t guide_frame_stride, int channels,
                          const uint8_t* d_mask, size_t mask_pitch, size_t mask_frame_stride, int width, int height,
                          rtdm_point* d_points, size_t points_frame_stride, int capacity, int* d_counts, void* hip_stream);
/* estimator.cpp:56 + 75-77 in one call: bm->compute(left, right) and the cloud of its map, which stays in HBM (disp, optional,
 * receives it).  The handles live on the same device and xyz's min_disparity equals the matcher's, otherwise
 * RTDM_ERR_BAD_PARAM.  Synchronous. */
int rtdm_bm_compute_cloud(rtdm_bm* bm, rtdm_xyz* xyz, const uint8_t* left, size_t left_pitch, const uint8_t* right,
                          size_t right_pitch, int width, int height, const uint8_t* guide, size_t guide_pitch, int channels,
                          const uint8_t* mask, size_t mask_pitch, rtdm_point* points, int capacity, int* count, int16_t* disp,
                          size_t disp_pitch);

/* ---- DecoderDevice: baseline MJPEG frames decoded on the device (estimator.cpp:24-27, decoder/mjpeg-decoder-sw.cpp) ----------
 * Streams served: baseline sequential DCT (SOF0), 8-bit, Huffman coded, one interleaved scan; one component, or three (YCbCr)
 * with luma sampling 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and chroma 1x1; any size up to the handle's; up to four 8-bit
 * quantisation tables; Huffman tables from DHT or, where a frame carries none, the standard's typical tables (Annex K.3);
 * restart intervals of any length.  APPn / COM segments, fill bytes before a marker and bytes after EOI are skipped.
 * The result is what libjpeg gives with its defaults (JDCT_ISLOW, fancy upsampling), byte for byte: rules J1-J5, DESIGN.md
 * section 4.12.  The reference sets JDCT_IFAST, which this build does not serve.
 * Refused on the host before any device use: RTDM_ERR_UNSUPPORTED for any SOFn but SOF0, 12-bit samples, 16-bit quantisers,
 * component counts other than 1 or 3, other sampling factors, more than one scan; RTDM_ERR_BAD_SIZE for a frame whose size is
 * not the call's width x height, is larger than the handle's, or whose sampling differs from the other frames of the call;
 * RTDM_ERR_BAD_STREAM for no SOI at offset 0, a segment that runs past len, a scan that names a missing table, no SOS, no EOI.
 * Frames of one call may differ in tables, quantisers and restart interval. */
typedef struct rtdm_mjpeg_info {
    int width, height;
    int components;         /* 1 | 3 */
    int h_samp, v_samp;     /* luma sampling factors; 1, 1 for one component */
    int restart_interval;   /* MCUs per entropy segment as DRI gives it; 0: none */
    int segments;           /* entropy segments (1 without DRI); each is decoded on its own, and a frame of one segment is
                             * itself cut among lanes (rtdm_mjpeg_set_split) */
    int has_dht;            /* 0: the frame relies on the standard tables */
} rtdm_mjpeg_info;
typedef struct rtdm_mjpeg rtdm_mjpeg;
/* Parses the headers of one frame (len is a buffer size: it may exceed the frame); pure host code, no device needed. */
int rtdm_mjpeg_probe(const uint8_t* stream, size_t len, rtdm_mjpeg_info* out);
/* The handle owns all staging and scratch (page-locked stream staging of max_batch x max_stream_bytes, coefficient and
 * component planes for max_batch frames of max_width x max_height); no entry allocates per call.  A frame longer than
 * max_stream_bytes (SOI .. EOI) is RTDM_ERR_BAD_SIZE. */
int rtdm_mjpeg_create(int max_width, int max_height, int max_batch, size_t max_stream_bytes, int device, rtdm_mjpeg** out);
void rtdm_mjpeg_destroy(rtdm_mjpeg* h);
/* DecoderDevice::decode: one frame, host to host, rgb = height rows of width x 3 bytes (R first) `pitch` bytes apart.
 * Synchronous.  RTDM_ERR_BAD_STREAM also where the kernel found the entropy data damaged (rgb is then written, but undefined). */
int rtdm_mjpeg_decode(rtdm_mjpeg* h, const uint8_t* stream, size_t len, int width, int height, uint8_t* rgb, size_t pitch);
/* n host streams into n device frames (frame i at d_rgb + i * frame_stride).  The streams are copied before the call returns
 * (the caller may reuse them); the work is enqueued on hip_stream and NOT synchronised.  n may exceed max_batch (chunks; the
 * call then waits for the copies of all but its last chunk).  d_status (optional): n device ints, 0 or RTDM_ERR_BAD_STREAM
 * per frame.  Calls that share a handle must be ordered on one stream: they share its scratch. */
int rtdm_mjpeg_decode_batch_device(rtdm_mjpeg* h, int n, const uint8_t* const* streams, const size_t* lens, int width, int height,
                                   uint8_t* d_rgb, size_t pitch, size_t frame_stride, int* d_status, void* hip_stream);
/* A frame without restart intervals -- what UVC cameras send -- is one entropy segment.  The decoder cuts it into subsequences
 * of `subsequence_bytes` bytes (at least len / 1024, so that there are at most 1024) and gives one lane of a workgroup to each;
 * the lanes find the symbol boundaries by decoding speculatively until their hand-over states stop changing (DESIGN.md section
 * 4.12).  The result is that of one lane per segment, bit for bit.  subsequence_bytes: 0 = off (one lane per segment), 8 ..
 * 65536, or -1 for the built-in default; anything else is RTDM_ERR_BAD_PARAM (judged before the handle is looked at).  Takes
 * effect from the next call; a new handle starts at the default, which is on.  Frames with restart intervals are not affected. */
int rtdm_mjpeg_set_split(rtdm_mjpeg* h, int subsequence_bytes);
int rtdm_mjpeg_get_split(const rtdm_mjpeg* h, int* subsequence_bytes);
/* Totals since the handle was created: frames decoded the split way, the subsequences they were cut into, and the most rounds
 * of speculative decoding one of them took (never more than its subsequences).  SYNCHRONISES the stream of the handle's last
 * call, then reads the counters the kernel keeps on the device.  Any pointer may be NULL. */
int rtdm_mjpeg_get_split_stats(rtdm_mjpeg* h, long* frames_split, long* subsequences, int* max_rounds);
/* estimator.cpp:24-36 + 56 in one call: decode both frames, gray, remap, crop, match.  The RGB frames never leave HBM.  width x
 * height is the rectifier's frame; the three handles live on one device.  Synchronous. */
int rtdm_bm_compute_mjpeg(rtdm_bm* bm, rtdm_rectify* rc, rtdm_mjpeg* dec, const uint8_t* left, size_t left_len,
                          const uint8_t* right, size_t right_len, int width, int height, int16_t* disp, size_t disp_pitch);

/* ---- synthetic rectified-pair stream (stands in for stream/, which is out of
 * scope; decoder/ is served above): frame f of the stream uses seed + f; bit-identical to rt-depth-map_amd/synth.py. */
int rtdm_synth_pairs_device(uint64_t seed, int first_frame, int n, int width, int height,
                            int numDisparities, uint8_t* d_left, uint8_t* d_right, size_t pitch,
                            size_t frame_stride, int device, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RTDM_H_ */
