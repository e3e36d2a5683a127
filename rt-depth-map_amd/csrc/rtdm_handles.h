// rtdm_handles.h -- the handle structs more than one file of the C ABI layer has to see, and the internal functions that
// cross those files (all in namespace rtdm: the library's global symbols are the entry points of include/rtdm.h alone).
#pragma once
#include "rtdm_host.h"
#include "rtdm_kernels.h"
#include "rtdm_calib.h"
#include "rtdm_mjpeg.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>

struct StageEvent { hipEvent_t a, b; int stage; int frames; };

namespace rtdm {
// What rtdm_morph_set_op / rtdm_objects_set_morph keep: the caller's values and the element as the kernels take it.
struct MorphSetting { int op, iterations; rtdm_morph_element el; MorphBits bits; bool is_default; };
}

struct rtdm_bm {
    rtdm_bm_params p;
    int prefilter_type, prefilter_size;   // rtdm_bm_set_prefilter: cv::StereoBM's preFilterType / preFilterSize (XSOBEL, 9)
    int maxW, maxH, maxB, device;
    int roi1[4], roi2[4];
    hipStream_t stream;
    hipStream_t sBorder;           // batches: the border-column search runs here, next to the tile search
    hipStream_t sSpare[2];         // idle: they keep the runtime's stream-to-queue layout (rtdm_bm_create)
    hipEvent_t evFork, evJoin;     // ... behind this event of the compute stream, which then waits for that one
    hipEvent_t evBand[2];          // rtdm_bm_compute: one per band of the result on its way back
    hipStream_t sIn, sOut;         // rtdm_bm_compute_batch: copies in / out beside the compute stream
    hipEvent_t evH2D[2], evComp[2], evD2H[2];   // ... one set per half of the staging planes
    size_t ppitch;                 // pitch of the internal 8-bit planes
    uint8_t *dLp, *dRp;            // prefiltered planes   [maxB][maxH][ppitch]
    uint8_t *dInL, *dInR;          // staging for the host entry points
    int16_t* dOut;                 // internal disparity plane [maxB][maxH][Ws] (Ws = maxW rounded up to 8)
    rtdm::StripTuner tuner;        // measured strip counts of the batched search per work shape
    int32_t *dCost, *dLabel, *dSize, *dRowCnt;
    uint32_t* dRuns;
    int16_t* dHead;
    uint8_t* dMask;                // staging for rtdm_bm_compute_depth: mask plane + reduction scratch
    void* dDepth;
    // page-locked staging of the single-frame host entry points, laid out by rtdm_bm_create: the left and right planes (rows of
    // ppitch), then hD, the internal disparity plane of one frame, then hM, the mask of rtdm_bm_compute_depth
    uint8_t* hStage; int16_t* hD; uint8_t* hM;
    rtdm::AllocList mem;           // every d* / h* buffer above
    bool profiling;
    std::vector<StageEvent> pending;
    double stage_ms[RTDM_NUM_STAGES];
    long stage_launches[RTDM_NUM_STAGES], stage_frames[RTDM_NUM_STAGES];
    std::string variant;
};

struct rtdm_rectify {
    int W, H, rx, ry, rw, rh, maxB, device;
    int16_t* dMap1[2];            // roi part of the maps: rh x rw x 2
    uint16_t* dMap2[2];           // rh x rw
    uint8_t* dRgb[2];             // staging for host frames: H x W x 3 (+ padding)
    uint8_t* dOut;                // staging for host outputs: rh x rw x 3
    uint8_t* dGray[2];            // rectified gray pair for the chained matcher call: rh x pitch
    size_t gpitch;
    uint8_t* hStage;              // pinned: 2 RGB frames in, rh x rw x 3 out
    rtdm::AllocList mem;
    hipStream_t stream;
};

struct rtdm_objects {
    int W, H, device, maxRec;
    int maxB, maxC;               // frames x class planes of one launch (rtdm_objects_create_batch)
    size_t mpitch;                // row pitch of the class planes in dMaskIn / dMaskOut: W rounded up to 4
    uint8_t *dRgb, *dMaskIn, *dMaskOut, *dT0, *dT1;   // [maxB] frames, [maxB * maxC] planes each
    rtdm::MorphSetting morph;     // rtdm_objects_set_morph
    void* dScratch;               // [maxB * maxC] x cc_plane_bytes
    int* dMeta;                   // host entry points: [maxB * maxC] counts, then [maxB] union boxes
    rtdm::CcObject* dObj;         // host entry points: object lists, grown on demand (objCap entries; not in `mem`)
    size_t objCap;
    int32_t* dLab; size_t labBytes;       // rtdm_objects_detect_labels_batch: a chunk's label planes and moments, grown on
    rtdm::CcStats* dStats; size_t statCap;   // demand like dObj (not in `mem`)
    int* hRec;                    // pinned: [0] = count, then the first HEAD records (the batched calls: counts, union boxes)
    std::vector<int> all;         // host copy of every record when there are more than HEAD
    rtdm::AllocList mem;
    hipStream_t stream;
};

struct rtdm_wls {
    rtdm_wls_params p;
    int maxW, maxH, maxB, device;
    hipStream_t stream;
    float* dLut;                   // W5: lut[k] = exp(-sqrt(k) / sigma), k = 0 .. 3 * 255^2
    float2* dF;                    // [maxB][maxH][maxW] the two right-hand sides / solutions
    float *dWh, *dWv;              // neighbour weights
    uint8_t* dConf;                // C in {0, 255}
    rtdm::WlsMM *dMML, *dMMR;            // W3 row windows
    int16_t *dInL, *dInR, *dOut;   // single-frame staging of the host entry points
    uint8_t *dGuide, *dImgR;
    float *dConfOut, *dFilt;
    rtdm::AllocList mem;
};

struct rtdm_xyz {
    rtdm_xyz_params p;
    int maxW, maxH, maxB, device;
    hipStream_t stream;
    int *dMin, *dTile, *dCounts;   // [maxB] frame minima, [maxB][tiles of maxW x maxH] tile counts, [maxB] counts of a host call
    // single-frame staging of the host entry points
    int16_t* dDisp;
    uint8_t *dGuide, *dMask, *dImgL, *dImgR;
    float *dXYZ, *dZ;
    rtdm::XyzRec* dPts;
    rtdm::AllocList mem;
};

struct rtdm_mjpeg {
    int maxW, maxH, maxB, device;
    size_t maxBytes, slot;         // longest stream served; its slot in the staging area (maxBytes rounded up to 16)
    size_t maxSegs, maxBlocks;     // per frame: entropy segments (one MCU each at worst), 8 x 8 blocks of three full planes
    hipStream_t stream;
    hipEvent_t evStaged;           // the staging area is on its way to the device up to here ...
    bool staged;                   // ... and must not be overwritten before
    uint8_t* hStreams; rtdm::MjpegDesc* hDesc; rtdm::MjpegSeg* hSegs; int* hStatus;     // page-locked
    uint8_t* dStreams; rtdm::MjpegDesc* dDesc; rtdm::MjpegSeg* dSegs;
    int16_t* dCoef;                // [maxB][blocks][64] dequantised coefficients
    uint8_t* dPlanes;              // [maxB] planar Y, Cb, Cr at their own (padded) resolutions
    uint8_t* dRgb;                 // one frame for the host entry point
    int* dStatus;                  // [maxB + 1]
    int splitBytes;                // subsequence bytes asked for a frame without restart intervals; 0: one lane per segment
    unsigned long long* dSplitTotals;   // {frames, subsequences} k_mjpeg_huff_split decoded since creation ...
    int* dSplitRounds;             // ... and the most rounds one of them took
    hipStream_t lastStream;        // where the last call enqueued (what rtdm_mjpeg_get_split_stats waits for)
    bool used;                     // a call has enqueued work
    rtdm::AllocList mem;
};

struct rtdm_estimator {
    rtdm_bm* bm; rtdm_rectify* rc; rtdm_objects* ob;      // borrowed
    int device, chunk, cap;        // frames of one chunk; objects of a frame that are stored and measured
    size_t cpitch;                 // row pitch of the colour crops (objects_rgb_pitch)
    uint8_t* dRgb[2];              // host form: the raw frames of a chunk, [chunk] x H x W x 3 each
    uint8_t* dGray[2];             // rectified gray pairs [chunk][rh][gpitch]
    uint8_t* dCrop;                // left colour crops    [chunk][rh][cpitch]
    rtdm::CcObject* dObj; int* dCounts; double* dMean; int* dNpix;      // host form: [chunk] x cap, [chunk] x RTDM_MAX_CLASSES
    int* dRois;                    // [chunk] x 4
    void* dWork; size_t workBytes; // rtdm_depth_objects_device's workspace for a chunk
    bool deviceRoi;                // rtdm_estimator_set_device_roi: the matcher reads dRois itself, no read-back in front of it
    int32_t* dLabels;              // rtdm_estimator_set_own_pixels: [chunk] x [detector's max_classes] planes of rh x rw ints, or null
    // rtdm_estimate_batch_measured: made by the first measured call -- the measurement's workspace for a chunk, and for the
    // host form the chunk's records on the device and page-locked
    void* dMeasWork; size_t measWorkBytes;
    rtdm::MeasRecord *dMeas, *hMeas;
    // page-locked: the read-back in front of the matcher, then what the host form brings back and takes in
    int *hCounts, *hRois, *hNpix; rtdm::CcObject* hObj; double* hMean; int16_t* hDisp; uint8_t* hRgb[2];
    rtdm::AllocList mem;
};

namespace rtdm {

// api_bm.hip.  bm_run_chunk: one chunk (n <= maxB) of device-resident frames, enqueued on s.  bm_upload_gray: a pageable gray
// pair through the staging area into dInL / dInR, in bands.  bm_download_disp: the internal plane on its way to the staging
// area; bm_scatter_disp, after the caller's synchronise: its rows into the caller's plane.
int bm_check_frame(const rtdm_bm* bm, int W, int H);
int bm_upload_gray(rtdm_bm* bm, const uint8_t* left, size_t left_pitch, const uint8_t* right, size_t right_pitch, int width, int height,
                   hipStream_t s);
int bm_run_chunk(rtdm_bm* bm, int n, Plane8 L, Plane8 R, int W, int H, Plane16W out, hipStream_t s);
// ... with frame f under ROI1 = d_rois[f] from device memory (w <= 0 or h <= 0: skipped); the results stay on the internal
// plane, and go to `out` as well where out.base is not null (rtdm_bm_compute_device_rois)
int bm_run_chunk_rois(rtdm_bm* bm, int n, Plane8 L, Plane8 R, int W, int H, const int* d_rois, Plane16W out, hipStream_t s);
int bm_download_disp(rtdm_bm* bm, int W, int H, hipStream_t s);
void bm_scatter_disp(const rtdm_bm* bm, int W, int H, int16_t* disp, size_t disp_pitch);
// the handle's internal disparity plane for W x H frames: rows of Ws = W rounded up to 8 elements (see bm_run_chunk)
inline size_t bm_ws(int W) { return (size_t)((W + 7) & ~7); }
inline Plane16W bm_internal_plane(const rtdm_bm* bm, int W, int H) { return Plane16W{bm->dOut, bm_ws(W), bm_ws(W) * (size_t)H}; }
int depth_check_regions(const rtdm_region* regions, int n, int W, int H, int* flat, int* maxh);   // (api_core.hip)
// api_core.hip: rule D6 up to the class count (elem: bytes of a plane element, 1 or 4; outputs: all result pointers are there)
int depth_objects_check(int n, const void* d_disp, size_t disp_pitch, size_t disp_frame_stride, int width, int height, const double* Q,
                        const void* d_planes, size_t plane_pitch, size_t plane_stride, size_t elem, int nclasses, const void* d_objects,
                        int capacity, const void* d_counts, bool outputs, const void* d_workspace);
// api_measure.hip: rule G10's RTDM_ERR_BAD_PARAM (p non-null); the kernels' form of Q and the params
int measure_params_check(const rtdm_measure_params* p);
void measure_params_kernel(const rtdm_measure_params* p, const double* Q, XyzParams* P, MeasQuant* mq);
// the other handles' files, by prefix
// api_morph.hip.  morph_setting_check: the refusals of rtdm_morph_set_op, no device needed.  morph_run: THE routing of the
// morphological filter -- the default setting with rtdm_debug_morph_general off runs launch_morph_open_close, everything
// else launch_morph_general; t0 / t1: n * W * H bytes of scratch each.
int morph_setting_check(int op, int iterations, const rtdm_morph_element* el);
void morph_setting_default(MorphSetting* s);
void morph_setting_store(MorphSetting* s, int op, int iterations, const rtdm_morph_element* el);
void morph_setting_get(const MorphSetting& s, int* op, int* iterations, rtdm_morph_element* el);
int morph_run(const MorphSetting& s, Plane8 in, Plane8W out, uint8_t* t0, uint8_t* t1, int W, int H, int n, hipStream_t stream);
int rectify_upload(rtdm_rectify* rc, const uint8_t* a, size_t apitch, const uint8_t* b, size_t bpitch, hipStream_t s);
void rectify_gray_launch(rtdm_rectify* rc, const uint8_t* dl, const uint8_t* dr, int n, Plane8W ol, Plane8W orr, hipStream_t s);
int objects_run(rtdm_objects* ob, const rtdm_hsv_range* range, int min_area, int zero_border, rtdm_region* boxes, int max_boxes,
                int* nboxes, rtdm_region* roi, hipStream_t s);
// api_objects.hip, the batched detector.  objects_classes_check: the refusals that concern ranges and classes (no handle
// needed) and the kernel's form of them.  objects_run_chunk: one chunk (m <= maxB) of device frames enqueued on s; d_masks
// null: the filtered planes stay in ob->dMaskOut (rows of ob->mpitch).  objects_stage: ob->dObj holds `entries` records.
size_t objects_rgb_pitch(const rtdm_objects* ob);
int objects_classes_check(const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, HsvClasses* C);
int objects_run_chunk(rtdm_objects* ob, int m, const uint8_t* d_rgb, size_t pitch, size_t frame_stride, const HsvClasses& C,
                      int min_area, int zero_border, uint8_t* d_masks, size_t mask_pitch, size_t mask_plane_stride,
                      CcObject* d_objects, int capacity, int* d_counts, int* d_rois, hipStream_t s,
                      const CcLabelsOut& lab = CcLabelsOut{nullptr, 0, 0, nullptr});
int objects_stage(rtdm_objects* ob, size_t entries);
int wls_check(const rtdm_wls* h, int channels, int W, int H);
int wls_chunk(rtdm_wls* h, int n, WlsDisp dl, WlsDisp dr, WlsGuide G, WlsOut o, int W, int H, hipStream_t s);
int wls_download(rtdm_wls* h, int W, int H, int16_t* out, size_t out_pitch, float* conf, size_t conf_pitch, float* filtered,
                 size_t filtered_pitch, hipStream_t s);
int xyz_cloud_check(const rtdm_xyz* h, const void* disp, const void* guide, int channels, int width, int height, const void* points,
                    int capacity, const void* count);
int xyz_cloud_staged(rtdm_xyz* h, int channels, bool mask, int width, int height, rtdm_point* points, int capacity, int* count,
                     hipStream_t s);
int mjpeg_check(const rtdm_mjpeg* h, const uint8_t* stream, size_t len, int W, int H);   // parseable, the call's size, within the handle?
int mjpeg_chunk(rtdm_mjpeg* h, int m, const uint8_t* const* streams, const size_t* lens, int W, int H, uint8_t* d_rgb, size_t pitch,
                size_t frame_stride, int* d_status, hipStream_t s, MjpegDesc* shape);

}  // namespace rtdm
