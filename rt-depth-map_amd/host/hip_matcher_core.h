// hip_matcher_core.h -- OpenCV-free C++ host layer over the C ABI (include/rtdm.h).
//
// HIPMatcherCore has the constructor shape, method names, argument meaning and error behaviour of
// the reference's SWMatcherKonolige (/root/reference/include/stereo-matcher/bm-sw.h:28-35):
// the same twelve constructor arguments in the same order (roi1, roi2 and maxDisparity are
// accepted and ignored, as bm-sw.cpp:12-26 does), compute() returns an int that is 0 on success,
// setROI1/setROI2 forward a rectangle.  The only differences are forced by the missing OpenCV:
// images are (pointer, pitch, rows, cols) instead of cv::InputArray, rectangles are rtdm::Rect.
// bm-hip.{h,cpp} wrap this class into the real `class HIPMatcher : public BlockMatcher`.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rtdm.h"

namespace rtdm {

struct Rect { int x = 0, y = 0, width = 0, height = 0; };

class HIPMatcherCore {
public:
    // Frame size is needed up front because the device buffers are allocated once, like the
    // reference's FPGA matcher (bm-hw-ip.h:74: HWMatcherDisparityCoprocessor(name, width, height)).
    HIPMatcherCore(const Rect& roi1, const Rect& roi2, int preFilterCap, int blockSize, int minDisparity,
                   int textureThreshold, int numOfDisparities, int maxDisparity, int uniquenessRatio,
                   int speckleWindowSize, int speckleRange, int disp12MaxDiff,
                   int maxWidth, int maxHeight, int maxBatch = 1, int device = 0, bool legacyRightClamp = false);
    // legacyRightClamp: rtdm_bm_params.legacy_right_clamp -- the right-border sampling rule of OpenCV 3.1-3.2, the era
    // the reference links (Makefile.include:18-23); the default is the 4.x rule.
    ~HIPMatcherCore();
    HIPMatcherCore(const HIPMatcherCore&) = delete;
    HIPMatcherCore& operator=(const HIPMatcherCore&) = delete;

    void setROI1(const Rect& roi1);
    void setROI2(const Rect& roi2);
    // cv::StereoBM::setPreFilterType (RTDM_PREFILTER_XSOBEL, the default, or RTDM_PREFILTER_NORMALIZED_RESPONSE) and
    // setPreFilterSize (odd, 5 .. 255; read by the normalised response only), from the next compute on.  Return the status.
    int setPreFilterType(int preFilterType);
    int setPreFilterSize(int preFilterSize);
    int preFilterType() const { return preFilterType_; }
    int preFilterSize() const { return preFilterSize_; }
    // 8-bit single-channel inputs with free row pitch, 16-bit signed fixed-point (x16) output.
    // Returns 0 on success, a negative rtdm_status otherwise (the reference's compute() returns
    // int and its caller ignores it, estimator.cpp:56; nothing here throws).
    int compute(const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep,
                int rows, int cols, int16_t* out, size_t outStep);
    // n contiguous frames (frameStride bytes apart), host memory, processed in device batches.
    int computeBatch(int n, const uint8_t* left, const uint8_t* right, size_t step, size_t frameStride,
                     int rows, int cols, int16_t* out, size_t outStep, size_t outFrameStride);

    // n device-resident frames, frame f under ROI1 = dRois[f] read from DEVICE memory (rtdm_bm_compute_device_rois, rules B1-B6 of
    // DESIGN.md section 4.19): what setROI1(roi f) + a device compute of frame f alone writes, in one launch set for all of them;
    // a frame whose rectangle has width <= 0 or height <= 0 is skipped.  Enqueued on hipStream, not synchronised; this
    // object's own ROI1 is not touched.
    int computeDeviceRois(int n, const uint8_t* dLeft, const uint8_t* dRight, size_t step, size_t frameStride, int rows, int cols,
                          const Rect* dRois, int16_t* dOut, size_t outStep, size_t outFrameStride, void* hipStream);

    // The caller's next three lines in one call (estimator.cpp:75-77): left_disp /= 16., reprojectImageTo3D with
    // Q (row-major 4x4), calc_depth over `regions` under `mask`; the disparity stays on the device unless `out`
    // is given.  meanCm[i] = mean Z * calibrationUnit / 10, counts[i] = pixels that entered the mean.
    int computeDepth(const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep, int rows, int cols,
                     const double* Q, const uint8_t* mask, size_t maskStep, const Rect* regions, int nregions,
                     double calibrationUnit, double* meanCm, int* counts, int16_t* out = nullptr, size_t outStep = 0);

    int status() const { return status_; }           // result of construction / last call
    const char* statusText() const { return rtdm_strerror(status_); }
    int filteredValue() const { return (params_.minDisparity - 1) * 16; }
    const rtdm_bm_params& params() const { return params_; }
    int maxWidth() const { return maxWidth_; }
    int maxHeight() const { return maxHeight_; }
    int device() const { return device_; }
    rtdm_bm* handle() { return bm_; }

private:
    rtdm_bm_params params_;
    rtdm_bm* bm_ = nullptr;
    int status_ = RTDM_OK;
    int maxWidth_ = 0, maxHeight_ = 0, device_ = 0;
    int preFilterType_ = RTDM_PREFILTER_XSOBEL, preFilterSize_ = 9;
    int setPrefilter(int type, int size);
};

// SWSemiGlobalMatcher counterpart (/root/reference/include/stereo-matcher/sgbm-sw.h:24-37): the same seven
// constructor arguments in the same order plus the frame size; P1 = 600 and P2 = 2400 as sgbm-sw.cpp:17-18
// hard-codes them; setROI1/2 are no-ops there too.  paths = 8 (BASELINE config 5) or 5: the directions of
// cv::StereoSGBM's default MODE_SGBM, which is what sgbm-sw.cpp:15 creates -- the adapter sgbm-hip.cpp passes 5 unless told
// another mode; 4: MODE_HH4 (left, right, down, up).  pathsForMode maps cv::StereoSGBM::setMode's values to the direction
// count; MODE_SGBM_3WAY maps to 3, which rtdm_sgm_create refuses (RTDM_ERR_UNSUPPORTED; setMode serves it), anything else to 0
// (RTDM_ERR_BAD_PARAM).
enum SGMMode { MODE_SGBM = 0, MODE_HH = 1, MODE_SGBM_3WAY = 2, MODE_HH4 = 3 };   // cv::StereoSGBM's values
class HIPSGMCore {
public:
    static int pathsForMode(int mode)
    { return mode == MODE_SGBM ? 5 : (mode == MODE_HH ? 8 : (mode == MODE_SGBM_3WAY ? 3 : (mode == MODE_HH4 ? 4 : 0))); }
    HIPSGMCore(int blockSize, int minDisparity, int numOfDisparities, int uniquenessRatio, int speckleWindowSize,
               int speckleRange, int disp12MaxDiff, int maxWidth, int maxHeight, int device = 0, int paths = 8);
    ~HIPSGMCore();
    HIPSGMCore(const HIPSGMCore&) = delete;
    HIPSGMCore& operator=(const HIPSGMCore&) = delete;
    int compute(const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep,
                int rows, int cols, int16_t* out, size_t outStep);
    // channels = 1 (the call above) or 3: interleaved colour (CV_8UC3), steps in bytes
    int compute(int channels, const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep,
                int rows, int cols, int16_t* out, size_t outStep);
    // cv::StereoSGBM::setPreFilterCap (0 .. 127), from the next compute on
    int setPreFilterCap(int preFilterCap);
    // rtdm_sgm_set_cost, from the next compute on: RTDM_SGM_COST_BT (cv::StereoSGBM's pixel cost, the default) or
    // RTDM_SGM_COST_CENSUS over a cw x ch window (cw 3, 5, 7, 9; ch 3, 5, 7; gray frames only) -- the project's own cost for
    // pairs whose cameras expose differently; the library has no counterpart
    int setCost(int cost, int cw = 9, int ch = 7);
    // cv::StereoSGBM::setMode on the live matcher (rtdm_sgm_set_mode), from the next compute on: MODE_SGBM, MODE_HH, MODE_HH4 or
    // MODE_SGBM_3WAY -- the one door to the last (rules T1-T8; numOfDisparities <= 256); params().paths
    // follows it (3 under MODE_SGBM_3WAY), createdPaths() stays what the matcher was created with
    int setMode(int mode);
    int mode() const { return mode_; }
    int createdPaths() const { return createdPaths_; }
    int status() const { return status_; }
    const rtdm_sgm_params& params() const { return params_; }
    int preFilterCap() const { return preFilterCap_; }
    int cost() const { return cost_; }
    int censusWidth() const { return censusWidth_; }
    int censusHeight() const { return censusHeight_; }
    int maxWidth() const { return maxWidth_; }
    int maxHeight() const { return maxHeight_; }
    int device() const { return device_; }

private:
    rtdm_sgm* sg_ = nullptr;
    int status_ = RTDM_OK;
    rtdm_sgm_params params_;
    int preFilterCap_ = 0, maxWidth_ = 0, maxHeight_ = 0, device_ = 0;
    int cost_ = RTDM_SGM_COST_BT, censusWidth_ = 9, censusHeight_ = 7;
    int mode_ = MODE_HH, createdPaths_ = 8;
};

// The disparity WLS post-filter (cv::ximgproc::DisparityWLSFilter, the reference's ENABLE_POST_FILTER block,
// /root/reference/estimator.cpp:57-70): rules W1-W8 of DESIGN.md section 4.9.  Constructed from the left matcher's
// parameters (createDisparityWLSFilter, W2) or from explicit ones.  filter() has ximgproc's argument order: left map,
// left view (the guide, 1 or 3 interleaved channels), filtered output, right map (may be null without confidence).
class HIPWLSCore {
public:
    HIPWLSCore(const rtdm_wls_params& params, int maxWidth, int maxHeight, int device = 0);
    HIPWLSCore(const HIPMatcherCore& leftMatcher);
    HIPWLSCore(const HIPSGMCore& leftMatcher);
    ~HIPWLSCore();
    HIPWLSCore(const HIPWLSCore&) = delete;
    HIPWLSCore& operator=(const HIPWLSCore&) = delete;
    int setLambda(double lambda);
    double getLambda() const { return params_.lambda; }
    int setSigmaColor(double sigma);
    double getSigmaColor() const { return params_.sigma_color; }
    int setLRCthresh(int thresh);
    int getLRCthresh() const { return params_.lrc_thresh; }
    int setDepthDiscontinuityRadius(int radius);
    int getDepthDiscontinuityRadius() const { return params_.depth_discontinuity_radius; }
    // steps in bytes; filtered (optional) receives the float map before rounding.  The confidence of the call stays
    // readable through confidenceMap() (rows x cols floats, 0 / 255) until the next call.
    int filter(const int16_t* left, size_t leftStep, const uint8_t* guide, size_t guideStep, int channels, int rows, int cols,
               int16_t* out, size_t outStep, const int16_t* right, size_t rightStep, float* filtered = nullptr,
               size_t filteredStep = 0);
    const float* confidenceMap() const { return conf_; }
    Rect roi(int rows, int cols) const;     // the valid ROI (W2); empty: all zero
    // estimator.cpp:56-61 in one call (rtdm_bm_compute_filtered); right = the core createRightMatcher made
    int computeFiltered(HIPMatcherCore& left, HIPMatcherCore& right, const uint8_t* l, size_t lStep, const uint8_t* r,
                        size_t rStep, int rows, int cols, int16_t* out, size_t outStep, int16_t* rawLeft = nullptr,
                        size_t rawLeftStep = 0);
    int status() const { return status_; }
    rtdm_wls* handle() { return wls_; }

private:
    void create(int maxWidth, int maxHeight, int device);
    int set(const rtdm_wls_params& p);
    rtdm_wls_params params_;
    rtdm_wls* wls_ = nullptr;
    float* conf_ = nullptr;
    int status_ = RTDM_OK;
};

// createRightMatcher (W1): new cores that match right against left (compute(right, left)); the caller deletes them
HIPMatcherCore* createRightMatcher(const HIPMatcherCore& left);
HIPSGMCore* createRightMatcher(const HIPSGMCore& left);

// The caller's two lines after the matcher (/root/reference/estimator.cpp:75-76): left_disp /= 16.; reprojectImageTo3D(left_disp,
// xyz, Q, true, CV_32F) -- the xyz image calc_depth reads -- and the coloured point cloud of the pixels calc_depth keeps (:235).
// Rules X1-X8 of DESIGN.md section 4.11.  Disparity maps are the matchers' 16-bit x16 maps; steps in bytes.
class HIPXYZCore {
public:
    HIPXYZCore(const double Q[16], int maxWidth, int maxHeight, int minDisparity = 0, int disparityMode = RTDM_XYZ_ROUNDED,
               bool handleMissingValues = true, double maxZ = 10000.0, int device = 0);
    ~HIPXYZCore();
    HIPXYZCore(const HIPXYZCore&) = delete;
    HIPXYZCore& operator=(const HIPXYZCore&) = delete;
    int setQ(const double Q[16]);
    int setDisparityMode(int disparityMode);
    int setHandleMissingValues(bool handleMissingValues);
    int setMaxZ(double maxZ);
    // xyz: rows x cols x 3 floats (CV_32FC3), z: rows x cols floats; either may be null, not both
    int reprojectImageTo3D(const int16_t* disp, size_t dispStep, int rows, int cols, float* xyz, size_t xyzStep,
                           float* z = nullptr, size_t zStep = 0);
    // guide: channels 0 (none), 1 or 3 (R first); mask may be null.  *count = kept pixels; min(*count, capacity) are stored
    int cloud(const int16_t* disp, size_t dispStep, const uint8_t* guide, size_t guideStep, int channels, const uint8_t* mask,
              size_t maskStep, int rows, int cols, rtdm_point* points, int capacity, int* count);
    // estimator.cpp:56 + 75-77 in one call (rtdm_bm_compute_cloud); disp (optional) receives the matcher's map
    int computeCloud(HIPMatcherCore& matcher, const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep,
                     int rows, int cols, const uint8_t* guide, size_t guideStep, int channels, const uint8_t* mask,
                     size_t maskStep, rtdm_point* points, int capacity, int* count, int16_t* disp = nullptr, size_t dispStep = 0);
    int status() const { return status_; }
    const rtdm_xyz_params& params() const { return params_; }
    int maxWidth() const { return maxWidth_; }
    int maxHeight() const { return maxHeight_; }
    rtdm_xyz* handle() { return xyz_; }

private:
    int set(const rtdm_xyz_params& p);
    rtdm_xyz_params params_;
    rtdm_xyz* xyz_ = nullptr;
    int status_ = RTDM_OK, maxWidth_ = 0, maxHeight_ = 0;
};

// The caller's lines in front of the matcher (/root/reference/estimator.cpp:29-39): cvtColor(RGB2GRAY) + remap with
// the CV_16SC2 maps of main.cpp:95-96 + crop to roif, for both cameras, on the device.  Not behind an interface in
// the reference (OpenCV is called inline there), so using it means replacing those lines.
class HIPRectifierCore {
public:
    // map1*: rows x cols x 2 int16, map2*: rows x cols uint16 (continuous Mats: remap_left1.data ...); roif = crop
    HIPRectifierCore(const int16_t* map1Left, const uint16_t* map2Left, const int16_t* map1Right, const uint16_t* map2Right,
                     int rows, int cols, const Rect& roif, int device = 0);
    ~HIPRectifierCore();
    HIPRectifierCore(const HIPRectifierCore&) = delete;
    HIPRectifierCore& operator=(const HIPRectifierCore&) = delete;
    // rgb*: rows x cols x 3 bytes (first channel R); *Rect: roif.height x roif.width bytes
    int rectifyGray(const uint8_t* rgbLeft, size_t leftStep, const uint8_t* rgbRight, size_t rightStep,
                    uint8_t* leftRect, size_t leftRectStep, uint8_t* rightRect, size_t rightRectStep);
    // remap + crop of the colour frame (estimator.cpp:38-39); which = 0: left maps, 1: right maps
    int rectifyColour(int which, const uint8_t* rgb, size_t step, uint8_t* out, size_t outStep);
    // estimator.cpp:29-36 + 56 in one call: raw frames in, x16 disparity of the cropped pair out
    int compute(HIPMatcherCore& matcher, const uint8_t* rgbLeft, size_t leftStep, const uint8_t* rgbRight, size_t rightStep,
                int16_t* out, size_t outStep);
    int status() const { return status_; }
    rtdm_rectify* handle() { return rc_; }

private:
    rtdm_rectify* rc_ = nullptr;
    int status_ = RTDM_OK;
};

// The caller's lines between rectification and the matcher (/root/reference/estimator.cpp:40-53): HSV threshold of the
// rectified colour crop, the morphological filter, findContours(RETR_EXTERNAL) + boundingRect + the minimum-size filter
// (fill_bounding_rects_of_contours, :167-174) and the union box (find_relevant_matching_region, :176-204).
// estimateFrame() is one whole iteration of Estimator::run without capture, decode and drawing (:29-77).
class HIPObjectsCore {
public:
    HIPObjectsCore(int cols, int rows, int device = 0);       // size of the crop (roif)
    // for frame batches and several colour classes: up to maxBatch frames x maxClasses class planes per launch
    HIPObjectsCore(int cols, int rows, int device, int maxBatch, int maxClasses);
    ~HIPObjectsCore();
    HIPObjectsCore(const HIPObjectsCore&) = delete;
    HIPObjectsCore& operator=(const HIPObjectsCore&) = delete;
    // thresholds as the Estimator's members iLowH ... iHighV (estimator.cpp:110-115)
    void setRange(int lowH, int lowS, int lowV, int highH, int highS, int highV);
    // rgb: rows x cols x 3 (R first); maskOut (filter_out) may be null.  Returns the number of boxes (>= 0; only
    // maxBoxes are stored) or a negative status.  zeroBorder: true = findContours of OpenCV <= 3.1.
    int detect(const uint8_t* rgb, size_t step, int minObjSize, bool zeroBorder, uint8_t* maskOut, size_t maskStep,
               Rect* boxes, int maxBoxes, Rect* matchingRoi);
    int estimateFrame(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, const uint8_t* rgbLeft, size_t leftStep,
                      const uint8_t* rgbRight, size_t rightStep, const double* Q, int minObjSize, bool zeroBorder,
                      double calibrationUnit, Rect* boxes, double* meanCm, int* counts, int maxBoxes,
                      int16_t* disp = nullptr, size_t dispStep = 0);
    // Several colour classes (include/rtdm.h, rules O1-O6): nranges ranges, cls[r] in [0, nclasses) the class of range r, every
    // class with a range of its own (red: {0..9} and {170..179} in one class).  Kept for detectDevice / estimateFrameClasses;
    // setRange and detect / estimateFrame are not touched by it.  Returns a status.
    int setRanges(const rtdm_hsv_range* ranges, const int* cls, int nranges, int nclasses);
    int classes() const { return nclasses_; }
    // n device-resident frames on hipStream, not synchronised: frame f's objects at dObjects + f * capacity (class ascending),
    // dCounts[f * classes() + c], dRois[f]; dMasks (plane f * classes() + c) may be null.  Returns a status.
    int detectDevice(int n, const uint8_t* dRgb, size_t step, size_t frameStride, int minObjSize, bool zeroBorder, uint8_t* dMasks,
                     size_t maskStep, size_t maskPlaneStride, rtdm_object* dObjects, int capacity, int* dCounts, Rect* dRois,
                     void* hipStream);
    // detectDevice with the pixels of every object (include/rtdm.h, rules L1-L4): dLabels -- one int32 plane per (frame, class),
    // 1 + the object's index in its frame's list on the pixels of its component, 0 elsewhere -- and dStats -- the raw moments of
    // those pixels at dStats + f * capacity -- may each be null.  Returns a status.
    int detectLabelsDevice(int n, const uint8_t* dRgb, size_t step, size_t frameStride, int minObjSize, bool zeroBorder,
                           uint8_t* dMasks, size_t maskStep, size_t maskPlaneStride, rtdm_object* dObjects, int capacity, int* dCounts,
                           Rect* dRois, int32_t* dLabels, size_t labelStep, size_t labelPlaneStride, rtdm_object_stats* dStats,
                           void* hipStream);
    // estimateBatch measures every object over its own pixels instead of its class's mask inside its box (rule L7); kept
    // across the estimator handles this object makes.
    void setOwnPixels(bool on);
    bool ownPixels() const { return ownPixels_; }
    // estimateBatch lets the matcher read every frame's union box from device memory (rtdm_estimator_set_device_roi): no
    // read-back in front of the matcher, same outputs; the matcher's ROI1 stays as its owner set it.  Kept like setOwnPixels.
    void setDeviceRoi(bool on);
    bool deviceRoi() const { return deviceRoi_; }
    // estimateFrame for the classes of setRanges: every object with its class, measured under its class's mask.  Returns the
    // number of objects (only maxObjects are stored) or a negative status.
    int estimateFrameClasses(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, const uint8_t* rgbLeft, size_t leftStep,
                             const uint8_t* rgbRight, size_t rightStep, const double* Q, int minObjSize, bool zeroBorder,
                             double calibrationUnit, rtdm_object* objects, double* meanCm, int* counts, int maxObjects,
                             int16_t* disp = nullptr, size_t dispStep = 0);
    // estimateFrameClasses for n frame pairs per call (rtdm_estimate_batch): frame f at rgb + f * frameStride, its objects at
    // objects + f * capacity (every stored one is measured: meanCm / npix[f * capacity + i]), counts[f * classes() + c], its map
    // at disp + f * dispFrameStride bytes (disp may be null).  Frames without objects keep what the arrays held.  The estimator
    // handle is made by the first call and made anew when the matcher, the rectifier, maxBatch or capacity differ from the
    // call before; matcher and rectifier must live as long as this object uses them.  Returns a status.
    int estimateBatch(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, int maxBatch, int capacity, int n,
                      const uint8_t* rgbLeft, size_t leftStep, size_t leftFrameStride, const uint8_t* rgbRight, size_t rightStep,
                      size_t rightFrameStride, const double* Q, int minObjSize, bool zeroBorder, double calibrationUnit,
                      rtdm_object* objects, int* counts, double* meanCm, int* npix, int16_t* disp = nullptr, size_t dispStep = 0,
                      size_t dispFrameStride = 0);
    // estimateBatch that also measures every stored object (rtdm_estimate_batch_measured, rules G1-G10): Z quantiles, extent and
    // centre in camera coordinates at measures[f * capacity + i]; over the object's own pixels when setOwnPixels is on.
    int estimateBatchMeasured(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, int maxBatch, int capacity, int n,
                              const uint8_t* rgbLeft, size_t leftStep, size_t leftFrameStride, const uint8_t* rgbRight,
                              size_t rightStep, size_t rightFrameStride, const double* Q, int minObjSize, bool zeroBorder,
                              double calibrationUnit, rtdm_object* objects, int* counts, double* meanCm, int* npix,
                              const rtdm_measure_params& params, rtdm_object_measure* measures, int16_t* disp = nullptr,
                              size_t dispStep = 0, size_t dispFrameStride = 0);
    int status() const { return status_; }

private:
    int estimator(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, int maxBatch, int capacity);   // est_ for these; a status
    rtdm_objects* ob_ = nullptr;
    rtdm_estimator* est_ = nullptr;                          // estimateBatch: the handle and what it was made for
    rtdm_bm* estBm_ = nullptr;
    rtdm_rectify* estRc_ = nullptr;
    int estBatch_ = 0, estCap_ = 0;
    bool ownPixels_ = false, deviceRoi_ = false;
    rtdm_hsv_range range_;
    rtdm_hsv_range ranges_[RTDM_MAX_HSV_RANGES];
    int cls_[RTDM_MAX_HSV_RANGES];
    int nranges_ = 0, nclasses_ = 0;
    int status_ = RTDM_OK;
};

// DecoderDevice counterpart (the reference's include/decoder/decoder.h:9-15, decoder/mjpeg-decoder-sw.cpp:95-142): one baseline
// MJPEG frame -> interleaved RGB, decoded on the device with libjpeg's default methods (JDCT_ISLOW, fancy upsampling; rules
// J1-J5 of DESIGN.md section 4.12 -- the reference asks libjpeg for JDCT_IFAST, which is not served).
class HIPMJPEGCore {
public:
    // maxStreamBytes 0: width * height * 3 (no baseline frame of that size is longer in practice), at least 4096
    HIPMJPEGCore(int maxWidth, int maxHeight, size_t maxStreamBytes = 0, int device = 0);
    ~HIPMJPEGCore();
    HIPMJPEGCore(const HIPMJPEGCore&) = delete;
    HIPMJPEGCore& operator=(const HIPMJPEGCore&) = delete;
    // out: height rows of width x 3 bytes (R first), outStep bytes apart (0: width * 3)
    int decode(const uint8_t* in, size_t len, int width, int height, uint8_t* out, size_t outStep = 0);
    // estimator.cpp:24-36 + 56 in one call (rtdm_bm_compute_mjpeg): both cameras' frames in, x16 disparity of the crop out
    int compute(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, const uint8_t* left, size_t leftLen, const uint8_t* right,
                size_t rightLen, int width, int height, int16_t* out, size_t outStep);
    static int probe(const uint8_t* in, size_t len, rtdm_mjpeg_info* info) { return rtdm_mjpeg_probe(in, len, info); }
    // a frame without restart intervals is cut into subsequences of this many bytes, one lane each (rtdm_mjpeg_set_split):
    // 0 off, 8 .. 65536, -1 the built-in default (which a new decoder starts with)
    int setSplit(int subsequenceBytes);
    // totals since construction; synchronises the last call's stream (rtdm_mjpeg_get_split_stats)
    int splitStats(long* framesSplit, long* subsequences, int* maxRounds);
    int status() const { return status_; }
    rtdm_mjpeg* handle() { return dec_; }

private:
    rtdm_mjpeg* dec_ = nullptr;
    int status_ = RTDM_OK;
};

// VideoFilterDevice counterpart (/root/reference/include/filter/filter.h:13-37,
// /root/reference/filter/mf-sw.cpp:10-28): owns the frame buffers it hands out.
class HIPMorphCore {
public:
    HIPMorphCore(int w, int h, int bpp, int device = 0);
    ~HIPMorphCore();
    HIPMorphCore(const HIPMorphCore&) = delete;
    HIPMorphCore& operator=(const HIPMorphCore&) = delete;
    char* getVideoInBuffer();
    char* getVideoOutBuffer();
    int getFrameSize() const { return width_ * height_ * (bpp_ >> 3); }
    int run(const uint8_t* in, size_t inStep, uint8_t* out, size_t outStep, int rows, int cols);
    // cv::getStructuringElement(shape, Size(width, height)) / the operation and iteration count of cv::morphologyEx
    // (RTDM_MORPH_*), from the next run on (rtdm_morph_set_op); each keeps what the other one set.
    int setElement(int shape, int width, int height);
    int setOperation(int op, int iterations = 1);
    int status() const { return status_; }

private:
    rtdm_morph* mf_ = nullptr;
    int width_, height_, bpp_, status_ = RTDM_OK;
};

}  // namespace rtdm
