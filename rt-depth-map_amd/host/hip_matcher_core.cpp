#include "hip_matcher_core.h"

#include <cstdio>

namespace rtdm {

HIPMatcherCore::HIPMatcherCore(const Rect& roi1, const Rect& roi2, int preFilterCap, int blockSize, int minDisparity,
                               int textureThreshold, int numOfDisparities, int maxDisparity, int uniquenessRatio,
                               int speckleWindowSize, int speckleRange, int disp12MaxDiff,
                               int maxWidth, int maxHeight, int maxBatch, int device, bool legacyRightClamp)
{
    (void)roi1; (void)roi2; (void)maxDisparity;   // ignored by the reference constructor as well (bm-sw.cpp:12-26)
    params_.preFilterCap = preFilterCap;
    params_.blockSize = blockSize;
    params_.minDisparity = minDisparity;
    params_.numDisparities = numOfDisparities;
    params_.textureThreshold = textureThreshold;
    params_.uniquenessRatio = uniquenessRatio;
    params_.speckleWindowSize = speckleWindowSize;
    params_.speckleRange = speckleRange;
    params_.disp12MaxDiff = disp12MaxDiff;
    params_.legacy_right_clamp = legacyRightClamp ? 1 : 0;
    maxWidth_ = maxWidth; maxHeight_ = maxHeight; device_ = device;
    status_ = rtdm_bm_create(&params_, maxWidth, maxHeight, maxBatch, device, &bm_);
    if (status_ != RTDM_OK)
        std::fprintf(stderr, "HIPMatcher: %s%s%s\n", rtdm_strerror(status_),
                     status_ == RTDM_ERR_HIP ? ": " : "", status_ == RTDM_ERR_HIP ? rtdm_last_hip_error() : "");
}

HIPMatcherCore::~HIPMatcherCore() { rtdm_bm_destroy(bm_); }

void HIPMatcherCore::setROI1(const Rect& r) { if (bm_) status_ = rtdm_bm_set_roi(bm_, 1, r.x, r.y, r.width, r.height); }
void HIPMatcherCore::setROI2(const Rect& r) { if (bm_) status_ = rtdm_bm_set_roi(bm_, 2, r.x, r.y, r.width, r.height); }

int HIPMatcherCore::setPrefilter(int type, int size)
{
    if (!bm_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    const int rc = rtdm_bm_set_prefilter(bm_, type, size);
    if (rc == RTDM_OK) { preFilterType_ = type; preFilterSize_ = size; }
    return rc;
}
int HIPMatcherCore::setPreFilterType(int preFilterType) { return setPrefilter(preFilterType, preFilterSize_); }
int HIPMatcherCore::setPreFilterSize(int preFilterSize) { return setPrefilter(preFilterType_, preFilterSize); }

int HIPMatcherCore::compute(const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep,
                            int rows, int cols, int16_t* out, size_t outStep)
{
    if (!bm_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;   // loud: no CPU fallback
    status_ = rtdm_bm_compute(bm_, left, leftStep, right, rightStep, cols, rows, out, outStep);
    return status_;
}

int HIPMatcherCore::computeBatch(int n, const uint8_t* left, const uint8_t* right, size_t step, size_t frameStride,
                                 int rows, int cols, int16_t* out, size_t outStep, size_t outFrameStride)
{
    if (!bm_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_bm_compute_batch(bm_, n, left, right, step, frameStride, cols, rows, out, outStep, outFrameStride);
    return status_;
}

int HIPMatcherCore::computeDeviceRois(int n, const uint8_t* dLeft, const uint8_t* dRight, size_t step, size_t frameStride, int rows,
                                      int cols, const Rect* dRois, int16_t* dOut, size_t outStep, size_t outFrameStride, void* hipStream)
{
    if (!bm_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    static_assert(sizeof(Rect) == 4 * sizeof(int), "a Rect is the four ints of a device ROI");
    status_ = rtdm_bm_compute_device_rois(bm_, n, dLeft, dRight, step, frameStride, cols, rows, reinterpret_cast<const int*>(dRois),
                                          dOut, outStep, outFrameStride, hipStream);
    return status_;
}

int HIPMatcherCore::computeDepth(const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep, int rows,
                                 int cols, const double* Q, const uint8_t* mask, size_t maskStep, const Rect* regions,
                                 int nregions, double calibrationUnit, double* meanCm, int* counts, int16_t* out, size_t outStep)
{
    if (!bm_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    static_assert(sizeof(Rect) == sizeof(rtdm_region), "Rect and rtdm_region share their layout");
    status_ = rtdm_bm_compute_depth(bm_, left, leftStep, right, rightStep, cols, rows, Q, mask, maskStep,
                                    reinterpret_cast<const rtdm_region*>(regions), nregions, calibrationUnit, meanCm, counts,
                                    out, outStep);
    return status_;
}

HIPRectifierCore::HIPRectifierCore(const int16_t* map1Left, const uint16_t* map2Left, const int16_t* map1Right,
                                   const uint16_t* map2Right, int rows, int cols, const Rect& roif, int device)
{
    status_ = rtdm_rectify_create(map1Left, map2Left, map1Right, map2Right, cols, rows, roif.x, roif.y, roif.width, roif.height,
                                  1, device, &rc_);
    if (status_ != RTDM_OK) std::fprintf(stderr, "HIPRectifier: %s\n", rtdm_strerror(status_));
}
HIPRectifierCore::~HIPRectifierCore() { rtdm_rectify_destroy(rc_); }
int HIPRectifierCore::rectifyGray(const uint8_t* rgbLeft, size_t leftStep, const uint8_t* rgbRight, size_t rightStep,
                                  uint8_t* leftRect, size_t leftRectStep, uint8_t* rightRect, size_t rightRectStep)
{
    if (!rc_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    return status_ = rtdm_rectify_gray(rc_, rgbLeft, leftStep, rgbRight, rightStep, leftRect, leftRectStep, rightRect, rightRectStep);
}
int HIPRectifierCore::rectifyColour(int which, const uint8_t* rgb, size_t step, uint8_t* out, size_t outStep)
{
    if (!rc_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    return status_ = rtdm_rectify_rgb(rc_, which, rgb, step, out, outStep);
}
int HIPRectifierCore::compute(HIPMatcherCore& matcher, const uint8_t* rgbLeft, size_t leftStep, const uint8_t* rgbRight,
                              size_t rightStep, int16_t* out, size_t outStep)
{
    if (!rc_ || !matcher.handle()) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    return status_ = rtdm_bm_compute_rgb(matcher.handle(), rc_, rgbLeft, leftStep, rgbRight, rightStep, out, outStep);
}

HIPObjectsCore::HIPObjectsCore(int cols, int rows, int device)
{
    setRange(0, 150, 0, 9, 255, 255);                                  // estimator.cpp:110-115
    status_ = rtdm_objects_create(cols, rows, device, &ob_);
    if (status_ != RTDM_OK) std::fprintf(stderr, "HIPObjects: %s\n", rtdm_strerror(status_));
}
HIPObjectsCore::HIPObjectsCore(int cols, int rows, int device, int maxBatch, int maxClasses)
{
    setRange(0, 150, 0, 9, 255, 255);
    status_ = rtdm_objects_create_batch(cols, rows, maxBatch, maxClasses, device, &ob_);
    if (status_ != RTDM_OK) std::fprintf(stderr, "HIPObjects: %s\n", rtdm_strerror(status_));
}
HIPObjectsCore::~HIPObjectsCore() { rtdm_estimator_destroy(est_); rtdm_objects_destroy(ob_); }
int HIPObjectsCore::estimator(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, int maxBatch, int capacity)
{
    if (!ob_ || !matcher.handle() || !rectifier.handle()) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    if (!est_ || estBm_ != matcher.handle() || estRc_ != rectifier.handle() || estBatch_ != maxBatch || estCap_ != capacity) {
        rtdm_estimator_destroy(est_);
        est_ = nullptr;
        status_ = rtdm_estimator_create(matcher.handle(), rectifier.handle(), ob_, maxBatch, capacity, &est_);
        if (status_ != RTDM_OK) return status_;
        estBm_ = matcher.handle(); estRc_ = rectifier.handle(); estBatch_ = maxBatch; estCap_ = capacity;
    }
    status_ = rtdm_estimator_set_own_pixels(est_, ownPixels_ ? 1 : 0);          // (nothing happens unless the setting changed)
    if (status_ != RTDM_OK) return status_;
    return status_ = rtdm_estimator_set_device_roi(est_, deviceRoi_ ? 1 : 0);
}
int HIPObjectsCore::estimateBatch(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, int maxBatch, int capacity, int n,
                                  const uint8_t* rgbLeft, size_t leftStep, size_t leftFrameStride, const uint8_t* rgbRight,
                                  size_t rightStep, size_t rightFrameStride, const double* Q, int minObjSize, bool zeroBorder,
                                  double calibrationUnit, rtdm_object* objects, int* counts, double* meanCm, int* npix, int16_t* disp,
                                  size_t dispStep, size_t dispFrameStride)
{
    const int st = estimator(matcher, rectifier, maxBatch, capacity);
    if (st != RTDM_OK) return st;
    return status_ = rtdm_estimate_batch(est_, n, rgbLeft, leftStep, leftFrameStride, rgbRight, rightStep, rightFrameStride, Q, ranges_,
                                         cls_, nranges_, nclasses_, minObjSize, zeroBorder ? 1 : 0, calibrationUnit, objects, counts,
                                         meanCm, npix, disp, dispStep, dispFrameStride);
}
int HIPObjectsCore::estimateBatchMeasured(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, int maxBatch, int capacity, int n,
                                          const uint8_t* rgbLeft, size_t leftStep, size_t leftFrameStride, const uint8_t* rgbRight,
                                          size_t rightStep, size_t rightFrameStride, const double* Q, int minObjSize, bool zeroBorder,
                                          double calibrationUnit, rtdm_object* objects, int* counts, double* meanCm, int* npix,
                                          const rtdm_measure_params& params, rtdm_object_measure* measures, int16_t* disp,
                                          size_t dispStep, size_t dispFrameStride)
{
    const int st = estimator(matcher, rectifier, maxBatch, capacity);
    if (st != RTDM_OK) return st;
    return status_ = rtdm_estimate_batch_measured(est_, n, rgbLeft, leftStep, leftFrameStride, rgbRight, rightStep, rightFrameStride, Q,
                                                  ranges_, cls_, nranges_, nclasses_, minObjSize, zeroBorder ? 1 : 0, calibrationUnit,
                                                  objects, counts, meanCm, npix, disp, dispStep, dispFrameStride, &params, measures);
}
int HIPObjectsCore::setRanges(const rtdm_hsv_range* ranges, const int* cls, int nranges, int nclasses)
{
    if (!ranges || !cls) return RTDM_ERR_NULL;
    if (nranges < 1 || nranges > RTDM_MAX_HSV_RANGES || nclasses < 1 || nclasses > RTDM_MAX_CLASSES) return RTDM_ERR_BAD_PARAM;
    for (int i = 0; i < nranges; ++i) { ranges_[i] = ranges[i]; cls_[i] = cls[i]; }
    nranges_ = nranges; nclasses_ = nclasses;
    return RTDM_OK;
}
int HIPObjectsCore::detectDevice(int n, const uint8_t* dRgb, size_t step, size_t frameStride, int minObjSize, bool zeroBorder,
                                 uint8_t* dMasks, size_t maskStep, size_t maskPlaneStride, rtdm_object* dObjects, int capacity,
                                 int* dCounts, Rect* dRois, void* hipStream)
{
    if (!ob_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    return status_ = rtdm_objects_detect_device(ob_, n, dRgb, step, frameStride, ranges_, cls_, nranges_, nclasses_, minObjSize,
                                                zeroBorder ? 1 : 0, dMasks, maskStep, maskPlaneStride, dObjects, capacity, dCounts,
                                                reinterpret_cast<rtdm_region*>(dRois), hipStream);
}
void HIPObjectsCore::setOwnPixels(bool on) { ownPixels_ = on; }
void HIPObjectsCore::setDeviceRoi(bool on) { deviceRoi_ = on; }
int HIPObjectsCore::detectLabelsDevice(int n, const uint8_t* dRgb, size_t step, size_t frameStride, int minObjSize, bool zeroBorder,
                                       uint8_t* dMasks, size_t maskStep, size_t maskPlaneStride, rtdm_object* dObjects, int capacity,
                                       int* dCounts, Rect* dRois, int32_t* dLabels, size_t labelStep, size_t labelPlaneStride,
                                       rtdm_object_stats* dStats, void* hipStream)
{
    if (!ob_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    return status_ = rtdm_objects_detect_labels_device(ob_, n, dRgb, step, frameStride, ranges_, cls_, nranges_, nclasses_, minObjSize,
                                                       zeroBorder ? 1 : 0, dMasks, maskStep, maskPlaneStride, dObjects, capacity,
                                                       dCounts, reinterpret_cast<rtdm_region*>(dRois), dLabels, labelStep,
                                                       labelPlaneStride, dStats, hipStream);
}
int HIPObjectsCore::estimateFrameClasses(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, const uint8_t* rgbLeft, size_t leftStep,
                                         const uint8_t* rgbRight, size_t rightStep, const double* Q, int minObjSize, bool zeroBorder,
                                         double calibrationUnit, rtdm_object* objects, double* meanCm, int* counts, int maxObjects,
                                         int16_t* disp, size_t dispStep)
{
    if (!ob_ || !matcher.handle() || !rectifier.handle()) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    int n = 0;
    status_ = rtdm_estimate_frame_classes(matcher.handle(), rectifier.handle(), ob_, rgbLeft, leftStep, rgbRight, rightStep, Q, ranges_,
                                          cls_, nranges_, nclasses_, minObjSize, zeroBorder ? 1 : 0, calibrationUnit, objects, meanCm,
                                          counts, maxObjects, &n, disp, dispStep);
    return status_ == RTDM_OK ? n : status_;
}
void HIPObjectsCore::setRange(int lowH, int lowS, int lowV, int highH, int highS, int highV)
{
    range_.low[0] = lowH; range_.low[1] = lowS; range_.low[2] = lowV;
    range_.high[0] = highH; range_.high[1] = highS; range_.high[2] = highV;
}
int HIPObjectsCore::detect(const uint8_t* rgb, size_t step, int minObjSize, bool zeroBorder, uint8_t* maskOut, size_t maskStep,
                           Rect* boxes, int maxBoxes, Rect* matchingRoi)
{
    if (!ob_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    static_assert(sizeof(Rect) == sizeof(rtdm_region), "Rect and rtdm_region share their layout");
    int n = 0;
    status_ = rtdm_objects_detect(ob_, rgb, step, &range_, minObjSize, zeroBorder ? 1 : 0, maskOut, maskStep,
                                  reinterpret_cast<rtdm_region*>(boxes), maxBoxes, &n, reinterpret_cast<rtdm_region*>(matchingRoi));
    return status_ == RTDM_OK ? n : status_;
}
int HIPObjectsCore::estimateFrame(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, const uint8_t* rgbLeft, size_t leftStep,
                                  const uint8_t* rgbRight, size_t rightStep, const double* Q, int minObjSize, bool zeroBorder,
                                  double calibrationUnit, Rect* boxes, double* meanCm, int* counts, int maxBoxes,
                                  int16_t* disp, size_t dispStep)
{
    if (!ob_ || !matcher.handle() || !rectifier.handle()) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    int n = 0;
    status_ = rtdm_estimate_frame(matcher.handle(), rectifier.handle(), ob_, rgbLeft, leftStep, rgbRight, rightStep, Q, &range_,
                                  minObjSize, zeroBorder ? 1 : 0, calibrationUnit, reinterpret_cast<rtdm_region*>(boxes), meanCm,
                                  counts, maxBoxes, &n, disp, dispStep);
    return status_ == RTDM_OK ? n : status_;
}

HIPSGMCore::HIPSGMCore(int blockSize, int minDisparity, int numOfDisparities, int uniquenessRatio, int speckleWindowSize,
                       int speckleRange, int disp12MaxDiff, int maxWidth, int maxHeight, int device, int paths)
{
    rtdm_sgm_params p;
    rtdm_sgm_default_params(&p, numOfDisparities, blockSize);     // P1 = 8*3*5*5, P2 = 32*3*5*5 (sgbm-sw.cpp:17-18)
    p.minDisparity = minDisparity; p.uniquenessRatio = uniquenessRatio; p.speckleWindowSize = speckleWindowSize;
    p.speckleRange = speckleRange; p.disp12MaxDiff = disp12MaxDiff; p.paths = paths;
    params_ = p; maxWidth_ = maxWidth; maxHeight_ = maxHeight; device_ = device; createdPaths_ = paths;
    status_ = rtdm_sgm_create(&p, maxWidth, maxHeight, 1, device, &sg_);
    if (status_ != RTDM_OK) std::fprintf(stderr, "HIPSemiGlobalMatcher: %s\n", rtdm_strerror(status_));
    else rtdm_sgm_get_mode(sg_, &mode_);
}
HIPSGMCore::~HIPSGMCore() { rtdm_sgm_destroy(sg_); }
int HIPSGMCore::compute(const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep, int rows, int cols,
                        int16_t* out, size_t outStep)
{
    if (!sg_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_sgm_compute(sg_, left, leftStep, right, rightStep, cols, rows, out, outStep);
    return status_;
}
int HIPSGMCore::compute(int channels, const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep, int rows,
                        int cols, int16_t* out, size_t outStep)
{
    if (!sg_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_sgm_compute_cn(sg_, channels, left, leftStep, right, rightStep, cols, rows, out, outStep);
    return status_;
}
int HIPSGMCore::setPreFilterCap(int preFilterCap)
{
    if (!sg_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    const int rc = rtdm_sgm_set_prefilter_cap(sg_, preFilterCap);
    if (rc == RTDM_OK) preFilterCap_ = preFilterCap;
    return rc;
}
int HIPSGMCore::setCost(int cost, int cw, int ch)
{
    if (!sg_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    const int rc = rtdm_sgm_set_cost(sg_, cost, cw, ch);
    if (rc == RTDM_OK) rtdm_sgm_get_cost(sg_, &cost_, &censusWidth_, &censusHeight_);
    return rc;
}

int HIPSGMCore::setMode(int mode)
{
    if (!sg_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    const int rc = rtdm_sgm_set_mode(sg_, mode);
    if (rc == RTDM_OK) { mode_ = mode; params_.paths = pathsForMode(mode); }
    return rc;
}

HIPWLSCore::HIPWLSCore(const rtdm_wls_params& params, int maxWidth, int maxHeight, int device) : params_(params)
{
    create(maxWidth, maxHeight, device);
}
HIPWLSCore::HIPWLSCore(const HIPMatcherCore& m)
{
    rtdm_wls_params_for_bm(&m.params(), &params_);
    create(m.maxWidth(), m.maxHeight(), m.device());
}
HIPWLSCore::HIPWLSCore(const HIPSGMCore& m)
{
    rtdm_wls_params_for_sgm(&m.params(), &params_);
    create(m.maxWidth(), m.maxHeight(), m.device());
}
void HIPWLSCore::create(int maxWidth, int maxHeight, int device)
{
    status_ = rtdm_wls_create(&params_, maxWidth, maxHeight, 1, device, &wls_);
    if (status_ == RTDM_OK) conf_ = new float[(size_t)maxWidth * maxHeight]();
    else std::fprintf(stderr, "HIPDisparityWLSFilter: %s\n", rtdm_strerror(status_));
}
HIPWLSCore::~HIPWLSCore() { rtdm_wls_destroy(wls_); delete[] conf_; }
int HIPWLSCore::set(const rtdm_wls_params& p)
{
    if (!wls_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_wls_set_params(wls_, &p);
    if (status_ == RTDM_OK) params_ = p;
    return status_;
}
int HIPWLSCore::setLambda(double v) { rtdm_wls_params p = params_; p.lambda = v; return set(p); }
int HIPWLSCore::setSigmaColor(double v) { rtdm_wls_params p = params_; p.sigma_color = v; return set(p); }
int HIPWLSCore::setLRCthresh(int v) { rtdm_wls_params p = params_; p.lrc_thresh = v; return set(p); }
int HIPWLSCore::setDepthDiscontinuityRadius(int v) { rtdm_wls_params p = params_; p.depth_discontinuity_radius = v; return set(p); }
int HIPWLSCore::filter(const int16_t* left, size_t leftStep, const uint8_t* guide, size_t guideStep, int channels, int rows,
                       int cols, int16_t* out, size_t outStep, const int16_t* right, size_t rightStep, float* filtered,
                       size_t filteredStep)
{
    if (!wls_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_wls_filter(wls_, left, leftStep, right, rightStep, guide, guideStep, channels, cols, rows, out, outStep,
                              conf_, (size_t)cols * sizeof(float), filtered, filteredStep);
    return status_;
}
Rect HIPWLSCore::roi(int rows, int cols) const
{
    Rect r;
    const int w = cols - params_.roi_left - params_.roi_right, h = rows - params_.roi_top - params_.roi_bottom;
    if (w > 0 && h > 0) { r.x = params_.roi_left; r.y = params_.roi_top; r.width = w; r.height = h; }
    return r;
}
int HIPWLSCore::computeFiltered(HIPMatcherCore& left, HIPMatcherCore& right, const uint8_t* l, size_t lStep, const uint8_t* r,
                                size_t rStep, int rows, int cols, int16_t* out, size_t outStep, int16_t* rawLeft,
                                size_t rawLeftStep)
{
    if (!wls_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_bm_compute_filtered(left.handle(), right.handle(), wls_, l, lStep, r, rStep, cols, rows, out, outStep,
                                       rawLeft, rawLeftStep);
    return status_;
}

HIPMatcherCore* createRightMatcher(const HIPMatcherCore& left)
{
    rtdm_bm_params p;
    rtdm_bm_right_params(&left.params(), &p);
    Rect none;
    HIPMatcherCore* m = new HIPMatcherCore(none, none, p.preFilterCap, p.blockSize, p.minDisparity, p.textureThreshold,
                                           p.numDisparities, p.numDisparities, p.uniquenessRatio, p.speckleWindowSize,
                                           p.speckleRange, p.disp12MaxDiff, left.maxWidth(), left.maxHeight(), 1, left.device(),
                                           p.legacy_right_clamp != 0);
    // not part of rtdm_bm_params (W1: createRightMatcher copies preFilterType and preFilterSize)
    if (left.preFilterType() != RTDM_PREFILTER_XSOBEL || left.preFilterSize() != 9) {
        m->setPreFilterSize(left.preFilterSize());
        m->setPreFilterType(left.preFilterType());
    }
    return m;
}
HIPSGMCore* createRightMatcher(const HIPSGMCore& left)
{
    rtdm_sgm_params p;
    rtdm_sgm_right_params(&left.params(), &p);
    // (created as the left one was -- paths = 3 cannot be created --, the mode set on it since is copied below)
    HIPSGMCore* m = new HIPSGMCore(p.blockSize, p.minDisparity, p.numDisparities, p.uniquenessRatio, p.speckleWindowSize,
                                   p.speckleRange, p.disp12MaxDiff, left.maxWidth(), left.maxHeight(), left.device(), left.createdPaths());
    if (left.preFilterCap()) m->setPreFilterCap(left.preFilterCap());     // not part of rtdm_sgm_params (W1)
    if (left.cost() != RTDM_SGM_COST_BT) m->setCost(left.cost(), left.censusWidth(), left.censusHeight());   // nor is the pixel cost
    if (left.mode() != m->mode()) m->setMode(left.mode());               // nor a mode set on the live matcher
    return m;
}

HIPXYZCore::HIPXYZCore(const double Q[16], int maxWidth, int maxHeight, int minDisparity, int disparityMode,
                       bool handleMissingValues, double maxZ, int device) : maxWidth_(maxWidth), maxHeight_(maxHeight)
{
    rtdm_xyz_default_params(&params_, Q, minDisparity);
    params_.disparity_mode = disparityMode; params_.handle_missing_values = handleMissingValues ? 1 : 0; params_.max_z = maxZ;
    status_ = rtdm_xyz_create(&params_, maxWidth, maxHeight, 1, device, &xyz_);
    if (status_ != RTDM_OK) std::fprintf(stderr, "HIPXYZCore: %s\n", rtdm_strerror(status_));
}
HIPXYZCore::~HIPXYZCore() { rtdm_xyz_destroy(xyz_); }
int HIPXYZCore::set(const rtdm_xyz_params& p)
{
    if (!xyz_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_xyz_set_params(xyz_, &p);
    if (status_ == RTDM_OK) params_ = p;
    return status_;
}
int HIPXYZCore::setQ(const double Q[16])
{
    if (!Q) return status_ = RTDM_ERR_NULL;
    rtdm_xyz_params p = params_;
    for (int i = 0; i < 16; ++i) p.Q[i] = Q[i];
    return set(p);
}
int HIPXYZCore::setDisparityMode(int v) { rtdm_xyz_params p = params_; p.disparity_mode = v; return set(p); }
int HIPXYZCore::setHandleMissingValues(bool v) { rtdm_xyz_params p = params_; p.handle_missing_values = v ? 1 : 0; return set(p); }
int HIPXYZCore::setMaxZ(double v) { rtdm_xyz_params p = params_; p.max_z = v; return set(p); }
int HIPXYZCore::reprojectImageTo3D(const int16_t* disp, size_t dispStep, int rows, int cols, float* xyz, size_t xyzStep, float* z,
                                   size_t zStep)
{
    if (!xyz_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_xyz_map(xyz_, disp, dispStep, cols, rows, xyz, xyzStep, z, zStep);
    return status_;
}
int HIPXYZCore::cloud(const int16_t* disp, size_t dispStep, const uint8_t* guide, size_t guideStep, int channels,
                      const uint8_t* mask, size_t maskStep, int rows, int cols, rtdm_point* points, int capacity, int* count)
{
    if (!xyz_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_xyz_cloud(xyz_, disp, dispStep, guide, guideStep, channels, mask, maskStep, cols, rows, points, capacity, count);
    return status_;
}
int HIPXYZCore::computeCloud(HIPMatcherCore& matcher, const uint8_t* left, size_t leftStep, const uint8_t* right, size_t rightStep,
                             int rows, int cols, const uint8_t* guide, size_t guideStep, int channels, const uint8_t* mask,
                             size_t maskStep, rtdm_point* points, int capacity, int* count, int16_t* disp, size_t dispStep)
{
    if (!xyz_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_bm_compute_cloud(matcher.handle(), xyz_, left, leftStep, right, rightStep, cols, rows, guide, guideStep,
                                    channels, mask, maskStep, points, capacity, count, disp, dispStep);
    return status_;
}

HIPMJPEGCore::HIPMJPEGCore(int maxWidth, int maxHeight, size_t maxStreamBytes, int device)
{
    if (maxStreamBytes == 0 && maxWidth > 0 && maxHeight > 0) {
        maxStreamBytes = (size_t)maxWidth * maxHeight * 3;
        if (maxStreamBytes < 4096) maxStreamBytes = 4096;
    }
    status_ = rtdm_mjpeg_create(maxWidth, maxHeight, 1, maxStreamBytes, device, &dec_);
    if (status_ != RTDM_OK) std::fprintf(stderr, "HIPMJPEGDecoder: %s\n", rtdm_strerror(status_));
}
HIPMJPEGCore::~HIPMJPEGCore() { rtdm_mjpeg_destroy(dec_); }
int HIPMJPEGCore::decode(const uint8_t* in, size_t len, int width, int height, uint8_t* out, size_t outStep)
{
    if (!dec_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    return rtdm_mjpeg_decode(dec_, in, len, width, height, out, outStep ? outStep : (size_t)width * 3);
}
int HIPMJPEGCore::compute(HIPMatcherCore& matcher, HIPRectifierCore& rectifier, const uint8_t* left, size_t leftLen,
                          const uint8_t* right, size_t rightLen, int width, int height, int16_t* out, size_t outStep)
{
    if (!dec_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    return rtdm_bm_compute_mjpeg(matcher.handle(), rectifier.handle(), dec_, left, leftLen, right, rightLen, width, height, out,
                                 outStep);
}

int HIPMJPEGCore::setSplit(int subsequenceBytes)
{
    if (!dec_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    return rtdm_mjpeg_set_split(dec_, subsequenceBytes);
}
int HIPMJPEGCore::splitStats(long* framesSplit, long* subsequences, int* maxRounds)
{
    if (!dec_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    return rtdm_mjpeg_get_split_stats(dec_, framesSplit, subsequences, maxRounds);
}

HIPMorphCore::HIPMorphCore(int w, int h, int bpp, int device) : width_(w), height_(h), bpp_(bpp)
{
    status_ = (bpp == 8) ? rtdm_morph_create(w, h, 1, device, &mf_) : RTDM_ERR_UNSUPPORTED;
    if (status_ != RTDM_OK) std::fprintf(stderr, "HIPMorphologicalFilter: %s\n", rtdm_strerror(status_));
}
HIPMorphCore::~HIPMorphCore() { rtdm_morph_destroy(mf_); }
char* HIPMorphCore::getVideoInBuffer() { return (char*)rtdm_morph_in_buffer(mf_); }
char* HIPMorphCore::getVideoOutBuffer() { return (char*)rtdm_morph_out_buffer(mf_); }
int HIPMorphCore::run(const uint8_t* in, size_t inStep, uint8_t* out, size_t outStep, int rows, int cols)
{
    if (!mf_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    status_ = rtdm_morph_run(mf_, in, inStep, out, outStep, cols, rows);
    return status_;
}
int HIPMorphCore::setElement(int shape, int width, int height)
{
    rtdm_morph_element el;
    int op = 0, iterations = 0;
    int rc = rtdm_morph_make_element(shape, width, height, &el);
    if (rc != RTDM_OK) return rc;
    if (!mf_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    rc = rtdm_morph_get_op(mf_, &op, &iterations, NULL);
    return rc != RTDM_OK ? rc : rtdm_morph_set_op(mf_, op, iterations, &el);
}
int HIPMorphCore::setOperation(int op, int iterations)
{
    if (!mf_) return status_ != RTDM_OK ? status_ : RTDM_ERR_NO_DEVICE;
    rtdm_morph_element el;
    const int rc = rtdm_morph_get_op(mf_, NULL, NULL, &el);
    return rc != RTDM_OK ? rc : rtdm_morph_set_op(mf_, op, iterations, &el);
}

}  // namespace rtdm
