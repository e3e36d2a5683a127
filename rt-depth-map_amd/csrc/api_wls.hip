// api_wls.hip -- rtdm_wls: the disparity WLS post-filter (ENABLE_POST_FILTER, estimator.cpp:57-70; rules W1-W8, DESIGN.md
// section 4.9) and the parameter helpers of its right matcher.
#include "rtdm_handles.h"

using namespace rtdm;

static const int WLS_LUT_N = 3 * 255 * 255 + 1;

static int wls_validate(const rtdm_wls_params& p)
{
    if (!(p.lambda >= 0.0) || !(p.sigma_color > 0.0) || p.lrc_thresh < 0 || p.depth_discontinuity_radius < 0) return RTDM_ERR_BAD_PARAM;
    if (p.roi_left < 0 || p.roi_right < 0 || p.roi_top < 0 || p.roi_bottom < 0) return RTDM_ERR_BAD_PARAM;
    if (p.num_iter < 1 || p.num_iter > RTDM_WLS_MAX_ITER || !(p.attenuation > 0.0 && p.attenuation <= 1.0)) return RTDM_ERR_BAD_PARAM;
    if (p.use_confidence != 0 && p.use_confidence != 1) return RTDM_ERR_BAD_PARAM;
    // both invalid values, (minD - 1) * 16 and -(minD + numD) * 16, are int16 (the matchers' own bound)
    if (p.num_disparities <= 0 || p.min_disparity < -2047 || (long)p.min_disparity + p.num_disparities > 2047) return RTDM_ERR_BAD_PARAM;
    return RTDM_OK;
}

// W5: computed in double, rounded to float, values below FLT_MIN flushed to 0 (tests/wls_ref.py builds the same table)
static int wls_upload_lut(rtdm_wls* h)
{
    std::vector<float> lut(WLS_LUT_N);
    for (int k = 0; k < WLS_LUT_N; ++k) {
        const float v = (float)std::exp(-std::sqrt((double)k) / h->p.sigma_color);
        lut[k] = v < FLT_MIN ? 0.0f : v;
    }
    HIPC(hipMemcpy(h->dLut, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
    return RTDM_OK;
}

static WlsGeom wls_geom(const rtdm_wls_params& p, int W, int H)
{
    WlsGeom g{p.roi_left, W - p.roi_right, p.roi_top, H - p.roi_bottom};
    if (g.x1 <= g.x0 || g.y1 <= g.y0) g = WlsGeom{0, 0, 0, 0};     // empty ROI: the whole output is invalid
    return g;
}

int rtdm_wls_params_for_bm(const rtdm_bm_params* left, rtdm_wls_params* out)
{
    if (!left || !out) return RTDM_ERR_NULL;
    const int w = left->blockSize, minD = left->minDisparity, numD = left->numDisparities;
    out->lambda = 8000.0; out->sigma_color = 1.5; out->lrc_thresh = 24; out->num_iter = 3; out->attenuation = 0.25;
    out->use_confidence = 1;
    out->depth_discontinuity_radius = (int)std::ceil(0.33 * w);
    out->min_disparity = minD; out->num_disparities = numD;
    out->roi_left = std::max(0, minD + numD) + w / 2;
    out->roi_right = std::max(0, -minD) + w / 2;
    out->roi_top = w / 2; out->roi_bottom = w / 2;
    return RTDM_OK;
}

int rtdm_wls_params_for_sgm(const rtdm_sgm_params* left, rtdm_wls_params* out)
{
    if (!left || !out) return RTDM_ERR_NULL;
    const int w = left->blockSize, minD = left->minDisparity, numD = left->numDisparities;
    out->lambda = 8000.0; out->sigma_color = 1.5; out->lrc_thresh = 24; out->num_iter = 3; out->attenuation = 0.25;
    out->use_confidence = 1;
    out->depth_discontinuity_radius = (int)std::ceil(0.5 * w);
    out->min_disparity = minD; out->num_disparities = numD;
    out->roi_left = std::max(0, minD + numD);
    out->roi_right = std::max(0, -minD);
    out->roi_top = 0; out->roi_bottom = 0;
    return RTDM_OK;
}

int rtdm_bm_right_params(const rtdm_bm_params* left, rtdm_bm_params* right)
{
    if (!left || !right) return RTDM_ERR_NULL;
    *right = *left;                // numDisparities, blockSize, preFilterCap (and the border rule) carry over
    right->minDisparity = -(left->minDisparity + left->numDisparities) + 1;
    right->textureThreshold = 0; right->uniquenessRatio = 0; right->speckleWindowSize = 0; right->disp12MaxDiff = 1000000;
    return RTDM_OK;
}

int rtdm_sgm_right_params(const rtdm_sgm_params* left, rtdm_sgm_params* right)
{
    if (!left || !right) return RTDM_ERR_NULL;
    *right = *left;                // numDisparities, blockSize, P1, P2, paths carry over; preFilterCap is the caller's to copy
    right->minDisparity = -(left->minDisparity + left->numDisparities) + 1;
    right->uniquenessRatio = 0; right->speckleWindowSize = 0; right->disp12MaxDiff = 1000000;
    return RTDM_OK;
}

void rtdm_wls_destroy(rtdm_wls* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->mem.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int rtdm_wls_create(const rtdm_wls_params* params, int max_width, int max_height, int max_batch, int device, rtdm_wls** out)
{
    if (!params || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    int rc = wls_validate(*params);
    if (rc) return rc;
    if (max_width <= 0 || max_height <= 0 || max_batch <= 0) return RTDM_ERR_BAD_SIZE;
    if (max_width > 4096 || max_height > 4096) return RTDM_ERR_UNSUPPORTED;   // one wave solves a whole row / column segment
    if ((long)max_batch * max_width * max_height >= (1L << 31)) return RTDM_ERR_BAD_SIZE;
    rc = use_device(device);
    if (rc) return rc;
    rtdm_wls* h = new (std::nothrow) rtdm_wls();
    if (!h) return RTDM_ERR_NOMEM;
    h->p = *params; h->maxW = max_width; h->maxH = max_height; h->maxB = max_batch; h->device = device;
    const size_t px = (size_t)max_width * max_height * max_batch, fr = (size_t)max_width * max_height;
    AllocList& m = h->mem;
    m.err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    m.dev(&h->dLut, WLS_LUT_N * sizeof(float)); m.dev(&h->dF, px * sizeof(float2)); m.dev(&h->dWh, px * 4); m.dev(&h->dWv, px * 4);
    m.dev(&h->dConf, px); m.dev(&h->dMML, px * sizeof(WlsMM)); m.dev(&h->dMMR, px * sizeof(WlsMM));
    m.dev(&h->dInL, fr * 2); m.dev(&h->dInR, fr * 2); m.dev(&h->dOut, fr * 2); m.dev(&h->dGuide, fr * 3); m.dev(&h->dImgR, fr);
    m.dev(&h->dConfOut, fr * 4); m.dev(&h->dFilt, fr * 4);
    if (m.err != hipSuccess) { const hipError_t e = m.err; rtdm_wls_destroy(h); return create_failed("rtdm_wls_create", e); }
    rc = wls_upload_lut(h);
    if (rc) { rtdm_wls_destroy(h); return rc; }
    *out = h;
    return RTDM_OK;
}

int rtdm_wls_set_params(rtdm_wls* h, const rtdm_wls_params* params)
{
    if (!h || !params) return RTDM_ERR_NULL;
    const int rc = wls_validate(*params);
    if (rc) return rc;
    const bool lut = params->sigma_color != h->p.sigma_color;
    h->p = *params;
    if (!lut) return RTDM_OK;
    HIPC(hipSetDevice(h->device));
    HIPC(hipDeviceSynchronize());  // a filter call in flight on any stream may still read the old table
    return wls_upload_lut(h);
}

int rtdm_wls_get_params(const rtdm_wls* h, rtdm_wls_params* out)
{
    if (!h || !out) return RTDM_ERR_NULL;
    *out = h->p;
    return RTDM_OK;
}

// one chunk of <= maxB frames through the launch sequence of k_wls.hip
int rtdm::wls_chunk(rtdm_wls* h, int n, WlsDisp dl, WlsDisp dr, WlsGuide G, WlsOut o, int W, int H, hipStream_t s)
{
    const rtdm_wls_params& p = h->p;
    WlsLaunch L{};
    L.dl = dl; L.dr = dr; L.guide = G; L.out = o;
    L.g = wls_geom(p, W, H);
    L.W = W; L.H = H; L.r = p.depth_discontinuity_radius; L.T = p.lrc_thresh;
    L.invL = (p.min_disparity - 1) * 16;
    L.invR = -(p.min_disparity + p.num_disparities) * 16;       // (minDR - 1) * 16, minDR = -(minD + numD) + 1
    L.use_conf = p.use_confidence; L.num_iter = p.num_iter;
    // W6: lambda_0 = 1.5 lambda 4^(T-1) / (4^T - 1), then * attenuation per iteration (double, rounded once per pass)
    double lam = 1.5 * p.lambda * std::pow(4.0, p.num_iter - 1) / (std::pow(4.0, p.num_iter) - 1.0);
    for (int t = 0; t < p.num_iter; ++t) { L.lambda[t] = (float)lam; lam *= p.attenuation; }
    L.lut = h->dLut;
    L.pitch = (size_t)h->maxW; L.frame = (size_t)h->maxW * h->maxH;
    L.F = h->dF; L.wh = h->dWh; L.wv = h->dWv; L.conf = h->dConf; L.mmL = h->dMML; L.mmR = h->dMMR;
    launch_wls(L, n, s);
    HIPC(hipGetLastError());
    return RTDM_OK;
}

int rtdm::wls_check(const rtdm_wls* h, int channels, int W, int H)
{
    if (channels != 1 && channels != 3) return RTDM_ERR_BAD_PARAM;
    if (W <= 0 || H <= 0 || W > h->maxW || H > h->maxH) return RTDM_ERR_BAD_SIZE;
    return RTDM_OK;
}

int rtdm_wls_filter_device(rtdm_wls* h, int n, const int16_t* d_left, size_t left_pitch, size_t left_frame_stride,
                           const int16_t* d_right, size_t right_pitch, size_t right_frame_stride, const uint8_t* d_guide,
                           size_t guide_pitch, size_t guide_frame_stride, int channels, int width, int height,
                           int16_t* d_out, size_t out_pitch, size_t out_frame_stride, float* d_conf, size_t conf_pitch,
                           size_t conf_frame_stride, float* d_filtered, size_t filtered_pitch, size_t filtered_frame_stride,
                           void* hip_stream)
{
    if (!h || !d_left || !d_guide || !d_out || (h->p.use_confidence && !d_right)) return RTDM_ERR_NULL;
    int rc = wls_check(h, channels, width, height);
    if (rc) return rc;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    const size_t W = (size_t)width;
    const bool cr = h->p.use_confidence;
    if (left_pitch < 2 * W || ((left_pitch | left_frame_stride) & 1) || guide_pitch < W * channels ||
        out_pitch < 2 * W || ((out_pitch | out_frame_stride) & 1) ||
        (cr && (right_pitch < 2 * W || ((right_pitch | right_frame_stride) & 1))) ||
        (d_conf && (conf_pitch < 4 * W || ((conf_pitch | conf_frame_stride) & 3))) ||
        (d_filtered && (filtered_pitch < 4 * W || ((filtered_pitch | filtered_frame_stride) & 3))))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    for (int i0 = 0; i0 < n; i0 += h->maxB) {
        const int m = std::min(h->maxB, n - i0);
        WlsDisp dl{d_left + (size_t)i0 * (left_frame_stride / 2), left_pitch / 2, left_frame_stride / 2};
        WlsDisp dr{cr ? d_right + (size_t)i0 * (right_frame_stride / 2) : d_left, cr ? right_pitch / 2 : 0, cr ? right_frame_stride / 2 : 0};
        WlsGuide G{d_guide + (size_t)i0 * guide_frame_stride, guide_pitch, guide_frame_stride, channels};
        WlsOut o{d_out + (size_t)i0 * (out_frame_stride / 2), out_pitch / 2, out_frame_stride / 2,
                 d_filtered ? d_filtered + (size_t)i0 * (filtered_frame_stride / 4) : nullptr, filtered_pitch / 4, filtered_frame_stride / 4,
                 d_conf ? d_conf + (size_t)i0 * (conf_frame_stride / 4) : nullptr, conf_pitch / 4, conf_frame_stride / 4};
        rc = wls_chunk(h, m, dl, dr, G, o, width, height, s);
        if (rc) return rc;
    }
    return RTDM_OK;
}

// the outputs of one staged frame back to the caller's planes
int rtdm::wls_download(rtdm_wls* h, int W, int H, int16_t* out, size_t out_pitch, float* conf, size_t conf_pitch, float* filtered,
                       size_t filtered_pitch, hipStream_t s)
{
    HIPC(hipMemcpy2DAsync(out, out_pitch, h->dOut, (size_t)W * 2, (size_t)W * 2, H, hipMemcpyDeviceToHost, s));
    if (conf) HIPC(hipMemcpy2DAsync(conf, conf_pitch, h->dConfOut, (size_t)W * 4, (size_t)W * 4, H, hipMemcpyDeviceToHost, s));
    if (filtered) HIPC(hipMemcpy2DAsync(filtered, filtered_pitch, h->dFilt, (size_t)W * 4, (size_t)W * 4, H, hipMemcpyDeviceToHost, s));
    return RTDM_OK;
}

int rtdm_wls_filter(rtdm_wls* h, const int16_t* disp_left, size_t left_pitch, const int16_t* disp_right, size_t right_pitch,
                    const uint8_t* guide, size_t guide_pitch, int channels, int width, int height, int16_t* out,
                    size_t out_pitch, float* conf, size_t conf_pitch, float* filtered, size_t filtered_pitch)
{
    if (!h || !disp_left || !guide || !out || (h->p.use_confidence && !disp_right)) return RTDM_ERR_NULL;
    int rc = wls_check(h, channels, width, height);
    if (rc) return rc;
    const size_t W = (size_t)width;
    const bool cr = h->p.use_confidence;
    if (left_pitch < 2 * W || (cr && right_pitch < 2 * W) || guide_pitch < W * channels || out_pitch < 2 * W ||
        (conf && conf_pitch < 4 * W) || (filtered && filtered_pitch < 4 * W))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(h->dInL, W * 2, disp_left, left_pitch, W * 2, height, hipMemcpyHostToDevice, s));
    if (cr) HIPC(hipMemcpy2DAsync(h->dInR, W * 2, disp_right, right_pitch, W * 2, height, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpy2DAsync(h->dGuide, W * channels, guide, guide_pitch, W * channels, height, hipMemcpyHostToDevice, s));
    const size_t fr = W * height;
    WlsDisp dl{h->dInL, W, fr}, dr{h->dInR, W, fr};
    WlsGuide G{h->dGuide, W * channels, fr * channels, channels};
    WlsOut o{h->dOut, W, fr, filtered ? h->dFilt : nullptr, W, fr, conf ? h->dConfOut : nullptr, W, fr};
    rc = wls_chunk(h, 1, dl, dr, G, o, width, height, s);
    if (rc) return rc;
    rc = wls_download(h, width, height, out, out_pitch, conf, conf_pitch, filtered, filtered_pitch, s);
    if (rc) return rc;
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    return RTDM_OK;
}
