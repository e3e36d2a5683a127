// api_chain.hip -- the entry points that run two or three handles in one call, on one stream.
#include "rtdm_handles.h"

using namespace rtdm;

// gray + remap + crop of n device frames into the rectifier's planes, then the matcher, chunk by chunk
static int rgb_chunks(rtdm_bm* bm, rtdm_rectify* rc, int n, const uint8_t* dl, const uint8_t* dr, Plane16W out, hipStream_t s)
{
    const size_t fbytes = (size_t)rc->W * rc->H * 3, gframe = rc->gpitch * rc->rh;
    const int chunk = std::min(bm->maxB, rc->maxB);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        rectify_gray_launch(rc, dl + (size_t)i0 * fbytes, dr + (size_t)i0 * fbytes, m,
                            Plane8W{rc->dGray[0], rc->gpitch, gframe}, Plane8W{rc->dGray[1], rc->gpitch, gframe}, s);
        HIPC(hipGetLastError());
        const int st = bm_run_chunk(bm, m, Plane8{rc->dGray[0], rc->gpitch, gframe}, Plane8{rc->dGray[1], rc->gpitch, gframe},
                                 rc->rw, rc->rh, Plane16W{out.base + (size_t)i0 * out.frame_e, out.pitch_e, out.frame_e}, s);
        if (st) return st;
    }
    return RTDM_OK;
}

int rtdm_bm_compute_rgb_device(rtdm_bm* bm, rtdm_rectify* rc, int n, const uint8_t* d_rgb_left,
                               const uint8_t* d_rgb_right, int16_t* d_disp, void* hip_stream)
{
    if (!bm || !rc || !d_rgb_left || !d_rgb_right || !d_disp) return RTDM_ERR_NULL;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    if (bm->device != rc->device) return RTDM_ERR_BAD_PARAM;
    int st = bm_check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    HIPC(hipSetDevice(bm->device));
    const size_t oframe = (size_t)rc->rw * rc->rh;
    return rgb_chunks(bm, rc, n, d_rgb_left, d_rgb_right, Plane16W{d_disp, (size_t)rc->rw, oframe}, (hipStream_t)hip_stream);
}

int rtdm_bm_compute_rgb(rtdm_bm* bm, rtdm_rectify* rc, const uint8_t* rgb_left, size_t left_pitch,
                        const uint8_t* rgb_right, size_t right_pitch, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !rc || !rgb_left || !rgb_right || !disp) return RTDM_ERR_NULL;
    if (bm->device != rc->device) return RTDM_ERR_BAD_PARAM;
    int st = bm_check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    const size_t row = (size_t)rc->W * 3;
    if (left_pitch < row || right_pitch < row || disp_pitch < (size_t)rc->rw * 2) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    DrainOnError drain{s};
    st = rectify_upload(rc, rgb_left, left_pitch, rgb_right, right_pitch, s);
    if (st) return st;
    st = rgb_chunks(bm, rc, 1, rc->dRgb[0], rc->dRgb[1], bm_internal_plane(bm, rc->rw, rc->rh), s);
    if (st == RTDM_OK) st = bm_download_disp(bm, rc->rw, rc->rh, s);
    if (st) return st;
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    bm_scatter_disp(bm, rc->rw, rc->rh, disp, disp_pitch);
    return RTDM_OK;
}

// the boxes [first, first + count) of a single-frame estimate are measured under this mask plane (rows of `pitch` bytes)
struct MaskRun { const uint8_t* mask; size_t pitch; int first, count; };

// The end of both single-frame estimates (estimator.cpp:54-56, 75-77): the matcher inside the objects' union box `roi`, the depth
// of every box under its run's mask (one minimum per map: reuse_min from the second run on), the disparity map on request.
static int estimate_tail(rtdm_bm* bm, rtdm_rectify* rc, const int* roi, const rtdm_region* boxes, int nreg, const MaskRun* runs, int nruns,
                         const double* Q, double calibration_unit, double* mean_cm, int* counts, int16_t* disp, size_t disp_pitch,
                         DrainOnError* drain)
{
    hipStream_t s = bm->stream;
    const int W = rc->rw, H = rc->rh;
    const size_t gframe = rc->gpitch * H;
    int st = rtdm_bm_set_roi(bm, 1, roi[0], roi[1], roi[2], roi[3]);
    if (st) return st;
    const Plane16W O = bm_internal_plane(bm, W, H);
    st = bm_run_chunk(bm, 1, Plane8{rc->dGray[0], rc->gpitch, gframe}, Plane8{rc->dGray[1], rc->gpitch, gframe}, W, H, O, s);
    if (st) return st;
    int flat[4 * RTDM_MAX_REGIONS], maxh = 1;
    st = depth_check_regions(boxes, nreg, W, H, flat, &maxh);
    if (st) return st;
    DepthQ q; std::copy(Q, Q + 16, q.q);
    for (int r = 0; r < nruns; ++r)
        launch_depth_stats(bm->dOut, O.pitch_e, W, H, q, runs[r].mask, runs[r].pitch, flat + 4 * runs[r].first, runs[r].count, bm->maxH,
                           calibration_unit, bm->dDepth, mean_cm + runs[r].first, counts + runs[r].first, s, r > 0);
    if (disp) { st = bm_download_disp(bm, W, H, s); if (st) return st; }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    drain->armed = false;
    if (disp) bm_scatter_disp(bm, W, H, disp, disp_pitch);
    return RTDM_OK;
}

int rtdm_estimate_frame(rtdm_bm* bm, rtdm_rectify* rc, rtdm_objects* ob, const uint8_t* rgb_left, size_t left_pitch,
                        const uint8_t* rgb_right, size_t right_pitch, const double* Q, const rtdm_hsv_range* range,
                        int min_area, int zero_border, double calibration_unit, rtdm_region* boxes, double* mean_cm,
                        int* counts, int max_boxes, int* nboxes, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !rc || !ob || !rgb_left || !rgb_right || !Q || !range || !boxes || !mean_cm || !counts || !nboxes) return RTDM_ERR_NULL;
    if (bm->device != rc->device || bm->device != ob->device) return RTDM_ERR_BAD_PARAM;
    if (ob->W != rc->rw || ob->H != rc->rh || max_boxes <= 0) return RTDM_ERR_BAD_SIZE;
    int st = bm_check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    const int W = rc->rw, H = rc->rh;
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H;
    if (left_pitch < row || right_pitch < row || (disp && disp_pitch < (size_t)W * 2)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    DrainOnError drain{s};
    st = rectify_upload(rc, rgb_left, left_pitch, rgb_right, right_pitch, s);
    if (st) return st;
    // estimator.cpp:29-39: both gray crops and the colour crop of the left frame
    const size_t gframe = rc->gpitch * H;
    rectify_gray_launch(rc, rc->dRgb[0], rc->dRgb[1], 1, Plane8W{rc->dGray[0], rc->gpitch, gframe}, Plane8W{rc->dGray[1], rc->gpitch, gframe}, s);
    launch_rectify_rgb(RectifySrc{rc->dRgb[0], row, fbytes}, rc->dMap1[0], rc->dMap2[0], rc->W, rc->H, W, H,
                       Plane8W{ob->dRgb, (size_t)W * 3, (size_t)W * 3 * H}, 1, s);
    // estimator.cpp:40-53
    rtdm_region roi;
    st = objects_run(ob, range, min_area, zero_border, boxes, max_boxes, nboxes, &roi, s);
    if (st) return st;
    if (*nboxes == 0) { drain.armed = false; return RTDM_OK; }      // estimator.cpp:48: nothing to measure in this frame
    const int nreg = std::min(std::min(*nboxes, max_boxes), RTDM_MAX_REGIONS);
    const int box[4] = {roi.x, roi.y, roi.width, roi.height};
    const MaskRun run{ob->dMaskOut, (size_t)W, 0, nreg};
    return estimate_tail(bm, rc, box, boxes, nreg, &run, 1, Q, calibration_unit, mean_cm, counts, disp, disp_pitch, &drain);
}

// rtdm_estimate_frame with several colour classes: the batched detector on the one rectified frame, selection on the device;
// the read-back that decides ROI1 brings the per-class counts, the union box and the stored objects.
int rtdm_estimate_frame_classes(rtdm_bm* bm, rtdm_rectify* rc, rtdm_objects* ob, const uint8_t* rgb_left, size_t left_pitch,
                                const uint8_t* rgb_right, size_t right_pitch, const double* Q, const rtdm_hsv_range* ranges,
                                const int* range_class, int nranges, int nclasses, int min_area, int zero_border,
                                double calibration_unit, rtdm_object* objects, double* mean_cm, int* counts, int max_objects,
                                int* nobjects, int16_t* disp, size_t disp_pitch)
{
    if (!rgb_left || !rgb_right || !Q || !objects || !mean_cm || !counts || !nobjects) return RTDM_ERR_NULL;
    HsvClasses C;
    int st = objects_classes_check(ranges, range_class, nranges, nclasses, &C);
    if (st) return st;
    if (!bm || !rc || !ob) return RTDM_ERR_NULL;
    if (bm->device != rc->device || bm->device != ob->device || nclasses > ob->maxC) return RTDM_ERR_BAD_PARAM;
    if (ob->W != rc->rw || ob->H != rc->rh || max_objects <= 0) return RTDM_ERR_BAD_SIZE;
    st = bm_check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    const int W = rc->rw, H = rc->rh, K = nclasses;
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H;
    if (left_pitch < row || right_pitch < row || (disp && disp_pitch < (size_t)W * 2)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    DrainOnError drain{s};
    const int cap = (int)std::min((size_t)max_objects, (size_t)K * ob->maxRec);
    st = objects_stage(ob, (size_t)cap);
    if (st) return st;
    st = rectify_upload(rc, rgb_left, left_pitch, rgb_right, right_pitch, s);
    if (st) return st;
    const size_t gframe = rc->gpitch * H, cp = objects_rgb_pitch(ob);
    rectify_gray_launch(rc, rc->dRgb[0], rc->dRgb[1], 1, Plane8W{rc->dGray[0], rc->gpitch, gframe}, Plane8W{rc->dGray[1], rc->gpitch, gframe}, s);
    launch_rectify_rgb(RectifySrc{rc->dRgb[0], row, fbytes}, rc->dMap1[0], rc->dMap2[0], rc->W, rc->H, W, H,
                       Plane8W{ob->dRgb, cp, cp * H}, 1, s);
    int* dCounts = ob->dMeta;
    int* dRoi = ob->dMeta + (size_t)ob->maxB * ob->maxC;
    st = objects_run_chunk(ob, 1, ob->dRgb, cp, cp * H, C, min_area, zero_border, nullptr, 0, 0, ob->dObj, cap, dCounts, dRoi, s);
    if (st) return st;
    int* hCounts = ob->hRec;
    int* hRoi = ob->hRec + K;
    HIPC(hipMemcpyAsync(hCounts, dCounts, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(hRoi, dRoi, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    long total = 0;
    for (int c = 0; c < K; ++c) total += hCounts[c];
    *nobjects = (int)total;
    if (total == 0) { drain.armed = false; return RTDM_OK; }        // estimator.cpp:48: nothing to measure in this frame
    const int stored = (int)std::min<long>(total, cap);
    HIPC(hipMemcpy(objects, ob->dObj, (size_t)stored * sizeof(rtdm_object), hipMemcpyDeviceToHost));
    const int nreg = std::min(stored, RTDM_MAX_REGIONS);
    // every class's objects over that class's filtered mask; the lists lie class after class
    rtdm_region boxes[RTDM_MAX_REGIONS];
    MaskRun runs[RTDM_MAX_REGIONS];
    int nruns = 0;
    for (int i = 0; i < nreg; ++i) {
        boxes[i] = rtdm_region{objects[i].x, objects[i].y, objects[i].width, objects[i].height};
        if (i > 0 && objects[i].cls == objects[i - 1].cls) { ++runs[nruns - 1].count; continue; }
        runs[nruns++] = MaskRun{ob->dMaskOut + (size_t)objects[i].cls * ob->mpitch * H, ob->mpitch, i, 1};
    }
    return estimate_tail(bm, rc, hRoi, boxes, nreg, runs, nruns, Q, calibration_unit, mean_cm, counts, disp, disp_pitch, &drain);
}

int rtdm_bm_compute_filtered(rtdm_bm* left_bm, rtdm_bm* right_bm, rtdm_wls* wls, const uint8_t* left, size_t left_pitch,
                             const uint8_t* right, size_t right_pitch, int width, int height, int16_t* out, size_t out_pitch,
                             int16_t* raw_left, size_t raw_left_pitch)
{
    if (!left_bm || !wls || !left || !right || !out || (wls->p.use_confidence && !right_bm)) return RTDM_ERR_NULL;
    const bool cr = wls->p.use_confidence;
    if (left_bm->device != wls->device || (cr && right_bm->device != wls->device)) return RTDM_ERR_BAD_PARAM;
    int rc = wls_check(wls, 1, width, height);
    if (rc) return rc;
    const size_t W = (size_t)width, fr = W * height;
    if (left_pitch < W || right_pitch < W || out_pitch < 2 * W || (raw_left && raw_left_pitch < 2 * W)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(wls->device));
    hipStream_t s = wls->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(wls->dGuide, W, left, left_pitch, W, height, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpy2DAsync(wls->dImgR, W, right, right_pitch, W, height, hipMemcpyHostToDevice, s));
    rc = rtdm_bm_compute_device(left_bm, 1, wls->dGuide, wls->dImgR, W, fr, width, height, wls->dInL, W * 2, fr * 2, s);
    if (rc) return rc;
    if (cr) {                      // createRightMatcher's handle, called as compute(right, left)
        rc = rtdm_bm_compute_device(right_bm, 1, wls->dImgR, wls->dGuide, W, fr, width, height, wls->dInR, W * 2, fr * 2, s);
        if (rc) return rc;
    }
    HIPC(hipSetDevice(wls->device));
    WlsDisp dl{wls->dInL, W, fr}, dr{wls->dInR, W, fr};
    WlsGuide G{wls->dGuide, W, fr, 1};
    WlsOut o{wls->dOut, W, fr, nullptr, W, fr, nullptr, W, fr};
    rc = wls_chunk(wls, 1, dl, dr, G, o, width, height, s);
    if (rc) return rc;
    rc = wls_download(wls, width, height, out, out_pitch, nullptr, 0, nullptr, 0, s);
    if (rc) return rc;
    if (raw_left) HIPC(hipMemcpy2DAsync(raw_left, raw_left_pitch, wls->dInL, W * 2, W * 2, height, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    return RTDM_OK;
}

int rtdm_bm_compute_cloud(rtdm_bm* bm, rtdm_xyz* h, const uint8_t* left, size_t left_pitch, const uint8_t* right,
                          size_t right_pitch, int width, int height, const uint8_t* guide, size_t guide_pitch, int channels,
                          const uint8_t* mask, size_t mask_pitch, rtdm_point* points, int capacity, int* count, int16_t* disp,
                          size_t disp_pitch)
{
    if (!bm || !left || !right) return RTDM_ERR_NULL;
    int rc = xyz_cloud_check(h, left, guide, channels, width, height, points, capacity, count);
    if (rc) return rc;
    if (bm->device != h->device || bm->p.minDisparity != h->p.min_disparity) return RTDM_ERR_BAD_PARAM;
    rc = bm_check_frame(bm, width, height);
    if (rc) return rc;
    const size_t W = (size_t)width, fr = W * height;
    if (left_pitch < W || right_pitch < W || (channels && guide_pitch < W * channels) || (mask && mask_pitch < W) ||
        (disp && disp_pitch < 2 * W))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(h->dImgL, W, left, left_pitch, W, height, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpy2DAsync(h->dImgR, W, right, right_pitch, W, height, hipMemcpyHostToDevice, s));
    if (channels) HIPC(hipMemcpy2DAsync(h->dGuide, W * channels, guide, guide_pitch, W * channels, height, hipMemcpyHostToDevice, s));
    if (mask) HIPC(hipMemcpy2DAsync(h->dMask, W, mask, mask_pitch, W, height, hipMemcpyHostToDevice, s));
    rc = rtdm_bm_compute_device(bm, 1, h->dImgL, h->dImgR, W, fr, width, height, h->dDisp, W * 2, fr * 2, s);
    if (rc) return rc;
    HIPC(hipSetDevice(h->device));
    rc = xyz_cloud_staged(h, channels, mask != nullptr, width, height, points, capacity, count, s);
    if (rc) return rc;
    if (disp) {
        HIPC(hipMemcpy2DAsync(disp, disp_pitch, h->dDisp, W * 2, W * 2, height, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
    }
    drain.armed = false;
    return RTDM_OK;
}

int rtdm_bm_compute_mjpeg(rtdm_bm* bm, rtdm_rectify* rc, rtdm_mjpeg* dec, const uint8_t* left, size_t left_len,
                          const uint8_t* right, size_t right_len, int width, int height, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !rc || !dec || !left || !right || !disp) return RTDM_ERR_NULL;
    if (bm->device != rc->device || bm->device != dec->device) return RTDM_ERR_BAD_PARAM;
    if (width != rc->W || height != rc->H || width > dec->maxW || height > dec->maxH) return RTDM_ERR_BAD_SIZE;
    int st = bm_check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    if (disp_pitch < (size_t)rc->rw * 2) return RTDM_ERR_BAD_SIZE;
    const uint8_t* src[2] = {left, right};
    const size_t len[2] = {left_len, right_len};
    for (int k = 0; k < 2; ++k) {                    // refusals before any device use
        st = mjpeg_check(dec, src[k], len[k], width, height);
        if (st) return st;
    }
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    DrainOnError drain{s};
    const size_t row = (size_t)width * 3;
    for (int k = 0; k < 2; ++k) {                    // the two cameras may differ in sampling: one chunk each
        MjpegDesc shape;
        shape.ncomp = 0;
        st = mjpeg_chunk(dec, 1, src + k, len + k, width, height, rc->dRgb[k], row, row * height, dec->dStatus + k, s, &shape);
        if (st) return st;
    }
    HIPC(hipMemcpyAsync(dec->hStatus, dec->dStatus, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    st = rgb_chunks(bm, rc, 1, rc->dRgb[0], rc->dRgb[1], bm_internal_plane(bm, rc->rw, rc->rh), s);
    if (st == RTDM_OK) st = bm_download_disp(bm, rc->rw, rc->rh, s);
    if (st) return st;
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    if (dec->hStatus[0] || dec->hStatus[1]) return RTDM_ERR_BAD_STREAM;
    bm_scatter_disp(bm, rc->rw, rc->rh, disp, disp_pitch);
    return RTDM_OK;
}
