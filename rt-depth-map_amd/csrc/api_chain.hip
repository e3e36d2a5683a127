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
    st = rectify_upload(rc, rgb_left, left_pitch, rgb_right, right_pitch, s);
    if (st) return st;
    st = rgb_chunks(bm, rc, 1, rc->dRgb[0], rc->dRgb[1], bm_internal_plane(bm, rc->rw, rc->rh), s);
    if (st == RTDM_OK) st = bm_download_disp(bm, rc->rw, rc->rh, s);
    if (st) return st;
    HIPC(hipStreamSynchronize(s));
    bm_scatter_disp(bm, rc->rw, rc->rh, disp, disp_pitch);
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
    if (*nboxes == 0) return RTDM_OK;                     // estimator.cpp:48: nothing to measure in this frame
    const int nreg = std::min(std::min(*nboxes, max_boxes), RTDM_MAX_REGIONS);
    // estimator.cpp:54-56
    st = rtdm_bm_set_roi(bm, 1, roi.x, roi.y, roi.width, roi.height);
    if (st) return st;
    const Plane16W O = bm_internal_plane(bm, W, H);
    st = bm_run_chunk(bm, 1, Plane8{rc->dGray[0], rc->gpitch, gframe}, Plane8{rc->dGray[1], rc->gpitch, gframe}, W, H, O, s);
    if (st) return st;
    // estimator.cpp:75-77
    int flat[4 * RTDM_MAX_REGIONS], maxh = 1;
    st = depth_check_regions(boxes, nreg, W, H, flat, &maxh);
    if (st) return st;
    DepthQ q; std::copy(Q, Q + 16, q.q);
    launch_depth_stats(bm->dOut, O.pitch_e, W, H, q, ob->dMaskOut, (size_t)W, flat, nreg, bm->maxH, calibration_unit, bm->dDepth,
                       mean_cm, counts, s);
    if (disp) { st = bm_download_disp(bm, W, H, s); if (st) return st; }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    if (disp) bm_scatter_disp(bm, W, H, disp, disp_pitch);
    return RTDM_OK;
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
    if (total == 0) return RTDM_OK;                       // estimator.cpp:48: nothing to measure in this frame
    const int stored = (int)std::min<long>(total, cap);
    HIPC(hipMemcpy(objects, ob->dObj, (size_t)stored * sizeof(rtdm_object), hipMemcpyDeviceToHost));
    const int nreg = std::min(stored, RTDM_MAX_REGIONS);
    st = rtdm_bm_set_roi(bm, 1, hRoi[0], hRoi[1], hRoi[2], hRoi[3]);
    if (st) return st;
    const Plane16W O = bm_internal_plane(bm, W, H);
    st = bm_run_chunk(bm, 1, Plane8{rc->dGray[0], rc->gpitch, gframe}, Plane8{rc->dGray[1], rc->gpitch, gframe}, W, H, O, s);
    if (st) return st;
    // every class's objects over that class's filtered mask; the lists lie class after class
    rtdm_region boxes[RTDM_MAX_REGIONS];
    for (int i = 0; i < nreg; ++i) boxes[i] = rtdm_region{objects[i].x, objects[i].y, objects[i].width, objects[i].height};
    int flat[4 * RTDM_MAX_REGIONS], maxh = 1;
    st = depth_check_regions(boxes, nreg, W, H, flat, &maxh);
    if (st) return st;
    DepthQ q; std::copy(Q, Q + 16, q.q);
    for (int i0 = 0; i0 < nreg;) {
        int i1 = i0 + 1;
        while (i1 < nreg && objects[i1].cls == objects[i0].cls) ++i1;
        launch_depth_stats(bm->dOut, O.pitch_e, W, H, q, ob->dMaskOut + (size_t)objects[i0].cls * ob->mpitch * H, ob->mpitch, flat + 4 * i0,
                           i1 - i0, bm->maxH, calibration_unit, bm->dDepth, mean_cm + i0, counts + i0, s, i0 > 0);   // one minimum per map
        i0 = i1;
    }
    if (disp) { st = bm_download_disp(bm, W, H, s); if (st) return st; }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    if (disp) bm_scatter_disp(bm, W, H, disp, disp_pitch);
    return RTDM_OK;
}

// ---- the loop body on frame batches (rtdm_estimator) ------------------------------------------------
void rtdm_estimator_destroy(rtdm_estimator* E)
{
    if (!E) return;
    (void)hipSetDevice(E->device);
    (void)hipDeviceSynchronize();                       // its buffers may be in use on any stream; the borrowed handles are not touched
    E->mem.release();
    if (E->dLabels) (void)hipFree(E->dLabels);
    if (E->dMeasWork) (void)hipFree(E->dMeasWork);
    if (E->dMeas) (void)hipFree(E->dMeas);
    if (E->hMeas) (void)hipHostFree(E->hMeas);
    delete E;
}

// L7.  The label planes of a chunk live from the call that switches own pixels on to the one that switches them off.
int rtdm_estimator_set_own_pixels(rtdm_estimator* E, int on)
{
    if (!E) return RTDM_ERR_NULL;
    if ((on != 0) == (E->dLabels != nullptr)) return RTDM_OK;
    HIPC(hipSetDevice(E->device));
    HIPC(hipDeviceSynchronize());                       // (the planes may be in use on any stream)
    if (!on) { HIPC(hipFree(E->dLabels)); E->dLabels = nullptr; return RTDM_OK; }
    const size_t bytes = (size_t)E->chunk * E->ob->maxC * E->rc->rw * E->rc->rh * sizeof(int32_t);
    const hipError_t e = hipMalloc(&E->dLabels, bytes);
    if (e != hipSuccess) { E->dLabels = nullptr; return create_failed("rtdm_estimator_set_own_pixels", e); }
    return RTDM_OK;
}

int rtdm_estimator_get_own_pixels(const rtdm_estimator* E, int* on)
{
    if (!E || !on) return RTDM_ERR_NULL;
    *on = E->dLabels != nullptr;
    return RTDM_OK;
}

int rtdm_estimator_create(rtdm_bm* bm, rtdm_rectify* rc, rtdm_objects* ob, int max_batch, int capacity, rtdm_estimator** out)
{
    if (!out) return RTDM_ERR_NULL;
    *out = nullptr;
    if (max_batch < 1 || capacity < 1) return RTDM_ERR_BAD_SIZE;
    if (!bm || !rc || !ob) return RTDM_ERR_NULL;
    if (bm->device != rc->device || bm->device != ob->device) return RTDM_ERR_BAD_PARAM;
    if (ob->W != rc->rw || ob->H != rc->rh) return RTDM_ERR_BAD_SIZE;
    int st = bm_check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    st = use_device(bm->device);
    if (st) return st;
    rtdm_estimator* E = new (std::nothrow) rtdm_estimator();
    if (!E) return RTDM_ERR_NOMEM;
    E->bm = bm; E->rc = rc; E->ob = ob; E->device = bm->device; E->cap = capacity;
    E->chunk = std::min(max_batch, std::min(bm->maxB, ob->maxB));
    E->cpitch = objects_rgb_pitch(ob);
    const size_t B = (size_t)E->chunk, slots = B * capacity, fbytes = (size_t)rc->W * rc->H * 3, px = (size_t)rc->rw * rc->rh;
    E->workBytes = depth_objects_bytes(E->chunk, capacity, rc->rh);
    AllocList& m = E->mem;
    for (int k = 0; k < 2; ++k) {
        m.dev(&E->dRgb[k], B * fbytes + 16); m.dev(&E->dGray[k], B * rc->gpitch * rc->rh);
        m.host(&E->hRgb[k], B * fbytes);
    }
    m.dev(&E->dCrop, B * E->cpitch * rc->rh + 16);
    m.dev(&E->dObj, slots * sizeof(CcObject)); m.dev(&E->dMean, slots * sizeof(double)); m.dev(&E->dNpix, slots * sizeof(int));
    m.dev(&E->dCounts, B * RTDM_MAX_CLASSES * sizeof(int)); m.dev(&E->dRois, B * 4 * sizeof(int));
    m.dev(&E->dWork, E->workBytes);
    m.host(&E->hCounts, B * RTDM_MAX_CLASSES * sizeof(int)); m.host(&E->hRois, B * 4 * sizeof(int));
    m.host(&E->hObj, slots * sizeof(CcObject)); m.host(&E->hMean, slots * sizeof(double)); m.host(&E->hNpix, slots * sizeof(int));
    m.host(&E->hDisp, B * px * sizeof(int16_t));
    if (m.err != hipSuccess) { const hipError_t e = m.err; m.release(); delete E; return create_failed("rtdm_estimator_create", e); }
    *out = E;
    return RTDM_OK;
}

// one call's frames and outputs: all of them in device memory (the device form) or all on the host
struct EstIo {
    bool device;
    const uint8_t* rgb[2]; size_t pitch[2], stride[2];
    rtdm_object* objects; int* counts; double* mean; int* npix;
    int16_t* disp; size_t disp_pitch, disp_stride;
    const rtdm_measure_params* mp; rtdm_object_measure* measures;       // both or neither (rtdm_estimate_batch_measured)
};

// the refusals of both forms, in the order include/rtdm.h gives
static int est_check(const rtdm_estimator* E, int n, const EstIo& io, const double* Q, const rtdm_hsv_range* ranges,
                     const int* range_class, int nranges, int nclasses, HsvClasses* C)
{
    if (!io.rgb[0] || !io.rgb[1] || !Q || !io.objects || !io.counts || !io.mean || !io.npix) return RTDM_ERR_NULL;
    if ((io.mp != nullptr) != (io.measures != nullptr)) return RTDM_ERR_NULL;
    int st = objects_classes_check(ranges, range_class, nranges, nclasses, C);
    if (st) return st;
    if (n < 0) return RTDM_ERR_BAD_SIZE;
    if (!E) return RTDM_ERR_NULL;
    if (nclasses > E->ob->maxC) return RTDM_ERR_BAD_PARAM;
    const rtdm_rectify* rc = E->rc;
    const size_t row = (size_t)rc->W * 3;
    if (io.pitch[0] < row || io.pitch[1] < row) return RTDM_ERR_BAD_SIZE;
    if (io.disp && (io.disp_pitch < (size_t)rc->rw * 2 || (io.disp_pitch & 1) || (io.disp_stride & 1))) return RTDM_ERR_BAD_SIZE;
    if (n > 1 && (io.stride[0] < io.pitch[0] * rc->H || io.stride[1] < io.pitch[1] * rc->H ||
                  (io.disp && io.disp_stride < io.disp_pitch * rc->rh)))
        return RTDM_ERR_BAD_SIZE;
    st = bm_check_frame(E->bm, rc->rw, rc->rh);
    if (st || !io.mp) return st;
    st = measure_params_check(io.mp);
    if (st) return st;
    return (size_t)io.measures % 8 ? RTDM_ERR_BAD_SIZE : RTDM_OK;
}

// the first measured call makes the measurement's workspace for a chunk, the first measured host call the records' staging
static int est_measure_stage(rtdm_estimator* E, bool host_form)
{
    const size_t slots = (size_t)E->chunk * E->cap;
    if (!E->dMeasWork) {
        const size_t bytes = measure_bytes(E->chunk, E->cap, E->rc->rh, 8);
        HIPC(hipMalloc(&E->dMeasWork, bytes));
        E->measWorkBytes = bytes;
    }
    if (host_form && !E->dMeas) HIPC(hipMalloc((void**)&E->dMeas, slots * sizeof(MeasRecord)));
    if (host_form && !E->hMeas) HIPC(hipHostMalloc((void**)&E->hMeas, slots * sizeof(MeasRecord)));
    return RTDM_OK;
}

// Gray pair and left colour crop of m frames.  k_rectify reads whole dwords up to RectifySrc::frame bytes from a frame's start:
// `exact` (the frames end the caller's device buffer) runs the last frame with its own last byte as that limit.
static void est_rectify(rtdm_estimator* E, RectifySrc L, RectifySrc R, int m, bool exact, hipStream_t s)
{
    const rtdm_rectify* rc = E->rc;
    const size_t gframe = rc->gpitch * rc->rh, cframe = E->cpitch * rc->rh, row = (size_t)rc->W * 3;
    const size_t endL = L.pitch * (rc->H - 1) + row, endR = R.pitch * (rc->H - 1) + row;
    const int head = (exact && (L.frame != endL || R.frame != endR)) ? m - 1 : m;
    for (int j0 = 0; j0 < m; j0 += std::max(head, 1)) {
        const int k = j0 < head ? head : m - j0;
        RectifySrc l{L.base + (size_t)j0 * L.frame, L.pitch, j0 < head ? L.frame : endL};
        RectifySrc r{R.base + (size_t)j0 * R.frame, R.pitch, j0 < head ? R.frame : endR};
        launch_rectify_gray(l, r, rc->dMap1[0], rc->dMap2[0], rc->dMap1[1], rc->dMap2[1], rc->W, rc->H, rc->rw, rc->rh,
                            Plane8W{E->dGray[0] + j0 * gframe, rc->gpitch, gframe}, Plane8W{E->dGray[1] + j0 * gframe, rc->gpitch, gframe}, k, s);
        launch_rectify_rgb(l, rc->dMap1[0], rc->dMap2[0], rc->W, rc->H, rc->rw, rc->rh,
                           Plane8W{E->dCrop + j0 * cframe, E->cpitch, cframe}, k, s);
    }
}

static int est_run(rtdm_estimator* E, int n, const EstIo& io, const double* Q, const HsvClasses& C, int min_area, int zero_border,
                   double unit, hipStream_t s)
{
    rtdm_bm* bm = E->bm; rtdm_rectify* rc = E->rc; rtdm_objects* ob = E->ob;
    const int W = rc->rw, H = rc->rh, K = C.nclasses, cap = E->cap;
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H, gframe = rc->gpitch * H, cframe = E->cpitch * H;
    const Plane16W O = bm_internal_plane(bm, W, H);
    DepthQ q; std::copy(Q, Q + 16, q.q);
    XyzParams mP; MeasQuant mQ;
    if (io.mp) {
        const int st = est_measure_stage(E, !io.device);
        if (st) return st;
        measure_params_kernel(io.mp, Q, &mP, &mQ);
    }
    for (int i0 = 0; i0 < n; i0 += E->chunk) {
        const int m = std::min(E->chunk, n - i0);
        // 1. the chunk's frames -> gray pairs and colour crops
        RectifySrc S[2];
        for (int k = 0; k < 2; ++k) {
            if (io.device) { S[k] = RectifySrc{io.rgb[k] + (size_t)i0 * io.stride[k], io.pitch[k], n > 1 ? io.stride[k] : io.pitch[k] * (rc->H - 1) + row}; continue; }
            for (int j = 0; j < m; ++j) {
                const uint8_t* src = io.rgb[k] + (size_t)(i0 + j) * io.stride[k];
                uint8_t* h = E->hRgb[k] + (size_t)j * fbytes;
                if (io.pitch[k] == row) memcpy(h, src, fbytes);
                else for (int y = 0; y < rc->H; ++y) memcpy(h + (size_t)y * row, src + (size_t)y * io.pitch[k], row);
            }
            HIPC(hipMemcpyAsync(E->dRgb[k], E->hRgb[k], (size_t)m * fbytes, hipMemcpyHostToDevice, s));
            S[k] = RectifySrc{E->dRgb[k], row, fbytes};
        }
        est_rectify(E, S[0], S[1], m, io.device && i0 + m == n, s);
        HIPC(hipGetLastError());
        // 2. the detector, lists on the device
        CcObject* dObj = io.device ? (CcObject*)io.objects + (size_t)i0 * cap : E->dObj;
        int* dCounts = io.device ? io.counts + (size_t)i0 * K : E->dCounts;
        double* dMean = io.device ? io.mean + (size_t)i0 * cap : E->dMean;
        int* dNpix = io.device ? io.npix + (size_t)i0 * cap : E->dNpix;
        const size_t lpitch = (size_t)W * sizeof(int32_t), lplane = lpitch * H;       // own pixels (L7): the chunk's label planes
        int st = objects_run_chunk(ob, m, E->dCrop, E->cpitch, cframe, C, min_area, zero_border, nullptr, 0, 0, dObj, cap, dCounts, E->dRois, s,
                                   CcLabelsOut{E->dLabels, lpitch, lplane, nullptr});
        if (st) return st;
        // 3. the one read-back in front of the matcher: per-class counts and union boxes
        HIPC(hipMemcpyAsync(E->hCounts, dCounts, (size_t)m * K * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(E->hRois, E->dRois, (size_t)m * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        long total[64];                                   // (a detector serves at most 64 frames per launch)
        bool any = false;
        for (int j = 0; j < m; ++j) {
            total[j] = 0;
            for (int c = 0; c < K; ++c) total[j] += E->hCounts[j * K + c];
            if (!io.device) std::copy(E->hCounts + j * K, E->hCounts + (j + 1) * K, io.counts + (size_t)(i0 + j) * K);
            any = any || total[j] > 0;
        }
        if (!any) continue;                               // estimator.cpp:48 for the whole chunk
        // 4. the matcher: a frame without objects is skipped, consecutive frames with one union box share a launch set
        for (int j = 0; j < m;) {
            if (total[j] == 0) { ++j; continue; }
            const int* roi = E->hRois + 4 * j;
            int j1 = j + 1;
            while (j1 < m && total[j1] > 0 && std::equal(roi, roi + 4, E->hRois + 4 * j1)) ++j1;
            st = rtdm_bm_set_roi(bm, 1, roi[0], roi[1], roi[2], roi[3]);
            if (st) return st;
            st = bm_run_chunk(bm, j1 - j, Plane8{E->dGray[0] + j * gframe, rc->gpitch, gframe}, Plane8{E->dGray[1] + j * gframe, rc->gpitch, gframe},
                              W, H, Plane16W{O.base + j * O.frame_e, O.pitch_e, O.frame_e}, s);
            if (st) return st;
            j = j1;
        }
        // 5. every object of the chunk under its own class's mask, against its own frame's plane of the matcher
        // (with own pixels: under its own label on its class's label plane)
        const DepthObjects a{bm->dOut, O.pitch_e, O.frame_e, E->dLabels ? (const uint8_t*)E->dLabels : ob->dMaskOut,
                             E->dLabels ? lpitch : ob->mpitch, E->dLabels ? lplane : ob->mpitch * H, dObj, dCounts, m, W, H, K, cap, 0};
        launch_depth_objects(a, q, unit, E->dWork, dMean, dNpix, s, E->dLabels != nullptr);
        MeasRecord* dMeas = io.mp ? (io.device ? (MeasRecord*)io.measures + (size_t)i0 * cap : E->dMeas) : nullptr;
        if (io.mp) launch_measure(a, mP, mQ, E->dMeasWork, dMeas, s, E->dLabels != nullptr);     // ... and measured (G1-G10)
        HIPC(hipGetLastError());
        // 6. the results; frames without objects keep what the caller's arrays held
        for (int j = 0; io.disp && j < m; ++j) {
            if (total[j] == 0) continue;
            if (io.device) HIPC(hipMemcpy2DAsync((uint8_t*)io.disp + (size_t)(i0 + j) * io.disp_stride, io.disp_pitch, O.base + j * O.frame_e,
                                                 O.pitch_e * 2, (size_t)W * 2, H, hipMemcpyDeviceToDevice, s));
            else HIPC(hipMemcpy2DAsync(E->hDisp + (size_t)j * W * H, (size_t)W * 2, O.base + j * O.frame_e, O.pitch_e * 2, (size_t)W * 2, H,
                                       hipMemcpyDeviceToHost, s));
        }
        if (io.device) continue;
        const size_t slots = (size_t)m * cap;
        HIPC(hipMemcpyAsync(E->hObj, dObj, slots * sizeof(CcObject), hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(E->hMean, dMean, slots * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(E->hNpix, dNpix, slots * sizeof(int), hipMemcpyDeviceToHost, s));
        if (io.mp) HIPC(hipMemcpyAsync(E->hMeas, dMeas, slots * sizeof(MeasRecord), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        for (int j = 0; j < m; ++j) {
            const size_t stored = (size_t)std::min<long>(total[j], cap), at = (size_t)(i0 + j) * cap, from = (size_t)j * cap;
            if (!stored) continue;
            memcpy(io.objects + at, E->hObj + from, stored * sizeof(rtdm_object));
            std::copy(E->hMean + from, E->hMean + from + stored, io.mean + at);
            std::copy(E->hNpix + from, E->hNpix + from + stored, io.npix + at);
            if (io.mp) memcpy(io.measures + at, E->hMeas + from, stored * sizeof(rtdm_object_measure));
            for (int y = 0; io.disp && y < H; ++y)
                memcpy((uint8_t*)io.disp + (size_t)(i0 + j) * io.disp_stride + (size_t)y * io.disp_pitch, E->hDisp + ((size_t)j * H + y) * W, (size_t)W * 2);
        }
    }
    return RTDM_OK;
}

int rtdm_estimate_batch_measured(rtdm_estimator* E, int n, const uint8_t* rgb_left, size_t left_pitch, size_t left_frame_stride,
                                 const uint8_t* rgb_right, size_t right_pitch, size_t right_frame_stride, const double* Q,
                                 const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, int min_area,
                                 int zero_border, double calibration_unit, rtdm_object* objects, int* counts, double* mean_cm,
                                 int* npix, int16_t* disp, size_t disp_pitch, size_t disp_frame_stride,
                                 const rtdm_measure_params* mp, rtdm_object_measure* measures)
{
    const EstIo io{false, {rgb_left, rgb_right}, {left_pitch, right_pitch}, {left_frame_stride, right_frame_stride}, objects, counts,
                   mean_cm, npix, disp, disp_pitch, disp_frame_stride, mp, measures};
    HsvClasses C;
    const int st = est_check(E, n, io, Q, ranges, range_class, nranges, nclasses, &C);
    if (st || n == 0) return st;
    HIPC(hipSetDevice(E->device));
    DrainOnError drain{E->bm->stream};
    const int rc = est_run(E, n, io, Q, C, min_area, zero_border, calibration_unit, E->bm->stream);
    if (rc == RTDM_OK) drain.armed = false;             // (every chunk has synchronised)
    return rc;
}

int rtdm_estimate_batch(rtdm_estimator* E, int n, const uint8_t* rgb_left, size_t left_pitch, size_t left_frame_stride,
                        const uint8_t* rgb_right, size_t right_pitch, size_t right_frame_stride, const double* Q,
                        const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, int min_area,
                        int zero_border, double calibration_unit, rtdm_object* objects, int* counts, double* mean_cm, int* npix,
                        int16_t* disp, size_t disp_pitch, size_t disp_frame_stride)
{
    return rtdm_estimate_batch_measured(E, n, rgb_left, left_pitch, left_frame_stride, rgb_right, right_pitch, right_frame_stride, Q, ranges,
                                        range_class, nranges, nclasses, min_area, zero_border, calibration_unit, objects, counts, mean_cm,
                                        npix, disp, disp_pitch, disp_frame_stride, nullptr, nullptr);
}

int rtdm_estimate_batch_measured_device(rtdm_estimator* E, int n, const uint8_t* d_rgb_left, size_t left_pitch,
                                        size_t left_frame_stride, const uint8_t* d_rgb_right, size_t right_pitch,
                                        size_t right_frame_stride, const double* Q, const rtdm_hsv_range* ranges,
                                        const int* range_class, int nranges, int nclasses, int min_area, int zero_border,
                                        double calibration_unit, rtdm_object* d_objects, int* d_counts, double* d_mean_cm,
                                        int* d_npix, int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                                        void* hip_stream, const rtdm_measure_params* mp, rtdm_object_measure* d_measures)
{
    const EstIo io{true, {d_rgb_left, d_rgb_right}, {left_pitch, right_pitch}, {left_frame_stride, right_frame_stride}, d_objects, d_counts,
                   d_mean_cm, d_npix, d_disp, disp_pitch, disp_frame_stride, mp, d_measures};
    HsvClasses C;
    const int st = est_check(E, n, io, Q, ranges, range_class, nranges, nclasses, &C);
    if (st || n == 0) return st;
    HIPC(hipSetDevice(E->device));
    return est_run(E, n, io, Q, C, min_area, zero_border, calibration_unit, (hipStream_t)hip_stream);
}

int rtdm_estimate_batch_device(rtdm_estimator* E, int n, const uint8_t* d_rgb_left, size_t left_pitch,
                               size_t left_frame_stride, const uint8_t* d_rgb_right, size_t right_pitch,
                               size_t right_frame_stride, const double* Q, const rtdm_hsv_range* ranges, const int* range_class,
                               int nranges, int nclasses, int min_area, int zero_border, double calibration_unit,
                               rtdm_object* d_objects, int* d_counts, double* d_mean_cm, int* d_npix, int16_t* d_disp,
                               size_t disp_pitch, size_t disp_frame_stride, void* hip_stream)
{
    return rtdm_estimate_batch_measured_device(E, n, d_rgb_left, left_pitch, left_frame_stride, d_rgb_right, right_pitch, right_frame_stride,
                                               Q, ranges, range_class, nranges, nclasses, min_area, zero_border, calibration_unit, d_objects,
                                               d_counts, d_mean_cm, d_npix, d_disp, disp_pitch, disp_frame_stride, hip_stream, nullptr,
                                               nullptr);
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
