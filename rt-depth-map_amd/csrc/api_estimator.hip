// api_estimator.hip -- rtdm_estimator: the loop body on frame batches, host and device form.
#include "rtdm_handles.h"

#include <numeric>

using namespace rtdm;

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

// B-rules of DESIGN.md section 4.19 for the estimator: a flag, nothing is allocated or waited for.
int rtdm_estimator_set_device_roi(rtdm_estimator* E, int on)
{
    if (!E) return RTDM_ERR_NULL;
    E->deviceRoi = on != 0;
    return RTDM_OK;
}

int rtdm_estimator_get_device_roi(const rtdm_estimator* E, int* on)
{
    if (!E || !on) return RTDM_ERR_NULL;
    *on = E->deviceRoi;
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

// one call's frames and outputs, all of them in device memory (the device form) or all on the host, and its parameters
struct EstIo {
    const uint8_t* rgb[2]; size_t pitch[2], stride[2];
    rtdm_object* objects; int* counts; double* mean; int* npix;
    int16_t* disp; size_t disp_pitch, disp_stride;
    const rtdm_measure_params* mp; rtdm_object_measure* measures;       // both or neither (rtdm_estimate_batch_measured)
    int min_area, zero_border; double unit;
    HsvClasses C; DepthQ q; XyzParams mP; MeasQuant mQ;                 // the kernels' form of the ranges (est_check), Q and mp
};

// the refusals of both forms, in the order include/rtdm.h gives
static int est_check(const rtdm_estimator* E, int n, EstIo& io, const double* Q, const rtdm_hsv_range* ranges, const int* range_class,
                     int nranges, int nclasses)
{
    if (!io.rgb[0] || !io.rgb[1] || !Q || !io.objects || !io.counts || !io.mean || !io.npix) return RTDM_ERR_NULL;
    if ((io.mp != nullptr) != (io.measures != nullptr)) return RTDM_ERR_NULL;
    int st = objects_classes_check(ranges, range_class, nranges, nclasses, &io.C);
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

// The kernels' form of Q and mp.  The first measured call makes the measurement's workspace for a chunk, the first measured host
// call the records' staging.
static int est_measure_stage(rtdm_estimator* E, EstIo& io, const double* Q, bool host_form)
{
    std::copy(Q, Q + 16, io.q.q);
    if (!io.mp) return RTDM_OK;
    measure_params_kernel(io.mp, Q, &io.mP, &io.mQ);
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

// One chunk's frames and results, all in device memory: the caller's (device form) or the estimator's staging (host form).
struct EstChunk {
    RectifySrc src[2]; bool exact;                      // est_rectify
    CcObject* obj; int* counts; double* mean; int* npix; MeasRecord* meas;      // meas: null unless the call measures
    uint8_t* disp; size_t disp_pitch, disp_stride;      // where the frames' disparity maps go (null: nowhere), by copies of `kind`
    hipMemcpyKind kind;
};

// Steps 1 to 6 of a chunk of m frames, enqueued on s with one synchronisation in the middle (none with
// rtdm_estimator_set_device_roi); total[j]: the objects of frame j (-1: not known on the host).
static int est_chunk(rtdm_estimator* E, int m, const EstChunk& d, const EstIo& c, hipStream_t s, long* total)
{
    rtdm_bm* bm = E->bm; rtdm_rectify* rc = E->rc; rtdm_objects* ob = E->ob;
    const int W = rc->rw, H = rc->rh, K = c.C.nclasses, cap = E->cap;
    const size_t gframe = rc->gpitch * H, cframe = E->cpitch * H;
    const Plane16W O = bm_internal_plane(bm, W, H);
    // 1. the chunk's frames -> gray pairs and colour crops
    est_rectify(E, d.src[0], d.src[1], m, d.exact, s);
    HIPC(hipGetLastError());
    // 2. the detector, lists on the device
    const size_t lpitch = (size_t)W * sizeof(int32_t), lplane = lpitch * H;       // own pixels (L7): the chunk's label planes
    int st = objects_run_chunk(ob, m, E->dCrop, E->cpitch, cframe, c.C, c.min_area, c.zero_border, nullptr, 0, 0, d.obj, cap, d.counts, E->dRois, s,
                               CcLabelsOut{E->dLabels, lpitch, lplane, nullptr});
    if (st) return st;
    const DepthObjects a{bm->dOut, O.pitch_e, O.frame_e, E->dLabels ? (const uint8_t*)E->dLabels : ob->dMaskOut,
                         E->dLabels ? lpitch : ob->mpitch, E->dLabels ? lplane : ob->mpitch * H, d.obj, d.counts, m, W, H, K, cap, 0};
    if (E->deviceRoi) {
        // 3 + 4 without the host (rtdm_estimator_set_device_roi): the matcher takes the union boxes where the detector left them --
        // a frame without kept objects has a box of negative width there (k_cc_scan, k_cc_roi), which is that call's "skipped" --
        // in one launch set for the chunk; total[] stays unknown here (-1), the host form counts after its one synchronisation
        std::fill(total, total + m, -1L);
        st = bm_run_chunk_rois(bm, m, Plane8{E->dGray[0], rc->gpitch, gframe}, Plane8{E->dGray[1], rc->gpitch, gframe}, W, H, E->dRois,
                               Plane16W{nullptr, 0, 0}, s);
        if (st) return st;
        // 5 as below: a frame without objects has no object to measure
        launch_depth_objects(a, c.q, c.unit, E->dWork, d.mean, d.npix, s, E->dLabels != nullptr);
        if (d.meas) launch_measure(a, c.mP, c.mQ, E->dMeasWork, d.meas, s, E->dLabels != nullptr);
        HIPC(hipGetLastError());
        // 6. device form: the copy skips the frames without objects on the device; host form: every plane comes to the staging
        // area in one copy (the internal planes are contiguous), and the caller of this function scatters those with objects
        if (d.disp && d.kind == hipMemcpyDeviceToDevice)
            launch_copy16_rois(O, Plane16W{(int16_t*)d.disp, d.disp_pitch / 2, d.disp_stride / 2}, W, H, m, E->dRois, s);
        else if (d.disp)
            HIPC(hipMemcpy2DAsync(d.disp, d.disp_pitch, O.base, O.pitch_e * 2, (size_t)W * 2, (size_t)H * m, d.kind, s));
        HIPC(hipGetLastError());
        return RTDM_OK;
    }
    // 3. the one read-back in front of the matcher: per-class counts and union boxes
    HIPC(hipMemcpyAsync(E->hCounts, d.counts, (size_t)m * K * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(E->hRois, E->dRois, (size_t)m * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    bool any = false;
    for (int j = 0; j < m; ++j) {
        total[j] = 0;
        for (int k = 0; k < K; ++k) total[j] += E->hCounts[j * K + k];
        any = any || total[j] > 0;
    }
    if (!any) return RTDM_OK;                             // estimator.cpp:48 for the whole chunk
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
    launch_depth_objects(a, c.q, c.unit, E->dWork, d.mean, d.npix, s, E->dLabels != nullptr);
    if (d.meas) launch_measure(a, c.mP, c.mQ, E->dMeasWork, d.meas, s, E->dLabels != nullptr);     // ... and measured (G1-G10)
    HIPC(hipGetLastError());
    // 6. the disparity maps; frames without objects keep what the destination held
    for (int j = 0; d.disp && j < m; ++j)
        if (total[j]) HIPC(hipMemcpy2DAsync(d.disp + (size_t)j * d.disp_stride, d.disp_pitch, O.base + j * O.frame_e, O.pitch_e * 2, (size_t)W * 2, H, d.kind, s));
    return RTDM_OK;
}

// Host form: a chunk's frames go through the page-locked staging to the estimator's device buffers, its results come back
// the same way and are scattered into the caller's arrays; frames without objects keep what those held.
int rtdm_estimate_batch_measured(rtdm_estimator* E, int n, const uint8_t* rgb_left, size_t left_pitch, size_t left_frame_stride,
                                 const uint8_t* rgb_right, size_t right_pitch, size_t right_frame_stride, const double* Q,
                                 const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, int min_area,
                                 int zero_border, double calibration_unit, rtdm_object* objects, int* counts, double* mean_cm,
                                 int* npix, int16_t* disp, size_t disp_pitch, size_t disp_frame_stride,
                                 const rtdm_measure_params* mp, rtdm_object_measure* measures)
{
    EstIo io{{rgb_left, rgb_right}, {left_pitch, right_pitch}, {left_frame_stride, right_frame_stride}, objects, counts, mean_cm, npix,
             disp, disp_pitch, disp_frame_stride, mp, measures, min_area, zero_border, calibration_unit};
    int st = est_check(E, n, io, Q, ranges, range_class, nranges, nclasses);
    if (st || n == 0) return st;
    HIPC(hipSetDevice(E->device));
    hipStream_t s = E->bm->stream;
    DrainOnError drain{s};
    st = est_measure_stage(E, io, Q, true);
    if (st) return st;
    const rtdm_rectify* rc = E->rc;
    const int W = rc->rw, H = rc->rh, K = nclasses, cap = E->cap;
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H, dpitch = (size_t)W * 2, dframe = dpitch * H;
    for (int i0 = 0; i0 < n; i0 += E->chunk) {
        const int m = std::min(E->chunk, n - i0);
        for (int k = 0; k < 2; ++k) {
            for (int j = 0; j < m; ++j)
                copy_rows(E->hRgb[k] + (size_t)j * fbytes, row, io.rgb[k] + (size_t)(i0 + j) * io.stride[k], io.pitch[k], row, rc->H, RowPad::OURS);
            HIPC(hipMemcpyAsync(E->dRgb[k], E->hRgb[k], (size_t)m * fbytes, hipMemcpyHostToDevice, s));
        }
        const EstChunk d{{RectifySrc{E->dRgb[0], row, fbytes}, RectifySrc{E->dRgb[1], row, fbytes}}, false, E->dObj, E->dCounts, E->dMean, E->dNpix,
                         mp ? E->dMeas : nullptr, disp ? (uint8_t*)E->hDisp : nullptr, dpitch, dframe, hipMemcpyDeviceToHost};
        long total[64];                                   // (a detector serves at most 64 frames per launch)
        st = est_chunk(E, m, d, io, s, total);
        if (st) return st;
        const size_t slots = (size_t)m * cap;
        if (E->deviceRoi)                                 // the counts come back with the results, behind everything else
            HIPC(hipMemcpyAsync(E->hCounts, d.counts, (size_t)m * K * sizeof(int), hipMemcpyDeviceToHost, s));
        else {
            std::copy(E->hCounts, E->hCounts + (size_t)m * K, counts + (size_t)i0 * K);
            if (std::count(total, total + m, 0L) == m) continue;
        }
        HIPC(hipMemcpyAsync(E->hObj, d.obj, slots * sizeof(CcObject), hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(E->hMean, d.mean, slots * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(E->hNpix, d.npix, slots * sizeof(int), hipMemcpyDeviceToHost, s));
        if (mp) HIPC(hipMemcpyAsync(E->hMeas, d.meas, slots * sizeof(MeasRecord), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        if (E->deviceRoi) {                               // the chunk's one synchronisation lies behind: now the host counts
            std::copy(E->hCounts, E->hCounts + (size_t)m * K, counts + (size_t)i0 * K);
            for (int j = 0; j < m; ++j) total[j] = std::accumulate(E->hCounts + (size_t)j * K, E->hCounts + (size_t)(j + 1) * K, 0L);
        }
        for (int j = 0; j < m; ++j) {
            const size_t stored = (size_t)std::min<long>(total[j], cap), at = (size_t)(i0 + j) * cap, from = (size_t)j * cap;
            if (!stored) continue;
            memcpy(objects + at, E->hObj + from, stored * sizeof(rtdm_object));
            std::copy(E->hMean + from, E->hMean + from + stored, mean_cm + at);
            std::copy(E->hNpix + from, E->hNpix + from + stored, npix + at);
            if (mp) memcpy(measures + at, E->hMeas + from, stored * sizeof(rtdm_object_measure));
            if (disp) copy_rows((uint8_t*)disp + (i0 + j) * disp_frame_stride, disp_pitch, d.disp + j * dframe, dpitch, dpitch, H, RowPad::KEEP);
        }
    }
    drain.armed = false;                                // (every chunk has synchronised)
    return RTDM_OK;
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
    EstIo io{{d_rgb_left, d_rgb_right}, {left_pitch, right_pitch}, {left_frame_stride, right_frame_stride}, d_objects, d_counts, d_mean_cm,
             d_npix, d_disp, disp_pitch, disp_frame_stride, mp, d_measures, min_area, zero_border, calibration_unit};
    int st = est_check(E, n, io, Q, ranges, range_class, nranges, nclasses);
    if (st || n == 0) return st;
    HIPC(hipSetDevice(E->device));
    st = est_measure_stage(E, io, Q, false);
    if (st) return st;
    const size_t K = (size_t)nclasses, cap = (size_t)E->cap, row = (size_t)E->rc->W * 3;
    for (int i0 = 0; i0 < n; i0 += E->chunk) {          // every chunk on the caller's pointers
        const int m = std::min(E->chunk, n - i0);
        EstChunk d{{}, i0 + m == n, (CcObject*)d_objects + i0 * cap, d_counts + i0 * K, d_mean_cm + i0 * cap, d_npix + i0 * cap,
                   mp ? (MeasRecord*)d_measures + i0 * cap : nullptr, d_disp ? (uint8_t*)d_disp + i0 * disp_frame_stride : nullptr,
                   disp_pitch, disp_frame_stride, hipMemcpyDeviceToDevice};
        for (int k = 0; k < 2; ++k)
            d.src[k] = RectifySrc{io.rgb[k] + i0 * io.stride[k], io.pitch[k], n > 1 ? io.stride[k] : io.pitch[k] * (E->rc->H - 1) + row};
        long total[64];
        st = est_chunk(E, m, d, io, (hipStream_t)hip_stream, total);
        if (st) return st;
    }
    return RTDM_OK;
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
