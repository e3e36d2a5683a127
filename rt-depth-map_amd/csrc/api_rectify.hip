// api_rectify.hip -- rtdm_rectify: rectification in front of the matcher (estimator.cpp:29-39), from ready maps or from
// the calibration files (main.cpp:53-98; rtdm_calib.h, k_rectmap.hip).
#include "rtdm_handles.h"

using namespace rtdm;

void rtdm_rectify_destroy(rtdm_rectify* rc)
{
    if (!rc) return;
    (void)hipSetDevice(rc->device);
    if (rc->stream) (void)hipStreamSynchronize(rc->stream);
    rc->mem.release();
    if (rc->stream) (void)hipStreamDestroy(rc->stream);
    delete rc;
}

// stream, device buffers and the pinned staging area of a handle whose geometry is set
static hipError_t rectify_alloc(rtdm_rectify* rc)
{
    const size_t npx = (size_t)rc->rw * rc->rh, fbytes = (size_t)rc->W * rc->H * 3;
    AllocList& m = rc->mem;
    m.err = hipStreamCreateWithFlags(&rc->stream, hipStreamNonBlocking);
    for (int k = 0; k < 2; ++k) {
        m.dev(&rc->dMap1[k], npx * 4); m.dev(&rc->dMap2[k], npx * 2);
        m.dev(&rc->dRgb[k], fbytes + 16); m.dev(&rc->dGray[k], rc->gpitch * rc->rh * (size_t)rc->maxB);
    }
    m.dev(&rc->dOut, npx * 3);
    m.host(&rc->hStage, 2 * fbytes + npx * 3 + 128 * (size_t)rc->rh);
    return m.err;
}

static int rectify_check_geometry(int width, int height, int roi_x, int roi_y, int roi_width, int roi_height, int max_batch)
{
    if (width <= 0 || height <= 0 || width > 32767 || height > 32767 || max_batch <= 0) return RTDM_ERR_BAD_SIZE;
    if (roi_x < 0 || roi_y < 0 || roi_width <= 0 || roi_height <= 0 || roi_x + roi_width > width || roi_y + roi_height > height)
        return RTDM_ERR_BAD_SIZE;
    return RTDM_OK;
}

static rtdm_rectify* rectify_new(int width, int height, int roi_x, int roi_y, int roi_width, int roi_height, int max_batch, int device)
{
    rtdm_rectify* rc = new (std::nothrow) rtdm_rectify();
    if (!rc) return nullptr;
    rc->W = width; rc->H = height; rc->rx = roi_x; rc->ry = roi_y; rc->rw = roi_width; rc->rh = roi_height;
    rc->maxB = max_batch; rc->device = device;
    rc->gpitch = ((size_t)roi_width + 63) & ~(size_t)63;
    return rc;
}

int rtdm_rectify_create(const int16_t* map1_left, const uint16_t* map2_left, const int16_t* map1_right,
                        const uint16_t* map2_right, int width, int height, int roi_x, int roi_y, int roi_width,
                        int roi_height, int max_batch, int device, rtdm_rectify** out)
{
    if (!map1_left || !map2_left || !map1_right || !map2_right || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    int st = rectify_check_geometry(width, height, roi_x, roi_y, roi_width, roi_height, max_batch);
    if (st) return st;
    st = use_device(device);
    if (st) return st;
    rtdm_rectify* rc = rectify_new(width, height, roi_x, roi_y, roi_width, roi_height, max_batch, device);
    if (!rc) return RTDM_ERR_NOMEM;
    const size_t npx = (size_t)roi_width * roi_height;
    hipError_t e = rectify_alloc(rc);
    // crop the maps on the host (through the pinned area), one linear copy each
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        const int16_t* m1 = k ? map1_right : map1_left;
        const uint16_t* m2 = k ? map2_right : map2_left;
        int16_t* h1 = (int16_t*)rc->hStage;
        uint16_t* h2 = (uint16_t*)(rc->hStage + npx * 4);
        copy_rows(h1, (size_t)roi_width * 4, m1 + ((size_t)roi_y * width + roi_x) * 2, (size_t)width * 4, (size_t)roi_width * 4, roi_height, RowPad::OURS);
        copy_rows(h2, (size_t)roi_width * 2, m2 + (size_t)roi_y * width + roi_x, (size_t)width * 2, (size_t)roi_width * 2, roi_height, RowPad::OURS);
        e = hipMemcpy(rc->dMap1[k], h1, npx * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(rc->dMap2[k], h2, npx * 2, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { rtdm_rectify_destroy(rc); return create_failed("rtdm_rectify_create", e); }
    *out = rc;
    return RTDM_OK;
}

// ---- from the calibration files ---------------------------------------------------------------------------------------------------
static_assert(sizeof(rtdm_calib) == sizeof(Calib) && sizeof(rtdm_rectification) == sizeof(Rectification) &&
              sizeof(rtdm_region) == sizeof(CalibRegion), "rtdm_calib.h restates the layouts of rtdm.h");

int rtdm_calib_load(const char* intrinsics_path, const char* extrinsics_path, rtdm_calib* calib, rtdm_rectification* stored,
                    unsigned* stored_mask)
{
    if (!intrinsics_path || !extrinsics_path || !calib) return RTDM_ERR_NULL;
    Calib c;
    Rectification r;
    unsigned mask = 0;
    const int st = calib_load(intrinsics_path, extrinsics_path, &c, &r, &mask);
    if (st) return st;
    memcpy(calib, &c, sizeof c);
    if (stored) memcpy(stored, &r, sizeof r);
    if (stored_mask) *stored_mask = mask;
    return RTDM_OK;
}

int rtdm_stereo_rectify(const rtdm_calib* calib, int flags, double alpha, int new_width, int new_height, rtdm_rectification* out)
{
    if (!calib || !out) return RTDM_ERR_NULL;
    Calib c;
    Rectification r;
    memcpy(&c, calib, sizeof c);
    const int st = calib_stereo_rectify(&c, flags, alpha, new_width, new_height, &r);
    if (st) return st;
    memcpy(out, &r, sizeof r);
    return RTDM_OK;
}

static int rectmap_params(const double* M, const double* D, const double* R, const double* P, int width, int height, RectMapParams* o)
{
    const int st = calib_rectmap_check(M, D, R, P, width, height, o->ir);
    if (st) return st;
    o->fx = M[0]; o->fy = M[4]; o->u0 = M[2]; o->v0 = M[5];
    for (int i = 0; i < 12; ++i) o->k[i] = D[i];
    return RTDM_OK;
}

// the full maps of one camera into device memory; returns when they are complete
static int rectmap_full(const RectMapParams& P, int width, int height, int16_t* d_map1, uint16_t* d_map2, hipStream_t s)
{
    double* ckpt = nullptr;
    HIPC(hipMalloc((void**)&ckpt, rectmap_scratch_bytes(0, width, height)));
    launch_rectmap(P, 0, 0, width, height, ckpt, d_map1, d_map2, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(ckpt);
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_undistort_rectify_map: ") + hipGetErrorString(e);
        return RTDM_ERR_HIP;
    }
    return RTDM_OK;
}

int rtdm_undistort_rectify_map_device(const double* M, const double* D, const double* R, const double* P, int width, int height,
                                      int device, int16_t* d_map1, uint16_t* d_map2, void* hip_stream)
{
    if (!M || !D || !R || !P || !d_map1 || !d_map2) return RTDM_ERR_NULL;
    RectMapParams prm;
    int st = rectmap_params(M, D, R, P, width, height, &prm);
    if (st) return st;
    if (((uintptr_t)d_map1 & 3) || ((uintptr_t)d_map2 & 1)) return RTDM_ERR_BAD_SIZE;
    st = use_device(device);
    if (st) return st;
    return rectmap_full(prm, width, height, d_map1, d_map2, (hipStream_t)hip_stream);
}

int rtdm_undistort_rectify_map(const double* M, const double* D, const double* R, const double* P, int width, int height,
                               int device, int16_t* map1, uint16_t* map2)
{
    if (!M || !D || !R || !P || !map1 || !map2) return RTDM_ERR_NULL;
    RectMapParams prm;
    int st = rectmap_params(M, D, R, P, width, height, &prm);
    if (st) return st;
    st = use_device(device);
    if (st) return st;
    const size_t npx = (size_t)width * height;
    int16_t* d1 = nullptr;
    HIPC(hipMalloc((void**)&d1, npx * 6));                   // map1, then map2 behind it
    uint16_t* d2 = (uint16_t*)(d1 + npx * 2);
    st = rectmap_full(prm, width, height, d1, d2, nullptr);
    hipError_t e = hipSuccess;
    if (st == RTDM_OK) e = hipMemcpy(map1, d1, npx * 4, hipMemcpyDeviceToHost);
    if (st == RTDM_OK && e == hipSuccess) e = hipMemcpy(map2, d2, npx * 2, hipMemcpyDeviceToHost);
    (void)hipFree(d1);
    if (st) return st;
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_undistort_rectify_map: ") + hipGetErrorString(e);
        return RTDM_ERR_HIP;
    }
    return RTDM_OK;
}

int rtdm_rectify_create_calib(const rtdm_calib* calib, const rtdm_rectification* rect, int roi_x, int roi_y, int roi_width,
                              int roi_height, int max_batch, int device, rtdm_rectify** out)
{
    if (!calib || !rect || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    const int width = calib->width, height = calib->height;
    int st = rectify_check_geometry(width, height, roi_x, roi_y, roi_width, roi_height, max_batch);
    if (st) return st;
    RectMapParams prm[2];
    st = rectmap_params(calib->M1, calib->D1, rect->R1, rect->P1, width, height, &prm[0]);
    if (st == RTDM_OK) st = rectmap_params(calib->M2, calib->D2, rect->R2, rect->P2, width, height, &prm[1]);
    if (st) return st;
    st = use_device(device);
    if (st) return st;
    rtdm_rectify* rc = rectify_new(width, height, roi_x, roi_y, roi_width, roi_height, max_batch, device);
    if (!rc) return RTDM_ERR_NOMEM;
    hipError_t e = rectify_alloc(rc);
    double* ckpt = nullptr;
    const size_t cbytes = rectmap_scratch_bytes(roi_x, roi_width, roi_height);
    if (e == hipSuccess) e = hipMalloc((void**)&ckpt, 2 * cbytes);
    if (e == hipSuccess) {
        for (int k = 0; k < 2; ++k)
            launch_rectmap(prm[k], roi_x, roi_y, roi_width, roi_height, ckpt + k * (cbytes / sizeof(double)), rc->dMap1[k], rc->dMap2[k],
                           rc->stream);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(rc->stream);
    }
    if (ckpt) (void)hipFree(ckpt);
    if (e != hipSuccess) { rtdm_rectify_destroy(rc); return create_failed("rtdm_rectify_create_calib", e); }
    *out = rc;
    return RTDM_OK;
}

// host RGB frames -> dRgb[0/1] through the pinned staging area
int rtdm::rectify_upload(rtdm_rectify* rc, const uint8_t* a, size_t apitch, const uint8_t* b, size_t bpitch, hipStream_t s)
{
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H;
    const uint8_t* src[2] = {a, b};
    const size_t pit[2] = {apitch, bpitch};
    for (int k = 0; k < 2; ++k) {
        if (!src[k]) continue;
        uint8_t* h = rc->hStage + k * fbytes;
        copy_rows(h, row, src[k], pit[k], row, rc->H, RowPad::OURS);
        HIPC(hipMemcpyAsync(rc->dRgb[k], h, fbytes, hipMemcpyHostToDevice, s));
    }
    return RTDM_OK;
}

void rtdm::rectify_gray_launch(rtdm_rectify* rc, const uint8_t* dl, const uint8_t* dr, int n, Plane8W ol, Plane8W orr, hipStream_t s)
{
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H;
    RectifySrc L{dl, row, fbytes}, R{dr, row, fbytes};
    launch_rectify_gray(L, R, rc->dMap1[0], rc->dMap2[0], rc->dMap1[1], rc->dMap2[1], rc->W, rc->H, rc->rw, rc->rh, ol, orr, n, s);
}

int rtdm_rectify_gray(rtdm_rectify* rc, const uint8_t* rgb_left, size_t left_pitch, const uint8_t* rgb_right,
                      size_t right_pitch, uint8_t* left_rect, size_t left_rect_pitch, uint8_t* right_rect,
                      size_t right_rect_pitch)
{
    if (!rc || !rgb_left || !rgb_right || !left_rect || !right_rect) return RTDM_ERR_NULL;
    const size_t row = (size_t)rc->W * 3;
    if (left_pitch < row || right_pitch < row || left_rect_pitch < (size_t)rc->rw || right_rect_pitch < (size_t)rc->rw) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(rc->device));
    hipStream_t s = rc->stream;
    DrainOnError drain{s};
    int st = rectify_upload(rc, rgb_left, left_pitch, rgb_right, right_pitch, s);
    if (st) return st;
    const size_t gframe = rc->gpitch * rc->rh;
    rectify_gray_launch(rc, rc->dRgb[0], rc->dRgb[1], 1, Plane8W{rc->dGray[0], rc->gpitch, gframe}, Plane8W{rc->dGray[1], rc->gpitch, gframe}, s);
    HIPC(hipGetLastError());
    // back through the page-locked area (2-D copies into pageable memory take the slow path)
    uint8_t* hl = rc->hStage + 2 * (size_t)rc->W * rc->H * 3;
    uint8_t* hr = hl + gframe;
    HIPC(hipMemcpyAsync(hl, rc->dGray[0], gframe, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(hr, rc->dGray[1], gframe, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    copy_rows(left_rect, left_rect_pitch, hl, rc->gpitch, (size_t)rc->rw, rc->rh, RowPad::KEEP);
    copy_rows(right_rect, right_rect_pitch, hr, rc->gpitch, (size_t)rc->rw, rc->rh, RowPad::KEEP);
    return RTDM_OK;
}

int rtdm_rectify_rgb(rtdm_rectify* rc, int which, const uint8_t* rgb, size_t pitch, uint8_t* out, size_t out_pitch)
{
    if (!rc || !rgb || !out) return RTDM_ERR_NULL;
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H;
    if ((which != 0 && which != 1) || pitch < row || out_pitch < (size_t)rc->rw * 3) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(rc->device));
    hipStream_t s = rc->stream;
    DrainOnError drain{s};
    int st = rectify_upload(rc, rgb, pitch, nullptr, 0, s);
    if (st) return st;
    launch_rectify_rgb(RectifySrc{rc->dRgb[0], row, fbytes}, rc->dMap1[which], rc->dMap2[which], rc->W, rc->H, rc->rw, rc->rh,
                       Plane8W{rc->dOut, (size_t)rc->rw * 3, (size_t)rc->rw * 3 * rc->rh}, 1, s);
    HIPC(hipGetLastError());
    uint8_t* ho = rc->hStage + 2 * fbytes;
    HIPC(hipMemcpyAsync(ho, rc->dOut, (size_t)rc->rw * 3 * rc->rh, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    copy_rows(out, out_pitch, ho, (size_t)rc->rw * 3, (size_t)rc->rw * 3, rc->rh, RowPad::KEEP);
    return RTDM_OK;
}

int rtdm_rectify_gray_device(rtdm_rectify* rc, int n, const uint8_t* d_rgb_left, const uint8_t* d_rgb_right,
                             uint8_t* d_left_rect, uint8_t* d_right_rect, void* hip_stream)
{
    if (!rc || !d_rgb_left || !d_rgb_right || !d_left_rect || !d_right_rect) return RTDM_ERR_NULL;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(rc->device));
    const size_t oframe = (size_t)rc->rw * rc->rh;
    rectify_gray_launch(rc, d_rgb_left, d_rgb_right, n, Plane8W{d_left_rect, (size_t)rc->rw, oframe},
                        Plane8W{d_right_rect, (size_t)rc->rw, oframe}, (hipStream_t)hip_stream);
    HIPC(hipGetLastError());
    return RTDM_OK;
}
