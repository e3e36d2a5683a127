// api_xyz.hip -- rtdm_xyz: reprojectImageTo3D and the point cloud (estimator.cpp:75-77, :235; rules X1-X8).
#include "rtdm_handles.h"

using namespace rtdm;

static_assert(sizeof(rtdm_point) == 16 && sizeof(XyzRec) == 16, "rtdm_point is a 16-byte record");

static int xyz_validate(const rtdm_xyz_params& p)
{
    if (p.disparity_mode != RTDM_XYZ_FIXED16 && p.disparity_mode != RTDM_XYZ_ROUNDED) return RTDM_ERR_BAD_PARAM;
    if (p.handle_missing_values != 0 && p.handle_missing_values != 1) return RTDM_ERR_BAD_PARAM;
    for (int i = 0; i < 16; ++i) if (!std::isfinite(p.Q[i])) return RTDM_ERR_BAD_PARAM;
    if (!(p.max_z > 0.0)) return RTDM_ERR_BAD_PARAM;
    return RTDM_OK;
}

static XyzParams xyz_kernel_params(const rtdm_xyz_params& p)
{
    XyzParams P;
    std::copy(p.Q, p.Q + 16, P.q);
    P.max_z = p.max_z; P.mode = p.disparity_mode; P.hmv = p.handle_missing_values;
    // (min_disparity - 1) * 16 as the int the 16-bit map is compared with; outside int16 no pixel carries it
    const long inv = ((long)p.min_disparity - 1) * 16;
    P.invalid16 = inv >= INT16_MIN && inv <= INT16_MAX ? (int)inv : INT32_MIN;
    return P;
}

void rtdm_xyz_default_params(rtdm_xyz_params* p, const double* Q, int min_disparity)
{
    if (!p) return;
    for (int i = 0; i < 16; ++i) p->Q[i] = Q ? Q[i] : (i % 5 == 0 ? 1.0 : 0.0);
    p->disparity_mode = RTDM_XYZ_ROUNDED; p->handle_missing_values = 1; p->min_disparity = min_disparity; p->max_z = 10000.0;
}

void rtdm_xyz_destroy(rtdm_xyz* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->mem.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int rtdm_xyz_create(const rtdm_xyz_params* params, int max_width, int max_height, int max_batch, int device, rtdm_xyz** out)
{
    if (!params || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    int rc = xyz_validate(*params);
    if (rc) return rc;
    if (max_width <= 0 || max_height <= 0 || max_batch <= 0 || max_batch > 65535) return RTDM_ERR_BAD_SIZE;
    if ((long)max_width * max_height > (long)INT32_MAX) return RTDM_ERR_UNSUPPORTED;   // counts and record numbers are ints
    rc = use_device(device);
    if (rc) return rc;
    rtdm_xyz* h = new (std::nothrow) rtdm_xyz();
    if (!h) return RTDM_ERR_NOMEM;
    h->p = *params; h->maxW = max_width; h->maxH = max_height; h->maxB = max_batch; h->device = device;
    AllocList& m = h->mem;
    m.err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    m.dev(&h->dMin, (size_t)max_batch * sizeof(int));
    m.dev(&h->dTile, (size_t)max_batch * xyz_tiles(max_width, max_height) * sizeof(int));
    m.dev(&h->dCounts, (size_t)max_batch * sizeof(int));
    // single-frame staging of the host entry points: 40 bytes per pixel of max_width x max_height
    const size_t fr = (size_t)max_width * max_height;
    m.dev(&h->dDisp, fr * 2); m.dev(&h->dGuide, fr * 3); m.dev(&h->dMask, fr); m.dev(&h->dImgL, fr); m.dev(&h->dImgR, fr);
    m.dev(&h->dXYZ, fr * 12); m.dev(&h->dZ, fr * 4); m.dev(&h->dPts, fr * sizeof(XyzRec));
    if (m.err != hipSuccess) { const hipError_t e = m.err; rtdm_xyz_destroy(h); return create_failed("rtdm_xyz_create", e); }
    *out = h;
    return RTDM_OK;
}

int rtdm_xyz_set_params(rtdm_xyz* h, const rtdm_xyz_params* params)
{
    if (!h || !params) return RTDM_ERR_NULL;
    const int rc = xyz_validate(*params);
    if (rc) return rc;
    h->p = *params;                // kernels take the parameters by value: calls already enqueued keep theirs
    return RTDM_OK;
}

int rtdm_xyz_get_params(const rtdm_xyz* h, rtdm_xyz_params* out)
{
    if (!h || !out) return RTDM_ERR_NULL;
    *out = h->p;
    return RTDM_OK;
}

static int xyz_check(const rtdm_xyz* h, int W, int H)
{
    if (W <= 0 || H <= 0 || W > h->maxW || H > h->maxH) return RTDM_ERR_BAD_SIZE;
    return RTDM_OK;
}

int rtdm_xyz_map_device(rtdm_xyz* h, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride, int width,
                        int height, float* d_xyz, size_t xyz_pitch, size_t xyz_frame_stride, float* d_z, size_t z_pitch,
                        size_t z_frame_stride, void* hip_stream)
{
    if (!h || !d_disp) return RTDM_ERR_NULL;
    int rc = xyz_check(h, width, height);
    if (rc) return rc;
    if (n <= 0 || (!d_xyz && !d_z)) return RTDM_ERR_BAD_SIZE;
    const size_t W = (size_t)width;
    if (disp_pitch < 2 * W || ((disp_pitch | disp_frame_stride) & 1) ||
        (d_xyz && (xyz_pitch < 12 * W || ((xyz_pitch | xyz_frame_stride) & 3))) ||
        (d_z && (z_pitch < 4 * W || ((z_pitch | z_frame_stride) & 3))))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    const XyzParams P = xyz_kernel_params(h->p);
    for (int i0 = 0; i0 < n; i0 += h->maxB) {
        const int m = std::min(h->maxB, n - i0);
        XyzDisp D{d_disp + (size_t)i0 * (disp_frame_stride / 2), disp_pitch / 2, disp_frame_stride / 2};
        XyzMap O{d_xyz ? d_xyz + (size_t)i0 * (xyz_frame_stride / 4) : nullptr, xyz_pitch / 4, xyz_frame_stride / 4,
                 d_z ? d_z + (size_t)i0 * (z_frame_stride / 4) : nullptr, z_pitch / 4, z_frame_stride / 4};
        launch_xyz_map(D, m, width, height, P, h->dMin, O, s);
        HIPC(hipGetLastError());
    }
    return RTDM_OK;
}

int rtdm_xyz_map(rtdm_xyz* h, const int16_t* disp, size_t disp_pitch, int width, int height, float* xyz, size_t xyz_pitch,
                 float* z, size_t z_pitch)
{
    if (!h || !disp) return RTDM_ERR_NULL;
    int rc = xyz_check(h, width, height);
    if (rc) return rc;
    const size_t W = (size_t)width, fr = W * height;
    if ((!xyz && !z) || disp_pitch < 2 * W || (xyz && xyz_pitch < 12 * W) || (z && z_pitch < 4 * W)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(h->dDisp, W * 2, disp, disp_pitch, W * 2, height, hipMemcpyHostToDevice, s));
    XyzDisp D{h->dDisp, W, fr};
    XyzMap O{xyz ? h->dXYZ : nullptr, 3 * W, 3 * fr, z ? h->dZ : nullptr, W, fr};
    launch_xyz_map(D, 1, width, height, xyz_kernel_params(h->p), h->dMin, O, s);
    HIPC(hipGetLastError());
    if (xyz) HIPC(hipMemcpy2DAsync(xyz, xyz_pitch, h->dXYZ, W * 12, W * 12, height, hipMemcpyDeviceToHost, s));
    if (z) HIPC(hipMemcpy2DAsync(z, z_pitch, h->dZ, W * 4, W * 4, height, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    return RTDM_OK;
}

// what both cloud entries check of the optional planes, before any device use
int rtdm::xyz_cloud_check(const rtdm_xyz* h, const void* disp, const void* guide, int channels, int width, int height, const void* points,
                          int capacity, const void* count)
{
    if (!h || !disp || !count || (channels != 0 && !guide) || (capacity > 0 && !points)) return RTDM_ERR_NULL;
    if ((channels != 0 && channels != 1 && channels != 3) || capacity < 0) return RTDM_ERR_BAD_PARAM;
    return xyz_check(h, width, height);
}

int rtdm_xyz_cloud_device(rtdm_xyz* h, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                          const uint8_t* d_guide, size_t guide_pitch, size_t guide_frame_stride, int channels,
                          const uint8_t* d_mask, size_t mask_pitch, size_t mask_frame_stride, int width, int height,
                          rtdm_point* d_points, size_t points_frame_stride, int capacity, int* d_counts, void* hip_stream)
{
    int rc = xyz_cloud_check(h, d_disp, d_guide, channels, width, height, d_points, capacity, d_counts);
    if (rc) return rc;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    const size_t W = (size_t)width;
    if (disp_pitch < 2 * W || ((disp_pitch | disp_frame_stride) & 1) || (channels && guide_pitch < W * channels) ||
        (d_mask && mask_pitch < W) ||
        (capacity > 0 && (((uintptr_t)d_points | points_frame_stride) & 3)) ||
        (capacity > 0 && n > 1 && points_frame_stride < (size_t)capacity * sizeof(rtdm_point)))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    const XyzParams P = xyz_kernel_params(h->p);
    for (int i0 = 0; i0 < n; i0 += h->maxB) {
        const int m = std::min(h->maxB, n - i0);
        XyzCloudIn I{};
        I.disp = XyzDisp{d_disp + (size_t)i0 * (disp_frame_stride / 2), disp_pitch / 2, disp_frame_stride / 2};
        I.cn = channels;
        if (channels) { I.guide = d_guide + (size_t)i0 * guide_frame_stride; I.gpitch = guide_pitch; I.gframe = guide_frame_stride; }
        if (d_mask) { I.mask = d_mask + (size_t)i0 * mask_frame_stride; I.mpitch = mask_pitch; I.mframe = mask_frame_stride; }
        XyzRec* pts = capacity > 0 ? (XyzRec*)((unsigned char*)d_points + (size_t)i0 * points_frame_stride) : nullptr;
        launch_xyz_cloud(I, m, width, height, P, h->dMin, h->dTile, pts, points_frame_stride, capacity, d_counts + i0, s);
        HIPC(hipGetLastError());
    }
    return RTDM_OK;
}

// the staged disparity map (and guide / mask) of one frame -> count and the first min(count, capacity) records, synchronous
int rtdm::xyz_cloud_staged(rtdm_xyz* h, int channels, bool mask, int width, int height, rtdm_point* points, int capacity, int* count,
                           hipStream_t s)
{
    const size_t W = (size_t)width, fr = W * height;
    const int cap = (int)std::min((size_t)capacity, fr);        // a frame has at most W * H records
    XyzCloudIn I{};
    I.disp = XyzDisp{h->dDisp, W, fr};
    I.cn = channels;
    if (channels) { I.guide = h->dGuide; I.gpitch = W * channels; I.gframe = fr * channels; }
    if (mask) { I.mask = h->dMask; I.mpitch = W; I.mframe = fr; }
    launch_xyz_cloud(I, 1, width, height, xyz_kernel_params(h->p), h->dMin, h->dTile, h->dPts, 0, cap, h->dCounts, s);
    HIPC(hipGetLastError());
    int c = 0;
    HIPC(hipMemcpyAsync(&c, h->dCounts, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    const int wr = std::min(c, cap);
    if (wr > 0) {
        HIPC(hipMemcpyAsync(points, h->dPts, (size_t)wr * sizeof(rtdm_point), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
    }
    *count = c;
    return RTDM_OK;
}

int rtdm_xyz_cloud(rtdm_xyz* h, const int16_t* disp, size_t disp_pitch, const uint8_t* guide, size_t guide_pitch, int channels,
                   const uint8_t* mask, size_t mask_pitch, int width, int height, rtdm_point* points, int capacity, int* count)
{
    int rc = xyz_cloud_check(h, disp, guide, channels, width, height, points, capacity, count);
    if (rc) return rc;
    const size_t W = (size_t)width;
    if (disp_pitch < 2 * W || (channels && guide_pitch < W * channels) || (mask && mask_pitch < W)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(h->dDisp, W * 2, disp, disp_pitch, W * 2, height, hipMemcpyHostToDevice, s));
    if (channels) HIPC(hipMemcpy2DAsync(h->dGuide, W * channels, guide, guide_pitch, W * channels, height, hipMemcpyHostToDevice, s));
    if (mask) HIPC(hipMemcpy2DAsync(h->dMask, W, mask, mask_pitch, W, height, hipMemcpyHostToDevice, s));
    rc = xyz_cloud_staged(h, channels, mask != nullptr, width, height, points, capacity, count, s);
    if (rc) return rc;
    drain.armed = false;
    return RTDM_OK;
}
