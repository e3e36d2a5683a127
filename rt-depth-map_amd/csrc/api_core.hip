// api_core.hip -- status strings, the last-error string, device count; the handle-free device entry points.
// There is no CPU fallback anywhere in the C ABI layer (api_*.hip): every entry point that computes needs a HIP device.
#include "rtdm_handles.h"

using namespace rtdm;

thread_local std::string rtdm::g_hip_err;

const char* rtdm_strerror(int s)
{
    switch (s) {
        case RTDM_OK: return "ok";
        case RTDM_ERR_BAD_PARAM: return "invalid StereoBM parameter";
        case RTDM_ERR_BAD_SIZE: return "invalid frame size or pitch";
        case RTDM_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
        case RTDM_ERR_HIP: return "HIP runtime error";
        case RTDM_ERR_NOMEM: return "out of memory";
        case RTDM_ERR_UNSUPPORTED: return "configuration not supported by this build";
        case RTDM_ERR_NULL: return "null pointer";
        case RTDM_ERR_BAD_STREAM: return "damaged or incomplete JPEG stream";
        default: return "unknown rtdm status";
    }
}

const char* rtdm_last_hip_error(void) { return g_hip_err.c_str(); }
int rtdm_abi_version(void) { return RTDM_ABI_VERSION; }

int rtdm_device_count(int* count)
{
    if (!count) return RTDM_ERR_NULL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return n > 0 ? RTDM_OK : RTDM_ERR_NO_DEVICE;
}

// ---- synthetic stream ------------------------------------------------------------------------
int rtdm_synth_pairs_device(uint64_t seed, int first_frame, int n, int width, int height, int numDisparities,
                            uint8_t* d_left, uint8_t* d_right, size_t pitch, size_t frame_stride, int device,
                            void* hip_stream)
{
    if (!d_left || !d_right) return RTDM_ERR_NULL;
    if (n <= 0 || width <= 0 || height <= 0 || pitch < (size_t)width) return RTDM_ERR_BAD_SIZE;
    int rc = use_device(device);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    void* scratch = nullptr;
    HIPC(hipMalloc(&scratch, synth_scratch_bytes(n)));
    Plane8W L{d_left, pitch, frame_stride}, R{d_right, pitch, frame_stride};
    launch_synth(seed, first_frame, n, width, height, numDisparities, L, R, scratch, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    HIPC(e);
    return RTDM_OK;
}

// ---- the step after the matcher ---------------------------------------------------------------
int rtdm::depth_check_regions(const rtdm_region* regions, int n, int W, int H, int* flat, int* maxh)
{
    if (n < 0 || n > RTDM_MAX_REGIONS || (n > 0 && !regions)) return RTDM_ERR_BAD_SIZE;
    *maxh = 1;
    for (int i = 0; i < n; ++i) {
        const rtdm_region& r = regions[i];
        if (r.x < 0 || r.y < 0 || r.width < 0 || r.height < 0 || r.x + r.width > W || r.y + r.height > H) return RTDM_ERR_BAD_SIZE;
        flat[4 * i] = r.x; flat[4 * i + 1] = r.y; flat[4 * i + 2] = r.width; flat[4 * i + 3] = r.height;
        *maxh = std::max(*maxh, r.height);
    }
    return RTDM_OK;
}

int rtdm_depth_stats_device(int device, const int16_t* d_disp, size_t disp_pitch, int width, int height, const double* Q,
                            const uint8_t* d_mask, size_t mask_pitch, const rtdm_region* regions, int nregions,
                            double calibration_unit, double* mean_cm, int* counts, void* hip_stream)
{
    if (!d_disp || !Q || !d_mask || !mean_cm || !counts) return RTDM_ERR_NULL;
    if (width <= 0 || height <= 0 || disp_pitch < (size_t)width * 2 || (disp_pitch & 1) || mask_pitch < (size_t)width) return RTDM_ERR_BAD_SIZE;
    int flat[4 * RTDM_MAX_REGIONS], maxh = 1;
    int rc = depth_check_regions(regions, nregions, width, height, flat, &maxh);
    if (rc) return rc;
    rc = use_device(device);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    void* scratch = nullptr;
    HIPC(hipMalloc(&scratch, depth_scratch_bytes(std::max(nregions, 1), maxh)));
    DepthQ q; std::copy(Q, Q + 16, q.q);
    launch_depth_stats(d_disp, disp_pitch / 2, width, height, q, d_mask, mask_pitch, flat, nregions, maxh, calibration_unit,
                       scratch, mean_cm, counts, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    HIPC(e);
    return RTDM_OK;
}

// ---- ... for frame batches, from the detector's device lists (rules D1-D6) --------------------------------------------------
size_t rtdm_depth_objects_workspace_bytes(int n, int capacity, int height) { return depth_objects_bytes(n, capacity, height); }

// D6 up to the class count, for both forms of the planes: mask bytes (elem 1) or the detector's int32 labels (elem 4: rule L5,
// and L8 for the pitches).  outputs: the call's result pointers are all there.
int rtdm::depth_objects_check(int n, const void* d_disp, size_t disp_pitch, size_t disp_frame_stride, int width, int height,
                              const double* Q, const void* d_planes, size_t plane_pitch, size_t plane_stride, size_t elem, int nclasses,
                              const void* d_objects, int capacity, const void* d_counts, bool outputs, const void* d_workspace)
{
    if (!d_disp || !Q || !d_planes || !d_counts || !outputs || !d_workspace || (capacity > 0 && !d_objects)) return RTDM_ERR_NULL;
    if (n < 0 || capacity < 0 || width <= 0 || height <= 0) return RTDM_ERR_BAD_SIZE;
    if ((disp_pitch & 1) || (disp_frame_stride & 1) || disp_pitch < (size_t)width * 2 || plane_pitch < (size_t)width * elem) return RTDM_ERR_BAD_SIZE;
    if (plane_pitch % elem || plane_stride % elem || (size_t)d_planes % elem) return RTDM_ERR_BAD_SIZE;
    if (n > 1 && disp_frame_stride < disp_pitch * height) return RTDM_ERR_BAD_SIZE;
    if (n > 0 && (long)n * nclasses > 1 && plane_stride < plane_pitch * height) return RTDM_ERR_BAD_SIZE;
    if (nclasses < 1 || nclasses > RTDM_MAX_CLASSES) return RTDM_ERR_BAD_PARAM;
    return RTDM_OK;
}

static int depth_objects_call(int device, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride, int width,
                              int height, const double* Q, const void* d_planes, size_t plane_pitch, size_t plane_stride, size_t elem,
                              int nclasses, const rtdm_object* d_objects, int capacity, const int* d_counts, double calibration_unit,
                              double* d_mean_cm, int* d_npix, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    // D6, before any device use
    const int st = depth_objects_check(n, d_disp, disp_pitch, disp_frame_stride, width, height, Q, d_planes, plane_pitch, plane_stride, elem,
                                       nclasses, d_objects, capacity, d_counts, d_mean_cm && d_npix, d_workspace);
    if (st) return st;
    if (workspace_bytes < depth_objects_bytes(n, capacity, height)) return RTDM_ERR_BAD_SIZE;      // D5
    if (n == 0) return RTDM_OK;
    const int rc = use_device(device);
    if (rc) return rc;
    DepthQ q; std::copy(Q, Q + 16, q.q);
    DepthObjects a{d_disp, disp_pitch / 2, disp_frame_stride / 2, (const uint8_t*)d_planes, plane_pitch, plane_stride,
                   (const CcObject*)d_objects, d_counts, n, width, height, nclasses, capacity, 0};
    launch_depth_objects(a, q, calibration_unit, d_workspace, d_mean_cm, d_npix, (hipStream_t)hip_stream, elem == 4);
    HIPC(hipGetLastError());
    return RTDM_OK;
}

int rtdm_depth_objects_device(int device, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                              int width, int height, const double* Q, const uint8_t* d_masks, size_t mask_pitch,
                              size_t mask_plane_stride, int nclasses, const rtdm_object* d_objects, int capacity,
                              const int* d_counts, double calibration_unit, double* d_mean_cm, int* d_npix,
                              void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    return depth_objects_call(device, n, d_disp, disp_pitch, disp_frame_stride, width, height, Q, d_masks, mask_pitch, mask_plane_stride, 1,
                              nclasses, d_objects, capacity, d_counts, calibration_unit, d_mean_cm, d_npix, d_workspace, workspace_bytes,
                              hip_stream);
}

int rtdm_depth_objects_labels_device(int device, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                                     int width, int height, const double* Q, const int32_t* d_labels, size_t label_pitch,
                                     size_t label_plane_stride, int nclasses, const rtdm_object* d_objects, int capacity,
                                     const int* d_counts, double calibration_unit, double* d_mean_cm, int* d_npix,
                                     void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    return depth_objects_call(device, n, d_disp, disp_pitch, disp_frame_stride, width, height, Q, d_labels, label_pitch, label_plane_stride,
                              4, nclasses, d_objects, capacity, d_counts, calibration_unit, d_mean_cm, d_npix, d_workspace,
                              workspace_bytes, hip_stream);
}
