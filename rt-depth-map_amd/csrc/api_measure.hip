// api_measure.hip -- rtdm_objects_measure_device: Z quantiles, extent and centre per object from the detector's device lists
// (rules G1-G10).  Handle-free, like rtdm_depth_objects_device.
#include "rtdm_handles.h"

#include <cmath>

using namespace rtdm;

void rtdm_measure_default_params(rtdm_measure_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->disparity_mode = RTDM_XYZ_ROUNDED;
    p->max_z = 1e4;
    p->nquant = 3;
    p->permille[0] = 500; p->permille[1] = 250; p->permille[2] = 750;
}

size_t rtdm_objects_measure_workspace_bytes(int n, int capacity, int height, int nquant) { return measure_bytes(n, capacity, height, nquant); }

int rtdm::measure_params_check(const rtdm_measure_params* p)
{
    if (p->disparity_mode != RTDM_XYZ_FIXED16 && p->disparity_mode != RTDM_XYZ_ROUNDED) return RTDM_ERR_BAD_PARAM;
    if (!std::isfinite(p->max_z) || p->max_z <= 0.0) return RTDM_ERR_BAD_PARAM;
    if (p->nquant < 0 || p->nquant > 8) return RTDM_ERR_BAD_PARAM;
    for (int k = 0; k < p->nquant; ++k)
        if (p->permille[k] < 0 || p->permille[k] > 1000) return RTDM_ERR_BAD_PARAM;
    return RTDM_OK;
}

void rtdm::measure_params_kernel(const rtdm_measure_params* p, const double* Q, XyzParams* P, MeasQuant* mq)
{
    std::copy(Q, Q + 16, P->q);
    P->max_z = p->max_z; P->mode = p->disparity_mode; P->hmv = 1; P->invalid16 = 0;      // G3: X4 always on; G4: no marker clause
    memset(mq, 0, sizeof *mq);
    mq->nquant = p->nquant;
    std::copy(p->permille, p->permille + p->nquant, mq->permille);
}

int rtdm_objects_measure_device(int device, const rtdm_measure_params* params, int n, const int16_t* d_disp, size_t disp_pitch,
                                size_t disp_frame_stride, int width, int height, const double* Q, const void* d_planes,
                                size_t plane_pitch, size_t plane_stride, int planes_are_labels, int nclasses,
                                const struct rtdm_object* d_objects, int capacity, const int* d_counts,
                                rtdm_object_measure* d_measures, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    static_assert(sizeof(rtdm_object_measure) == 88 && sizeof(MeasRecord) == sizeof(rtdm_object_measure), "one record layout");
    // G10, before any device use
    int st = depth_objects_check(n, d_disp, disp_pitch, disp_frame_stride, width, height, Q, d_planes, plane_pitch, plane_stride,
                                 planes_are_labels ? 4 : 1, nclasses, d_objects, capacity, d_counts, true, d_workspace);
    if (st) return st;
    if (!params || !d_measures) return RTDM_ERR_NULL;
    st = measure_params_check(params);
    if (st) return st;
    if ((size_t)d_measures % 8) return RTDM_ERR_BAD_SIZE;
    if (workspace_bytes < measure_bytes(n, capacity, height, params->nquant)) return RTDM_ERR_BAD_SIZE;
    if ((long long)width * height >= (1LL << 31)) return RTDM_ERR_UNSUPPORTED;     // (rtdm_xyz's limit for the same points; G10 keeps it)
    if (n == 0) return RTDM_OK;
    st = use_device(device);
    if (st) return st;
    XyzParams P; MeasQuant mq;
    measure_params_kernel(params, Q, &P, &mq);
    const DepthObjects a{d_disp, disp_pitch / 2, disp_frame_stride / 2, (const uint8_t*)d_planes, plane_pitch, plane_stride,
                         (const CcObject*)d_objects, d_counts, n, width, height, nclasses, capacity, 0};
    launch_measure(a, P, mq, d_workspace, (MeasRecord*)d_measures, (hipStream_t)hip_stream, planes_are_labels != 0);
    HIPC(hipGetLastError());
    return RTDM_OK;
}
