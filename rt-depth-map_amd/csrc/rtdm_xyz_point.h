// rtdm_xyz_point.h -- the point of a pixel, one statement per rule so that every kernel gives the same bits.  Rules X1-X4 and
// the Z part of X6 -- the disparity key, the unfused homogeneous point, Z and its keep test -- for
// k_xyz.hip (the frame minimum, the dense map and the cloud) and k_measure.hip (the per-object measurements); calc_depth's
// older pixel rule D2 (section 4.16) for k_depth.hip and k_depth_objects.hip.  Device code only.
#pragma once
#include "rtdm_kernels.h"

#include <cfloat>

namespace rtdm {

__device__ __forceinline__ int xyz_rhe_div16(int d)     // d / 16, ties to even (Mat /= 16. on CV_16S)
{
    int q = d >> 4;
    const int r = d & 15;
    if (r > 8 || (r == 8 && (q & 1))) ++q;
    return q;
}

// X1 as an integer key: equal keys <=> equal d, and the order of the keys is the order of d, so the frame minimum and the
// X4 test are integer work.  FIXED16: the raw x16 value; ROUNDED: the rounded quotient.
__device__ __forceinline__ int xyz_key(int disp, int mode) { return mode ? xyz_rhe_div16(disp) : disp; }
__device__ __forceinline__ double xyz_d(int key, int mode) { return mode ? (double)key : (double)key * 0.0625; }   // exact

// X2: h_r = ((Q[4r] x + Q[4r+1] y) + Q[4r+2] d) + Q[4r+3], no fused multiply-add
__device__ __forceinline__ double xyz_h(const XyzParams& P, int r, double x, double y, double d)
{
#pragma clang fp contract(off)
    const double a = P.q[4 * r] * x;
    const double b = P.q[4 * r + 1] * y;
    const double c = P.q[4 * r + 2] * d;
    return ((a + b) + c) + P.q[4 * r + 3];
}

// X3 + X4: Z of a pixel; x4: X4 is on and mk is the frame's minimum key.  *h3 for the other two components.
__device__ __forceinline__ float xyz_z(const XyzParams& P, int key, bool x4, int mk, double xd, double yd, double d, double* h3)
{
    *h3 = xyz_h(P, 3, xd, yd, d);
    const float z = (float)(xyz_h(P, 2, xd, yd, d) / *h3);
    return (x4 && key == mk) ? 10000.0f : z;
}

// the Z part of X6, G4 (NaN fails both tests)
__device__ __forceinline__ bool xyz_keep_z(const XyzParams& P, float z)
{
    const double zd = (double)z;
    return fabs(zd - 10000.0) >= (double)FLT_EPSILON && fabs(zd) <= P.max_z;
}

// D2: calc_depth's rule for pixel (x, y) with the raw x16 disparity `raw` in a frame whose smallest rounded disparity is mind:
// does the pixel count, and *zd = its Z.  The bits of Z are those of this expression as the compiler contracts it here, which
// is not xyz_h's unfused order: the text stays as it is.
__device__ __forceinline__ bool depth_pixel(const DepthQ& q, int x, int y, int raw, int mind, double* zd_out)
{
    const int d = xyz_rhe_div16(raw);
    const double Zh = q.q[8] * x + q.q[9] * y + q.q[10] * d + q.q[11];
    const double Wh = q.q[12] * x + q.q[13] * y + q.q[14] * d + q.q[15];
    float z = (float)(Zh / Wh);
    if (d == mind) z = 10000.0f;
    const double zd = (double)z;
    *zd_out = zd;
    return !(fabs(zd - 10000.0) < 1.1920928955078125e-07 || fabs(zd) > 10000.0);
}

}  // namespace rtdm
