// rtdm_xyz_point.h -- the point of a pixel (rules X1-X3), shared by k_xyz.hip (the dense map and the
// cloud) and k_measure.hip (the per-object measurements): one statement of the disparity key and of the unfused homogeneous
// point, so that both give the same bits.  Device code only.
#pragma once
#include "rtdm_kernels.h"

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

}  // namespace rtdm
