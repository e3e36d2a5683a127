// k_rectmap.hip -- initUndistortRectifyMap(M, D, R, P, size, CV_16SC2) on the device (main.cpp:95-96): the two fixed-point
// remap tables, bit-identical to orc_init_undistort_rectify_map ("the map kernel").
//
// The ray of pixel (i, j) is NOT ir * (j, i, 1): the library's scalar loop, and the oracle, start every row at
// (i ir[1] + ir[2], i ir[4] + ir[5], i ir[7] + ir[8]) and ADD (ir[0], ir[3], ir[6]) once per column, so column j carries j
// roundings.  That chain is kept, in two passes:
//   k_rectmap_walk   one lane per row: only the three additions per column, from column 0 of the full frame, leaving the
//                    running ray at every 64th column (a checkpoint: 3 doubles; lane-consecutive stores, row fastest);
//   k_rectmap_pixel  one lane per map entry: the checkpoint of its 64-column chunk, its remaining j & 63 additions, then the
//                    distortion model, two divisions, rint(u * 32), the int32 clamp and the packing, as the oracle writes
//                    them.  Lanes of a row are column-consecutive: one 4-byte store (map1) and one 2-byte store (map2) each.
// Only the entries of the rectangle (rx, ry, rw, rh) are written, rh x rw; the walk still starts at column 0.
//
// Floating point: every multiply, add and division is a double operation rounded on its own, in the written order --
// contraction is off for this file; divisions are IEEE.
#include "rtdm_kernels.h"

#pragma clang fp contract(off)

namespace rtdm {

__global__ __launch_bounds__(64) void k_rectmap_walk(RectMapParams P, int ry, int rh, int cols, int nck, double* ckpt)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= rh) return;
    const double i = (double)(ry + r);
    double x = i * P.ir[1] + P.ir[2], y = i * P.ir[4] + P.ir[5], w = i * P.ir[7] + P.ir[8];
    for (int c = 0; c < nck; ++c) {
        double* o = ckpt + (size_t)c * 3 * rh + r;
        o[0] = x; o[rh] = y; o[2 * (size_t)rh] = w;
        const int steps = min(64, cols - c * 64);
        for (int s = 0; s < steps; ++s) { x += P.ir[0]; y += P.ir[3]; w += P.ir[6]; }
    }
}

__global__ __launch_bounds__(256) void k_rectmap_pixel(RectMapParams P, int rx, int rw, int rh, const double* ckpt, int16_t* map1,
                                                       uint16_t* map2)
{
    const int jo = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (jo >= rw) return;
    const int j = rx + jo;
    const double* ck = ckpt + (size_t)(j >> 6) * 3 * rh + r;
    double _x = ck[0], _y = ck[rh], _w = ck[2 * (size_t)rh];
    for (int s = j & 63; s > 0; --s) { _x += P.ir[0]; _y += P.ir[3]; _w += P.ir[6]; }
    const double k1 = P.k[0], k2 = P.k[1], p1 = P.k[2], p2 = P.k[3], k3 = P.k[4], k4 = P.k[5], k5 = P.k[6], k6 = P.k[7];
    const double s1 = P.k[8], s2 = P.k[9], s3 = P.k[10], s4 = P.k[11];
    const double w = 1. / _w, x = _x * w, y = _y * w;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2;
    const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2;
    const double u = P.fx * xd + P.u0, v = P.fy * yd + P.v0;
    double su = rint(u * 32.0), sv = rint(v * 32.0);                 // round half to even
    su = fmin(fmax(su, -2147483648.0), 2147483647.0);
    sv = fmin(fmax(sv, -2147483648.0), 2147483647.0);
    const int iu = (int)su, iv = (int)sv;
    const size_t e = (size_t)r * rw + jo;
    short2 m;
    m.x = (short)(iu >> 5); m.y = (short)(iv >> 5);
    reinterpret_cast<short2*>(map1)[e] = m;
    map2[e] = (uint16_t)((iv & 31) * 32 + (iu & 31));
}

int rectmap_chunks(int rx, int rw) { return (rx + rw + 63) / 64; }
size_t rectmap_scratch_bytes(int rx, int rw, int rh) { return (size_t)rectmap_chunks(rx, rw) * 3 * (size_t)rh * sizeof(double); }

void launch_rectmap(const RectMapParams& P, int rx, int ry, int rw, int rh, double* ckpt, int16_t* map1, uint16_t* map2,
                    hipStream_t stream)
{
    const int cols = rx + rw, nck = rectmap_chunks(rx, rw);
    hipLaunchKernelGGL(k_rectmap_walk, dim3((rh + 63) / 64), dim3(64), 0, stream, P, ry, rh, cols, nck, ckpt);
    hipLaunchKernelGGL(k_rectmap_pixel, dim3((rw + 255) / 256, rh), dim3(256), 0, stream, P, rx, rw, rh, ckpt, map1, map2);
}

}  // namespace rtdm
