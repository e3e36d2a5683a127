// k_depth.hip -- the step right after the matcher, kept on the device:
//     left_disp /= 16.;  reprojectImageTo3D(left_disp, xyz, Q, true, CV_32F);  calc_depth(...)
// (estimator.cpp:75-77 and 206-263).  Only the per-object mean Z leaves the GPU.
// Semantics and the floating-point contract: oracle/depth_oracle.c (Z = (float)(Zh/Wh) from double
// arithmetic, mean = double sum / count).  The sum order here is fixed (tree per row, rows in order), so the
// result is reproducible run to run; against the oracle's row-major order it agrees to ~1e-15 relative.
// The pixel rule (depth_pixel, with the ties-to-even / 16) is rtdm_xyz_point.h's, shared with k_depth_objects.hip; the
// frame minimum is k_xyz.hip's launch_xyz_min on ROUNDED keys.
#include "rtdm_kernels.h"
#include "rtdm_xyz_point.h"

namespace rtdm {

// one workgroup = one row of one region: partial (sum of Z, count)
__global__ __launch_bounds__(256) void k_depth_rows(const int16_t* disp, size_t pitch_e, const uint8_t* mask, size_t mpitch,
                                                    DepthQ q, const int* regions, const int* minval, int maxH,
                                                    double* psum, int* pcnt)
{
    __shared__ double rs[256];
    __shared__ int rc[256];
    const int i = blockIdx.y, r = blockIdx.x;
    const int rx = regions[4 * i], ry = regions[4 * i + 1], rw = regions[4 * i + 2], rh = regions[4 * i + 3];
    double s = 0.0;
    int c = 0;
    if (r < rh) {
        const int y = ry + r, mind = *minval;
        for (int x = rx + threadIdx.x; x < rx + rw; x += 256) {
            double zd;
            if (!depth_pixel(q, x, y, disp[(size_t)y * pitch_e + x], mind, &zd) || mask[(size_t)y * mpitch + x] == 0) continue;
            s += zd; ++c;
        }
    }
    rs[threadIdx.x] = s; rc[threadIdx.x] = c;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) { rs[threadIdx.x] += rs[threadIdx.x + k]; rc[threadIdx.x] += rc[threadIdx.x + k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { psum[(size_t)i * maxH + r] = rs[0]; pcnt[(size_t)i * maxH + r] = rc[0]; }
}

__global__ void k_depth_final(const double* psum, const int* pcnt, const int* regions, int n, int maxH, double unit,
                              double* mean, int* counts)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int rh = regions[4 * i + 3];
    double s = 0.0;
    int c = 0;
    for (int r = 0; r < rh; ++r) { s += psum[(size_t)i * maxH + r]; c += pcnt[(size_t)i * maxH + r]; }
    counts[i] = c;
    mean[i] = c > 0 ? (s / c) * unit / 10.0 : 0.0;
}

size_t depth_scratch_bytes(int max_regions, int maxH)
{ return 16 + (size_t)max_regions * 16 + (size_t)max_regions * maxH * 12 + (size_t)max_regions * 12 + 64; }

// scratch layout: [minval | regions n*4 int | psum n*maxH double | pcnt n*maxH int | mean n double | counts n int]
void launch_depth_stats(const int16_t* disp, size_t pitch_e, int W, int H, const DepthQ& q, const uint8_t* mask, size_t mpitch,
                        const int* h_regions, int n, int maxH, double unit, void* scratch, double* h_mean, int* h_counts,
                        hipStream_t stream, bool reuse_min)
{
    unsigned char* p = (unsigned char*)scratch;
    int* minval = (int*)p; p += 16;
    int* dreg = (int*)p; p += (size_t)n * 16;
    p = (unsigned char*)(((size_t)p + 7) & ~(size_t)7);
    double* psum = (double*)p; p += (size_t)n * maxH * 8;
    double* mean = (double*)p; p += (size_t)n * 8;
    int* pcnt = (int*)p; p += (size_t)n * maxH * 4;
    int* counts = (int*)p;
    (void)hipMemcpyAsync(dreg, h_regions, (size_t)n * 16, hipMemcpyHostToDevice, stream);
    if (!reuse_min) launch_xyz_min(XyzDisp{disp, pitch_e, 0}, 1, W, H, XYZ_MODE_ROUNDED, minval, stream);
    if (n > 0) {
        hipLaunchKernelGGL(k_depth_rows, dim3(maxH, n), dim3(256), 0, stream, disp, pitch_e, mask, mpitch, q, dreg, minval, maxH, psum, pcnt);
        hipLaunchKernelGGL(k_depth_final, dim3((n + 63) / 64), dim3(64), 0, stream, psum, pcnt, dreg, n, maxH, unit, mean, counts);
        (void)hipMemcpyAsync(h_mean, mean, (size_t)n * 8, hipMemcpyDeviceToHost, stream);
        (void)hipMemcpyAsync(h_counts, counts, (size_t)n * 4, hipMemcpyDeviceToHost, stream);
    }
}

}  // namespace rtdm
