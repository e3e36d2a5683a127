// k_depth_objects.hip -- calc_depth (estimator.cpp:206-263) for a batch of frames whose object lists lie in device memory as
// rtdm_objects_detect_device leaves them (rules D1-D6).  The pixel rule is k_depth.hip's; what differs
// is where the regions come from (the device lists: no host knowledge of the counts, no limit on their number) and how the
// lanes are laid over a box: one wave per band of DOBJ_BAND rows of an object, the lanes folded over as many rows as the box
// width lets fit into 64, the band's partial in the workspace, and a second kernel that adds the bands of an object in order.
#include "rtdm_kernels.h"
#include "rtdm_objslot.h"

#include <climits>

namespace rtdm {

__device__ __forceinline__ int dobj_div16(int d)    // d/16, ties to even (Mat /= 16. on CV_16S), as k_depth.hip
{
    int q = d >> 4;
    const int r = d & 15;
    if (r > 8 || (r == 8 && (q & 1))) ++q;
    return q;
}

// grid: (row groups, n frames); minval[f] starts above every int16
__global__ __launch_bounds__(256) void k_dobj_min(const int16_t* disp, size_t pitch_e, size_t frame_e, int W, int H, int* minval)
{
    __shared__ int red[4];
    const int16_t* p = disp + (size_t)blockIdx.y * frame_e;
    int m = INT_MAX;
    for (int y = blockIdx.x; y < H; y += gridDim.x)
        for (int x = threadIdx.x; x < W; x += 256) m = min(m, dobj_div16(p[(size_t)y * pitch_e + x]));
    for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMin(minval + blockIdx.y, min(min(red[0], red[1]), min(red[2], red[3])));
}

// one wave = one band of one object slot; the waves stride over all n * cap * nb of them.  LABELS (rule L5): the planes are
// the detector's int32 label planes and slot i counts the pixels that carry i + 1 -- the value is compared, never used
// (L6); the walk and the reduction tree are the same code for both predicates.
template <bool LABELS>
__global__ __launch_bounds__(256) void k_dobj_bands(DepthObjects a, DepthQ q, const int* minval, double* psum, int* pcnt)
{
    const int lane = threadIdx.x & 63;
    const long long items = (long long)a.n * a.cap * a.nb;
    for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * 4) {
        const int band = (int)(it % a.nb);
        const long long slot = it / a.nb;
        const int i = (int)(slot % a.cap), f = (int)(slot / a.cap);
        DobjBox b;
        if (!dobj_slot(a, f, i, &b)) continue;
        const int cw = b.x1 - b.x0, ch = b.y1 - b.y0, r0 = band * DOBJ_BAND;
        if (r0 >= ch) continue;
        const int r1 = min(r0 + DOBJ_BAND, ch);
        int lw = 1;                                    // lanes of a row: the box width rounded up to a power of two, at most 64
        while (lw < cw && lw < 64) lw <<= 1;
        const int col = lane & (lw - 1), rof = lane / lw, rstep = 64 / lw;
        const int16_t* dp = a.disp + (size_t)f * a.dframe_e;
        const uint8_t* mp = a.mask + ((size_t)f * a.K + b.cls) * a.mplane;
        const int mind = minval[f];
        double s = 0.0;
        int c = 0;
        for (int r = r0 + rof; r < r1; r += rstep) {
            const int y = b.y0 + r;
            for (int x = b.x0 + col; x < b.x1; x += lw) {
                const int d = dobj_div16(dp[(size_t)y * a.dpitch_e + x]);
                const double Zh = q.q[8] * x + q.q[9] * y + q.q[10] * d + q.q[11];
                const double Wh = q.q[12] * x + q.q[13] * y + q.q[14] * d + q.q[15];
                float z = (float)(Zh / Wh);
                if (d == mind) z = 10000.0f;
                const double zd = (double)z;
                if (fabs(zd - 10000.0) < 1.1920928955078125e-07 || fabs(zd) > 10000.0) continue;
                if (LABELS ? *(const int32_t*)(mp + (size_t)y * a.mpitch + (size_t)x * 4) != i + 1 : mp[(size_t)y * a.mpitch + x] == 0) continue;
                s += zd; ++c;
            }
        }
        for (int off = 32; off > 0; off >>= 1) { s += __shfl_down(s, off); c += __shfl_down(c, off); }
        if (lane == 0) { psum[(size_t)slot * a.nb + band] = s; pcnt[(size_t)slot * a.nb + band] = c; }
    }
}

// one lane = one object slot: its bands in ascending order
__global__ __launch_bounds__(256) void k_dobj_final(DepthObjects a, const double* psum, const int* pcnt, double unit, double* mean, int* npix)
{
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= (long long)a.n * a.cap) return;
    DobjBox b;
    if (!dobj_slot(a, (int)(slot / a.cap), (int)(slot % a.cap), &b)) return;
    const int bands = (b.y1 - b.y0 + DOBJ_BAND - 1) / DOBJ_BAND;
    double s = 0.0;
    int c = 0;
    for (int k = 0; k < bands; ++k) { s += psum[(size_t)slot * a.nb + k]; c += pcnt[(size_t)slot * a.nb + k]; }
    npix[slot] = c;
    mean[slot] = c > 0 ? (s / c) * unit / 10.0 : 0.0;
}

static size_t dobj_bands(int H) { return (size_t)((std::max(H, 0) + DOBJ_BAND - 1) / DOBJ_BAND); }
static size_t dobj_min_bytes(int n) { return ((size_t)std::max(n, 0) * sizeof(int) + 63) & ~(size_t)63; }

// workspace layout, from its address rounded up to 8 (the 64 bytes on top pay for that):
// [n minima, padded to 64 bytes | psum n * cap * nb double | pcnt n * cap * nb int]
size_t depth_objects_bytes(int n, int cap, int H)
{
    return 64 + dobj_min_bytes(n) + (size_t)std::max(n, 0) * std::max(cap, 0) * dobj_bands(H) * (sizeof(double) + sizeof(int));
}

void launch_depth_objects(DepthObjects a, const DepthQ& q, double unit, void* workspace, double* mean, int* npix, hipStream_t stream,
                          bool labels)
{
    if (a.n <= 0) return;
    a.nb = (int)dobj_bands(a.H);
    unsigned char* p = (unsigned char*)(((size_t)workspace + 7) & ~(size_t)7);
    int* minval = (int*)p; p += dobj_min_bytes(a.n);
    const size_t parts = (size_t)a.n * a.cap * a.nb;
    double* psum = (double*)p; p += parts * sizeof(double);
    int* pcnt = (int*)p;
    (void)hipMemsetAsync(minval, 0x7f, (size_t)a.n * sizeof(int), stream);           // 0x7f7f7f7f is above any int16
    for (int f0 = 0; f0 < a.n; f0 += 32768)           // (the grid's second dimension ends at 65535)
        hipLaunchKernelGGL(k_dobj_min, dim3(std::min(a.H, 64), std::min(a.n - f0, 32768)), dim3(256), 0, stream,
                           a.disp + (size_t)f0 * a.dframe_e, a.dpitch_e, a.dframe_e, a.W, a.H, minval + f0);
    if (a.cap <= 0) return;
    const size_t blocks = std::min<size_t>((parts + 3) / 4, (size_t)1 << 16);
    if (labels) hipLaunchKernelGGL(k_dobj_bands<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a, q, minval, psum, pcnt);
    else hipLaunchKernelGGL(k_dobj_bands<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a, q, minval, psum, pcnt);
    const size_t slots = (size_t)a.n * a.cap;
    hipLaunchKernelGGL(k_dobj_final, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, a, psum, pcnt, unit, mean, npix);
}

}  // namespace rtdm
