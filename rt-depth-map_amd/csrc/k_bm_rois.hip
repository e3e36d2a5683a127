// k_bm_rois.hip -- the row stage of the block matcher under PER-FRAME ROIs that lie in device memory
// (rtdm_bm_compute_device_rois, rules B1-B6 in DESIGN.md section 4.19).  The search runs once for the batch under the envelope
// of every ROI1 (rtdm_bm_geom.h); k_roi_mask then gives each frame the state its own restricted search would have left
// (FILTERED outside its searched columns and valid rows), and after the left-right check the frame's valid rectangle;
// k_copy16_rois brings the planes to the caller and leaves the skipped frames alone.  A frame's four ints become its
// rectangles on the device, in 64 bits (bm_roi_rect); they only ever enter COMPARISONS with the coordinates a thread took
// from its grid index, so no address depends on them.
#include "rtdm_kernels.h"
#include "rtdm_bm_geom.h"
#include "rtdm_pk16.h"

namespace rtdm {

// B2: a frame whose rectangle has w <= 0 or h <= 0 is skipped (not rtdm_bm_set_roi's "no ROI")
__device__ __forceinline__ bool roi_skipped(const int* rois, int f) { return rois[4 * f + 2] <= 0 || rois[4 * f + 3] <= 0; }

// One thread per 8-column chunk of a row of the handle's internal plane (rows of W rounded up to 8 elements, 16-byte aligned;
// the padding columns are the plane's own and become FILTERED with the rest).  grid (chunks of a frame / 256, n).
template <RoiMask WHAT>
__global__ __launch_bounds__(256) void k_roi_mask(Plane16W d, BMRoiGeom G, const int* __restrict__ rois, int inv)
{
    const int nch = (G.W + 7) >> 3;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nch * G.H) return;
    const int f = blockIdx.y;
    if (roi_skipped(rois, f)) return;
    const int roi[4] = {rois[4 * f], rois[4 * f + 1], rois[4 * f + 2], rois[4 * f + 3]};
    const BMRoiRect q = bm_roi_rect(G, roi, false);
    int x0 = WHAT == RoiMask::VALID ? q.vx0 : WHAT == RoiMask::SEARCHED ? q.cx0 : max(q.cx0, q.vx0);
    int x1 = WHAT == RoiMask::VALID ? q.vx1 : WHAT == RoiMask::SEARCHED ? q.cx1 : min(q.cx1, q.vx1);
    int y0 = q.vy0, y1 = q.vy1;
    if (!q.any) { x0 = 0; x1 = 0; y0 = 0; y1 = 0; }                   // the whole frame is FILTERED
    const int y = idx / nch, xs = (idx - y * nch) * 8;
    const bool row_in = y >= y0 && y < y1;
    if (row_in && xs >= x0 && xs + 8 <= x1) return;                   // inside: stays what it is
    Short8* p = (Short8*)(d.base + (size_t)f * d.frame_e + (size_t)y * d.pitch_e + xs);
    Short8 v;
    if (!row_in || xs + 8 <= x0 || xs >= x1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v.v[k] = (int16_t)inv;
    } else {
        v = *p;
#pragma unroll
        for (int k = 0; k < 8; ++k) if (xs + k < x0 || xs + k >= x1) v.v[k] = (int16_t)inv;
    }
    *p = v;
}

void launch_roi_mask(RoiMask what, Plane16W disp, const BMRoiGeom& G, const int* d_rois, int n, int filtered, hipStream_t stream)
{
    const dim3 grid((unsigned)((((G.W + 7) >> 3) * G.H + 255) / 256), (unsigned)n), block(256);
    switch (what) {
        case RoiMask::SEARCHED: hipLaunchKernelGGL(k_roi_mask<RoiMask::SEARCHED>, grid, block, 0, stream, disp, G, d_rois, filtered); break;
        case RoiMask::VALID:    hipLaunchKernelGGL(k_roi_mask<RoiMask::VALID>, grid, block, 0, stream, disp, G, d_rois, filtered); break;
        case RoiMask::BOTH:     hipLaunchKernelGGL(k_roi_mask<RoiMask::BOTH>, grid, block, 0, stream, disp, G, d_rois, filtered); break;
    }
}

// k_copy16 (k_prefilter.hip) for the frames that are not skipped: W x H elements of every other frame, nothing else (B2)
__global__ __launch_bounds__(256) void k_copy16_rois(Plane16W src, Plane16W dst, int W, int H, const int* __restrict__ rois)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W * H || roi_skipped(rois, blockIdx.y)) return;
    const int y = idx / W, x = idx - y * W;
    dst.base[(size_t)blockIdx.y * dst.frame_e + (size_t)y * dst.pitch_e + x] = src.base[(size_t)blockIdx.y * src.frame_e + (size_t)y * src.pitch_e + x];
}

void launch_copy16_rois(Plane16W src, Plane16W dst, int W, int H, int n, const int* d_rois, hipStream_t stream)
{
    hipLaunchKernelGGL(k_copy16_rois, dim3((W * H + 255) / 256, n), dim3(256), 0, stream, src, dst, W, H, d_rois);
}

}  // namespace rtdm
