// k_depth_objects.hip -- calc_depth (estimator.cpp:206-263) for a batch of frames whose object lists lie in device memory as
// rtdm_objects_detect_device leaves them (rules D1-D6).  The pixel rule is k_depth.hip's (depth_pixel,
// rtdm_xyz_point.h) and the frame minimum is k_xyz.hip's (launch_xyz_min on ROUNDED keys); what differs is where the regions
// come from (the device lists: no host knowledge of the counts, no limit on their number) and how the lanes are laid over a
// box.  That walk -- one wave per band of DOBJ_BAND rows of an object, the lanes folded over as many rows as the box width
// lets fit into 64 -- is rtdm_objslot.h's; here are what a pixel adds, the band's partial in the workspace, and a second
// kernel that adds the bands of an object in order.
#include "rtdm_kernels.h"
#include "rtdm_objslot.h"
#include "rtdm_xyz_point.h"

namespace rtdm {

// LABELS (rule L5): the planes are the detector's int32 label planes and slot i counts the pixels that carry i + 1; the walk
// and the reduction tree are the same code for both predicates.
template <bool LABELS>
__global__ __launch_bounds__(256) void k_dobj_bands(DepthObjects a, DepthQ q, const int* minval, double* psum, int* pcnt)
{
    dobj_for_bands(a, [&](const DobjItem& t) {
        const int mind = minval[t.f];
        double s = 0.0;
        int c = 0;
        dobj_for_pixels(t, [&](int x, int y) {
            double zd;
            if (!depth_pixel(q, x, y, t.dp[(size_t)y * a.dpitch_e + x], mind, &zd)) return;
            if (!dobj_plane<LABELS>(t.mp, a.mpitch, x, y, t.i)) return;
            s += zd; ++c;
        });
        s = dobj_fold(s, DobjAdd()); c = dobj_fold(c, DobjAdd());
        if ((threadIdx.x & 63) == 0) { psum[(size_t)t.slot * a.nb + t.band] = s; pcnt[(size_t)t.slot * a.nb + t.band] = c; }
    });
}

// one lane = one object slot: its bands in ascending order
__global__ __launch_bounds__(256) void k_dobj_final(DepthObjects a, const double* psum, const int* pcnt, double unit, double* mean, int* npix)
{
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= (long long)a.n * a.cap) return;
    DobjBox b;
    if (!dobj_slot(a, (int)(slot / a.cap), (int)(slot % a.cap), &b)) return;
    const int bands = dobj_box_bands(b);
    double s = 0.0;
    int c = 0;
    for (int k = 0; k < bands; ++k) { s += psum[(size_t)slot * a.nb + k]; c += pcnt[(size_t)slot * a.nb + k]; }
    npix[slot] = c;
    mean[slot] = c > 0 ? (s / c) * unit / 10.0 : 0.0;
}

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
    unsigned char* p;
    int* minval = dobj_carve_min(workspace, a.n, &p);
    const size_t parts = (size_t)a.n * a.cap * a.nb;
    double* psum = (double*)p; p += parts * sizeof(double);
    int* pcnt = (int*)p;
    launch_xyz_min(XyzDisp{a.disp, a.dpitch_e, a.dframe_e}, a.n, a.W, a.H, XYZ_MODE_ROUNDED, minval, stream);
    if (a.cap <= 0) return;
    const size_t blocks = std::min<size_t>((parts + 3) / 4, (size_t)1 << 16);
    if (labels) hipLaunchKernelGGL(k_dobj_bands<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a, q, minval, psum, pcnt);
    else hipLaunchKernelGGL(k_dobj_bands<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a, q, minval, psum, pcnt);
    const size_t slots = (size_t)a.n * a.cap;
    hipLaunchKernelGGL(k_dobj_final, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, a, psum, pcnt, unit, mean, npix);
}

}  // namespace rtdm
