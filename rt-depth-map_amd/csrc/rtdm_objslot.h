// rtdm_objslot.h -- an object's pixels, stated once for k_depth_objects.hip and k_measure.hip: which slots of the detector's
// device lists hold an object and which pixels it covers (rules D1 / D4), which of them its plane
// passes (L5 / G2), and the walk of its box (D3): the order in which the band kernels add is part of their output bits, so
// the item loop, the lane layout, the pixel loop and the lane fold exist here and nowhere else.  Behind them the host side of
// the two workspaces: the band count, the frame minima in front and the pointer behind them.
#pragma once
#include "rtdm_kernels.h"

namespace rtdm {

#define DOBJ_BAND 16              // rows of a box one wave sums (D3: part of the summation order)

struct DobjBox { int x0, y0, x1, y1, cls; };

// D1 / D4: is slot i of frame f a stored object, and which pixels of the frame does it cover?  false: the slot is not
// written at all.  A stored object whose class is no plane or whose clipped box is empty comes back with x1 == x0.
__device__ __forceinline__ bool dobj_slot(const DepthObjects& a, int f, int i, DobjBox* b)
{
    long long total = 0;
    for (int c = 0; c < a.K; ++c) total += max(a.counts[(size_t)f * a.K + c], 0);
    if ((long long)i >= min(total, (long long)a.cap)) return false;
    const CcObject o = a.obj[(size_t)f * a.cap + i];
    const long long x0 = max((long long)o.x, 0LL), y0 = max((long long)o.y, 0LL);
    const long long x1 = min((long long)o.x + o.w, (long long)a.W), y1 = min((long long)o.y + o.h, (long long)a.H);
    const bool ok = o.cls >= 0 && o.cls < a.K && o.w > 0 && o.h > 0 && x1 > x0 && y1 > y0;
    b->x0 = ok ? (int)x0 : 0; b->y0 = ok ? (int)y0 : 0; b->x1 = ok ? (int)x1 : 0; b->y1 = ok ? (int)y1 : 0;
    b->cls = ok ? o.cls : 0;
    return true;
}

__device__ __forceinline__ int dobj_box_bands(const DobjBox& b) { return (b.y1 - b.y0 + DOBJ_BAND - 1) / DOBJ_BAND; }

// L5 / G2: does the plane pass pixel (x, y) for slot i?  A mask byte that is not 0, or the label i + 1 -- the value is
// compared, never used (L6).
template <bool LABELS>
__device__ __forceinline__ bool dobj_plane(const uint8_t* mp, size_t mpitch, int x, int y, int i)
{
    return LABELS ? *(const int32_t*)(mp + (size_t)y * mpitch + (size_t)x * 4) == i + 1 : mp[(size_t)y * mpitch + x] != 0;
}

// D3: the lanes of a wave over a box of width cw.  lw lanes per row -- the width rounded up to a power of two, at most 64 --
// and 64 / lw rows at once: this lane owns column col of a row's groups of lw and row rof of every rstep rows.
struct DobjLanes { int lw, col, rof, rstep; };
__device__ __forceinline__ DobjLanes dobj_lanes(int cw, int lane)
{
    int lw = 1;
    while (lw < cw && lw < 64) lw <<= 1;
    return DobjLanes{lw, lane & (lw - 1), lane / lw, 64 / lw};
}

// D3: one wave = one band of one object slot; the waves of a grid of 256-lane workgroups stride over all n * cap * nb of
// them.  body(it) runs once for every band that holds rows of a stored object.
struct DobjItem {
    long long slot; int f, i, band;               // slot = f * cap + i
    DobjBox b; int r0, r1;                        // the band's rows of the clipped box: b.y0 + r0 .. b.y0 + r1 - 1
    const int16_t* dp; const uint8_t* mp;         // the frame's map and the plane of the object's class
};
template <class Body>
__device__ __forceinline__ void dobj_for_bands(const DepthObjects& a, Body body)
{
    const long long items = (long long)a.n * a.cap * a.nb;
    for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * 4) {
        DobjItem t;
        t.band = (int)(it % a.nb);
        t.slot = it / a.nb;
        t.i = (int)(t.slot % a.cap); t.f = (int)(t.slot / a.cap);
        if (!dobj_slot(a, t.f, t.i, &t.b)) continue;
        const int ch = t.b.y1 - t.b.y0;
        t.r0 = t.band * DOBJ_BAND;
        if (t.r0 >= ch) continue;
        t.r1 = min(t.r0 + DOBJ_BAND, ch);
        t.dp = a.disp + (size_t)t.f * a.dframe_e;
        t.mp = a.mask + ((size_t)t.f * a.K + t.b.cls) * a.mplane;
        body(t);
    }
}

// D3: the pixels of a band that this lane owns, in the order it adds them: its rows ascending, inside a row its columns
// ascending.
template <class Pixel>
__device__ __forceinline__ void dobj_for_pixels(const DobjItem& t, Pixel pixel)
{
    const DobjLanes L = dobj_lanes(t.b.x1 - t.b.x0, threadIdx.x & 63);
    for (int r = t.r0 + L.rof; r < t.r1; r += L.rstep) {
        const int y = t.b.y0 + r;
        for (int x = t.b.x0 + L.col; x < t.b.x1; x += L.lw) pixel(x, y);
    }
}

// D3: the lanes of a wave folded into lane 0 -- 32 and 32, 16 and 16, ... -- with op(mine, the other lane's)
struct DobjAdd { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
template <class T, class Op>
__device__ __forceinline__ T dobj_fold(T v, Op op)
{
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_down(v, off));
    return v;
}

// ---- host side: both workspaces begin, from their address rounded up to 8, with the n frame minima padded to 64 bytes -------
inline size_t dobj_bands(int H) { return (size_t)((std::max(H, 0) + DOBJ_BAND - 1) / DOBJ_BAND); }
inline size_t dobj_min_bytes(int n) { return ((size_t)std::max(n, 0) * sizeof(int) + 63) & ~(size_t)63; }
inline int* dobj_carve_min(void* workspace, int n, unsigned char** behind)
{
    unsigned char* p = (unsigned char*)(((size_t)workspace + 7) & ~(size_t)7);
    *behind = p + dobj_min_bytes(n);
    return (int*)p;
}

}  // namespace rtdm
