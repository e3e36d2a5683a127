// rtdm_objslot.h -- which slots of the detector's device lists hold an object and which pixels it covers (rules D1 / D4,
// DESIGN.md section 4.16), shared by k_depth_objects.hip and k_measure.hip.  Device code only.
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

}  // namespace rtdm
