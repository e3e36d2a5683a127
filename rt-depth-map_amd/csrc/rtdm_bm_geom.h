// rtdm_bm_geom.h -- the rectangles of one StereoBM frame under its ROIs: the valid-disparity
// rectangle (getValidDisparityROI, clipped to the image and to rows that have a full window) and the columns worth searching.
// ONE statement of that arithmetic for the host's make_geom (api_bm.hip) and for the kernels that take a frame's ROI1 from
// device memory (k_bm_rois.hip, rule B3 of DESIGN.md section 4.19); plain C++, so that tests/bm_geom_host.cpp runs it under
// the sanitizers.  Everything is computed in 64 bits and saturated to int at the end: whatever the four ints of a rectangle
// hold, nothing overflows, and the result is what 32-bit arithmetic gives wherever that does not overflow.
#pragma once

#if defined(__HIPCC__)
#define RTDM_HD __host__ __device__
#else
#define RTDM_HD
#endif

namespace rtdm {

// What the handle knows on the host: frame size, numDisparities, minDisparity, blockSize / 2, "the left-right check is on"
// (disp12MaxDiff >= 0) and ROI2 as rtdm_bm_set_roi stored it (x, y, w, h; w <= 0 or h <= 0: none).
struct BMRoiGeom { int W, H, D, minD, r, lr; int roi2[4]; };
// [vx0, vx1) x [vy0, vy1): the valid rectangle; [cx0, cx1): the searched columns; any = 0: the whole frame is FILTERED.
struct BMRoiRect { int vx0, vx1, vy0, vy1, cx0, cx1, any; };

RTDM_HD inline long long bm_geom_max(long long a, long long b) { return a > b ? a : b; }
RTDM_HD inline long long bm_geom_min(long long a, long long b) { return a < b ? a : b; }
RTDM_HD inline int bm_geom_sat(long long v)
{
    return (int)bm_geom_min(bm_geom_max(v, -2147483647LL - 1), 2147483647LL);
}

// roi1: x, y, w, h, or null; w <= 0 or h <= 0: no ROI1 (rtdm_bm_set_roi's meaning of an empty rectangle).
// envelope: ROI1 is left out altogether -- the rectangle that contains the rectangle of EVERY ROI1 (xmin and ymin grow with
// the rectangle's origin, xmax and ymax with its far corner; "no ROI1" is the frame itself, and a rectangle that reaches
// beyond the frame can yield columns the frame's own does not).
RTDM_HD inline BMRoiRect bm_roi_rect(const BMRoiGeom& G, const int* roi1, bool envelope)
{
    typedef long long ll;
    const ll W = G.W, H = G.H, D = G.D, minD = G.minD, r = G.r;
    const ll big = 1LL << 40;                       // beyond every sum of two ints
    ll a0 = 0, b0 = 0, a1 = W, b1 = H;               // ROI1 as [a0, a1) x [b0, b1)
    if (roi1 && roi1[2] > 0 && roi1[3] > 0) { a0 = roi1[0]; b0 = roi1[1]; a1 = a0 + roi1[2]; b1 = b0 + roi1[3]; }
    if (envelope) { a0 = -big; b0 = -big; a1 = big; b1 = big; }
    ll p0 = 0, q0 = 0, p1 = W, q1 = H;               // ROI2
    if (G.roi2[2] > 0 && G.roi2[3] > 0) { p0 = G.roi2[0]; q0 = G.roi2[1]; p1 = p0 + G.roi2[2]; q1 = q0 + G.roi2[3]; }
    const ll lofs = bm_geom_max(D - 1 + minD, 0), rofs = -bm_geom_min(D - 1 + minD, 0), width1 = W - rofs - D + 1;
    const ll maxD = minD + D - 1;
    ll xmin = bm_geom_max(a0, p0 + maxD) + r;
    ll xmax = bm_geom_min(a1, p1 - minD) - r;
    ll ymin = bm_geom_max(b0, q0) + r;
    ll ymax = bm_geom_min(b1, q1) - r;
    xmin = bm_geom_max(xmin, 0); xmax = bm_geom_min(xmax, W);
    ymin = bm_geom_max(ymin, r); ymax = bm_geom_min(ymax, H - r);
    // Columns worth searching (estimator.cpp:54 shrinks the rectangle every frame with setROI1):
    // validateDisparity lets column x vote for x - round(d/16) in [x - maxD - 1, x - minD + 1] and
    // reads the votes of x - floor/ceil(d/16), so a valid column depends on searched columns at
    // most D + |minD| + 2 away.  Everything else is masked to FILTERED anyway.
    const ll reach = G.lr ? D + (minD < 0 ? -minD : minD) + 2 : 0;
    BMRoiRect q;
    q.vx0 = bm_geom_sat(xmin); q.vx1 = bm_geom_sat(xmax); q.vy0 = bm_geom_sat(ymin); q.vy1 = bm_geom_sat(ymax);
    q.cx0 = bm_geom_sat(bm_geom_max(lofs, xmin - reach));
    q.cx1 = bm_geom_sat(bm_geom_min(bm_geom_min(W, lofs + width1), xmax + reach));
    q.any = !(lofs >= W || rofs >= W || width1 < 1) && xmax > xmin && ymax > ymin;
    return q;
}

}  // namespace rtdm
