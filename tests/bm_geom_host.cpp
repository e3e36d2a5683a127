// bm_geom_host.cpp -- the matcher's geometry header (csrc/rtdm_bm_geom.h) as a stand-alone host program: reads one case per
// line from stdin (W H D minD r lr, ROI2 x y w h, has-ROI1, ROI1 x y w h, envelope) and prints the seven numbers of
// bm_roi_rect for it.  tests/test_bm_rois_cpu.py builds it with -fsanitize=address,undefined and compares the lines with
// make_geom restated in Python integers.
#include <cstdio>

#include "rtdm_bm_geom.h"

int main()
{
    rtdm::BMRoiGeom G;
    int has1, roi[4], env, n = 0;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &G.W, &G.H, &G.D, &G.minD, &G.r, &G.lr, &G.roi2[0], &G.roi2[1],
                      &G.roi2[2], &G.roi2[3], &has1, &roi[0], &roi[1], &roi[2], &roi[3], &env) == 16) {
        const rtdm::BMRoiRect q = rtdm::bm_roi_rect(G, has1 ? roi : nullptr, env != 0);
        std::printf("%d %d %d %d %d %d %d\n", q.vx0, q.vx1, q.vy0, q.vy1, q.cx0, q.cx1, q.any);
        ++n;
    }
    return n > 0 ? 0 : 1;
}
