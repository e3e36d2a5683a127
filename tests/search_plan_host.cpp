// search_plan_host.cpp -- prints what plan_search (rt-depth-map_amd/csrc/k_search.hip) plans, one line per configuration:
//     search_plan_host <n> <planes_contiguous> { <W> <H> <D> <w> <minD> <cap> <legacy> }...
// Linked against librtdm_hip.so; touches no device (plan_search makes no runtime call).  tests/test_search_plan_cpu.py.
#include "rtdm_kernels.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace rtdm;

// api_bm.hip's make_geom for a full frame without ROIs, disp12MaxDiff = 1, textureThreshold = uniquenessRatio = 10
static BMGeom geom(int W, int H, int D, int w, int minD, int cap, int legacy)
{
    BMGeom g{};
    g.W = W; g.H = H; g.Ws = (W + 7) & ~7; g.D = D; g.minD = minD; g.w = w; g.r = w / 2;
    g.cap = cap; g.tex = 10; g.uniq = 10;
    g.lofs = std::max(D - 1 + minD, 0);
    g.rofs = -std::min(D - 1 + minD, 0);
    g.width1 = W - g.rofs - D + 1;
    g.filtered = (minD - 1) * 16;
    g.want_cost = 1; g.cost16 = 2L * cap * w * w < 65536; g.mask_cols = 0; g.legacy = legacy;
    const int maxD = minD + D - 1;
    g.vx0 = std::max(std::max(0, maxD) + g.r, 0); g.vx1 = std::min(std::min(W, W - minD) - g.r, W);
    g.vy0 = g.r; g.vy1 = H - g.r;
    const int reach = D + std::abs(minD) + 2;
    g.cx0 = std::max(g.lofs, g.vx0 - reach);
    g.cx1 = std::min(std::min(W, g.lofs + g.width1), g.vx1 + reach);
    return g;
}

int main(int argc, char** argv)
{
    if (argc < 3 || (argc - 3) % 7 != 0) { fprintf(stderr, "usage: %s n contiguous {W H D w minD cap legacy}...\n", argv[0]); return 2; }
    const int n = atoi(argv[1]);
    const bool contiguous = atoi(argv[2]) != 0;
    static const char* const tiles[] = {"generic", "fast", "ring"};
    static const char* const forms[] = {"NONE", "ROWS", "DISP", "GENERIC"};
    static const char* const places[] = {"FUSED", "SIDE", "AFTER"};
    for (int a = 3; a < argc; a += 7) {
        int v[7];
        for (int k = 0; k < 7; ++k) v[k] = atoi(argv[a + k]);
        const BMGeom g = geom(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
        const SearchPlan p = plan_search(g, n, contiguous);
        const bool legacy = p.border.form == BorderForm::DISP && g.legacy;
        printf("%dx%d D=%d w=%d minD=%d cap=%d legacy=%d: tiles=%s lanes=%d interior=[%d,%d) border=%s%s place=%s left=[%d,%d) right=[%d,%d) grid=%dx%d variant=%s\n",
               v[0], v[1], v[2], v[3], v[4], v[5], v[6], tiles[(int)p.tiles], p.lanes, p.x0, p.x0 + p.nx, forms[(int)p.border.form],
               legacy ? "+LEGACY" : "", places[(int)p.place], p.lx0, p.lx1, p.rx0, p.rx1, p.border.gx, p.border.gy, p.variant);
    }
    return 0;
}
