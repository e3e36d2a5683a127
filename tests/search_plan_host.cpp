// search_plan_host.cpp -- prints what plan_search (rt-depth-map_amd/csrc/k_search.hip) plans, one line per configuration:
//     search_plan_host <n> <planes_contiguous> { <W> <H> <D> <w> <minD> <cap> <legacy> }...
// Second mode, for the configurations the ring kernel takes: how it cuts a frame of a batch of n into row strips,
//     search_plan_host strips <n> { <W> <H> <D> <w> <minD> <cap> <legacy> }...
// one line each: the strip count of ring_strips_model, the output rows per strip (a strip walks w - 1 rows more) and the rows
// between two rebases of its prefix rings (0: it does not rebase, its strips are short enough).
// Linked against librtdm_hip.so; touches no device (plan_search makes no runtime call).  tests/test_search_plan_cpu.py.
#include "rtdm_kernels.h"
#include "rtdm_search.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

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

// The strips of a ring launch.  ring_strips_model is the library's; what ring_launch_one (k_search_ring.hip) does with its
// answer, and the rebase interval (ring_rows_cap, ring_rebase_trips, RingCfg::TRIP), are restated here.
static int strips_mode(int argc, char** argv)
{
    if (argc < 3 || (argc - 3) % 7 != 0) { fprintf(stderr, "usage: %s strips n {W H D w minD cap legacy}...\n", argv[0]); return 2; }
    const int n = atoi(argv[2]);
    for (int a = 3; a < argc; a += 7) {
        int v[7];
        for (int k = 0; k < 7; ++k) v[k] = atoi(argv[a + k]);
        const BMGeom g = geom(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
        const SearchPlan p = plan_search(g, n, true);
        int strips = 0, rs = 0, rebase_rows = 0;
        if (p.tiles == SearchTiles::RING) {
            const int nrows = g.vy1 - g.vy0;
            const int rows_cap = 65535 / (g.w * 2 * g.cap) - g.w - 6;
            const int W1 = g.w + 1, rpg = g.D >= 96 ? 4 : p.lanes;
            const int trip = (W1 % rpg == 0) ? W1 : (2 * W1 % rpg == 0) ? 2 * W1 : 4 * W1;
            const int trips = rows_cap / trip;
            const int smin = trips > 0 ? 1 : std::max(1, (nrows + rows_cap - 1) / rows_cap);
            strips = std::max(ring_strips_model(p, g, n), smin);
            strips = std::max(1, std::min(strips, nrows));
            rs = (nrows + strips - 1) / strips;
            strips = (nrows + rs - 1) / rs;
            rebase_rows = trips * trip;
        }
        printf("%dx%d D=%d w=%d minD=%d cap=%d legacy=%d n=%d: lanes=%d strips=%d rows_per_strip=%d rebase_rows=%d\n",
               v[0], v[1], v[2], v[3], v[4], v[5], v[6], n, p.lanes, strips, rs, rebase_rows);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "strips") return strips_mode(argc, argv);
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
