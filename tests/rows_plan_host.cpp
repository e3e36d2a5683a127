// rows_plan_host.cpp -- prints what plan_lrcheck and plan_speckle (rt-depth-map_amd/csrc/k_rows.hip) plan for the two row
// stages behind the StereoBM search, one line per configuration:
//     rows_plan_host bm { <W> <H> <D> <w> <cap> <n> <disp12MaxDiff> <speckleWindowSize> <rows_aligned> }...
// the way api_bm.hip's chunk_back chains them (full frame, no ROI, minDisparity 0, speckleRange 32);
//     rows_plan_host sgm { <W> <H> <n> }...
// the hand-off of sgm_finish (per-pixel heads, nothing merged, every row, workspace rows of W elements, aligned plane);
//     rows_plan_host sweep <D> <w> <cap>
// the bm line for every W in 16..4096 that is a multiple of 8, n in {1, 16, 1024} and H in {w + 1, w + 3, 720};
//     rows_plan_host lr { <W> <H> <D> <w> <cap> <n> <disp12MaxDiff> <speckleWindowSize> <speckleRange> <minDisparity>
//                         <roi1 x> <roi1 y> <roi1 w> <roi1 h> }...
// the left-right check alone under any minDisparity, speckleRange and ROI1 (w or h <= 0: none), with the geometry of
// api_bm.hip's make_geom (rtdm_bm_geom.h) and aligned rows.
// Linked against librtdm_hip.so; touches no device (the plans make no runtime call).  tests/test_rows_plan_cpu.py.
#include "rtdm_kernels.h"
#include "rtdm_bm_geom.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace rtdm;

static const char* const HEADS[] = {"NONE", "PIXEL", "CHUNK"};

// api_bm.hip's make_geom for a full frame without ROIs, minDisparity 0 (what the plans read of it)
static BMGeom geom(int W, int H, int D, int w, int cap)
{
    BMGeom g{};
    g.W = W; g.H = H; g.Ws = (W + 7) & ~7; g.D = D; g.minD = 0; g.w = w; g.r = w / 2; g.cap = cap;
    g.filtered = -16; g.cost16 = 2L * cap * w * w < 65536;
    g.vx0 = std::min(D - 1 + g.r, W); g.vx1 = std::max(W - g.r, 0); g.vy0 = g.r; g.vy1 = H - g.r;
    return g;
}

// api_bm.hip's make_geom: any minDisparity, ROI1 as rtdm_bm_set_roi stores it, no ROI2; false: the whole frame is FILTERED
static bool geom_roi(int W, int H, int D, int w, int cap, int minD, bool lr, const int* roi1, BMGeom* g)
{
    *g = BMGeom{};
    g->W = W; g->H = H; g->Ws = (W + 7) & ~7; g->D = D; g->minD = minD; g->w = w; g->r = w / 2; g->cap = cap;
    g->lofs = std::max(D - 1 + minD, 0); g->rofs = -std::min(D - 1 + minD, 0); g->width1 = W - g->rofs - D + 1;
    g->filtered = (minD - 1) * 16; g->want_cost = lr; g->cost16 = 2L * cap * w * w < 65536; g->mask_cols = !lr;
    const BMRoiRect q = bm_roi_rect(BMRoiGeom{W, H, D, minD, w / 2, lr, {0, 0, 0, 0}}, roi1, false);
    g->vx0 = q.vx0; g->vx1 = q.vx1; g->vy0 = q.vy0; g->vy1 = q.vy1; g->cx0 = q.cx0; g->cx1 = q.cx1;
    return q.any != 0;
}

static const char* const FORMS[] = {"scalar_u16", "scalar_i32", "vec_wave", "vec_half", "vec_half2", "packed"};

static void lr_line(const int* v)
{
    const int W = v[0], H = v[1], D = v[2], w = v[3], cap = v[4], n = v[5], maxdiff = v[6], window = v[7], range = v[8], minD = v[9];
    BMGeom g;
    const bool any = geom_roi(W, H, D, w, cap, minD, maxdiff >= 0, v + 10, &g);
    const bool speckle = range >= 0 && window > 0;                   // chunk_back's condition
    printf("%dx%d D=%d w=%d cap=%d n=%d maxdiff=%d window=%d range=%d minD=%d roi=%d,%d,%d,%d: ", W, H, D, w, cap, n, maxdiff, window, range,
           minD, v[10], v[11], v[12], v[13]);
    if (!any || maxdiff < 0) { printf("lr: -\n"); return; }
    const LrPlan p = plan_lrcheck(g, maxdiff, speckle ? range : 0, n, speckle, true);
    printf("lr: form=%s init=%d threads=%u gy=%u gz=%u lds=%zu heads=%s block_rows=%d rect=%d,%d,%d,%d\n", FORMS[(int)p.form],
           p.heads != SpkHeads::NONE, p.threads, p.gy, p.n, p.lds, HEADS[(int)p.heads], p.block_rows, g.vx0, g.vy0, g.vx1 - g.vx0, g.vy1 - g.vy0);
}

static void print_spk(const SpkPlan& s, int y_hi)
{
    static const char* const merge[] = {"none", "rows", "strip<4,pixel>", "strip<1,chunk>", "strip<2,chunk>", "strip<4,chunk>",
                                        "strip<1,chunk,REC>"};
    printf("spk: init_lds=%zu heads=%s rec_own=%d rec_fused=%d rec_rows=%d rec_blk=%d merge=%s gx=%d first=%d npairs=%d ystep=%d y_hi=%d "
           "rows_gx=%d\n", s.init_lds, HEADS[(int)s.heads], s.rec_own.blocks, s.rec_fused.blocks, s.rec_own.nrows + s.rec_fused.nrows,
           s.rec_own.blk + s.rec_fused.blk, merge[(int)s.merge], s.merge_gx, s.first, s.npairs, s.ystep, y_hi, s.rows_gx);
}

static void bm_line(int W, int H, int D, int w, int cap, int n, int maxdiff, int window, int aligned)
{
    static const char* const forms[] = {"scalar_u16", "scalar_i32", "vec_wave", "vec_half", "vec_half2", "packed"};
    const BMGeom g = geom(W, H, D, w, cap);
    const bool speckle = window > 0;
    printf("%dx%d D=%d w=%d cap=%d n=%d maxdiff=%d window=%d aligned=%d: ", W, H, D, w, cap, n, maxdiff, window, aligned);
    SpkHeads heads = SpkHeads::NONE;
    int block_rows = 1;
    if (maxdiff >= 0) {
        const LrPlan p = plan_lrcheck(g, maxdiff, speckle ? 32 : 0, n, speckle, aligned != 0);
        printf("lr: form=%s threads=%u gy=%u gz=%u lds=%zu heads=%s block_rows=%d ", forms[(int)p.form], p.threads, p.gy, p.n, p.lds,
               HEADS[(int)p.heads], p.block_rows);
        heads = p.heads; block_rows = p.block_rows;
    } else printf("lr: - ");
    if (speckle) print_spk(plan_speckle(W, g.Ws, H, n, heads, block_rows, g.vy0, g.vy1, aligned != 0), heads == SpkHeads::NONE ? H : g.vy1);
    else printf("spk: -\n");
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "bm" && (argc - 2) % 9 == 0) {
        for (int a = 2; a < argc; a += 9) {
            int v[9];
            for (int k = 0; k < 9; ++k) v[k] = atoi(argv[a + k]);
            bm_line(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]);
        }
        return 0;
    }
    if (mode == "lr" && (argc - 2) % 14 == 0) {
        for (int a = 2; a < argc; a += 14) {
            int v[14];
            for (int k = 0; k < 14; ++k) v[k] = atoi(argv[a + k]);
            lr_line(v);
        }
        return 0;
    }
    if (mode == "sgm" && (argc - 2) % 3 == 0) {
        for (int a = 2; a < argc; a += 3) {
            const int W = atoi(argv[a]), H = atoi(argv[a + 1]), n = atoi(argv[a + 2]);
            printf("sgm %dx%d n=%d: ", W, H, n);
            print_spk(plan_speckle(W, W, H, n, SpkHeads::PIXEL, 1, 0, H, true), H);
        }
        return 0;
    }
    if (mode == "sweep" && argc == 5) {
        const int D = atoi(argv[2]), w = atoi(argv[3]), cap = atoi(argv[4]);
        for (int W = 16; W <= 4096; W += 8)
            for (int n : {1, 16, 1024})
                for (int H : {w + 1, w + 3, 720}) bm_line(W, H, D, w, cap, n, 1, 100, 1);
        return 0;
    }
    fprintf(stderr, "usage: %s bm {W H D w cap n disp12MaxDiff speckleWindowSize rows_aligned}... | sgm {W H n}... | sweep D w cap | "
                    "lr {W H D w cap n disp12MaxDiff speckleWindowSize speckleRange minDisparity roi1x roi1y roi1w roi1h}...\n", argv[0]);
    return 2;
}
