// k_search.hip -- K2, the search stage as one plan and one launch entry (host only: the kernels are in the k_search_*.hip files,
// which say through rtdm_search.h what they are instantiated for and launch what the plan tells them).
//
// The tile kernel takes the output columns whose window needs no border clamping.  The first and last w/2 searched columns
// do clamp; they lie outside the valid rectangle but vote in the left-right check, so they must be exact, and they go to a
// border form.  Routes per configuration: DESIGN.md, "K2: routes".
#include "rtdm_search.h"

#include <algorithm>

namespace rtdm {

// The searched output columns (setROI1: only the needed ones) split into the interior [x0, x0 + nx), whose windows need no
// border clamping, and what is left of it, [lx0, lx1), and right of it, [rx0, rx1).  false: no interior.
static bool search_ranges(const BMGeom& g, SearchPlan* p)
{
    const int r = g.r;
    int xl = 0, xh = g.width1 - 1;
    xl = std::max(xl, r - g.lofs); xl = std::max(xl, r - g.rofs);
    xh = std::min(xh, g.W - 1 - g.lofs - r); xh = std::min(xh, g.W - g.D - g.rofs - r);
    xl = std::max(xl, g.cx0 - g.lofs); xh = std::min(xh, g.cx1 - g.lofs - 1);
    p->x0 = xl; p->nx = xh - xl + 1;
    p->lx0 = std::max(0, g.cx0 - g.lofs); p->lx1 = xl; p->rx0 = xl + p->nx; p->rx1 = std::min(g.width1, g.cx1 - g.lofs);
    return xh >= xl;
}

SearchPlan plan_search(const BMGeom& g, int n, bool planes_contiguous)
{
    SearchPlan p{};
    // what the single-pass generic kernel cannot hold in LDS (D > 256, large windows at large D) -- or everything, when
    // rtdm_debug_disparity_slice forces it -- is searched by the disparity-sliced kernel over the whole range
    const bool sliced = generic_search_sliced(g);
    if (sliced || !search_ranges(g, &p) || !fast_form(g)) {
        p = SearchPlan{};
        p.tiles = SearchTiles::GENERIC; p.x0 = g.cx0 - g.lofs; p.nx = g.cx1 - g.cx0;
        p.border.form = BorderForm::NONE; p.place = BorderPlace::AFTER;
        p.variant = sliced ? (g.cost16 ? "generic_dslice_u16" : "generic_dslice_u32") : (g.cost16 ? "generic_u16" : "generic_u32");
        return p;
    }
    // (planes that are not one allocation: the ring kernel cannot address them)
    const RingForm rf = planes_contiguous ? ring_form(g) : RingForm{};
    p.tiles = rf.lpp ? SearchTiles::RING : SearchTiles::FAST; p.lanes = rf.lpp;
    p.variant = !rf.lpp ? "fast_qsad" : rf.lpp == 16 ? "fast_ring16_qsad" : rf.lpp == 8 ? "fast_ring8_qsad" : rf.lpp == 4 ? "fast_ring4_qsad" : "fast_ring_qsad";
    // Batches below 16: the border workgroups ride in the tile kernel's grid (one kernel less) where it can carry a form that
    // covers them -- k_search_fast only DISP, k_search_ring what its register budget allows.  The 3.x clamp exists in the
    // stand-alone border kernel only: the fused forms keep their register budget.
    p.border.form = BorderForm::GENERIC;
    if (n < 16 && !g.legacy) p.border = plan_border(g, n, p.lx0, p.lx1, p.rx0, p.rx1, rf.lpp && rf.can_fuse_rows, rf.lpp ? rf.can_fuse_disp : true);
    p.place = BorderPlace::FUSED;
    if (p.border.form == BorderForm::GENERIC) {
        p.border = plan_border(g, n, p.lx0, p.lx1, p.rx0, p.rx1, true, true);
        // Batches of 16 or more: the border columns run as a kernel of their own on a side stream, concurrently with the tile
        // kernel.  Its waves need 37-72 VGPRs and fit NEXT to the four tile waves of a SIMD, whereas inside the tile kernel's
        // grid a border workgroup takes a tile workgroup's slot for the length of its latency-bound walk (search -2 %).
        // (The two generic column ranges follow the tiles at every n: nothing has measured them beside the tiles.)
        p.place = n >= 16 && p.border.form != BorderForm::GENERIC ? BorderPlace::SIDE : BorderPlace::AFTER;
    }
    return p;
}

static void launch_tiles(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n, hipStream_t s, int strips)
{
    if (plan.tiles == SearchTiles::RING) launch_search_ring(plan, Lp, Rp, disp, cost, g, n, s, strips);
    else launch_search_fast(plan, Lp, Rp, disp, cost, g, n, s, strips);
}

static void launch_border(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n, hipStream_t s)
{
    switch (plan.border.form) {
        case BorderForm::ROWS: launch_border_rows(plan.border, Lp, Rp, disp, cost, g, n, s); break;
        case BorderForm::DISP: launch_border_disp(plan.border, Lp, Rp, disp, cost, g, n, s); break;
        case BorderForm::GENERIC:
            launch_search_generic(Lp, Rp, disp, cost, g, n, s, plan.lx0, plan.lx1);
            launch_search_generic(Lp, Rp, disp, cost, g, n, s, plan.rx0, plan.rx1);
            break;
        case BorderForm::NONE: break;
    }
}

int StripTuner::tune_strips(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n, hipStream_t s)
{
    const auto launch = [&](int c) { launch_tiles(plan, Lp, Rp, disp, cost, g, n, s, c); };
    static const bool enabled = env_int("RTDM_AUTOTUNE", 1) != 0 && getenv("RTDM_FAST_WGS") == nullptr;
    if (!enabled || n < 16) return 0;
    const bool ring = plan.tiles == SearchTiles::RING;
    const Key key{g.W, g.H, n, g.cx1 - g.cx0, g.vy1 - g.vy0, (plan.place == BorderPlace::FUSED ? 1 : 0) | plan.lanes};
    for (size_t i = 0; i < tuned.size(); ++i) {
        if (!(tuned[i].key == key)) continue;
        Entry e = tuned[i];
        tuned.erase(tuned.begin() + (long)i);                      // most recently used goes to the back
        if (e.strips == 0) {
            e.strips = -1;                                          // being measured: a failure below leaves the model in charge
            ++shapes;
            const int model = ring ? ring_strips_model(plan, g, n) : fast_strips_model(plan, g, n), cap = (g.vy1 - g.vy0 + 15) / 16;
            int best = model;
            float best_ms = 1e30f;
            hipEvent_t a, b;
            if (hipEventCreate(&a) == hipSuccess) {
                if (hipEventCreate(&b) == hipSuccess) {
                    static const float f[] = {0.6f, 0.7f, 0.8f, 0.9f, 1.0f, 1.1f, 1.2f, 1.35f, 1.5f, 1.75f};
                    int seen[10], nseen = 0;
                    for (float fk : f) {
                        const int c = std::max(1, std::min(cap, (int)(model * fk + 0.5f)));
                        bool dup = false;
                        for (int k = 0; k < nseen; ++k) dup |= seen[k] == c;
                        if (dup) continue;
                        seen[nseen++] = c;
                        launch(c);          // warm
                        launches += 3;
                        float ms = 1e30f;
                        for (int rep = 0; rep < 2; ++rep) {
                            (void)hipEventRecord(a, s);
                            launch(c);
                            (void)hipEventRecord(b, s);
                            float t = 0.f;
                            if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&t, a, b) == hipSuccess) ms = std::min(ms, t);
                        }
                        if (ms < best_ms) { best_ms = ms; best = c; }
                    }
                    e.strips = best;
                    (void)hipEventDestroy(b);
                }
                (void)hipEventDestroy(a);
            }
        }
        tuned.push_back(e);
        return e.strips > 0 ? e.strips : 0;
    }
    if (tuned.size() >= 16) tuned.erase(tuned.begin());             // least recently used
    tuned.push_back(Entry{key, 0});                                 // first sighting: remember, keep the model
    return 0;
}

hipError_t launch_search(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n,
                         hipStream_t stream, const SearchSide& side, StripTuner* tuner)
{
    if (plan.tiles == SearchTiles::GENERIC) {
        launch_search_generic(Lp, Rp, disp, cost, g, n, stream, plan.x0, plan.x0 + plan.nx);
        return hipSuccess;
    }
    hipError_t e = hipSuccess;
    // (measured, if at all, before the side stream forks: nothing else runs beside the timed launches)
    const int strips = tuner->tune_strips(plan, Lp, Rp, disp, cost, g, n, stream);
    const bool fork = plan.place == BorderPlace::SIDE && plan.border.form != BorderForm::NONE;
    if (fork) {
        if ((e = hipEventRecord(side.fork, stream)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(side.stream, side.fork, 0)) != hipSuccess) return e;
        launch_border(plan, Lp, Rp, disp, cost, g, n, side.stream);
        if ((e = hipEventRecord(side.join, side.stream)) != hipSuccess) return e;
    }
    launch_tiles(plan, Lp, Rp, disp, cost, g, n, stream, strips);
    if (fork) e = hipStreamWaitEvent(stream, side.join, 0);
    else if (plan.place == BorderPlace::AFTER) launch_border(plan, Lp, Rp, disp, cost, g, n, stream);
    return e;
}

}  // namespace rtdm
