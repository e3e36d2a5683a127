// rtdm_search.h -- what the files of K2 (k_search*.hip) tell k_search.hip, which decides: which configurations a kernel
// family is instantiated for, its strip model, and its launch for a finished plan.  Private to those files.
#pragma once
#include "rtdm_kernels.h"

namespace rtdm {

// k_search_generic.hip: every configuration.  Runs the single-pass form where its LDS fits (D <= 256, not every w at large D)
// and no slice width is forced, else the sliced form: the reversed disparity range walked in slices whose results are folded
// in index order per pixel, the same outputs bit for bit.  [gx0, gx1) restricts the output-column range (gx1 < 0: all of
// [0, width1)).  Returns the variant name.
const char* launch_search_generic(Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g,
                                  int n, hipStream_t stream, int gx0 = 0, int gx1 = -1);
bool generic_search_sliced(const BMGeom& g);   // the sliced form is needed or forced (no packed kernel runs then)

// k_search_fast.hip: packed-u8 quad-SAD kernel.  fast_form: instantiated for (D, w) and the sums fit.  Border columns of form
// DISP placed FUSED ride as extra workgroups of its grid.  strips > 0: row strips per frame (a measured choice), 0: the model.
bool fast_form(const BMGeom& g);
int fast_strips_model(const SearchPlan& plan, const BMGeom& g, int n);
void launch_search_fast(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n,
                        hipStream_t stream, int strips);

// k_search_ring.hip: prefix sums in a register ring instead of a leaving-row recomputation.  ring_form: lpp = lanes per pixel of
// the form (D, w) runs (0: none, or switched off by ring_set_mode), waves per SIMD it is compiled for, which border forms its
// grid can carry in front of its own workgroups, output columns per workgroup.
struct RingForm { int lpp, waves; bool can_fuse_rows, can_fuse_disp; int tile; };
RingForm ring_form(const BMGeom& g);
int ring_strips_model(const SearchPlan& plan, const BMGeom& g, int n);
void launch_search_ring(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n,
                        hipStream_t stream, int strips);

// k_search_border.hip / k_search_border2.hip: the border columns [lx0, lx1) and [rx0, rx1) of n frames.  plan_border: the first of
// the allowed forms that covers them -- ROWS (one wave = one column x 64 rows, 4-5x fewer instructions per pixel), then DISP
// (one wave per column, lanes = disparities) -- with its geometry; GENERIC: none does; NONE: there are no columns.
BorderPlan plan_border(const BMGeom& g, int n, int lx0, int lx1, int rx0, int rx1, bool allow_rows, bool allow_disp);
bool border_rows_form(const BMGeom& g, int lx0, int lx1, int rx0, int rx1);   // ROWS covers these columns (k_search_border2.hip)
size_t border_lds_bytes(int D, int w);   // the dynamic LDS of form DISP, for any frame of (D, w)
void launch_border_rows(const BorderPlan& b, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n, hipStream_t stream);
void launch_border_disp(const BorderPlan& b, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n, hipStream_t stream);

}  // namespace rtdm
