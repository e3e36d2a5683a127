// k_search_border.hip -- K2, border columns of the fast path.
//
// k_search_fast covers the output columns whose 9x9 (w x w) window needs no border clamping.  The
// first and last w/2 computed columns do clamp (left column = clamp(lofs+j,0,W-1), right column =
// clamp(rofs+j,0,W-D)+e); they lie outside the valid rectangle, so they
// are masked in the end, but validateDisparity's first pass lets them vote, so they must be exact.
// They are only 2*(w/2) columns, which suits the transposed mapping: one WAVE per border column,
// LANES = reversed disparity index e (e = lane + 64*c), walking down a strip of rows.
//   * per row the wave stages the (w-1+D)-byte right span (whole dwords) and the w left samples in LDS (8 rows
//     per batch so that global latency is paid once per batch); lane e's w window bytes R[rb(dx)+e] are gathered
//     from 8-byte spans by v_alignbyte + v_perm with wave-uniform selectors (they only depend on where the clamp
//     bites), so SAD(e) is ceil(w/4) four-byte v_sad_u8;
//   * vertical sliding window through an LDS ring of the last w row-SADs per e;
//   * selection with wave-level operations: min-reduce of the key sad<<8|e (first minimum),
//     __any() for the uniqueness test, readlane for sad[mind +- 1].
#include "rtdm_border.h"
#include "rtdm_search.h"

#include <cstdlib>
#include <type_traits>

namespace rtdm {

// Rows per border workgroup: 128 for batches (the w-1 halo rows are then 6 % of the visits), shorter when the whole launch
// would otherwise consist of a handful of long, latency-bound walks (single frames: the reference's real-time case).
static int border_rows(int nrows, int ncols, int n)
{
    const long want = (long)nrows * ((ncols + 3) / 4) * n / 256;     // rows per workgroup that still leave >= 256 workgroups
    return (int)std::min(128L, std::max(16L, want));
}

static int border_rsp(int D, int w) { return (D + w + 3 + 63 + 64) & ~3; }   // + one chunk of slack for lanes with e >= D

// dynamic LDS of a border workgroup (four waves): it depends on (D, w) alone
size_t border_lds_bytes(int D, int w)
{
    const int nch = (D + 63) / 64;
    const size_t per_wave = ((size_t)RB * border_rsp(D, w) + (size_t)RB * 32 + (size_t)w * (nch * 64) * 2 + (size_t)w * 4 + 15) & ~(size_t)15;
    return per_wave * 4;
}

BorderPlan plan_border(const BMGeom& g, int n, int lx0, int lx1, int rx0, int rx1, bool allow_rows, bool allow_disp)
{
    BorderPlan b{};
    lx1 = max(lx1, lx0); rx1 = max(rx1, rx0);
    const int ncols = (lx1 - lx0) + (rx1 - rx0), nrows = g.vy1 - g.vy0;
    b.form = ncols <= 0 ? BorderForm::NONE : BorderForm::GENERIC;
    if (ncols <= 0) return b;
    if (allow_rows && border_rows_form(g, lx0, lx1, rx0, rx1)) {
        b.form = BorderForm::ROWS;
        b.rows = Border2Geom{lx0, lx1, rx0, rx1, 64 - (g.w - 1)};
        b.gy = (nrows + b.rows.ro - 1) / b.rows.ro;
    } else if (allow_disp && g.w <= 21 && g.D <= 256 && 2L * g.cap * g.w * g.w <= 65535) {   // (32 left bytes per row, four chunks, u16 SADs)
        b.form = BorderForm::DISP;
        b.disp = BorderGeom{lx0, lx1, rx0, rx1, border_rows(nrows, ncols, n), border_rsp(g.D, g.w)};
        b.gy = (nrows + b.disp.rs - 1) / b.disp.rs;
        b.lds = border_lds_bytes(g.D, g.w);
    }
    if (b.form != BorderForm::GENERIC) b.gx = (ncols + 3) / 4;        // both forms: workgroups of four columns
    return b;
}

void launch_border_disp(const BorderPlan& b, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n, hipStream_t stream)
{
    const BorderGeom bg = b.disp;
    const size_t lds = b.lds;
    const int nch = (g.D + 63) / 64;
    dim3 grid(b.gx, b.gy, n), block(256);
    const auto go = [&](auto nc, auto lg) {
        hipLaunchKernelGGL((k_search_border<decltype(nc)::value, decltype(lg)::value>), grid, block, lds, stream, Lp, Rp, disp, (uint16_t*)cost, g, bg);
    };
    const auto pick = [&](auto lg) {
        switch (nch) {
            case 1: go(std::integral_constant<int, 1>{}, lg); break;
            case 2: go(std::integral_constant<int, 2>{}, lg); break;
            case 3: go(std::integral_constant<int, 3>{}, lg); break;
            default: go(std::integral_constant<int, 4>{}, lg); break;
        }
    };
    if (g.legacy) pick(std::true_type{});
    else pick(std::false_type{});
}

}  // namespace rtdm
