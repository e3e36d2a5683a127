// rtdm_sgm_stripes.h -- the row stripes of StereoSGBM's MODE_SGBM_3WAY (rule T1): plain host code, no
// HIP, shared by the launch (k_sgm.hip) and by tests/sgm_stripes_host.cpp.
#pragma once

namespace rtdm {

// Stripe s of a frame of H rows: output rows [o, e), first source row a <= o (rows [a, o) serve the vertical recurrence only);
// o >= e: the stripe is empty.  Always SGM3_STRIPES stripes, whatever the machine.
static constexpr int SGM3_STRIPES = 4;
struct Sgm3Stripe { int a, o, e; };
struct Sgm3Stripes { Sgm3Stripe s[SGM3_STRIPES]; };

// sz = (H + 3) / 4 rows per stripe, ovl = (blockSize / 2 + 1) + (sz + 9) / 10 rows of overlap above it ((sz + 9) / 10 is the
// library's (int)ceil(0.1 * sz) for every sz <= 200000)
inline Sgm3Stripes sgm3_stripes(int H, int blockSize)
{
    const auto lo = [](int u, int v) { return u < v ? u : v; };
    const int sz = (H + SGM3_STRIPES - 1) / SGM3_STRIPES, ovl = (blockSize / 2 + 1) + (sz + 9) / 10;
    Sgm3Stripes t;
    for (int s = 0; s < SGM3_STRIPES; ++s) {
        const int a = lo(s * sz - ovl, H);
        t.s[s].a = a > 0 ? a : 0;
        t.s[s].o = lo(s * sz, H);
        t.s[s].e = lo((s + 1) * sz, H);
    }
    return t;
}

// Rows of warm-up block costs C' (T3) kept per stripe: the first blockSize / 2 rows from a, never more than the frame has
inline int sgm3_warm_rows(int blockSize, int H) { return blockSize / 2 < H ? blockSize / 2 : H; }

}  // namespace rtdm
