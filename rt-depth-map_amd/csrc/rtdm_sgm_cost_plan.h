// rtdm_sgm_cost_plan.h -- which kernels the cost stage of a StereoSGBM call runs (k_sgm_cost.hip; the route table is in DESIGN.md,
// "SGM: cost routes"): plain host code, no HIP, shared by launch_sgm, api_sgm.hip (the limit of a call) and tests/sgm_cost_plan_host.cpp.
#pragma once

namespace rtdm {

// The pixel cost of a call (rtdm_sgm_set_cost): kind SGM_COST_BT (R1; cw, ch unused) or SGM_COST_CENSUS -- Hamming distance of
// cw x ch census descriptors (cw in {3, 5, 7, 9}, ch in {3, 5, 7}; rules N1-N5 of DESIGN.md section 4.20).  The kinds
// are RTDM_SGM_COST_* of include/rtdm.h.
enum { SGM_COST_BT = 0, SGM_COST_CENSUS = 1 };
struct SgmCostKind { int kind, cw, ch; };

// form: four consecutive pixel costs as Cost8, Cost16<1>, Cost16<3> or CostCensus (k_sgm_cost.hip) -- u8 where a pixel cost stays
// below 256, u16 for colour, for gray at ftzero >= 97 and under rtdm_debug_sgm_cost16.  sum: k_sgm_pixbox (no volume), or
// k_sgm_box<R> / k_sgm_box_any over a pixel-cost volume in b.pix (u8) or b.S (u16: S is not written before the first path pass).
enum class SgmCostForm { BT8, BT16_GRAY, BT16_COLOUR, CENSUS };
enum class SgmCostSum { FUSED, BOX, BOX_ANY };
enum class SgmCostVolume { NONE, PIX, S };
struct SgmCostPlan {
    SgmCostForm form;
    SgmCostSum sum;
    int R;                      // blockSize / 2
    bool colour_records;        // the 24-byte records of b.cl / b.cr (k_sgm_bounds<3>), not the 8-byte ones of b.gl / b.gr
    SgmCostVolume volume;
    bool check; int cost_limit; // block sums (and warm-up costs) above cost_limit (> 0 exactly where check) set *b.ovf
    bool warm; int wrows;       // MODE_SGBM_3WAY's k_sgm_warm3 runs, keeping wrows rows per stripe (sgm3_warm_rows)
    int ftz, cw, ch;            // what the bounds (ftz) or the descriptor kernel (cw, ch) is given; the others 0
    const char* variant;        // the row of "SGM: cost routes": <form>_<sum>[_chk][_w3]
};

// R1 generalised (restated for colour in tests/sgm_cn_ref.py): a pixel cost is at most M = cn (2 ftzero + 63), under the census cost (N4)
// cw ch - 1; a block cost at most M blockSize^2; where that + P2 can pass 32767 the block costs are checked against 32767 - P2 (0: no check)
inline long sgm_cost_max(SgmCostKind c, int cn, int ftz) { return c.kind == SGM_COST_CENSUS ? (long)c.cw * c.ch - 1 : (long)cn * (2 * ftz + 63); }
inline int sgm_block_cost_limit(SgmCostKind cost, int cn, int ftz, int blockSize, int P2)
{ return sgm_cost_max(cost, cn, ftz) * blockSize * blockSize + P2 > 32767 ? 32767 - P2 : 0; }

// D: numDisparities (a multiple of 16), H: the frame's rows, cn: 1 or 3 (census: 1, N5), ftz: R1's ftzero, paths: the mode (3:
// MODE_SGBM_3WAY), force16: rtdm_debug_sgm_cost16.  Census is always u8 on the 8-byte records, whatever force16 says.
inline SgmCostPlan plan_sgm_cost(int D, int H, int blockSize, int P2, int cn, int ftz, SgmCostKind cost, int paths, bool force16)
{
#define RTDM_V(f, s) {{f "_" s, f "_" s "_w3"}, {f "_" s "_chk", f "_" s "_chk_w3"}}
#define RTDM_VF(f) {RTDM_V(f, "fused"), RTDM_V(f, "box"), RTDM_V(f, "any")}
    static const char* const names[4][3][2][2] = {RTDM_VF("bt8"), RTDM_VF("bt16g"), RTDM_VF("bt16c"), RTDM_VF("census")};
#undef RTDM_VF
#undef RTDM_V
    const bool census = cost.kind == SGM_COST_CENSUS, u16 = !census && (cn != 1 || 2 * ftz + 63 > 255 || force16), u8 = !u16;
    SgmCostPlan p{};
    p.form = census ? SgmCostForm::CENSUS : (!u16 ? SgmCostForm::BT8 : (cn == 3 ? SgmCostForm::BT16_COLOUR : SgmCostForm::BT16_GRAY));
    p.R = blockSize / 2; p.colour_records = !census && cn == 3;
    p.cost_limit = sgm_block_cost_limit(cost, cn, ftz, blockSize, P2);
    p.check = p.cost_limit > 0;
    // the fused kernel: windows <= 7 and D in {16, 32, 64, 128, 256}; its u8 forms hold no check, its u16 forms their own
    const bool fusable = p.R <= 3 && (D == 16 || D == 32 || D == 64 || D == 128 || D == 256);
    if (fusable && !(u8 && p.check)) { p.sum = SgmCostSum::FUSED; p.volume = SgmCostVolume::NONE; }
    else {                                                   // k_sgm_box<R> serves up to R = 8 on a u8 volume, R = 6 on a u16 one
        p.sum = p.R <= (u8 ? 8 : 6) ? SgmCostSum::BOX : SgmCostSum::BOX_ANY;
        p.volume = u8 ? SgmCostVolume::PIX : SgmCostVolume::S;
    }
    p.warm = paths == 3 && p.R > 0;                          // blockSize 1: there is no C'
    p.wrows = p.warm ? (p.R < H ? p.R : H) : 0;
    if (census) { p.cw = cost.cw; p.ch = cost.ch; } else p.ftz = ftz;
    p.variant = names[(int)p.form][(int)p.sum][p.check][p.warm];
    return p;
}

}  // namespace rtdm
