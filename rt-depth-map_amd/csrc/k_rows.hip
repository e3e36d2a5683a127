// k_rows.hip -- K3 / K4, the launch policy of the two row stages behind the search as one plan each (host only: the kernels are
// in k_lrcheck.hip and k_speckle.hip, whose launch entries issue what the plan tells them).  plan_lrcheck also says what it
// leaves in the speckle filter's workspace (SpkHeads, block_rows), which is what plan_speckle starts from.  Neither makes a
// runtime call; the pointer-dependent conditions come in through rows_aligned (rtdm_kernels.h).  Routes per configuration:
// DESIGN.md, "K3 / K4: routes".
#include "rtdm_kernels.h"

#include <algorithm>

namespace rtdm {

static bool two_ok_for_pk(const BMGeom& g, int md, int spkDiff)
{
    return 2L * g.cap * g.w * g.w < 32768 && md >= 0 && md <= 8192 && spkDiff >= 0 && spkDiff <= 4096 &&
           g.minD >= -1024 && g.minD + g.D <= 1024 && g.W + 2 < 16384;
}

LrPlan plan_lrcheck(const BMGeom& g, int disp12MaxDiff, int spkDiff, int n, bool speckle, bool aligned)
{
    LrPlan p{};
    const int md = disp12MaxDiff * 16;
    const int nrows = g.vy1 - g.vy0;
    p.n = (unsigned)n; p.maxDiff16 = md; p.spkDiff = spkDiff;
    p.heads = speckle ? SpkHeads::PIXEL : SpkHeads::NONE; p.block_rows = 1;
    // 16-bit costs: 32-bit keys (cost << 16 | x; frames wider than 4096 are refused when the handle is created, so x fits)
    const size_t kb = g.cost16 ? 4 : 8;
    const int Wp = (g.W + 7) & ~7;
    // the forms that move 8 columns per 128-bit access: aligned rows, whole chunks in the workspace planes, 16-bit costs
    const bool vec = aligned && g.cost16 && (g.Ws & 7) == 0 && g.W <= 4096;
    if (!vec) {
        // (no ABI entry reaches SCALAR_U16: bm_run_chunk hands over a caller's plane only if it is aligned with W % 8 == 0 and
        // the handle's own plane otherwise -- DESIGN.md, "K3 / K4: routes")
        p.form = g.cost16 ? LrForm::SCALAR_U16 : LrForm::SCALAR_I32;
        p.threads = 256; p.gy = (unsigned)nrows;
        p.lds = (size_t)g.W * (kb + 2 + (speckle ? 2 : 0));
        return p;
    }
    if (speckle) p.heads = SpkHeads::CHUNK;
    const int chunks = Wp >> 3;
    const auto per_half = [&](int nb) { return (size_t)Wp * 4 + 16 + (size_t)nb * Wp * 2; };
    // row pairs a workgroup walks and merges (1: none -- every pair is left to k_spk_merge_strip, round 3's first form)
    // Two row pairs per workgroup with the vertical contacts inside the block found right here (k_lrcheck_vec<.., NIT = 2> +
    // k_spk_merge_rec): a frame's contacts are chains of dependent L2 round trips, and with half of them settled from the head
    // records the merge of one 720p frame takes 12 us instead of 29 (the whole frame 82 -> 66 us of kernels).  Measured against
    // the packed one-pair form (k_lrcheck_pk + k_spk_merge_strip<4>) over batch sizes (profiles/r03_lr_pairs_ab.txt): frames
    // up to 1024 wide -- faster or level at every batch size (640x480: -32 % at 12 pairs, -5 % at 128, level at 512); 1280
    // wide -- faster up to ~16 pairs per call (-9 % for one frame, -23 % at 4), 2-5 % slower beyond, where k_lrcheck_pk
    // streams and the merge is HBM bound.  RTDM_LR_PAIRS=1 / 2 (test hook) fixes the choice.
    static const int pairs_raw = env_int("RTDM_LR_PAIRS", 0);
    const int pairs = (pairs_raw == 1 || pairs_raw == 2) ? pairs_raw : ((g.W <= 1024 || (long)n * nrows <= 11520) ? 2 : 1);
    // two rows per workgroup (one per half-wave) where that fits 512 threads: it never takes more lanes than the whole-wave form
    const int waves1 = (chunks + 63) / 64, waves2 = (chunks + 31) / 32;
    const bool two = waves2 <= 8 && nrows >= 2;
    // packed form (k_lrcheck_pk): costs below 32768, every quantity of the consistency / closeness tests inside int16,
    // LDS byte addresses inside 16 bits.  RTDM_LR_PACKED=0 (test hook): k_lrcheck_vec, the form wherever these fail.
    static const int pk_env = env_int("RTDM_LR_PACKED", 1);
    const bool pk_ok = pk_env && two_ok_for_pk(g, md, spkDiff) && 2 * per_half(1) + 1024 < 65536;
    const bool contacts_here = two && speckle && nrows >= 4 && pairs > 1;   // k_lrcheck_vec<.., NIT = 2>
    if (!two) {
        p.form = LrForm::VEC_WAVE;
        p.threads = (unsigned)(waves1 * 64); p.gy = (unsigned)nrows; p.lds = per_half(1);
    } else if (contacts_here) {
        p.form = LrForm::VEC_HALF2;
        p.threads = (unsigned)(waves2 * 64); p.gy = (unsigned)((nrows + 3) / 4); p.lds = 2 * per_half(2);
        p.block_rows = 4;
    } else {
        p.form = pk_ok ? LrForm::PACKED : LrForm::VEC_HALF;
        p.threads = (unsigned)(waves2 * 64); p.gy = (unsigned)((nrows + 1) / 2); p.lds = 2 * per_half(1);
    }
    return p;
}

SpkPlan plan_speckle(int W, int Ws, int H, int n, SpkHeads heads, int block_rows, int y_lo, int y_hi, bool aligned)
{
    SpkPlan p{};
    p.W = W; p.Ws = Ws; p.H = H; p.n = n;
    if (heads == SpkHeads::NONE) {
        y_lo = 0; y_hi = H; block_rows = 1;
        heads = SpkHeads::PIXEL;
        p.init_lds = (size_t)W * 6;
    }
    p.heads = heads; p.ystep = 1;
    p.rows_gx = (n * H + 15) / 16;
    const bool chunk = heads == SpkHeads::CHUNK;
    // row pairs still to merge: (y, y+1), y = first + k*step.  The init pass may already have merged the pairs
    // inside blocks of block_rows rows (k_lrcheck_vec<.., NIT = 2>, chunk records); then only the pairs across blocks remain.
    const int step = block_rows > 1 ? block_rows : 1;
    const int first = y_lo + step - 1;
    const int last = std::min(y_hi, H) - 2;          // last y with y+1 initialised
    const int npairs = last >= first ? (last - first) / step + 1 : 0;
    const int nxb = (W + 7) / 8;
    p.first = first; p.npairs = npairs;
    // RTDM_MERGE_REC_FUSED=0 (test hook): k_spk_merge_rec as a launch of its own, as where no pair is left across blocks
    static const int fuse_rec = env_int("RTDM_MERGE_REC_FUSED", 1);
    if (chunk && step > 1) {                          // the contacts inside blocks of `step` rows are in the head records (k_lrcheck_vec<.., NIT > 1>)
        const int nr = std::min(y_hi, H) - y_lo, inside = (nr / step) * (step - 1) + std::max(nr % step - 1, 0);
        if (inside > 0) {
            const MergeRecArgs ra{(inside * nxb + 255) / 256, y_lo, nr, step, nxb};
            if (fuse_rec && npairs > 0) p.rec_fused = ra;   // rides in k_spk_merge_strip<1, true, true>
            else p.rec_own = ra;
        }
    }
    if (npairs == 0) return p;
    // strips of RS row pairs, the first at `first`; strips of one pair lie ystep rows apart
    const auto strip_blocks = [&](int rs) { return (nxb * ((npairs + rs - 1) / rs) + 255) / 256; };
    if (chunk && step > 1) {                          // k_lrcheck_vec<.., NIT > 1> has found the contacts inside blocks of `step` rows
        p.merge = p.rec_fused.blocks ? SpkMerge::STRIP1_CHUNK_REC : SpkMerge::STRIP1_CHUNK;
        p.merge_gx = strip_blocks(1) + p.rec_fused.blocks; p.ystep = step;
    } else if (chunk) {                               // written by the 128-bit forms of K3, whose conditions imply those of the strips
        // Strips of four row pairs read every row 1.25 times instead of twice -- what a batch wants (the kernel streams the
        // plane) -- but a single frame is 111 workgroups whose threads each work through up to four queued unions, chains of
        // dependent L2 round trips: 32 us, more than the frame's search.  Small launches take shorter strips: more workgroups,
        // one union per thread.
        int rsc = 4;
        while (rsc > 1 && (long)strip_blocks(rsc) * n < 1024) rsc >>= 1;
        p.merge = rsc == 4 ? SpkMerge::STRIP4_CHUNK : rsc == 2 ? SpkMerge::STRIP2_CHUNK : SpkMerge::STRIP1_CHUNK;
        p.merge_gx = strip_blocks(rsc);
    } else if (aligned && (Ws & 7) == 0) {            // (step == 1: without chunk records nothing was merged in blocks)
        p.merge = SpkMerge::STRIP4_PIXEL;
        p.merge_gx = strip_blocks(4);
    } else {                                          // rows that are not 16-byte aligned; a ragged last chunk is clamped
        p.merge = SpkMerge::ROWS;
        p.merge_gx = (nxb * npairs + 255) / 256;
    }
    return p;
}

}  // namespace rtdm
