// k_search_ring.hip -- K2, ring variant: the SAD window search with NO leaving-row recomputation.
//
// k_search_fast keeps the w-row window sums of a pixel in registers and pays for every row twice: once when it enters
// the window and once, w rows later, when it is recomputed from an LDS ring and subtracted.  Here a pixel's registers
// hold the running PREFIX sums over the rows of its strip instead,
//       P(t)[d] = sum_{rows 0..t} H(row)[d]            H = the horizontal w-byte SAD of one row
//       S(t)[d] = P(t)[d] - P(t-w)[d]                   the w x w window sum
// in a ring of w+1 register slots: v_qsad_pk_u16_u8 takes P(t-1) as its accumulator operand and writes P(t) into the
// slot of the dead P(t-w-1), so a row costs its quad-SADs once plus one subtraction per two disparities.  Ring slots
// are compile-time registers: one trip of the row loop is a whole number of rounds of the ring, unrolled, every row step a
// copy with its own register operands (a switch over the slot inside a rolled loop made the register allocator copy and spill
// the ring at every merge).
//
// A pixel's ring is (w+1) * D/2 registers (320 at D = 64, w = 9), so the D disparities of a pixel are split over LPP lanes
// of a wave -- p + h * 64/LPP, h = 0..LPP-1, each with a slice of D/LPP disparities -- and rows are processed in GROUPS of LPP:
// the lane with h = k owns row k of the group and produces its output pixel.
//   LPP = 2 (D <= 48; D = 64 as an A/B form): ring 160 registers at D = 64, w = 9 => two waves per SIMD
//   LPP = 4 (D = 64, 96): ring 80 registers at (64, 9) => three waves (four for w <= 7; two for D = 96)
//            (64, 9) -- the headline -- in the PAIRED layout: a lane holds two adjacent columns and an eighth of their
//            disparities each, the same 80 ring registers, and pays four window pieces per row for the pair instead of six
//            (RingCfg::PAIR, ring_step_pair)
//   LPP = 8 (D = 128): ring 96 registers at w = 11; two waves (the selection records, 17 KB per wave, allow no more)
// Selection wants all D values of a pixel in one place.  Two forms (rtdm_select.h):
//   * transposing (LPP = 2, D <= 32): one v_permlane32_swap per register hands the lower lane both halves of row t and the
//     upper lane both halves of row t+1; each lane runs the single-lane selection select_disparity_lds;
//   * GroupSelectRec (everything else): nothing is transposed.  As soon as a row's step is over (the SADs are dead after
//     that) each lane writes its slice of the row and the minima of the slice's groups of eight into the owner's LDS record;
//     nothing crosses between the lanes, and the owner selects from its record alone.
//
// Mapping: workgroup = 4 * 64/LPP output columns x `rs` rows of one frame; wave = byte phase phi, lane (p, h) = column
// x_tile + phi + 4 p (PAIR: wave = half of the tile and one of two 2-byte phases, lane (p, h) = the columns x0, x0 + 1 with
// x0 = x_tile + 32 (phi >> 1) + 2 (phi & 1) + 4 p).  The four waves never synchronise: each stages ITS byte-shifted copy
// of the entering rows (64 or 128 dwords, padded) into its own LDS slice, two rows ahead of their use, and the LDS queue of
// a wave is in order.  The texture sum is a prefix ring too (16 bits per pixel and slot, in LDS; PAIR: RingTexture).  Only columns whose window needs no border
// clamping are handled here; the border columns ride in front of the tiles or go to a launch of their own (k_search.hip).
// Semantics: SURVEY.md Appendix A.3b; oracle: oracle/bm_oracle.c.
//
// Measured instruction costs on gfx950 that shaped this (tools/ubench_valu.hip, SIMD cycles per wave-instruction):
// v_qsad/v_mqsad_pk_u16_u8 16.4; v_add/sub/and/xor/mov 2.6; everything else used here (packed u16 ops, v_perm,
// v_cndmask, v_min3, v_cmp, shifts, v_sad_u8) 4.2-4.7; v_permlane32_swap 8.1.
#include "rtdm_select.h"
#include "rtdm_border.h"
#include "rtdm_border2.h"
#include "rtdm_search.h"

#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace rtdm {

struct RingGeom {
    int x0, nx;          // output-column range [x0, x0+nx) handled by this kernel
    int rs;              // output rows per workgroup
    uint32_t lastmask;   // byte mask of the last (partial) window piece
    int tiles, strips;   // column tiles x row strips per frame
    unsigned nitems;     // workgroups over the whole batch
    unsigned chunk;      // ceil(nitems / 8): consecutive items one XCD works through (0: no remapping)
    uint32_t rdelta;     // the right prefiltered plane lies this many bytes behind the left one (direct loads)
    int rebase;          // > 0: every `rebase` trips of the row loop the ring is rebased (P -= the oldest live prefix sum), so a
                         // strip may be as long as the frame; 0: strips are short enough for 16-bit prefix sums (ring_rows_cap)
    unsigned nborder;    // border-column workgroups in FRONT of the tile workgroups (single frames and small batches, where a
    int bgx, bgy;        // second launch or a side stream costs more than it hides); 0: none
    int b2;              // 1: they run border2_body (rtdm_border2.h: rows in the lanes), 0: border_body (rtdm_border.h)
};

// LPP = lanes per pixel: the D disparities of a pixel are split over LPP lanes of a wave (p + h * 64/LPP, h = 0..LPP-1), and
// rows are processed in groups of LPP, one owner lane per row for the selection.
// RPG = rows per group: the lanes with h < RPG own the group's rows; RPG < LPP (GroupSelectRec's lanes exchange nothing)
// halves / quarters the number of selection records a wave needs -- what lets D = 192 and D = 256 (records of 432 / 592
// bytes) keep two workgroups per CU -- at the price of a selection that runs with RPG / LPP of its lanes.  Four rows per group
// from D = 96 up: 6-8 % faster at D = 128 than eight rows with a lane-exchange selection, and D = 96 with two rows and D = 256
// with eight are slower too (profiles/r03_ring_rows_per_group_ab.txt).
__host__ __device__ constexpr int ring_rpg(int D, int LPP) { return D >= 96 ? 4 : LPP; }

template <int D, int WS, int LPP = 2>
struct RingCfg {
    static constexpr int RPG = ring_rpg(D, LPP);
    // selection without transposing the lanes' slices (GroupSelectRec): always for four and more lanes per pixel; with two
    // lanes where it measured faster than transposing (profiles/r02_ring_split_select_ab.txt; round 3 re-measured: D = 32,
    // w = 5 joins (+10 %); the other D = 16 / 32 forms stay within +-1-5 % of transposing, profiles/r03_ring_split_select_ab.txt)
    static constexpr bool SPLIT = LPP != 2 || D >= 48 || (D == 32 && (WS == 9 || WS == 5));
    // D = 64: records in 8-byte pieces at a 34-dword stride (rtdm_select.h: four workgroups per CU at (64, 9, 4))
    static constexpr bool B64 = SPLIT && D == 64;
    using Rec = SelRecord<D, B64>;
    static constexpr int NP = (WS + 3) / 4;        // 4-byte pieces of a window row
    static constexpr int W1 = WS + 1;              // ring slots
    static constexpr int PPW = 64 / LPP;           // pixels (columns) per wave
    // PAIR: a lane holds TWO adjacent columns x0, x0 + 1 and, for both, half as many disparities.  With w = 4 (NP - 1) + 1 the
    // two windows share their NP - 1 middle dwords: the pair costs NP + 1 window pieces instead of 2 NP -- two shared ones, and
    // per column one masked piece with a single live byte (the header of ring_step_pair has the layout).  The headline form.
    static constexpr bool PAIR = D == 64 && WS == 9 && LPP == 4;
    static constexpr int LPG = PAIR ? 2 * LPP : LPP;   // lanes per group: they split the D disparities of a column (of a pair's two)
    static constexpr int GPW = 64 / LPG;           // lane groups per wave (= PPW columns, or PPW / 2 pairs)
    static constexpr int DL = D / LPG;             // disparities per lane (and column)
    static constexpr int NGL = DL / 4;             // quad-SAD groups per lane (and column)
    static constexpr int NRL = DL / 2;             // packed u16x2 registers per lane, slot (and column)
    static constexpr int NL = PAIR ? NP + 1 : NP;  // left dwords a lane reads of a row
    static constexpr int NW = NGL + NL - 1;        // distinct 8-byte right windows per lane and row
    static constexpr int LWD = GPW + NP;           // dwords of the wave's copy of the left row
    static constexpr int RWD = GPW + D / 4 + NP;   //                                 right row
    static constexpr int ITEMS = (LWD + RWD + 63) / 64;
    static constexpr int SLOT = ITEMS * 64;        // padded: every lane stores every item, no exec masking
    // rows per trip of the unrolled row loop: whole rounds of the ring AND whole groups
    static constexpr int TRIP = (W1 % RPG == 0) ? W1 : (2 * W1 % RPG == 0) ? 2 * W1 : 4 * W1;
    static_assert(W1 % 2 == 0 && TRIP % RPG == 0 && TRIP % W1 == 0, "block sizes are odd");
    // staged rows in flight per wave: three (row t is read while t+1 waits and t+2 arrives), or four where that makes the
    // slot of every unrolled step a constant and every LDS address base + immediate, 3-4 VALU per row less (one item per row
    // only: ds_read2's 8-bit dword offsets must reach the slots)
    static constexpr bool STATIC_SLOTS = ITEMS == 1 && TRIP % 4 == 0;
    static constexpr int NSLOT = STATIC_SLOTS ? 4 : 3;
    // dwords per wave: staged rows + the texture prefix ring [W1][PPW] + the window texture sums of a group's rows [RPG][PPW] (u16)
    // (PAIR: the prefix ring is [PPW][TRIP], one entry per column and unrolled row step, + the row terms of a group [PPW][RPG])
    static constexpr int TEXD = (PAIR ? (TRIP + RPG) : (W1 + RPG)) * PPW / 2;
    static constexpr int STG = (NSLOT * SLOT + TEXD + 3) & ~3;
    // PAIR: the records of a pair's LPG owners lie one behind the other at the bare record size (D/2 + D/16 = 36 dwords: 4 banks
    // on per owner) and pair p starts 2 (p & 1) + 8 (p >> 1) dwords behind that.  An 8-byte LDS access serves 16 lanes per cycle
    // from 32 banks; the 16 lanes here are the 8 pairs x 2 lanes whose slices lie 4 dwords apart in the target record, so the
    // pairs' records have to start at the banks {0, 2, 8, 10, 16, 18, 24, 26} + 4 x owner -- which the owners' own reads of
    // 16 neighbouring records cover without a conflict as well.  No record stride does that (with GPW records of stride 38
    // next to each other the bank-conflict cycles of the kernel rose sevenfold and ate the whole gain of the layout).
    static constexpr int PREC = D / 2 + D / 16;
    static constexpr int PREC_PAIR = LPG * PREC;   // from pair to pair
    __host__ __device__ static constexpr int pair_rec(int p, int o) { return p * PREC_PAIR + o * PREC + 2 * (p & 1) + 8 * (p >> 1); }
    static constexpr int REC_DWORDS = PAIR ? pair_rec(GPW - 1, LPG - 1) + PREC + 2 : PPW * RPG * Rec::DWORDS;
    static constexpr int WAVE_LDS = STG + REC_DWORDS;   // + the selection's records, one per owner lane (rtdm_select.h)
    // waves per SIMD the register budget is set for: the ring takes W1 * NRL registers, the rest of the kernel about 50
    static constexpr int RING_REGS = W1 * NRL * (PAIR ? 2 : 1);
    // two-lane forms: most ring registers a three-wave form may hold.  (32, 13) sits AT 112 and spills ten dwords at 168 VGPRs
    // -- and is still 9 % faster than as a two-wave form without (111): profiles/r03_ring_spills.txt
    static constexpr int W3_LIMIT = 112;
    // (tighter bounds spill; eight lanes per pixel = D = 128: the selection records, 17 KB per wave, allow two workgroups per CU)
    // (PAIR: three.  The 128 registers of four waves have no room for the shared sums and the fourth left piece, the records
    //  let three workgroups share a CU anyway, and four measured no faster when they fitted.  ring_strips_model sizes its
    //  strips by this value: it now counts the 768 workgroups the chip really holds, not 1024)
    static constexpr int WAVES = PAIR ? 3 : LPP >= 8 ? 2 : LPP == 4 ? (RING_REGS <= 80 ? 4 : (RING_REGS <= 96 && NRL <= 8) ? 3 : 2) : (RING_REGS <= 72 && NRL <= 8) ? 4 : RING_REGS <= W3_LIMIT ? 3 : 2;
    static constexpr int TILE = 4 * PPW;           // four byte phases
    // border-column workgroups may ride in this kernel's grid (small launches): border2_body in every form (it needs no LDS
    // and 52-120 VGPRs for D <= 64); border_body (configurations border2 does not cover) not in the four-wave forms, whose
    // 128 registers its code would overflow (nor in the paired form that took the place of one)
    static constexpr bool FUSE_BORDER = WAVES < 4 && !PAIR;
    static constexpr bool FUSE_BORDER2 = D <= 192;  // (border2_body<256, 4> needs 261 VGPRs: it stays a launch of its own)
    // LDS read addresses of a row: three registers that advance (3 VALU per row) or recomputed from the slot index (6 VALU,
    // no registers held) -- the latter for the two-lane configurations that sit at their three-wave register limit
    static constexpr bool ROW_PTRS = !(LPP == 2 && RING_REGS > 88 && WAVES == 3);
    // PREFETCH: a step requests the NEXT row's pieces and windows from LDS before its own quad-SADs, into a second RowRegs
    // set (NW * 2 + NL = 14 registers in the paired form, which has them to spare below its three-wave limit of 168), so
    // the SADs of a step run on registers asked for a whole step earlier instead of a few instructions earlier, behind the
    // previous step's record stores in the wave's in-order LDS queue.  Row t + 1 is resident all through step t (committed
    // at the end of step t - 1), and the commit at the end of step t goes to another slot, that of row t + 2.
    static constexpr bool PREFETCH = PAIR;
    // LOAD_SETS: register sets of global loads in flight per wave.  Two: step t loads row t + 3 into the set that row t + 1
    // left.  With the LDS read a step ahead a wave parks less on LDS, and what it parks on next is the load behind the
    // commit (vmcnt): four sets -- row t + 5 is requested in step t, one more VGPR per set (ITEMS = 1) -- measured fastest of
    // 2, 3, 4 and 6 (profiles/ring_prefetch_ab.txt).  The sets rotate by name (a queue, oldest first); the commit schedule,
    // two rows ahead into four static slots, is what it was.
    static constexpr int LOAD_SETS = PREFETCH ? 4 : 2;
    static_assert(!PREFETCH || (STATIC_SLOTS && NSLOT == 4), "the slot of row t + 1 is a constant of the step, distinct from that of row t + 2");
};

// The form with the border-column workgroups in its grid (BORDER: single frames, batches < 16 -- a handful of scheduling rounds,
// where the occupancy bound buys nothing) is compiled for one wave per SIMD less: border2_body on top of a form that sits at
// its register limit spilled two dwords ((64, 9, 4) at 128 VGPRs, (192, 15, 8) at 256).
template <int D, int WS, int LPP, bool BORDER>
struct RingBounds {
    using C = RingCfg<D, WS, LPP>;
    // (the paired form sits well below its three-wave limit: it keeps its bound)
    static constexpr int WAVES = BORDER && C::WAVES > 1 && !C::PAIR ? C::WAVES - 1 : C::WAVES;
};

template <int D, int WS, int LPP = 2>
struct RingState {                                                                       // only ever indexed with constants: registers
    uint64_t P[RingCfg<D, WS, LPP>::W1][RingCfg<D, WS, LPP>::NGL];
    uint64_t P2[RingCfg<D, WS, LPP>::PAIR ? RingCfg<D, WS, LPP>::W1 : 1][RingCfg<D, WS, LPP>::NGL];   // PAIR: the ring of column x0 + 1
};

// The registers a lane needs of one staged row: its NW right windows (8 bytes each) and its NP left pieces.
template <int D, int WS, int LPP = 2>
struct RowRegs { uint64_t win[RingCfg<D, WS, LPP>::NW]; uint32_t l[RingCfg<D, WS, LPP>::NL]; };

typedef __attribute__((address_space(3))) const uint32_t* lds_cptr;    // an LDS address held as what it is: 32 bits
__device__ __forceinline__ uint32_t lds_addr(const uint32_t* q) { return (uint32_t)(uintptr_t)(lds_cptr)q; }
__device__ __forceinline__ lds_cptr lds_at(uint32_t a) { return (lds_cptr)(uintptr_t)a; }

// lp / rp: this lane's left pieces / right windows of the staged row in LDS; rpo = rp + 1, as a pointer of its own.
template <int D, int WS, int LPP, typename PTR>
__device__ __forceinline__ void ring_load_row(PTR lp, PTR rp, PTR rpo, RowRegs<D, WS, LPP>& rw)
{
    using C = RingCfg<D, WS, LPP>;
    // 64-bit operands want even-aligned VGPR pairs: windows at odd dword offsets are loaded through a second pointer
    // (laundered by the caller), so that they get their own ds_read2_b32 instead of v_mov rebuilds.
    // Issue order = order of first use (the LDS returns data in order): the left pieces, then the windows by index.
#pragma unroll
    for (int k = 0; k < C::NL; ++k) rw.l[k] = lp[k];
#pragma unroll
    for (int j = 0; j < C::NW; ++j) {
        const PTR wp = (j & 1) ? rpo + (j - 1) : rp + j;
        rw.win[j] = (uint64_t)wp[0] | ((uint64_t)wp[1] << 32);
    }
}

// One row step on ring slot K: P[K] = P[K-1] + H(row), S = P[K] - P[K+1] (the slot that holds P(t-w));
// tnew += the row's texture term sum |L - cap|.
template <int D, int WS, int LPP, int K, int NRLc>
__device__ __forceinline__ void ring_step(RingState<D, WS, LPP>& st, const RowRegs<D, WS, LPP>& rw, uint32_t lastmask, uint32_t capb,
                                          uint32_t& tnew, uint32_t (&S)[NRLc])
{
    using C = RingCfg<D, WS, LPP>;
    auto& P = st.P;
    constexpr int NP = C::NP, NGL = C::NGL, W1 = C::W1;
    constexpr int KP = (K + W1 - 1) % W1, KO = (K + 1) % W1;
    uint32_t l[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) l[k] = rw.l[k];
    l[NP - 1] &= lastmask;
#pragma unroll
    for (int k = 0; k < NP - 1; ++k) tnew = __builtin_amdgcn_sad_u8(l[k], capb, tnew);
    tnew = __builtin_amdgcn_msad_u8(capb, l[NP - 1], tnew);   // zero bytes of the reference are skipped
#pragma unroll
    for (int j = 0; j < C::NW; ++j) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int gi = j - k;
            if (gi >= 0 && gi < NGL) {
                const uint64_t acc = k == 0 ? P[KP][gi] : P[K][gi];
                if (k == NP - 1) P[K][gi] = __builtin_amdgcn_mqsad_pk_u16_u8(rw.win[j], l[k], acc);
                else             P[K][gi] = __builtin_amdgcn_qsad_pk_u16_u8(rw.win[j], l[k], acc);
            }
        }
    }
#pragma unroll
    for (int gi = 0; gi < NGL; ++gi) {
        // plain 32-bit subtractions of the packed pairs (v_sub_u32 issues at 1.6x the rate of v_pk_sub_u16): a strip is
        // short enough that no prefix sum leaves 16 bits (ring_rows_cap), so each half of P(t) is >= that half of P(t-w)
        // and no borrow crosses from the low half into the high one
        S[2 * gi] = (uint32_t)P[K][gi] - (uint32_t)P[KO][gi];
        S[2 * gi + 1] = (uint32_t)(P[K][gi] >> 32) - (uint32_t)(P[KO][gi] >> 32);
    }
}

// two packed u16 pairs each; plain 32-bit additions (v_add_u32 issues at 1.6x the rate of v_pk_add_u16): the caller knows that
// no 16-bit half overflows
__device__ __forceinline__ uint64_t ring_add_halves(uint64_t a, uint64_t b)
{
    // (as a two-dword vector: written with shifts and an OR the upper half becomes a 64-bit addition with a zeroed low dword)
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint64_t, __builtin_bit_cast(u2, a) + __builtin_bit_cast(u2, b));
}

// The row step of the PAIRED layout (RingCfg::PAIR, w = 4 (NP - 1) + 1): the lane holds the columns x0 and x0 + 1.  Its left
// dwords are l[0] = image bytes [x0-r-3, x0-r], l[1] .. l[NP-1] the 4 (NP - 1) bytes behind, l[NP] = [x0+r+1, x0+r+4]:
//   window of x0     = byte 3 of l[0] | l[1] .. l[NP-1]
//   window of x0 + 1 =                  l[1] .. l[NP-1] | byte 0 of l[NP]
// and piece k of quad-group gi meets the right window win[gi + k] for both columns (one staged copy, one alignment).  Per
// quad-group: the shared pieces are summed once (sh, from 0), each column adds its one-byte piece (v_mqsad skips the zeroed
// reference bytes) on top of its own prefix sum, and sh joins both with plain additions -- NP + 1 quad-SADs for the pair
// instead of 2 NP.  No carry between the packed halves: e + sh IS the column's new prefix sum, which stays below 2^16
// (ring_rows_cap, rebase).  The texture term is not formed here: eight lanes would repeat it for every row, and each owner needs
// one per group -- RingTexture below.
template <int D, int WS, int LPP, int K, int NRLc>
__device__ __forceinline__ void ring_step_pair(RingState<D, WS, LPP>& st, const RowRegs<D, WS, LPP>& rw, uint32_t (&S)[NRLc], uint32_t (&S2)[NRLc])
{
    using C = RingCfg<D, WS, LPP>;
    static_assert(C::PAIR && WS % 4 == 1, "the two windows share whole dwords only for w = 1 (mod 4)");
    constexpr int NP = C::NP, NGL = C::NGL, W1 = C::W1;
    constexpr int KP = (K + W1 - 1) % W1, KO = (K + 1) % W1;
    const uint32_t lf = rw.l[0] & 0xff000000u, ll = rw.l[NP] & 0x000000ffu;
    uint64_t sh[NGL], e1[NGL], e2[NGL];
    // issue order = window index (the LDS returns the windows in order)
#pragma unroll
    for (int j = 0; j < C::NW; ++j) {
#pragma unroll
        for (int k = 0; k <= NP; ++k) {
            const int gi = j - k;
            if (gi >= 0 && gi < NGL) {
                if (k == 0)       e1[gi] = __builtin_amdgcn_mqsad_pk_u16_u8(rw.win[j], lf, st.P[KP][gi]);
                else if (k == NP) e2[gi] = __builtin_amdgcn_mqsad_pk_u16_u8(rw.win[j], ll, st.P2[KP][gi]);
                else              sh[gi] = __builtin_amdgcn_qsad_pk_u16_u8(rw.win[j], rw.l[k], k == 1 ? (uint64_t)0 : sh[gi]);
            }
        }
    }
#pragma unroll
    for (int gi = 0; gi < NGL; ++gi) {
        st.P[K][gi] = ring_add_halves(e1[gi], sh[gi]);
        st.P2[K][gi] = ring_add_halves(e2[gi], sh[gi]);
        // (no borrow between the halves: as in ring_step)
        S[2 * gi] = (uint32_t)st.P[K][gi] - (uint32_t)st.P[KO][gi];
        S[2 * gi + 1] = (uint32_t)(st.P[K][gi] >> 32) - (uint32_t)(st.P[KO][gi] >> 32);
        S2[2 * gi] = (uint32_t)st.P2[K][gi] - (uint32_t)st.P2[KO][gi];
        S2[2 * gi + 1] = (uint32_t)(st.P2[K][gi] >> 32) - (uint32_t)(st.P2[KO][gi] >> 32);
    }
}

// Orders everything that produces v[] before whatever follows (no instruction is emitted).
template <int N>
__device__ __forceinline__ void pin(uint32_t (&v)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(v[i]));
}

template <typename T>
__device__ __forceinline__ __attribute__((address_space(3))) T* lds_as(uint32_t a) { return (__attribute__((address_space(3))) T*)(uintptr_t)a; }

// The texture window sums of the PAIRED layout: one row term per OWNER and row group instead of one per lane and row.
// Slots are static and a trip is a multiple of four rows, so row R of every group sits in staging slot R; step U + R commits
// row U + R + 2 at its end.  Between the commits of steps U + 1 and U + 2 all four rows of the group are therefore resident,
// and the owner (p, h) of column x0 + j, row k (j = h & 1, k = h >> 1) reads ITS row's left bytes at lane-constant addresses:
// the two shared dwords and one edge byte (ds_read_u8 delivers it zero-extended; v_msad skips the three zero bytes).
//   term():   inside step U + 2, before its commit: the row term, as u16, to terms[column][k]  (term_load + term)
//   prefix(): (prefix_load + prefix) behind that commit: the four terms of the column in one 8-byte read; own prefix = the carried prefix (replicated
//             in the column's four owners) + the terms of the rows <= k (two v_dot2_u32_u16 with lane-constant 0/1 weights), to
//             ring[column][U + k]; the carried prefix moves on by all four
//   back():   the prefix w rows back, ring[column][(U + k - w) mod TRIP] -- base + immediate, but for the one group where the
//             wrap falls between the group's rows (U = w - 1: row -1 for k = 0), which has a lane-constant address of its own
// Everything is taken modulo 2^16 (window sums are < 2^16); the ring is zeroed in the prologue: rows above the strip read 0.
// (The four owners of a column read their rows from four slots 64 dwords apart -- the same banks.  Slots of 72 dwords take
//  those conflicts away and cost seven address additions, the offsets no longer fit ds_read2: measured, no gain, not kept.)
template <typename C>
struct RingTexture {
    static constexpr int TRIP = C::TRIP, RPG = C::RPG, WS = C::W1 - 1;
    static_assert(RPG == 4 && TRIP % RPG == 0 && TRIP >= WS + RPG && (WS - 1) % RPG == 0, "one straddling group, at U = w - 1");
    static constexpr int RING_BYTES = C::PPW * TRIP * 2;      // u16 [PPW][TRIP]; behind it the terms, u16 [PPW][RPG]
    uint32_t a_row, a_edge;       // the owned row's shared dwords / edge byte in the staging slots
    uint32_t a_term, a_col;       // terms[column][k], terms[column][0]
    uint32_t a_ring, a_wrap;      // ring[column][k], ring[column][(k + TRIP - 1) % TRIP]
    uint32_t w_lo, w_hi;          // packed 0/1 weights of the rows (0, 1) and (2, 3): rows <= k
    uint32_t carry;               // prefix sum of the column up to the last row of the previous group

    __device__ __forceinline__ void init(uint32_t stg_addr, uint32_t tex_addr, int p, int h)
    {
        const int k = h >> 1, j = h & 1, colw = 2 * p + j;
        a_row = stg_addr + (uint32_t)(k * C::SLOT + p + 1) * 4;
        a_edge = stg_addr + (uint32_t)(k * C::SLOT + p) * 4 + (j ? 12u : 3u);
        a_col = tex_addr + RING_BYTES + (uint32_t)colw * (RPG * 2);
        a_term = a_col + 2 * k;
        a_ring = tex_addr + (uint32_t)(colw * TRIP + k) * 2;
        a_wrap = tex_addr + (uint32_t)(colw * TRIP + (k + TRIP - 1) % TRIP) * 2;
        w_lo = k >= 1 ? 0x00010001u : 0x00000001u;
        w_hi = k >= 3 ? 0x00010001u : k == 2 ? 0x00000001u : 0u;
        carry = 0;
        // (laundered: every access below is one lane-constant register + an immediate)
        asm volatile("" : "+v"(a_row), "+v"(a_edge), "+v"(a_term), "+v"(a_col), "+v"(a_ring), "+v"(a_wrap), "+v"(w_lo), "+v"(w_hi));
    }
    template <int U>
    __device__ __forceinline__ uint32_t back() const
    {
        constexpr int lo = U - WS;                                    // the group's first row looks back to row `lo` of the trip
        if constexpr (lo < 0 && lo + RPG - 1 >= 0) {
            static_assert(lo == -1, "a_wrap is the address for U = w - 1");
            return *lds_as<const uint16_t>(a_wrap);
        } else {
            constexpr int idx = (lo + TRIP) % TRIP;
            static_assert(idx + RPG - 1 < TRIP, "no wrap inside the group");
            return *lds_as<const uint16_t>(a_ring + idx * 2);
        }
    }
    // (term and prefix in two halves each: the reads go out at the top of their step, in FRONT of the step's read-ahead of
    //  the next row, and are consumed behind the step's quad-SADs -- a wait for them in between would drain the read-ahead)
    struct TermIn { uint32_t l1, l2, e; };
    __device__ __forceinline__ TermIn term_load() const
    { return TermIn{*lds_as<const uint32_t>(a_row), *lds_as<const uint32_t>(a_row + 4), *lds_as<const uint8_t>(a_edge)}; }
    __device__ __forceinline__ void term(uint32_t capb, const TermIn& in) const
    {
        const uint32_t l1 = in.l1, l2 = in.l2, e = in.e;
        uint32_t t = __builtin_amdgcn_sad_u8(l1, capb, 0u);
        t = __builtin_amdgcn_sad_u8(l2, capb, t);
        t = __builtin_amdgcn_msad_u8(capb, e, t);                     // (zero reference bytes are skipped)
        *lds_as<uint16_t>(a_term) = (uint16_t)t;
    }
    __device__ __forceinline__ uint64_t prefix_load() const { return *lds_as<const uint64_t>(a_col); }
    template <int U>
    __device__ __forceinline__ uint32_t prefix(uint64_t q)
    {
        const sel_us2 lo = __builtin_bit_cast(sel_us2, (uint32_t)q), hi = __builtin_bit_cast(sel_us2, (uint32_t)(q >> 32));
        const sel_us2 ones = __builtin_bit_cast(sel_us2, 0x00010001u);
        uint32_t own = __builtin_amdgcn_udot2(lo, __builtin_bit_cast(sel_us2, w_lo), carry, false);
        own = __builtin_amdgcn_udot2(hi, __builtin_bit_cast(sel_us2, w_hi), own, false);
        carry = __builtin_amdgcn_udot2(lo, ones, carry, false);
        carry = __builtin_amdgcn_udot2(hi, ones, carry, false);
        *lds_as<uint16_t>(a_ring + U * 2) = (uint16_t)own;
        return own;
    }
};

// compile-time loops: over the row groups of one trip of the row loop (f returns false to stop) and over a group's rows
template <typename F, int... U>
__device__ __forceinline__ void ring_for_groups(std::integer_sequence<int, U...>, F&& f)
{ (void)(f(std::integral_constant<int, U>{}) && ...); }
template <typename F, int... R>
__device__ __forceinline__ void ring_for_rows(std::integer_sequence<int, R...>, F&& f)
{ (f(std::integral_constant<int, R>{}), ...); }

// FUSE: the grid starts with rg.nborder border-column workgroups (an instantiation of its own: with the border body inside,
// the tile loop of the batch form came out 1.6 % slower)
template <int D, int WS, int LPP, bool FUSE>
__global__ __launch_bounds__(256, (RingBounds<D, WS, LPP, FUSE>::WAVES)) void k_search_ring(Plane8 Lp, Plane8 Rp, Plane16W disp, uint16_t* cost, BMGeom g, RingGeom rg,
                                                                                   BorderGeom bg, Border2Geom b2g)
{
    using C = RingCfg<D, WS, LPP>;
    constexpr int NGL = C::NGL, NRL = C::NRL, W1 = C::W1, LWD = C::LWD, SLOT = C::SLOT, ITEMS = C::ITEMS, PPW = C::PPW, RPG = C::RPG;
    constexpr int GPW = C::GPW;
    constexpr bool SPLIT = C::SPLIT, PAIR = C::PAIR;
    static_assert(!PAIR || (SPLIT && C::STATIC_SLOTS && C::LPG == 2 * RPG), "the paired layout: one owner lane per (column, row) of a group");
    constexpr int RECD = C::Rec::DWORDS;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];

    // Workgroup ids go round-robin over the 8 XCDs, each with its own L2.  Item = (frame, strip, tile), tile fastest:
    // XCD k takes the items [k chunk, (k+1) chunk) in order, so the tiles of a strip -- which share their D + w column halo
    // -- and the strips of a frame -- which share w-1 rows -- meet in ONE L2 instead of being fetched into eight.
    unsigned fi = blockIdx.x;
    if constexpr (FUSE) {
        if (fi < rg.nborder) {
            // border columns: a latency-bound walk, dispatched first so that it runs under the tiles
            const unsigned per = (unsigned)(rg.bgx * rg.bgy), fr = fi / per, id = fi - fr * per;
            if (C::FUSE_BORDER2 && rg.b2) {
                const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
                border2_body<D, C::NP>(Lp, Rp, disp, cost, g, b2g, (int)(id % rg.bgx) * 4 + wave, (int)(id / rg.bgx), (int)fr);
            } else if constexpr (C::FUSE_BORDER) {
                border_body<(D + 63) / 64>((unsigned char*)lds, Lp, Rp, disp, cost, g, bg, (int)(id % rg.bgx), (int)(id / rg.bgx), (int)fr);
            }
            return;
        }
        fi -= rg.nborder;
    }
    if (rg.chunk) fi = (fi & 7u) * rg.chunk + (fi >> 3);
    if (fi >= rg.nitems) return;
    const int b_tile = (int)(fi % rg.tiles), b_strip = (int)((fi / rg.tiles) % rg.strips), f = (int)(fi / (rg.tiles * rg.strips));

    const int tid = threadIdx.x, lane = tid & 63;
    const int phi = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = lane & (GPW - 1), h = lane / GPW;
    const int x_tile = rg.x0 + b_tile * C::TILE;
    // PAIR: wave phi = (half, psi) takes the pairs x0 = x_tile + 32 half + 2 psi + 4 p; the lane with h = 2 k + j owns column
    // x0 + j in row k of every group -- `x`, `active`, the output offsets and the column mask below are those of the OWNED column
    const int xw = PAIR ? x_tile + (phi >> 1) * (C::TILE / 2) + 2 * (phi & 1) : x_tile + phi;   // the wave's first column
    const int hrow = PAIR ? h >> 1 : h;            // the row of a group this lane owns
    const int x = xw + 4 * p + (PAIR ? h & 1 : 0);
    const bool active = x < rg.x0 + rg.nx;
    const int ys0 = g.vy0 + b_strip * rg.rs;
    const int ys1 = min(ys0 + rg.rs, g.vy1);
    if (ys0 >= ys1) return;
    const int r = g.r;
    const uint8_t* Lb = Lp.base + (size_t)f * Lp.frame;
    // (PAIR: the copy starts PAIR_SHIFT = 3 bytes further left than that, so that a pair's shared window bytes are whole dwords
    //  of it: ring_step_pair.  The shift is part of the row POINTER below, not of these offsets: they are zero-extended 32-bit
    //  lane offsets and must not go negative -- with lofs = 0 (minDisparity <= 1 - D: createRightMatcher) the first tile's would)
    constexpr int PAIR_SHIFT = PAIR ? 3 : 0;
    const int Lbase = g.lofs + xw - r;             // image column of byte 0 (PAIR: byte 3) of this wave's copy (left)
    const int Rbase = g.rofs + xw - r;             //                                                            (right)
    const uint32_t capb = (uint32_t)(g.cap + PREFILTER_BIAS) * 0x01010101u;

    uint32_t* stg = lds + phi * C::WAVE_LDS;       // this wave's slice: nothing below is shared between waves
    // texture prefix ring [W1][PPW], 16 bits each (the lanes of a pixel write the same value; window sums are < 2^16 and
    // differences of prefix sums are taken modulo 2^16, so the prefix sums themselves may wrap)
    unsigned short* ptr = (unsigned short*)(stg + C::NSLOT * SLOT);
    // the window texture sum of row R of a group goes to ptw[R][p] (every lane of the pixel writes the same 16 bits) and the
    // row's owner reads its own at the end of the group: no per-row select in registers
    unsigned short* ptw = ptr + W1 * PPW;
    const bool owner = PAIR || RPG == LPP || h < RPG;   // this lane owns row h of every group
    const unsigned short* ptw_own = ptw + (owner ? hrow : 0) * PPW + p;
    // (PAIR: neither of the two -- a prefix ring per column and the row terms of a group in their place, RingTexture)
    struct None {};
    [[maybe_unused]] std::conditional_t<PAIR, RingTexture<C>, None> tex;
    static_assert(!PAIR || ((C::NSLOT * SLOT) % 2 == 0 && C::WAVE_LDS % 2 == 0), "the row terms of a column are read as 8 bytes");
    // this lane's selection record (lanes that own nothing: never used); rec0: the record of the lane group's first owner
    uint32_t* scr = stg + C::STG + (PAIR ? C::pair_rec(p, h) : (owner ? lane : 0) * RECD);
    uint32_t* const rec0 = stg + C::STG + (PAIR ? C::pair_rec(p, 0) : p * RECD);
    // SPLIT: where this lane's slice of the group's first row goes (PAIR: of column x0; the record of the owner with h = 2 k + j,
    // for column x0 + j in row k, lies 2 k + j records further)
    uint32_t* scr_w = rec0 + h * NRL;
    using GSel = GroupSelectRec<D, C::LPG, C::B64>;
    unsigned short* scr_m = (unsigned short*)(rec0 + D / 2) + h * (NRL / 4);   // ... and the minima of its groups
    if constexpr (SPLIT) GSel::init(scr);

    // --- staging: item idx = one dword of the wave's copy; dword m holds copy bytes [4m, 4m+4) (biased planes) ---------
    // Unconditional loads: bytes past a row's end only ever reach lanes that are not `active`, and the prefiltered planes
    // are allocated with 1 KB of slack behind the last row (api_bm.hip).  Two rows of loads are in flight (pre[0/1]; RingCfg::LOAD_SETS of
    // them in the forms that queue more).
    const int row0 = ys0 - r;
    const int Hm1 = g.H - 1;
    // One load per staged dword: address = the left plane's row (wave-uniform: lives in SGPRs and advances on the scalar
    // unit) + a 32-bit lane offset -- the right plane lies rg.rdelta bytes behind the left one (one allocation, api_bm.hip).
    // The byte phase makes the address unaligned; the memory pipeline takes unaligned dwords, and what arrives is what gets
    // staged: no second dword, no v_alignbyte, no 64-bit pointer arithmetic per lane.
    // (PAIR: row 0 of the first frame starts three bytes in front of the planes: api_bm.hip allocates slack there)
    const uint8_t* rowp = Lb + (size_t)row0 * Lp.pitch - PAIR_SHIFT;
    uint32_t loff[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int idx = lane + it * 64;
        const bool isr = idx >= LWD;
        // (PAIR: the lanes behind the copy's last dword repeat it -- the copy starts further right in the tile than a
        //  byte-phase copy does, and nothing may be read further behind a row's end than before)
        const int m = isr ? (PAIR ? min(idx - LWD, C::RWD - 1) : idx - LWD) : idx;
        loff[it] = (uint32_t)((isr ? Rbase : Lbase) + 4 * m) + (isr ? rg.rdelta : 0u);
    }
    int next_row = row0;
    constexpr int NPRE = C::LOAD_SETS;
    constexpr bool QUEUED = NPRE > 2;               // pre[0] is the oldest row in flight, pre[NPRE - 1] the newest
    uint32_t pre[NPRE][ITEMS];
    auto issue = [&](auto Sc) {                     // loads of the next row into register set Sc; rows past H-1 repeat H-1
        constexpr int SET = decltype(Sc)::value;
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            // (the empty asm keeps the zero-extension of the offset next to the load: hoisted out of the loop as a 64-bit
            //  value it hides the "SGPR base + 32-bit VGPR offset" addressing mode and costs a 64-bit VALU add per load)
            asm volatile("" : "+v"(loff[it]));
            pre[SET][it] = *(const uint32_t*)(rowp + loff[it]);
        }
        rowp += next_row < Hm1 ? Lp.pitch : 0;
        ++next_row;
    };
    auto commit = [&](auto Sc, auto slot) {        // slot: an int, or an integral_constant where the slots are static
        constexpr int SET = decltype(Sc)::value;
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) stg[slot * SLOT + lane + it * 64] = pre[SET][it];   // (the planes carry the +1 bias themselves)
        __builtin_amdgcn_wave_barrier();           // the wave's later reads stay behind these writes (LDS is in order per wave)
    };
    using Set0 = std::integral_constant<int, 0>;
    using Set1 = std::integral_constant<int, 1>;

    RingState<D, WS, LPP> st;
#pragma unroll
    for (int k = 0; k < W1; ++k)
#pragma unroll
        for (int i = 0; i < NGL; ++i) {
            st.P[k][i] = 0;
            if constexpr (PAIR) st.P2[k][i] = 0;
        }
    if constexpr (PAIR) {
        constexpr int RINGD = RingTexture<C>::RING_BYTES / 4;
#pragma unroll
        for (int i = 0; i < (RINGD + 63) / 64; ++i)
            if (i * 64 + 63 < RINGD || lane + i * 64 < RINGD) stg[C::NSLOT * SLOT + lane + i * 64] = 0;
        tex.init(lds_addr(stg), lds_addr(stg + C::NSLOT * SLOT), p, h);
    } else {
#pragma unroll
        for (int k = 0; k < W1; ++k) ptr[k * PPW + p] = 0;
    }
    uint32_t pt = 0;                                // texture prefix sum of the rows so far

    const int nsteps = (ys1 - ys0) + WS - 1;
    const int nstepsg = (nsteps + RPG - 1) / RPG * RPG;   // rows go in groups of RPG; padded last rows are computed and dropped
    issue(Set0{}); issue(Set1{});
    commit(Set0{}, 0); commit(Set1{}, 1);           // rows 0 and 1 -> slots 0 and 1
    issue(Set0{});                                  // row 2: committed at the end of step 0
    if constexpr (QUEUED)                           // rows 3 .. NPRE
        ring_for_rows(std::make_integer_sequence<int, NPRE - 2>{}, [&](auto Kc) { issue(std::integral_constant<int, decltype(Kc)::value + 1>{}); });

    // Output addresses: a wave-uniform frame base plus a 32-bit byte offset per lane that advances LPP rows per group
    // (the host checks that a frame's planes stay below 4 GB) -- no 64-bit multiply per store.
    char* const db = (char*)(disp.base + (size_t)f * disp.frame_e);
    char* const cb = (char*)(cost + (size_t)f * g.H * g.Ws);
    const int col = g.lofs + x;
    constexpr int TF = (WS - 1) / RPG * RPG;        // first group with an output row; its row h is strip row TF + h - (WS - 1)
    uint32_t dofs = (uint32_t)(((long long)(ys0 + TF + hrow - (WS - 1)) * (long long)disp.pitch_e + col) * 2);   // (mod 2^32; a row
    uint32_t cofs = (uint32_t)(((long long)(ys0 + TF + hrow - (WS - 1)) * (long long)g.Ws + col) * 2);           //  above the strip is never stored)
    const uint32_t dstep = (uint32_t)(disp.pitch_e * 2 * RPG), cstep = (uint32_t)(g.Ws * 2 * RPG);
    const bool masked_col = g.mask_cols && (col < g.vx0 || col >= g.vx1);

    uint32_t S[RPG][NRL];
    // Row t is read from LDS slot t mod 3 (t mod 4 with static slots), where it was put two steps earlier.  Step t issues the
    // global loads of row t+3 at its start and, at its end, writes row t+2 (issued one step earlier) to LDS -- BEHIND the step's
    // quad-SADs (the empty asm on S pins that order: left alone the compiler sinks the SADs below the commit and every step then
    // waits for its loads).  Rows past the strip's last are loaded and staged too (clamped to the frame) and never read:
    // no branch in the step.
    // The forms that queue their loads (LOAD_SETS > 2, the paired form): step t issues the loads of row t+LOAD_SETS+1 and its
    // commit writes row t+2, issued LOAD_SETS-1 steps earlier; with PREFETCH the LDS reads of row t+1 go out at the top of
    // step t as well, and the quad-SADs of step t run on what step t-1 requested.
    int sl_cur = 0;                                 // LDS slot of row t
    // this lane's read addresses in the slot of row t: three registers that move on by one slot per row (one v_add each
    // with a wave-uniform step; laundered so that every window offset folds into a ds_read immediate of ITS base)
    // (32-bit LDS addresses, not C++ pointers: a generic pointer that went through an asm loses its address space and
    //  turns every read into a flat load -- measured 2x slower)
    // Static slots (four of them, trip a multiple of four rows): the slot is a constant of the unrolled step and the three
    // registers never move -- every read is base + immediate.
    uint32_t la_cur = lds_addr(stg + p), ra_cur = lds_addr(stg + LWD + p + h * NGL), ro_cur = ra_cur + 4;
    if constexpr (C::STATIC_SLOTS) asm volatile("" : "+v"(la_cur), "+v"(ra_cur), "+v"(ro_cur));
    const auto lds_row = [&](auto SLc, RowRegs<D, WS, LPP>& rw) {
        if constexpr (C::STATIC_SLOTS) {
            constexpr uint32_t off = (uint32_t)(decltype(SLc)::value * SLOT * 4);
            ring_load_row<D, WS, LPP>(lds_at(la_cur + off), lds_at(ra_cur + off), lds_at(ro_cur + off), rw);
        } else if constexpr (C::ROW_PTRS) {
            asm volatile("" : "+v"(la_cur), "+v"(ra_cur), "+v"(ro_cur));
            ring_load_row<D, WS, LPP>(lds_at(la_cur), lds_at(ra_cur), lds_at(ro_cur), rw);
            const uint32_t adv = (uint32_t)((sl_cur == 2 ? -2 * SLOT : SLOT) * 4);   // (before the step moves sl_cur on)
            la_cur += adv; ra_cur += adv; ro_cur += adv;
        } else {
            int li = sl_cur * SLOT + p, ri = sl_cur * SLOT + LWD + p + h * NGL, one = 1;
            asm volatile("" : "+v"(li), "+v"(ri), "+v"(one));
            ring_load_row<D, WS, LPP, const uint32_t*>(stg + li, stg + ri, stg + ri + one, rw);
        }
    };
    // Sr / Sr2: the window sums of the row (PAIR: of column x0 / x0 + 1; Sr2 is not written otherwise)
    [[maybe_unused]] uint32_t tback = 0, tpre = 0;  // PAIR: the owned row's texture prefix sum and the one w rows back
    // ahead(): the LDS reads of the NEXT row (PREFETCH; nothing otherwise), issued behind the step's own texture reads
    auto step = [&](auto Kc, auto SLc, auto Rc, auto Uc, auto&& ahead, const RowRegs<D, WS, LPP>& rw, uint32_t (&Sr)[NRL], uint32_t (&Sr2)[NRL]) {
        constexpr int K = decltype(Kc)::value;            // ring slot of row t: a compile-time register set
        // (two load sets, not queued:)
        using SetIn = std::integral_constant<int, (K + 1) & 1>;    // row t+3 goes where row t+1 was (W1 is even: K and t have the same parity)
        using SetOut = std::integral_constant<int, K & 1>;         // row t+2
        if constexpr (QUEUED) issue(std::integral_constant<int, NPRE - 1>{});   // row t+NPRE+1, behind the queue
        else issue(SetIn{});
        uint32_t tnew = 0;
        constexpr int KO = (K + 1) % W1;
        if constexpr (PAIR) {
            constexpr int R = decltype(Rc)::value, U = decltype(Uc)::value;
            // the group's four rows are resident from the commit of step 1 to the commit of this step's end (RingTexture)
            [[maybe_unused]] typename RingTexture<C>::TermIn tin;
            [[maybe_unused]] uint64_t tq;
            if constexpr (R == 2) { tback = tex.template back<U>(); tin = tex.term_load(); }
            if constexpr (R == 3) tq = tex.prefix_load();
            ahead();
            // nothing but scalar work, global loads and LDS stores crosses: the reads above stay in front of the step's first
            // quad-SAD (left alone they sink to their first use, a step later) and the SADs stay behind them
            if constexpr (C::PREFETCH) __builtin_amdgcn_sched_barrier(0x214);
            ring_step_pair<D, WS, LPP, K>(st, rw, Sr, Sr2);
            pin(Sr2);
            // (the empty asm orders the use of what was read behind the quad-SADs: the wait for it is a counted one there)
            if constexpr (R == 2) { asm volatile("" : "+v"(tin.l1), "+v"(tin.l2), "+v"(tin.e)); tex.term(capb, tin); }
            if constexpr (R == 3) { asm volatile("" : "+v"(tq)); tpre = tex.template prefix<U>(tq); }
        } else {
            ahead();
            ring_step<D, WS, LPP, K>(st, rw, rg.lastmask, capb, tnew, Sr);
            pt += tnew;
            const uint32_t told = ptr[KO * PPW + p];                  // prefix sum w rows back (0 while the window fills)
            ptr[K * PPW + p] = (unsigned short)pt;
            ptw[decltype(Rc)::value * PPW + p] = (unsigned short)(pt - told);   // (mod 2^16: the window sum itself is < 2^16)
        }
        pin(Sr);
        if constexpr (QUEUED) {
            static_assert(C::STATIC_SLOTS, "the queued loads go with static slots");
            commit(Set0{}, std::integral_constant<int, (decltype(SLc)::value + 2) % 4>{});   // row t+2, the head of the queue
            // (the queue moves on: names only inside the unrolled trip, a few v_mov at its back edge)
#pragma unroll
            for (int it = 0; it < ITEMS; ++it)
#pragma unroll
                for (int k = 0; k + 1 < NPRE; ++k) pre[k][it] = pre[k + 1][it];
        } else if constexpr (C::STATIC_SLOTS) {
            commit(SetOut{}, std::integral_constant<int, (decltype(SLc)::value + 2) % 4>{});   // row t+2
        } else {
            const int sl_new = sl_cur == 0 ? 2 : sl_cur - 1;        // slot of row t+2 = (t + 2) mod 3
            sl_cur = sl_cur == 2 ? 0 : sl_cur + 1;
            commit(SetOut{}, sl_new);
        }
    };

    // One trip of the outer loop = whole rounds of the ring AND whole row groups (TRIP rows), unrolled: every row step has
    // its ring slot -- its registers -- fixed at compile time.
    // PREFETCH: two row register sets, alternating by the parity of the step (TRIP is even: a constant of every unrolled step,
    // the same in every trip).  Row 0 is requested here, behind the commits of rows 0 and 1; step t requests row t + 1 into
    // set (t + 1) & 1 and consumes set t & 1 -- across group, trip and rebase boundaries alike.  The last step's request goes
    // to a slot that holds a staged row like any other (rows past the strip are staged clamped) and is never used.
    [[maybe_unused]] RowRegs<D, WS, LPP> rwp[2];
    if constexpr (C::PREFETCH) lds_row(std::integral_constant<int, 0>{}, rwp[0]);
    int trips_since_rebase = 0;
    for (int t0 = 0; t0 < nstepsg; t0 += C::TRIP) {
        // Rebase (round 3): a trip starts on ring slot 0, whose content P(t-w-1) is dead; slot 1 holds the oldest prefix sum
        // still needed, P(t-w).  Subtracting it from every live slot (per 16-bit half, no borrow: prefix sums only grow)
        // leaves all window sums unchanged and keeps the halves below 2^16 for another rg.rebase trips -- strips no longer have
        // to be short, and a long strip pays the w-1 window-filling rows once instead of once per ~100 rows.
        if (rg.rebase && ++trips_since_rebase > rg.rebase) {
            trips_since_rebase = 1;
#pragma unroll
            for (int i = 0; i < NGL; ++i) {
                const uint32_t blo = (uint32_t)st.P[1][i], bhi = (uint32_t)(st.P[1][i] >> 32);
#pragma unroll
                for (int k = 1; k < W1; ++k) {
                    const uint32_t lo = (uint32_t)st.P[k][i] - blo, hi = (uint32_t)(st.P[k][i] >> 32) - bhi;
                    st.P[k][i] = (uint64_t)lo | ((uint64_t)hi << 32);
                }
                if constexpr (PAIR) {                                // the second column's ring likewise, by ITS oldest prefix sum
                    const uint32_t blo2 = (uint32_t)st.P2[1][i], bhi2 = (uint32_t)(st.P2[1][i] >> 32);
#pragma unroll
                    for (int k = 1; k < W1; ++k) {
                        const uint32_t lo = (uint32_t)st.P2[k][i] - blo2, hi = (uint32_t)(st.P2[k][i] >> 32) - bhi2;
                        st.P2[k][i] = (uint64_t)lo | ((uint64_t)hi << 32);
                    }
                }
            }
        }
        ring_for_groups(std::make_integer_sequence<int, C::TRIP / RPG>{}, [&](auto Uc) -> bool {
            constexpr int U = RPG * decltype(Uc)::value;
            const int t = t0 + U;
            if (t >= nstepsg) return false;
            GSel gsel;
            ring_for_rows(std::make_integer_sequence<int, RPG>{}, [&](auto Rc) {
                constexpr int R = decltype(Rc)::value;
                using SL = std::integral_constant<int, (U + R) % 4>;    // (static slots: TRIP % 4 == 0, so t % 4 == (U + R) % 4)
                uint32_t S2[NRL] = {};                                  // (PAIR only: column x0 + 1)
                if constexpr (C::PREFETCH) {
                    // The left pieces of THIS row, requested a step ago (the two oldest reads in the queue), are pinned here:
                    // without it the byte masks of the pair's edge pieces and the quad-SADs that start from zero -- work that
                    // depends on the row alone -- are lifted into the step that issued the reads, which then waits for them
                    // at once.  The windows are not pinned: their waits are the compiler's, counted.
                    pin(rwp[(U + R) & 1].l);
                    const auto ahead = [&] { lds_row(std::integral_constant<int, (U + R + 1) % 4>{}, rwp[(U + R + 1) & 1]); };   // row t + 1
                    step(std::integral_constant<int, (U + R) % W1>{}, SL{}, Rc, std::integral_constant<int, U>{}, ahead, rwp[(U + R) & 1], S[R], S2);
                } else {
                    RowRegs<D, WS, LPP> rw;
                    lds_row(SL{}, rw);
                    step(std::integral_constant<int, (U + R) % W1>{}, SL{}, Rc, std::integral_constant<int, U>{}, [] {}, rw, S[R], S2);
                }
                // the row's slice and the minima of its groups go to its owner's record at once: S[R] is dead after this
                // (also while the window fills: no branch around it)
                if constexpr (PAIR) {
                    gsel.template row<R>(S[R], scr_w + 2 * R * C::PREC, scr_m + 2 * R * (C::PREC * 2));
                    gsel.template row<R>(S2, scr_w + (2 * R + 1) * C::PREC, scr_m + (2 * R + 1) * (C::PREC * 2));
                } else if constexpr (SPLIT) gsel.template row<R>(S[R], scr_w + R * (PPW * RECD), scr_m + R * (PPW * RECD * 2));
            });
            if (t + RPG - 1 < WS - 1) return true;                  // the window is still filling
            // the lanes p + h PPW hold the LPP slices of a pixel for the rows t .. t+RPG-1; the lane with h = k < RPG owns row t+k
            const int y = ys0 + (t - (WS - 1)) + hrow;
            const bool row_ok = owner && y >= ys0 && y < ys1;
            const uint32_t dof = dofs, cof = cofs;
            dofs += dstep; cofs += cstep;
            // Selection is skipped for a wave none of whose pixels can produce a disparity here (untextured, outside the
            // tile, masked): exact, such a pixel is FILTERED and writes no cost whatever its SADs are.
            int tsum;                                                // the texture sum of the row this lane owns
            if constexpr (PAIR) tsum = (int)((tpre - tback) & 0xffffu);
            else tsum = *ptw_own;
            // (bitwise: one lane mask for the vote, no branch around the texture read)
            const bool dead = !active | !row_ok | masked_col | (tsum < g.tex);
            if (__builtin_amdgcn_ballot_w64(!dead) == 0) {
                if (active && row_ok) *(int16_t*)(db + dof) = (int16_t)g.filtered;
            } else {
                int m1; bool fail;
                int out;
                if constexpr (SPLIT) {
                    int uq = g.uniq;
                    asm volatile("" : "+s"(uq));                     // (tested here, on the scalar unit, not hoisted as a lane mask)
                    out = gsel.finish(tsum, g, uq > 0, scr, &m1, &fail);
                } else {
                    // two lanes per pixel: after the swap the lower lane has both halves of row t and the upper lane both
                    // halves of row t+1
                    uint32_t rr[D / 2];
#pragma unroll
                    for (int i = 0; i < NRL; ++i) {
                        const auto sw = __builtin_amdgcn_permlane32_swap(S[0][i], S[RPG - 1][i], false, false);
                        rr[i] = sw[0]; rr[NRL + i] = sw[1];
                    }
                    out = select_disparity_lds<D>(rr, tsum, g, scr, &m1, &fail);
                }
                if (active && row_ok) {
                    if (!fail && g.want_cost) *(uint16_t*)(cb + cof) = (uint16_t)m1;
                    *(int16_t*)(db + dof) = (int16_t)(masked_col ? g.filtered : out);
                }
            }
            return true;
        });
    }
}

// ---- host side ----------------------------------------------------------------------------

// rows a strip may have so that no prefix sum leaves 16 bits: a row adds at most w * 2 cap per disparity, and a strip of
// rs output rows walks rs + w - 1 rows plus up to seven padded rows (groups of eight)
static int ring_rows_cap(const BMGeom& g) { return 65535 / (g.w * 2 * g.cap) - g.w - 6; }
// trips of the row loop between two rebases of the ring (0: one trip is longer than the cap -- no rebasing, short strips)
static int ring_rebase_trips(const BMGeom& g, int lpp)
{
    const int W1 = g.w + 1, rpg = ring_rpg(g.D, lpp);
    const int trip = (W1 % rpg == 0) ? W1 : (2 * W1 % rpg == 0) ? 2 * W1 : 4 * W1;   // RingCfg::TRIP
    return ring_rows_cap(g) / trip;
}
// strips a frame must at least be cut into
static int ring_min_strips(const BMGeom& g, int lpp, int nrows)
{ return ring_rebase_trips(g, lpp) > 0 ? 1 : max(1, (nrows + ring_rows_cap(g) - 1) / ring_rows_cap(g)); }

// Instantiations: (D, blockSize, lanes per pixel).  Two lanes per pixel: every (D, blockSize) whose ring (blockSize+1) * D/4
// registers per lane leaves room for two waves per SIMD.  Four lanes per pixel: the D = 64 ones, whose two-lane ring holds
// them at two waves, and D = 96 (D = 32 with four lanes measured 0-8 % slower than with two: not instantiated).  Eight
// lanes: D = 128.
#ifdef RTDM_RING_DEV      // development builds (tools/ring_isa.sh): -DRTDM_RING_DEV="X(64, 9, 4)" = these instantiations only
#define RTDM_RING_TABLE(X) RTDM_RING_DEV
#else
#define RTDM_RING_TABLE(X) X(64, 9, 2) X(64, 7, 2) X(64, 5, 2) X(32, 7, 2) X(32, 9, 2) X(32, 11, 2) X(32, 13, 2) X(48, 7, 2) X(48, 9, 2) \
                           X(16, 5, 2) X(16, 7, 2) X(16, 9, 2) X(64, 9, 4) X(64, 7, 4) X(64, 5, 4) X(64, 11, 4) X(64, 13, 4) \
                           X(128, 7, 8) X(128, 9, 8) X(128, 11, 8) X(128, 13, 8) X(96, 7, 4) X(96, 9, 4) X(96, 11, 4) X(96, 13, 4) X(48, 11, 2) X(48, 13, 2) \
                           X(16, 11, 2) X(16, 13, 2) X(32, 5, 2) X(32, 15, 2) X(48, 5, 2) X(64, 15, 4) X(128, 15, 8) \
                           X(192, 9, 8) X(192, 11, 8) X(192, 13, 8) X(192, 15, 8) X(256, 9, 16) X(256, 11, 16) X(256, 13, 16) X(256, 15, 16)
#endif

// rtdm_debug_search_kernel (a process-wide diagnostic switch; one atomic word so that a launch on another thread sees a consistent
// pair): low byte = mode + 1 (0 never, 1 wherever instantiated, -1 default), next byte = lanes per pixel to force (0: none)
static std::atomic<int> g_ring_switch{0};
void ring_set_mode(int mode)
{
    const int m = mode < 0 ? -1 : mode == 0 ? 0 : 1, lpp = (mode == 2 || mode == 4 || mode == 8) ? mode : 0;
    g_ring_switch.store((m + 1) | (lpp << 8), std::memory_order_relaxed);
}
static int ring_mode() { return (g_ring_switch.load(std::memory_order_relaxed) & 0xff) - 1; }
static int ring_forced_lpp() { return g_ring_switch.load(std::memory_order_relaxed) >> 8; }

// lanes per pixel for a configuration (0: not instantiated).  rtdm_debug_search_kernel may force one form where it exists.
static int ring_lpp(const BMGeom& g)
{
    int have = 0;                          // bit mask of the forms instantiated for (D, w)
#define X(DD, WW, LL) if (g.D == DD && g.w == WW) have |= LL;
    RTDM_RING_TABLE(X)
#undef X
    const int want = ring_forced_lpp();
    if (want && (have & want) == want) return want;
    // measured (tools/ab_ring.py): more lanes per pixel win where the ring holds the two-lane form at two waves per SIMD
    return (have & 16) ? 16 : (have & 8) ? 8 : (have & 4) ? 4 : (have & 2) ? 2 : 0;
}

// the instantiation (D, w, lpp).  waves = workgroups resident per CU (a workgroup is four waves, one per SIMD)
static RingForm ring_form_of(const BMGeom& g, int lpp)
{
#define X(DD, WW, LL) if (g.D == DD && g.w == WW && lpp == LL) { using C = RingCfg<DD, WW, LL>; return RingForm{LL, C::WAVES, C::FUSE_BORDER2, C::FUSE_BORDER, C::TILE}; }
    RTDM_RING_TABLE(X)
#undef X
    return RingForm{};
}

RingForm ring_form(const BMGeom& g)
{
    const RingForm none{};
    if (ring_mode() == 0) return none;
    if (2L * g.cap * g.w * g.w > 32766) return none;       // packed u16 sums + the T+1 <= 32767 argument of the selection
    if (2L * g.cap * g.w * g.w >= 0x7C00) return none;     // ... and positive finite f16 for the group minima (sel_pk_min3_h; cap <= 63
                                                           //     keeps every ring form below: 2 * 63 * 15^2 = 28350)
    if (ring_rows_cap(g) < 2) return none;
    if ((size_t)g.H * (size_t)g.Ws * 2 >= ((size_t)1 << 32)) return none;   // 32-bit byte offsets inside a frame (pitch <= Ws)
    return ring_form_of(g, ring_lpp(g));
}

int ring_strips_model(const SearchPlan& plan, const BMGeom& g, int n)
{
    const int tile = 256 / plan.lanes, tiles = (plan.nx + tile - 1) / tile, nrows = g.vy1 - g.vy0;
    const int slots = 256 * ring_form_of(g, plan.lanes).waves;            // workgroups in flight on the chip
    const int smin = ring_min_strips(g, plan.lanes, nrows), smax = max(smin, (nrows + 15) / 16);
    // a strip pays w-1 filling rows at about half the price of an output row
    const float fill = 0.5f * (float)(g.w - 1);
    int s = (int)(sqrtf((float)nrows * (float)slots / (fill * (float)tiles * (float)n)) + 0.5f);
    s = max(smin, min(s, smax));
    if ((long)tiles * s * n < 6L * slots) {
        // Small jobs (single frames, small batches -- nothing measures their strip count): the grid is a handful of
        // scheduling rounds, and a round that is started is paid in full.  Time ~ rounds x (rows per workgroup + fill + a
        // fixed two rows' worth of prologue); take the strip count that minimises it.
        float best = 1e30f;
        for (int c = smin; c <= smax; ++c) {
            const int rs = (nrows + c - 1) / c, ce = (nrows + rs - 1) / rs;
            const long rounds = ((long)tiles * ce * n + slots - 1) / slots;
            const float t = (float)rounds * ((float)rs + fill + 2.0f);
            if (t < best) { best = t; s = ce; }
        }
    }
    return s;
}

template <int D, int WS, int LPP>
static void ring_launch_one(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n, hipStream_t stream,
                            int strips_hint)
{
    using C = RingCfg<D, WS, LPP>;
    RingGeom rg;
    rg.rdelta = (uint32_t)(Rp.base - Lp.base);       // (plan_search's planes_contiguous: it fits)
    rg.x0 = plan.x0; rg.nx = plan.nx;
    const int rem = g.w - 4 * (C::NP - 1);
    rg.lastmask = rem >= 4 ? 0xffffffffu : ((1u << (8 * rem)) - 1u);
    const int nrows = g.vy1 - g.vy0;
    const int tiles = (rg.nx + C::TILE - 1) / C::TILE;
    int strips = strips_hint > 0 ? strips_hint : ring_strips_model(plan, g, n);
    strips = max(strips, ring_min_strips(g, LPP, nrows));
    rg.rebase = ring_rebase_trips(g, LPP);            // (= ring_rows_cap / C::TRIP)
    strips = max(1, min(strips, nrows));
    rg.rs = (nrows + strips - 1) / strips;
    strips = (nrows + rg.rs - 1) / rg.rs;
    rg.tiles = tiles; rg.strips = strips;
    rg.nitems = (unsigned)tiles * strips * n;
    rg.chunk = (rg.nitems + 7) / 8;                   // XCD-local order (the kernel still accepts chunk == 0: plain order)
    const unsigned grid = rg.chunk * 8;
    BorderGeom bg{};
    Border2Geom b2g{};
    size_t blds = 0;
    rg.nborder = 0; rg.bgx = rg.bgy = 0; rg.b2 = 0;
    if (plan.place == BorderPlace::FUSED && plan.border.form != BorderForm::NONE) {   // (ROWS or DISP, as ring_form allowed)
        const BorderPlan& b = plan.border;
        if (b.form == BorderForm::ROWS) { b2g = b.rows; rg.b2 = 1; }
        else { bg = b.disp; blds = b.lds; }
        rg.bgx = b.gx; rg.bgy = b.gy;
        rg.nborder = (unsigned)(rg.bgx * rg.bgy) * (unsigned)n;
    }
    const size_t ldsb = max((size_t)4 * C::WAVE_LDS * sizeof(uint32_t), blds);
    const auto launch = [&](auto Fc) {
        constexpr bool F = decltype(Fc)::value;
        // The most this instantiation ever asks for depends on (D, w, LPP) alone: its ring records, or the border workgroups'
        // LDS where they ride in its grid.  Above 48 KB it is granted once per device of this process (a handle lives on one
        // device; a second thread that races the first caller on the same device sets the same value), never beyond the
        // device's LDS.
        constexpr size_t ring_lds = (size_t)4 * C::WAVE_LDS * sizeof(uint32_t);
        const size_t most = C::FUSE_BORDER ? max(ring_lds, border_lds_bytes(D, WS)) : ring_lds;
        static OncePerDevice once;
        if (most > 48 * 1024 && once.first()) {
            int dev = 0, lds_max = 0;
            size_t want = max(most, (size_t)64 * 1024);
            if (hipGetDevice(&dev) == hipSuccess &&
                hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess && lds_max > 0)
                want = min(want, (size_t)lds_max);
            (void)hipGetLastError();
            (void)hipFuncSetAttribute((const void*)k_search_ring<D, WS, LPP, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
        }
        hipLaunchKernelGGL((k_search_ring<D, WS, LPP, F>), dim3(grid + rg.nborder), dim3(256), ldsb, stream, Lp, Rp, disp, (uint16_t*)cost, g, rg, bg, b2g);
    };
    if (rg.nborder) launch(std::true_type{});
    else launch(std::false_type{});
}

void launch_search_ring(const SearchPlan& plan, Plane8 Lp, Plane8 Rp, Plane16W disp, void* cost, const BMGeom& g, int n, hipStream_t stream,
                        int strips)
{
#define X(DD, WW, LL) if (g.D == DD && g.w == WW && plan.lanes == LL) { ring_launch_one<DD, WW, LL>(plan, Lp, Rp, disp, cost, g, n, stream, strips); return; }
    RTDM_RING_TABLE(X)
#undef X
}

}  // namespace rtdm
