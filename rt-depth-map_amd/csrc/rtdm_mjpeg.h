// rtdm_mjpeg.h -- baseline JPEG (SOF0) for the MJPEG decoder: the host-side header parser and the per-segment entropy decoder
// (rule J1).  The segment decoder and the Huffman table builder compile for the device (k_mjpeg.hip)
// and as plain C++ (MJ_HD expands to nothing): tests/mjpeg_host.cpp runs them on the CPU, under the host sanitizers too,
// before any stream reaches a GPU.  Nothing here touches HIP.
#ifndef RTDM_MJPEG_H_
#define RTDM_MJPEG_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MJ_HD __host__ __device__ __forceinline__
#else
#define MJ_HD inline
#endif

namespace rtdm {

// status values of include/rtdm.h (this header stands alone so that the host harness needs nothing else)
enum { MJ_OK = 0, MJ_BAD_SIZE = -2, MJ_UNSUPPORTED = -6, MJ_NULL = -7, MJ_BAD_STREAM = -8 };

static const int MJ_LOOK = 8;   // codes of up to 8 bits are resolved by one table look-up

// Per frame, as the device sees it.  Table t of a component c: t = 2 c (DC), 2 c + 1 (AC), already resolved from the scan
// header's selectors, so the kernel follows no indirection.  Quantisers are in zigzag order, as DQT carries them.
struct MjpegDesc {
    uint32_t stream_off, stream_len;   // this frame's bytes inside the chunk's stream buffer (SOI .. EOI)
    uint32_t seg_first, nseg;          // its entropy segments inside the chunk's segment table
    int32_t W, H, ncomp, hs, vs;       // hs x vs: luma sampling (1 x 1 for a one-component frame)
    int32_t mcux, mcuy, ri;            // MCU grid; MCUs per segment (the whole frame when the stream has no DRI)
    uint8_t qt[3][64];
    uint8_t bits[6][16];
    uint8_t vals[6][256];
};
struct MjpegSeg { uint32_t begin, end; };   // byte range of one entropy segment inside the frame's stream, markers excluded

// A decoding table: look[v] for the next MJ_LOOK bits v = (length << 8 | symbol), 0 where the code is longer; then the
// standard's walk: a code of length l is valid iff code <= maxcode[l], its symbol is vals[valoff[l] + code].
struct MjpegHuff {
    uint16_t look[1 << MJ_LOOK];
    int32_t maxcode[17];    // -1: no code of this length
    int32_t valoff[17];
    uint8_t vals[256];
};

static const uint8_t MJ_ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                                      13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
                                      52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// bits[l - 1] codes of length l, their symbols in vals (the parser has checked that the counts fit: mjpeg_check_counts)
MJ_HD void mjpeg_build_table(const uint8_t* bits, const uint8_t* vals, MjpegHuff* t)
{
    for (int i = 0; i < (1 << MJ_LOOK); ++i) t->look[i] = 0;
    for (int i = 0; i < 256; ++i) t->vals[i] = vals[i];
    int code = 0, k = 0;
    t->maxcode[0] = -1; t->valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        t->valoff[l] = k - code;
        if (n && l <= MJ_LOOK) {
            for (int j = 0; j < n; ++j) {
                const int first = (code + j) << (MJ_LOOK - l), span = 1 << (MJ_LOOK - l);
                for (int e = 0; e < span; ++e)
                    if (first + e < (1 << MJ_LOOK)) t->look[first + e] = (uint16_t)((l << 8) | vals[(k + j) & 255]);
            }
        }
        code += n; k += n;
        t->maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
}

// Bit reader over one entropy segment s[begin, end): 0xFF00 unstuffs to 0xFF, a 0xFF before anything else ends the data, and
// every byte past the end reads as zero (counted, so that an overrun is noticed).  No read leaves [begin, end).
struct MjpegBits {
    const uint8_t* s;
    uint32_t p, end;
    uint64_t acc;
    int n;           // valid bits in acc (the low n)
    int fed;         // zero bytes supplied past the end
};

MJ_HD void mjpeg_fill(MjpegBits& b)
{
    while (b.n <= 56) {
        uint32_t byte = 0;
        if (b.p < b.end) {
            byte = b.s[b.p];
            if (byte == 0xFF) {
                if (b.p + 1 < b.end && b.s[b.p + 1] == 0) b.p += 2;
                else { b.p = b.end; byte = 0; ++b.fed; }      // a marker or a lone 0xFF: the data ends here
            } else ++b.p;
        } else ++b.fed;
        b.acc = (b.acc << 8) | byte;
        b.n += 8;
    }
}
MJ_HD uint32_t mjpeg_peek16(const MjpegBits& b) { return (uint32_t)(b.acc >> (b.n - 16)) & 0xFFFFu; }
MJ_HD uint32_t mjpeg_take(MjpegBits& b, int s)      // s in 0..16, at least s bits buffered
{
    b.n -= s;
    return (uint32_t)(b.acc >> b.n) & ((1u << s) - 1u);
}

// one symbol; -1 for a bit pattern that is no code.  Needs >= 16 buffered bits.
MJ_HD int mjpeg_symbol(MjpegBits& b, const MjpegHuff* t)
{
    const uint32_t v = mjpeg_peek16(b);
    const uint32_t e = t->look[v >> (16 - MJ_LOOK)];
    if (e) { b.n -= (int)(e >> 8); return (int)(e & 255u); }
    for (int l = MJ_LOOK + 1; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (code <= t->maxcode[l]) { b.n -= l; return t->vals[(t->valoff[l] + code) & 255]; }
    }
    return -1;
}

MJ_HD int mjpeg_extend(uint32_t v, int s) { return s == 0 ? 0 : ((int)v >= (1 << (s - 1)) ? (int)v : (int)v - (1 << s) + 1); }
MJ_HD int16_t mjpeg_sat16(int v) { return (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// first block of a component's plane inside a frame's coefficient buffer, in blocks
MJ_HD uint32_t mjpeg_comp_first_block(const MjpegDesc& d, int c)
{
    const uint32_t luma = (uint32_t)(d.mcux * d.hs) * (uint32_t)(d.mcuy * d.vs), chroma = (uint32_t)d.mcux * (uint32_t)d.mcuy;
    return c == 0 ? 0u : luma + (uint32_t)(c - 1) * chroma;
}
MJ_HD uint32_t mjpeg_frame_blocks(const MjpegDesc& d)
{
    return mjpeg_comp_first_block(d, d.ncomp);
}

// J1 for entropy segment `seg` of a frame: its MCUs [seg * ri, min((seg + 1) * ri, mcux * mcuy)).  coef: the frame's zeroed
// coefficient buffer, mjpeg_frame_blocks(d) * 64 int16, natural order, dequantised and saturated to 16 bits; only non-zero
// positions are written.  tabs: the six tables of the frame; zz: MJ_ZIGZAG (wherever the caller keeps it).  Returns MJ_OK
// or MJ_BAD_STREAM (a bit pattern that is no code, a coefficient index past 63, or more bits used than the segment holds);
// the loop ends there.  Every store is to a block of this segment's own MCUs and to an index 0..63.
MJ_HD int mjpeg_decode_segment(const uint8_t* stream, const MjpegDesc& d, const MjpegSeg sg, uint32_t seg, const MjpegHuff* tabs,
                               const uint8_t* zz, int16_t* coef)
{
    const uint32_t total = (uint32_t)d.mcux * (uint32_t)d.mcuy;
    const uint32_t per = d.ri > 0 ? (uint32_t)d.ri : total;
    const uint64_t first64 = (uint64_t)seg * per;
    if (first64 >= total) return MJ_BAD_STREAM;
    const uint32_t first = (uint32_t)first64, last = first + per < total ? first + per : total;
    const uint32_t nblocks = mjpeg_frame_blocks(d);
    MjpegBits b;
    b.s = stream; b.p = sg.begin; b.end = sg.end < d.stream_len ? sg.end : d.stream_len; b.acc = 0; b.n = 0; b.fed = 0;
    if (b.p > b.end) b.p = b.end;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    for (uint32_t mcu = first; mcu < last; ++mcu) {
        const uint32_t my = mcu / (uint32_t)d.mcux, mx = mcu - my * (uint32_t)d.mcux;
        for (int c = 0; c < d.ncomp; ++c) {
            const int h = c == 0 ? d.hs : 1, v = c == 0 ? d.vs : 1;
            const uint32_t pitch = (uint32_t)(d.mcux * h), base = mjpeg_comp_first_block(d, c);
            const MjpegHuff* dc = tabs + 2 * c;
            const MjpegHuff* ac = dc + 1;
            const uint8_t* q = d.qt[c];
            for (int j = 0; j < v; ++j) for (int i = 0; i < h; ++i) {
                const uint32_t blk = base + (my * (uint32_t)v + (uint32_t)j) * pitch + mx * (uint32_t)h + (uint32_t)i;
                if (blk >= nblocks) return MJ_BAD_STREAM;                 // cannot happen for a parsed frame; the guard stays
                int16_t* out = coef + (size_t)blk * 64;
                mjpeg_fill(b);
                int s = mjpeg_symbol(b, dc);
                if (s < 0 || s > 15) return MJ_BAD_STREAM;
                const int diff = mjpeg_extend(mjpeg_take(b, s), s);
                int pred = (c == 0 ? pred0 : (c == 1 ? pred1 : pred2)) + diff;
                pred = pred < -32768 ? -32768 : (pred > 32767 ? 32767 : pred);
                if (c == 0) pred0 = pred; else if (c == 1) pred1 = pred; else pred2 = pred;
                const int16_t dcv = mjpeg_sat16(pred * (int)q[0]);
                if (dcv) out[0] = dcv;
                for (int k = 1; k < 64;) {
                    mjpeg_fill(b);
                    const int rs = mjpeg_symbol(b, ac);
                    if (rs < 0) return MJ_BAD_STREAM;
                    const int r = rs >> 4;
                    s = rs & 15;
                    if (s == 0) {
                        if (r != 15) break;
                        k += 16;
                        continue;
                    }
                    k += r;
                    if (k > 63) return MJ_BAD_STREAM;
                    const int16_t val = mjpeg_sat16(mjpeg_extend(mjpeg_take(b, s), s) * (int)q[k]);
                    if (val) out[zz[k] & 63] = val;
                    ++k;
                }
                if (b.fed * 8 > b.n) return MJ_BAD_STREAM;               // bits were taken from beyond the segment
            }
        }
    }
    return MJ_OK;
}

// ---- one segment among many lanes ("A frame without restart intervals") -------------------------------
// A frame without DRI is ONE segment.  Its bytes [begin, end) are cut into nsub subsequences of sp bytes, one lane each.  Lane 0
// knows where it starts; every other lane guesses (its first byte, unit 0, index 0), decodes without storing to the end of its
// subsequence and hands the state it arrived in to the next lane, which starts over from it; Huffman codes self-synchronise, so
// after a few rounds nothing changes any more (lane i is right after round i at the latest).  A scan over the lanes' block
// counts and DC walks then gives every lane its first block and its predictors, and one more pass stores the coefficients.
// k_mjpeg_huff_split (k_mjpeg.hip) runs this with a workgroup; tests/mjpeg_split_host.cpp replays it with loops.
static const uint32_t MJ_SPLIT_LANES = 1024;     // the most subsequences a frame is cut into
static const int MJ_SPLIT_MIN = 8, MJ_SPLIT_MAX = 65536, MJ_SPLIT_DEFAULT = 64;   // subsequence bytes a caller may ask for

// -> the number of subsequences of a segment of len bytes when S bytes are asked for (0: no splitting), *sp: their size
MJ_HD uint32_t mjpeg_split_plan(uint32_t len, uint32_t S, uint32_t* sp)
{
    *sp = 0;
    if (S == 0 || len == 0) return 0;
    const uint32_t least = (len + MJ_SPLIT_LANES - 1) / MJ_SPLIT_LANES;
    *sp = S > least ? S : least;
    return (len + *sp - 1) / *sp;
}
MJ_HD uint32_t mjpeg_split_lanes(uint32_t nsub) { uint32_t l = 64; while (l < nsub && l < MJ_SPLIT_LANES) l *= 2; return l; }

// The decoder's state at a symbol boundary, as lanes hand it over.  pos / bit: the next unconsumed bit in the RAW stream, never
// inside the 00 of an FF 00 pair (the pair counts as the byte at its FF); u: the block inside the MCU (luma blocks first);
// k: 0 = a DC symbol is next, 1..63 = an AC symbol for that zigzag index.  The DC predictors are not part of it.  It is
// canonical: whatever a reader buffered ahead does not show, so two lanes that reach the same boundary hold equal states.
struct MjpegState { uint32_t pos, w; };          // w: bit | u << 3 | k << 6 | 1 << 12; every invalid state is {~0, 0}
MJ_HD MjpegState mjpeg_state(uint32_t pos, uint32_t bit, uint32_t u, uint32_t k)
{
    MjpegState s; s.pos = pos; s.w = bit | (u << 3) | (k << 6) | (1u << 12); return s;
}
MJ_HD MjpegState mjpeg_state_invalid() { MjpegState s; s.pos = 0xFFFFFFFFu; s.w = 0; return s; }
MJ_HD bool mjpeg_state_same(MjpegState a, MjpegState b) { return a.pos == b.pos && a.w == b.w; }

// mjpeg_fill reads ahead, so (p, n) of a reader says nothing another reader could start from.  This reader notes for each of the
// eight bytes its buffer can hold whether it came from the stream (`real`; not a zero supplied past the end) and whether it was
// an FF 00 pair (`pair`), newest byte in bit 0; the raw position of the next unconsumed bit follows from p.  At a marker or a
// lone 0xFF it stays where it is (mjpeg_fill jumps to the end; both supply zeros from there on).
struct MjpegSplitBits : MjpegBits { uint32_t real, pair; };

MJ_HD void mjpeg_split_fill(MjpegSplitBits& b)
{
    while (b.n <= 56) {
        uint32_t byte = 0, real = 0, pair = 0;
        if (b.p < b.end) {
            byte = b.s[b.p];
            if (byte == 0xFF) {
                if (b.p + 1 < b.end && b.s[b.p + 1] == 0) { b.p += 2; real = 1; pair = 1; }
                else { byte = 0; ++b.fed; }
            } else { ++b.p; real = 1; }
        } else ++b.fed;
        b.acc = (b.acc << 8) | byte;
        b.n += 8;
        b.real = (b.real << 1) | real;
        b.pair = (b.pair << 1) | pair;
    }
}
MJ_HD void mjpeg_split_open(MjpegSplitBits& b, const uint8_t* s, uint32_t pos, uint32_t bit, uint32_t end)
{
    b.s = s; b.p = pos < end ? pos : end; b.end = end; b.acc = 0; b.n = 0; b.fed = 0; b.real = 0; b.pair = 0;
    mjpeg_split_fill(b);
    b.n -= (int)bit;
}
// where the next unconsumed bit is.  Only asked while no bit from beyond the data was consumed (fed * 8 <= n): the byte that
// holds the bit is then a real one, or it is the first one past the data and the answer is (p, 0).
MJ_HD void mjpeg_split_pos(const MjpegSplitBits& b, uint32_t* pos, uint32_t* bit)
{
    if (b.n <= 0) { *pos = b.p; *bit = 0; return; }
    const uint32_t mask = (2u << ((b.n - 1) >> 3)) - 1u;       // the bytes not yet consumed to their end
    *pos = b.p - (uint32_t)__builtin_popcount(b.real & mask) - (uint32_t)__builtin_popcount(b.pair & mask);
    *bit = (uint32_t)(8 - (b.n & 7)) & 7u;
}

// where lane i > 0 tries first: the first byte of its subsequence, one further where that is the 00 of an FF 00 pair
MJ_HD MjpegState mjpeg_split_guess(const uint8_t* s, uint32_t begin, uint32_t end, uint32_t sp, uint32_t i)
{
    uint32_t p = begin + i * sp;
    if (i == 0) return mjpeg_state(begin, 0, 0, 0);
    if (p < end && s[p] == 0 && s[p - 1] == 0xFF) ++p;
    return mjpeg_state(p, 0, 0, 0);
}

// The DC predictor after a block is  min(max(pred + diff, -32768), 32767).  Maps  x -> min(max(x + a, l), h)  are closed under
// composition, so a lane records one per component for the blocks it decoded and a scan composes them.  Only x in
// [-32768, 32767] is ever asked for and l, h stay inside that range: once |a| >= 65536 the map is constant, it is stored as
// l = h, and a is pinned, so a never leaves 18 bits however many blocks are composed.
struct MjpegClamp { int a, l, h; };
MJ_HD MjpegClamp mjpeg_clamp_id() { MjpegClamp f; f.a = 0; f.l = -32768; f.h = 32767; return f; }
MJ_HD int mjpeg_clamp_to(int v, int l, int h) { return v < l ? l : (v > h ? h : v); }
MJ_HD MjpegClamp mjpeg_clamp_then(MjpegClamp f, MjpegClamp g)      // x -> g(f(x))
{
    MjpegClamp r;
    r.a = f.a + g.a;
    r.l = mjpeg_clamp_to(f.l + g.a, g.l, g.h);
    r.h = mjpeg_clamp_to(f.h + g.a, g.l, g.h);
    if (r.a >= 65536) { r.a = 65536; r.l = r.h; }
    else if (r.a <= -65536) { r.a = -65536; r.h = r.l; }
    return r;
}
MJ_HD int mjpeg_clamp_apply(MjpegClamp f, int x) { return mjpeg_clamp_to(x + f.a, f.l, f.h); }

// what a pass of a lane leaves: the state it stopped in, the blocks whose DC symbol it decoded and its DC walk per component
struct MjpegLane { MjpegState out; uint32_t blocks; MjpegClamp m0, m1, m2; };
MJ_HD void mjpeg_lane_clear(MjpegLane& r)
{
    r.out = mjpeg_state_invalid(); r.blocks = 0; r.m0 = r.m1 = r.m2 = mjpeg_clamp_id();
}

// One pass of one lane over s[.., end) from the state `in`, up to the first symbol boundary at or beyond byte `stop` (the last
// lane: ~0u, it never gets there).
//   coef == NULL   nothing is stored; *res gets the exit state and the counts.  Nothing is an error here.  A bit pattern that is
//                  no code is passed over one bit further and an index past 63 ends the block: a lane that guessed wrong
//                  meets both all the time, and it has to go on to fall into step (an invalid exit would be handed down the
//                  lanes and undo what they had found; measured, the rounds then equal the lanes).  From a true state the
//                  same two are real damage: what lies behind them is never used, because the final pass of this lane refuses
//                  the frame there.  A bit taken from beyond the data makes the exit state invalid; an invalid `in` gives an
//                  invalid exit with zero counts.  Returns MJ_OK.
//   coef != NULL   the final pass: `in` is the true state, ord the number of DC symbols before it (the block a DC symbol
//                  opens), pred0..2 the predictors.  Coefficients are stored as mjpeg_decode_segment stores them.  The pass also
//                  ends where a DC symbol would open block nblocks: the frame is complete, as the one-lane loop judges it.
//                  Returns MJ_BAD_STREAM for what that loop refuses (met inside a block below nblocks), else MJ_OK.
// The one-lane loop looks for bits taken from beyond the data at the end of a block; here every symbol boundary looks.  The
// count of such bits never falls, so both refuse the same streams.
MJ_HD int mjpeg_split_pass(const uint8_t* stream, const MjpegDesc& d, uint32_t end, const MjpegHuff* tabs, const uint8_t* zz,
                           MjpegState in, uint32_t stop, uint32_t ord, int pred0, int pred1, int pred2, int16_t* coef, MjpegLane* res)
{
    const bool store = coef != nullptr;
    mjpeg_lane_clear(*res);
    if (!(in.w >> 12)) return MJ_OK;
    const uint32_t hv = (uint32_t)(d.hs * d.vs), units = hv + (uint32_t)d.ncomp - 1u, nblocks = mjpeg_frame_blocks(d);
    uint32_t u = (in.w >> 3) & 7u, k = (in.w >> 6) & 63u;
    if (u >= units) return store ? MJ_BAD_STREAM : MJ_OK;
    MjpegSplitBits b;
    mjpeg_split_open(b, stream, in.pos, in.w & 7u, end);
    int c = u < hv ? 0 : (int)(u - hv) + 1;
    int16_t* out = nullptr;
    if (store && k > 0) {                                   // inside a block that an earlier lane opened
        if (ord == 0) return MJ_BAD_STREAM;                 // cannot happen: lane 0 starts with a DC symbol
        if (ord - 1 >= nblocks) return MJ_OK;               // what lies behind the frame's last block is not looked at
    }
    // every symbol takes at least one bit and the pass ends once a bit from beyond the data was taken: a counted loop
    for (uint64_t left = 8ull * (end - b.p) + 72; left; --left) {
        if (b.fed * 8 > b.n) return store ? MJ_BAD_STREAM : MJ_OK;
        if (store && k == 0 && ord >= nblocks) return MJ_OK;
        uint32_t pos, bit;
        mjpeg_split_pos(b, &pos, &bit);
        if (pos >= stop) { res->out = mjpeg_state(pos, bit, u, k); return MJ_OK; }
        if (store && !out) {                                // the block this lane is in: ord (a DC symbol is next) or ord - 1
            const uint32_t o = k == 0 ? ord : ord - 1, mcu = o / units, my = mcu / (uint32_t)d.mcux, mx = mcu - my * (uint32_t)d.mcux;
            const uint32_t h = c == 0 ? (uint32_t)d.hs : 1u, v = c == 0 ? (uint32_t)d.vs : 1u, j = c == 0 ? u / h : 0u, i = c == 0 ? u - j * h : 0u;
            const uint32_t blk = mjpeg_comp_first_block(d, c) + (my * v + j) * (uint32_t)d.mcux * h + mx * h + i;
            if (blk >= nblocks || o % units != u) return MJ_BAD_STREAM;      // cannot happen from a true state; the guard stays
            out = coef + (size_t)blk * 64;
        }
        const uint8_t* q = d.qt[c];
        mjpeg_split_fill(b);
        if (k == 0) {
            const int s = mjpeg_symbol(b, tabs + 2 * c);
            if (s < 0 || s > 15) {
                if (store) return MJ_BAD_STREAM;
                b.n -= 1;                                   // a guess went wrong: one bit further, and on
                continue;
            }
            const int diff = mjpeg_extend(mjpeg_take(b, s), s);
            if (store) {
                int pred = (c == 0 ? pred0 : (c == 1 ? pred1 : pred2)) + diff;
                pred = pred < -32768 ? -32768 : (pred > 32767 ? 32767 : pred);
                if (c == 0) pred0 = pred; else if (c == 1) pred1 = pred; else pred2 = pred;
                const int16_t dcv = mjpeg_sat16(pred * (int)q[0]);
                if (dcv) out[0] = dcv;
                ++ord;
            } else {
                MjpegClamp g = mjpeg_clamp_id();
                g.a = diff;
                if (c == 0) res->m0 = mjpeg_clamp_then(res->m0, g);
                else if (c == 1) res->m1 = mjpeg_clamp_then(res->m1, g);
                else res->m2 = mjpeg_clamp_then(res->m2, g);
                ++res->blocks;
            }
            k = 1;
        } else {
            const int rs = mjpeg_symbol(b, tabs + 2 * c + 1);
            if (rs < 0) {
                if (store) return MJ_BAD_STREAM;
                b.n -= 1;
                continue;
            }
            const uint32_t r = (uint32_t)rs >> 4;
            const int s = rs & 15;
            if (s == 0) k = r != 15 ? 64 : k + 16;
            else {
                k += r;
                if (k > 63) {
                    if (store) return MJ_BAD_STREAM;
                    k = 64;                                 // a guess went wrong: the block ends here, and on
                } else {
                    const int16_t val = mjpeg_sat16(mjpeg_extend(mjpeg_take(b, s), s) * (int)q[k]);
                    if (store && val) out[zz[k] & 63] = val;
                    ++k;
                }
            }
        }
        if (k >= 64) {                                      // the block is complete
            k = 0;
            u = u + 1 == units ? 0 : u + 1;
            c = u < hv ? 0 : (int)(u - hv) + 1;
            out = nullptr;
        }
    }
    return store ? MJ_BAD_STREAM : MJ_OK;                   // cannot happen: the count above is an upper bound
}

// ---- host only (plain functions: a HIP compilation treats them as host code): headers -> MjpegDesc + segment table --------------------------------------------------------------------
struct MjpegInfo {       // rtdm_mjpeg_info of include/rtdm.h, field for field
    int width, height, components, h_samp, v_samp, restart_interval, segments, has_dht;
};

// The JPEG standard's typical Huffman tables (ITU-T T.81 Annex K.3.3), for frames that carry no DHT (the usual camera form).
// tests/golden/mjpeg_aux.npz holds the DHT payload of a stream libjpeg wrote with them; test_mjpeg_cpu.py compares.
static const uint8_t MJ_STD_BITS[4][16] = {
    {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},        // DC luminance
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},     // AC luminance
    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},        // DC chrominance
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};    // AC chrominance
static const uint8_t MJ_STD_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t MJ_STD_AC_LUMA[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const uint8_t MJ_STD_AC_CHROMA[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// the standard table of class cls (0 DC, 1 AC) and id (0 luminance, 1 chrominance); false for another id
inline bool mjpeg_std_table(int cls, int id, uint8_t bits[16], uint8_t vals[256])
{
    if (id < 0 || id > 1) return false;
    memcpy(bits, MJ_STD_BITS[2 * id + cls], 16);
    memset(vals, 0, 256);
    if (cls == 0) memcpy(vals, MJ_STD_DC_VALS, sizeof MJ_STD_DC_VALS);
    else memcpy(vals, id == 0 ? MJ_STD_AC_LUMA : MJ_STD_AC_CHROMA, 162);
    return true;
}

// code counts that fit: at every length the codes used so far leave room, and there are at most 256 symbols
inline bool mjpeg_check_counts(const uint8_t bits[16])
{
    int code = 0, total = 0;
    for (int l = 1; l <= 16; ++l) {
        code += bits[l - 1]; total += bits[l - 1];
        if (code > (1 << l)) return false;
        code <<= 1;
    }
    return total <= 256;
}

// Parses the headers of the frame at s[0, len), finds its entropy segments (memchr for 0xFF: the host, not the device, finds
// the RSTn markers) and fills *d (stream_off and seg_first are left 0: the caller places the frame) and *info.  segs / max_segs:
// where the segment table goes; both may be 0 / NULL when only *info is wanted.  Everything the decoder refuses is refused here.
inline int mjpeg_parse(const uint8_t* s, size_t len, MjpegDesc* d, MjpegInfo* info, MjpegSeg* segs, size_t max_segs)
{
    if (!s || !d || !info) return MJ_NULL;
    memset(d, 0, sizeof *d);
    memset(info, 0, sizeof *info);
    if (len < 4 || s[0] != 0xFF || s[1] != 0xD8) return MJ_BAD_STREAM;
    uint8_t qt[4][64], hbits[2][4][16], hvals[2][4][256], comp_q[3] = {0, 0, 0};
    bool have_q[4] = {false, false, false, false}, have_h[2][4] = {{false, false, false, false}, {false, false, false, false}};
    bool have_sof = false, have_dht = false;
    int comp_id[3] = {0, 0, 0};
    size_t p = 2;
    for (;;) {
        if (p + 1 >= len || s[p] != 0xFF) return MJ_BAD_STREAM;
        while (p < len && s[p] == 0xFF) ++p;                       // fill bytes before a marker
        if (p >= len) return MJ_BAD_STREAM;
        const int m = s[p++];
        if (m == 0xD9) return MJ_BAD_STREAM;                        // EOI before any scan: no SOS
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;        // markers without a length
        if (m == 0x00 || m == 0xD8) return MJ_BAD_STREAM;
        if (p + 2 > len) return MJ_BAD_STREAM;
        const size_t L = ((size_t)s[p] << 8) | s[p + 1];
        if (L < 2 || p + L > len) return MJ_BAD_STREAM;             // a segment that runs past len
        const uint8_t* g = s + p + 2;
        const size_t n = L - 2;
        if (m == 0xC0) {
            if (have_sof || n < 6) return MJ_BAD_STREAM;
            if (g[0] != 8) return MJ_UNSUPPORTED;                   // 12-bit samples
            d->H = (g[1] << 8) | g[2]; d->W = (g[3] << 8) | g[4]; d->ncomp = g[5];
            if (d->ncomp != 1 && d->ncomp != 3) return MJ_UNSUPPORTED;
            if (n < 6 + 3 * (size_t)d->ncomp) return MJ_BAD_STREAM;
            if (d->H == 0) return MJ_UNSUPPORTED;                   // height deferred to a DNL marker
            if (d->W == 0) return MJ_BAD_STREAM;
            for (int c = 0; c < d->ncomp; ++c) {
                comp_id[c] = g[6 + 3 * c];
                const int h = g[7 + 3 * c] >> 4, v = g[7 + 3 * c] & 15;
                comp_q[c] = g[8 + 3 * c];
                if (comp_q[c] > 3 || h < 1 || h > 4 || v < 1 || v > 4) return MJ_BAD_STREAM;
                if (d->ncomp == 1) { d->hs = d->vs = 1; }           // a one-component scan is never interleaved: factors do not matter
                else if (c == 0) {
                    if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2))) return MJ_UNSUPPORTED;
                    d->hs = h; d->vs = v;
                } else if (h != 1 || v != 1) return MJ_UNSUPPORTED;
            }
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {
            return MJ_UNSUPPORTED;                                  // extended, progressive, lossless, arithmetic (SOFn, JPG, DAC)
        } else if (m == 0xDB) {
            size_t q = 0;
            while (q < n) {
                if (g[q] >> 4) return MJ_UNSUPPORTED;               // 16-bit quantisers
                const int id = g[q] & 15;
                if (id > 3 || q + 65 > n) return MJ_BAD_STREAM;
                memcpy(qt[id], g + q + 1, 64);
                have_q[id] = true;
                q += 65;
            }
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < n) {
                const int cls = g[q] >> 4, id = g[q] & 15;
                if (cls > 1 || id > 3 || q + 17 > n || !mjpeg_check_counts(g + q + 1)) return MJ_BAD_STREAM;
                size_t cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += g[q + 1 + i];
                if (q + 17 + cnt > n) return MJ_BAD_STREAM;
                memcpy(hbits[cls][id], g + q + 1, 16);
                memset(hvals[cls][id], 0, 256);
                memcpy(hvals[cls][id], g + q + 17, cnt);
                if (cls == 0) for (size_t i = 0; i < cnt; ++i) if (g[q + 17 + i] > 15) return MJ_BAD_STREAM;
                have_h[cls][id] = true;
                q += 17 + cnt;
            }
            have_dht = true;
        } else if (m == 0xDD) {
            if (n < 2) return MJ_BAD_STREAM;
            d->ri = (g[0] << 8) | g[1];
        } else if (m == 0xDA) {
            if (!have_sof || n < 1) return MJ_BAD_STREAM;
            const int ns = g[0];
            if (ns != d->ncomp) return ns >= 1 && ns <= 4 ? MJ_UNSUPPORTED : MJ_BAD_STREAM;   // a frame in several scans
            if (n < 1 + 2 * (size_t)ns + 3) return MJ_BAD_STREAM;
            for (int c = 0; c < ns; ++c) {
                if (g[1 + 2 * c] != comp_id[c]) return MJ_UNSUPPORTED;
                const int td = g[2 + 2 * c] >> 4, ta = g[2 + 2 * c] & 15;
                if (td > 3 || ta > 3) return MJ_BAD_STREAM;
                if (!have_q[comp_q[c]]) return MJ_BAD_STREAM;       // a scan that names a missing table
                memcpy(d->qt[c], qt[comp_q[c]], 64);
                const int sel[2] = {td, ta};
                for (int cls = 0; cls < 2; ++cls) {
                    uint8_t* bits = d->bits[2 * c + cls];
                    uint8_t* vals = d->vals[2 * c + cls];
                    if (have_h[cls][sel[cls]]) { memcpy(bits, hbits[cls][sel[cls]], 16); memcpy(vals, hvals[cls][sel[cls]], 256); }
                    else if (have_dht || !mjpeg_std_table(cls, sel[cls], bits, vals)) return MJ_BAD_STREAM;
                }
            }
            const uint8_t* t = g + 1 + 2 * ns;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return MJ_UNSUPPORTED;   // spectral selection / successive approximation
            p += L;
            break;
        }
        p += L;
    }
    d->mcux = (d->W + 8 * d->hs - 1) / (8 * d->hs);
    d->mcuy = (d->H + 8 * d->vs - 1) / (8 * d->vs);
    const size_t total = (size_t)d->mcux * d->mcuy;
    const size_t want = d->ri > 0 ? (total + d->ri - 1) / d->ri : 1;
    // the entropy data: stuffed bytes are skipped, RSTn splits, EOI ends
    size_t nseg = 0, start = p, q = p;
    for (;;) {
        const uint8_t* f = q < len ? (const uint8_t*)memchr(s + q, 0xFF, len - q) : NULL;
        if (!f || (size_t)(f - s) + 1 >= len) return MJ_BAD_STREAM;            // no EOI
        q = (size_t)(f - s);
        const int m = s[q + 1];
        if (m == 0x00) { q += 2; continue; }
        if (m == 0xFF) { q += 1; continue; }
        if ((m >= 0xD0 && m <= 0xD7) || m == 0xD9) {
            if (nseg >= want) return MJ_BAD_STREAM;                            // more restart markers than the frame has intervals
            if (segs) {
                if (nseg >= max_segs) return MJ_BAD_SIZE;
                segs[nseg].begin = (uint32_t)start; segs[nseg].end = (uint32_t)q;
            }
            ++nseg;
            q += 2;
            start = q;
            if (m == 0xD9) break;
            continue;
        }
        // another scan or its tables: a frame in more than one scan; anything else does not belong here
        return (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD || m == 0xDC) ? MJ_UNSUPPORTED : MJ_BAD_STREAM;
    }
    if (nseg != want) return MJ_BAD_STREAM;
    if (q > 0xFFFFFFFFu) return MJ_BAD_SIZE;
    info->restart_interval = d->ri;
    d->stream_len = (uint32_t)q;       // bytes after EOI are not part of the frame
    d->nseg = (uint32_t)nseg;
    if (d->ri <= 0 || (size_t)d->ri > total) d->ri = (int32_t)total;
    info->width = d->W; info->height = d->H; info->components = d->ncomp; info->h_samp = d->hs; info->v_samp = d->vs;
    info->segments = (int)nseg; info->has_dht = have_dht ? 1 : 0;
    return MJ_OK;
}
}  // namespace rtdm
#endif  // RTDM_MJPEG_H_
