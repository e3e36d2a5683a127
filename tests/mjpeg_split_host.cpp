// Host replay of k_mjpeg_huff_split (rt-depth-map_amd/csrc/k_mjpeg.hip): the workgroup as loops over the shared functions of
// rtdm_mjpeg.h -- lanes as an inner loop, rounds as an outer loop, the handed-over states double-buffered so that a round reads
// only what the round before it wrote.  test_mjpeg_split_cpu.py compiles this file with g++, once plainly and once with
// -fsanitize=address,undefined, and holds its records against those of mjpeg_host (the one-lane loop).
//     mjpeg_split_host STREAM OUT S[,S...] [POS VAL]...
// decodes STREAM -- or, for every POS VAL pair, a copy of it whose byte POS is VAL -- with S bytes per subsequence asked for, once
// for every S of the list (all decodes of the first S, then those of the second ...), and appends one record per decode to OUT:
// int32 parse status, decode status, blocks, nsub, rounds, then blocks * 64 int16 coefficients.  nsub is 0 for a frame with restart intervals and 1 for a segment too short to cut; both take the one-lane loop
// (rounds 0).  Stream and coefficient buffers are heap blocks of exactly their size, so that the address sanitizer sees any step
// outside them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rtdm_mjpeg.h"

using namespace rtdm;

// one frame of one segment, as the workgroup decodes it -> decode status; *rounds: the rounds it took
static int split_frame(const uint8_t* frame, const MjpegDesc& d, const MjpegSeg sg, uint32_t nsub, uint32_t sp, const MjpegHuff* tabs,
                       int16_t* coef, int32_t* rounds)
{
    if ((uint32_t)d.mcux * (uint32_t)d.mcuy == 0) return MJ_BAD_STREAM;
    const uint32_t end = sg.end < d.stream_len ? sg.end : d.stream_len, begin = sg.begin < end ? sg.begin : end;
    std::vector<MjpegState> E[2] = {std::vector<MjpegState>(nsub, mjpeg_state_invalid()), std::vector<MjpegState>(nsub, mjpeg_state_invalid())};
    std::vector<MjpegState> in(nsub, mjpeg_state_invalid()), ex(nsub, mjpeg_state_invalid());
    std::vector<MjpegLane> lane(nsub);
    for (uint32_t i = 0; i < nsub; ++i) mjpeg_lane_clear(lane[i]);
    int cur = 0;
    *rounds = 0;
    for (uint32_t r = 0; r + 1 < nsub; ++r) {
        bool changed = false;
        for (uint32_t i = 0; i < nsub; ++i) {
            const MjpegState ni = r == 0 ? mjpeg_split_guess(frame, begin, end, sp, i) : (i > 0 ? E[cur][i - 1] : in[i]);
            if (r == 0 || !mjpeg_state_same(ni, in[i])) {
                in[i] = ni;
                if (i + 1 < nsub) {
                    mjpeg_split_pass(frame, d, end, tabs, MJ_ZIGZAG, ni, begin + (i + 1) * sp, 0, 0, 0, 0, nullptr, &lane[i]);
                    changed = changed || r == 0 || !mjpeg_state_same(lane[i].out, ex[i]);
                    ex[i] = lane[i].out;
                }
            }
            E[cur ^ 1][i] = ex[i];
        }
        cur ^= 1;
        ++*rounds;
        if (!changed) break;
    }
    // the exclusive scan over the lanes, then the final pass
    int st = MJ_OK;
    uint32_t ord = 0;
    MjpegClamp f0 = mjpeg_clamp_id(), f1 = f0, f2 = f0;
    for (uint32_t i = 0; i < nsub; ++i) {
        const MjpegState start = i > 0 ? E[cur][i - 1] : in[0];
        MjpegLane unused;
        const int s = mjpeg_split_pass(frame, d, end, tabs, MJ_ZIGZAG, start, i + 1 < nsub ? begin + (i + 1) * sp : 0xFFFFFFFFu, ord,
                                       mjpeg_clamp_apply(f0, 0), mjpeg_clamp_apply(f1, 0), mjpeg_clamp_apply(f2, 0), coef, &unused);
        if (s != MJ_OK) st = s;
        ord += lane[i].blocks;
        f0 = mjpeg_clamp_then(f0, lane[i].m0); f1 = mjpeg_clamp_then(f1, lane[i].m1); f2 = mjpeg_clamp_then(f2, lane[i].m2);
    }
    return st;
}

static int run(const std::vector<uint8_t>& bytes, uint32_t S, FILE* out)
{
    uint8_t* s = (uint8_t*)malloc(bytes.size());
    memcpy(s, bytes.data(), bytes.size());
    MjpegDesc d;
    MjpegInfo info;
    int32_t head[5] = {0, 0, 0, 0, 0};
    head[0] = mjpeg_parse(s, bytes.size(), &d, &info, nullptr, 0);
    if (head[0] != MJ_OK) { fwrite(head, 4, 5, out); free(s); return 0; }
    MjpegSeg* segs = (MjpegSeg*)malloc(sizeof(MjpegSeg) * d.nseg);
    if (mjpeg_parse(s, bytes.size(), &d, &info, segs, d.nseg) != MJ_OK) return 2;
    uint8_t* frame = (uint8_t*)malloc(d.stream_len);
    memcpy(frame, s, d.stream_len);
    const uint32_t nb = mjpeg_frame_blocks(d);
    int16_t* coef = (int16_t*)calloc((size_t)nb * 64, sizeof(int16_t));
    MjpegHuff* tabs = (MjpegHuff*)malloc(sizeof(MjpegHuff) * 6);
    for (int t = 0; t < 2 * d.ncomp; ++t) mjpeg_build_table(d.bits[t], d.vals[t], &tabs[t]);
    uint32_t sp = 0, nsub = 0;
    if (d.nseg == 1) {
        const uint32_t end = segs[0].end < d.stream_len ? segs[0].end : d.stream_len;
        nsub = mjpeg_split_plan(end - (segs[0].begin < end ? segs[0].begin : end), S, &sp);
    }
    if (nsub >= 2) head[1] = split_frame(frame, d, segs[0], nsub, sp, tabs, coef, &head[4]);
    else for (uint32_t i = 0; i < d.nseg; ++i) {
        const int st = mjpeg_decode_segment(frame, d, segs[i], i, tabs, MJ_ZIGZAG, coef);
        if (st != MJ_OK) head[1] = st;
    }
    head[2] = (int32_t)nb;
    head[3] = (int32_t)nsub;
    fwrite(head, 4, 5, out);
    fwrite(coef, sizeof(int16_t), (size_t)nb * 64, out);
    free(tabs); free(coef); free(frame); free(segs); free(s);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 4) % 2) { fprintf(stderr, "usage: mjpeg_split_host STREAM OUT S[,S...] [POS VAL]...\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<uint8_t> bytes;
    for (int c; (c = fgetc(in)) != EOF;) bytes.push_back((uint8_t)c);
    fclose(in);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    int rc = 0;
    for (const char* list = argv[3]; *list && rc == 0;) {
        char* next;
        const uint32_t S = (uint32_t)strtoul(list, &next, 10);
        if (next == list) return 2;
        list = *next == ',' ? next + 1 : next;
        if (argc == 4) rc = run(bytes, S, out);
        for (int i = 4; i + 1 < argc && rc == 0; i += 2) {
            std::vector<uint8_t> b = bytes;
            const size_t pos = (size_t)atol(argv[i]);
            if (pos >= b.size()) return 2;
            b[pos] = (uint8_t)atoi(argv[i + 1]);
            rc = run(b, S, out);
        }
    }
    fclose(out);
    return rc;
}
