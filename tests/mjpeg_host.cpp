// Host build of the MJPEG entropy decoder (rt-depth-map_amd/csrc/rtdm_mjpeg.h): test_mjpeg_cpu.py compiles this file with g++,
// once plainly and once with -fsanitize=address,undefined, and runs it before any stream is given to a GPU.
//     mjpeg_host STREAM OUT [POS VAL]...
// decodes STREAM -- or, for every POS VAL pair, a copy of it whose byte POS is VAL -- and appends one record per decode to OUT:
// int32 parse status, int32 decode status, int32 blocks, then blocks * 64 int16 coefficients.  Stream and coefficient buffers
// are heap blocks of exactly their size, so that the address sanitizer sees any step outside them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rtdm_mjpeg.h"

using namespace rtdm;

static int run(const std::vector<uint8_t>& bytes, FILE* out)
{
    uint8_t* s = (uint8_t*)malloc(bytes.size());
    memcpy(s, bytes.data(), bytes.size());
    MjpegDesc d;
    MjpegInfo info;
    int32_t head[3] = {0, 0, 0};
    head[0] = mjpeg_parse(s, bytes.size(), &d, &info, nullptr, 0);
    if (head[0] != MJ_OK) { fwrite(head, 4, 3, out); free(s); return 0; }
    MjpegSeg* segs = (MjpegSeg*)malloc(sizeof(MjpegSeg) * d.nseg);
    if (mjpeg_parse(s, bytes.size(), &d, &info, segs, d.nseg) != MJ_OK) return 2;
    // what the device gets: the frame's own bytes, SOI .. EOI, and not one more
    uint8_t* frame = (uint8_t*)malloc(d.stream_len);
    memcpy(frame, s, d.stream_len);
    const uint32_t nb = mjpeg_frame_blocks(d);
    int16_t* coef = (int16_t*)calloc((size_t)nb * 64, sizeof(int16_t));
    MjpegHuff* tabs = (MjpegHuff*)malloc(sizeof(MjpegHuff) * 6);
    for (int t = 0; t < 2 * d.ncomp; ++t) mjpeg_build_table(d.bits[t], d.vals[t], &tabs[t]);
    for (uint32_t i = 0; i < d.nseg; ++i) {
        const int st = mjpeg_decode_segment(frame, d, segs[i], i, tabs, MJ_ZIGZAG, coef);
        if (st != MJ_OK) head[1] = st;
    }
    head[2] = (int32_t)nb;
    fwrite(head, 4, 3, out);
    fwrite(coef, sizeof(int16_t), (size_t)nb * 64, out);
    free(tabs); free(coef); free(frame); free(segs); free(s);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3 || (argc - 3) % 2) { fprintf(stderr, "usage: mjpeg_host STREAM OUT [POS VAL]...\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<uint8_t> bytes;
    for (int c; (c = fgetc(in)) != EOF;) bytes.push_back((uint8_t)c);
    fclose(in);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    int rc = 0;
    if (argc == 3) rc = run(bytes, out);
    for (int i = 3; i + 1 < argc && rc == 0; i += 2) {
        std::vector<uint8_t> b = bytes;
        const size_t pos = (size_t)atol(argv[i]);
        if (pos >= b.size()) return 2;
        b[pos] = (uint8_t)atoi(argv[i + 1]);
        rc = run(b, out);
    }
    fclose(out);
    return rc;
}
