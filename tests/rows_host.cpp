// Host sweep of rtdm::copy_rows (rt-depth-map_amd/csrc/rtdm_rows.h), built by tests/test_host_rows_cpu.py with g++, plainly and
// with -fsanitize=address,undefined.  Every buffer is heap-allocated to end exactly at the last row's last byte
// ((rows - 1) * pitch + row_bytes, no trailing pitch), so that the sanitizer sees any access behind it.  The destination is
// filled with a sentinel first: payload bytes must equal a plain per-row loop, and in KEEP mode the pad bytes between the rows
// must still hold the sentinel.  Prints "ok <cases>".
#include "rtdm_rows.h"

#include <cstdio>
#include <vector>

static const unsigned char SENTINEL = 0xA5;

static size_t extent(size_t pitch, size_t row_bytes, int rows) { return rows > 0 && row_bytes ? (size_t)(rows - 1) * pitch + row_bytes : 0; }

static int one_case(int rows, size_t row_bytes, size_t dst_pitch, size_t src_pitch, rtdm::RowPad pad, unsigned seed)
{
    const size_t dn = extent(dst_pitch, row_bytes, rows), sn = extent(src_pitch, row_bytes, rows);
    // (new[] of the exact extent; a zero extent still gets a live one-byte block that nothing may touch)
    unsigned char* src = new unsigned char[sn ? sn : 1];
    unsigned char* dst = new unsigned char[dn ? dn : 1];
    unsigned char* want = new unsigned char[dn ? dn : 1];
    for (size_t i = 0; i < (sn ? sn : 1); ++i) src[i] = (unsigned char)((i * 131u + seed * 29u + 7u) % 251u);
    for (size_t i = 0; i < (dn ? dn : 1); ++i) dst[i] = want[i] = SENTINEL;
    for (int y = 0; y < rows; ++y)
        for (size_t x = 0; x < row_bytes; ++x) want[(size_t)y * dst_pitch + x] = src[(size_t)y * src_pitch + x];
    rtdm::copy_rows(dn ? dst : nullptr, dst_pitch, sn ? src : nullptr, src_pitch, row_bytes, rows, pad);
    int bad = 0;
    if (!dn && dst[0] != SENTINEL) bad = 1;
    for (size_t i = 0; i < dn; ++i) {
        const bool payload = i % dst_pitch < row_bytes;
        if (payload ? dst[i] != want[i] : (pad == rtdm::RowPad::KEEP && dst[i] != SENTINEL)) bad = 1;
    }
    if (bad)
        fprintf(stderr, "rows=%d row_bytes=%zu dst_pitch=%zu src_pitch=%zu mode=%s: wrong bytes\n", rows, row_bytes, dst_pitch, src_pitch,
                pad == rtdm::RowPad::KEEP ? "KEEP" : "OURS");
    delete[] src; delete[] dst; delete[] want;
    return bad;
}

int main()
{
    const int rows[] = {0, 1, 2, 5};
    const size_t row_bytes[] = {0, 1, 7, 16};
    const rtdm::RowPad modes[] = {rtdm::RowPad::KEEP, rtdm::RowPad::OURS};
    int cases = 0, bad = 0;
    for (int r : rows)
        for (size_t rb : row_bytes) {
            const size_t pitches[] = {rb, rb + 3, 32};
            for (size_t dp : pitches)
                for (size_t sp : pitches)
                    for (rtdm::RowPad m : modes) { bad += one_case(r, rb, dp, sp, m, (unsigned)cases); ++cases; }
        }
    if (bad) { fprintf(stderr, "%d of %d cases failed\n", bad, cases); return 1; }
    printf("ok %d\n", cases);
    return 0;
}
