// morph_bits_host.cpp -- the host side of the general morphology path's element (morph_element_bits, csrc/rtdm_kernels.h) as a
// stand-alone program, so that it can run under AddressSanitizer / UBSan: every mask lives in a heap block of exactly w * h
// bytes, so a read past it is caught.  Checks the row words, the run count and kmax against a second, naive count, and walks
// the words the way the kernel's wave 0 does (run starts by popcount, runs by carry), for every size 1..63 x 1..63.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rtdm_kernels.h"

static unsigned rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 16; }

int main()
{
    unsigned seed = 7;
    long bad = 0, masks = 0;
    for (int w = 1; w <= MORPH_MAX_SIZE; ++w) for (int h = 1; h <= MORPH_MAX_SIZE; ++h) for (int kind = 0; kind < 3; ++kind) {
        uint8_t* m = (uint8_t*)malloc((size_t)w * h);
        for (int i = 0; i < w * h; ++i) m[i] = kind == 0 ? 1 : kind == 1 ? (uint8_t)(rnd(seed) % 2 ? 255 : 0) : (uint8_t)(i % 2);
        int runs = 0, longest = 0, members = 0;
        for (int i = 0; i < h; ++i) for (int j = 0; j < w; ++j) {
            if (!m[i * w + j]) continue;
            ++members;
            if (j == 0 || !m[i * w + j - 1]) ++runs;
            int len = 1;
            while (j + len < w && m[i * w + j + len]) ++len;
            if (len > longest) longest = len;
        }
        rtdm::MorphBits b;
        memset(&b, 0xee, sizeof b);
        const bool any = rtdm::morph_element_bits(m, w, h, w - 1, 0, &b);
        int kmax = 0;
        while ((2 << kmax) <= longest) ++kmax;
        bad += any != (members > 0) || b.nruns != runs || b.kmax != kmax || b.w != w || b.h != h || b.ax != w - 1 || b.ay != 0;
        int walked = 0, starts = 0;
        for (int i = 0; i < MORPH_MAX_SIZE; ++i) {
            unsigned long long r = b.rows[i];
            if (i >= h) { bad += r != 0; continue; }
            for (int j = 0; j < 64; ++j) bad += ((r >> j) & 1) != (unsigned long long)(j < w && m[i * w + j] != 0);
            starts += __builtin_popcountll(r & ~(r << 1));
            while (r) {
                const int j1 = __builtin_ctzll(r);
                const unsigned long long t = r + (1ull << j1);
                const int L = __builtin_ctzll(t) - j1;
                bad += L < 1 || L > longest || j1 + L > w;
                ++walked;
                r &= t;
            }
        }
        bad += walked != runs || starts != runs;
        ++masks;
        free(m);
    }
    std::printf("%s: %ld failed checks over %ld masks\n", bad ? "FAILED" : "ok", bad, masks);
    return bad ? 1 : 0;
}
