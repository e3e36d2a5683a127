// morph_core_host.cpp -- HIPMorphCore::setElement / setOperation (what host/mf-hip.cpp forwards to) from plain C++.
//   morph_core_host      : the refusals, which need no device; without a device every valid setting reports the create status
//   morph_core_host gpu  : CLOSE with CROSS 5x3, two iterations, on a small gray frame against the loops below
#include <cstdio>
#include <cstring>
#include <vector>

#include "hip_matcher_core.h"

static std::vector<uint8_t> pass(const std::vector<uint8_t>& s, int W, int H, bool dilate)
{
    std::vector<uint8_t> d(s.size());
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        int acc = dilate ? 0 : 255;
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 5; ++j) {
            if (i != 1 && j != 2) continue;                       // CROSS 5x3, anchor (2, 1)
            const int yy = y + i - 1, xx = x + j - 2;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const int v = s[(size_t)yy * W + xx];
            if (dilate ? v > acc : v < acc) acc = v;
        }
        d[(size_t)y * W + x] = (uint8_t)acc;
    }
    return d;
}

int main(int argc, char** argv)
{
    const int W = 75, H = 41;
    rtdm::HIPMorphCore core(W, H, 8);
    std::printf("bad shape: %d\n", core.setElement(3, 5, 5));
    std::printf("bad size: %d\n", core.setElement(RTDM_MORPH_RECT, 0, 5));
    std::printf("large: %d\n", core.setElement(RTDM_MORPH_RECT, 64, 5));
    const int e = core.setElement(RTDM_MORPH_CROSS, 5, 3), o = core.setOperation(RTDM_MORPH_CLOSE, 2);
    std::printf("set: %d %d\n", e, o);
    if (argc < 2 || std::strcmp(argv[1], "gpu")) return 0;
    if (e || o) return 1;
    std::printf("hitmiss: %d iterations: %d\n", core.setOperation(7), core.setOperation(RTDM_MORPH_CLOSE, 17));
    std::vector<uint8_t> src((size_t)W * H), got(src.size());
    unsigned r = 12345;
    for (size_t i = 0; i < src.size(); ++i) { r = r * 1664525u + 1013904223u; src[i] = (uint8_t)((i % W) * 2 + (r >> 27)); }
    if (core.run(src.data(), W, got.data(), W, H, W)) return 2;
    const std::vector<uint8_t> want = pass(pass(pass(pass(src, W, H, true), W, H, true), W, H, false), W, H, false);
    std::printf("close: %s, changed: %s\n", got == want ? "equal" : "DIFFERENT", want != src ? "yes" : "no");
    return got == want && want != src ? 0 : 3;
}
