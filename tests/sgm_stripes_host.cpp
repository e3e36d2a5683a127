// sgm_stripes_host.cpp -- prints the row stripes of StereoSGBM's MODE_SGBM_3WAY as the launch takes them from sgm3_stripes
// (rt-depth-map_amd/csrc/rtdm_sgm_stripes.h, rule T1 of DESIGN.md section 4.21):
//     sgm_stripes_host <H> <blockSize> [<H> <blockSize> ...]
// One line per pair: "H blockSize warm_rows a0 o0 e0 a1 o1 e1 a2 o2 e2 a3 o3 e3".  Plain host code: the header needs no HIP.
// tests/test_sgm_3way_cpu.py.
#include "rtdm_sgm_stripes.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 3 || (argc - 1) % 2) { fprintf(stderr, "usage: %s H blockSize [H blockSize ...]\n", argv[0]); return 2; }
    for (int i = 1; i + 1 < argc; i += 2) {
        const int H = atoi(argv[i]), bs = atoi(argv[i + 1]);
        const rtdm::Sgm3Stripes t = rtdm::sgm3_stripes(H, bs);
        printf("%d %d %d", H, bs, rtdm::sgm3_warm_rows(bs, H));
        for (int s = 0; s < rtdm::SGM3_STRIPES; ++s) printf(" %d %d %d", t.s[s].a, t.s[s].o, t.s[s].e);
        printf("\n");
    }
    return 0;
}
