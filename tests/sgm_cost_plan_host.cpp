// sgm_cost_plan_host.cpp -- prints what plan_sgm_cost (rt-depth-map_amd/csrc/rtdm_sgm_cost_plan.h) plans for the cost stage of a
// StereoSGBM call:
//     sgm_cost_plan_host <D> <H> <blockSize> <P2> <cn> <ftz> <kind> <cw> <ch> <paths> <force16>
// kind: 0 Birchfield-Tomasi, 1 census over cw x ch; force16: what rtdm_debug_sgm_cost16 was given.  One line per configuration,
// "<variant> form=. sum=. R=. records=8|24 volume=. check=. limit=. warm=. wrows=. ftz=. cw=. ch=.".  With the single argument
// "-" the configurations are read from standard input, one per line.  Includes the plan header and nothing else of the
// library: no HIP, no device, nothing to link.  tests/test_sgm_cost_plan_cpu.py.
#include "rtdm_sgm_cost_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace rtdm;

static const int NARGS = 11;

static void print_plan(const long long* v)
{
    static const char* const forms[] = {"BT8", "BT16_GRAY", "BT16_COLOUR", "CENSUS"};
    static const char* const sums[] = {"FUSED", "BOX", "BOX_ANY"};
    static const char* const vols[] = {"NONE", "PIX", "S"};
    static_assert(sizeof forms / sizeof *forms == (int)SgmCostForm::CENSUS + 1, "a name per SgmCostForm");
    static_assert(sizeof sums / sizeof *sums == (int)SgmCostSum::BOX_ANY + 1, "a name per SgmCostSum");
    static_assert(sizeof vols / sizeof *vols == (int)SgmCostVolume::S + 1, "a name per SgmCostVolume");
    const SgmCostPlan p = plan_sgm_cost((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5],
                                        SgmCostKind{(int)v[6], (int)v[7], (int)v[8]}, (int)v[9], v[10] != 0);
    printf("%s form=%s sum=%s R=%d records=%d volume=%s check=%d limit=%d warm=%d wrows=%d ftz=%d cw=%d ch=%d\n", p.variant,
           forms[(int)p.form], sums[(int)p.sum], p.R, p.colour_records ? 24 : 8, vols[(int)p.volume], (int)p.check, p.cost_limit,
           (int)p.warm, p.wrows, p.ftz, p.cw, p.ch);
}

int main(int argc, char** argv)
{
    long long v[NARGS];
    if (argc == 2 && !strcmp(argv[1], "-")) {
        char line[1024];
        while (fgets(line, sizeof line, stdin)) {
            char* s = line;
            for (int k = 0; k < NARGS; ++k) {
                char* e = nullptr;
                v[k] = strtoll(s, &e, 10);
                if (e == s) { fprintf(stderr, "a configuration has %d numbers: %s", NARGS, line); return 2; }
                s = e;
            }
            print_plan(v);
        }
        return 0;
    }
    if (argc != 1 + NARGS) {
        fprintf(stderr, "usage: %s D H blockSize P2 cn ftz kind cw ch paths force16 | %s - < configurations\n", argv[0], argv[0]);
        return 2;
    }
    for (int k = 0; k < NARGS; ++k) v[k] = atoll(argv[1 + k]);
    print_plan(v);
    return 0;
}
