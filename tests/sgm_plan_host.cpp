// sgm_plan_host.cpp -- prints what plan_sgm (rt-depth-map_amd/csrc/k_sgm.hip) plans for the path passes of a StereoSGBM call:
//     sgm_plan_host <D> <paths> <W1> <n> <s2> <sweep> <ring_words> <wide_mode> <done_dirs> <s2_pending> <swept> <cap x 12>
// cap: the SgmLimits capacities in storage order, [LAST 0 / 1][columns 1 / 2 / 4][ADD2 0 / 1]; wide_mode: what
// rtdm_debug_sgm_wide_paths was given (0, 1, 4); done_dirs / s2_pending / swept: the SgmDone of a replan (0 0 0: a whole call).
// One line per pass -- "<variant> <KIND> (<dx>,<dy>) first=. last=. s2=." and, for SWEEP, "cols=. strips=. items=. grid=.", for
// WIDE, "waves=." -- and a line "end".  With the single argument "-" the configurations are read from standard input, one
// per line.  The hooks RTDM_SGM_SWEEP, RTDM_SGM_DUAL and RTDM_SGM_SWEEP_COLS come from the environment, as in the library.
// Linked against librtdm_hip.so; touches no device (plan_sgm makes no runtime call).  tests/test_sgm_plan_cpu.py.
#include "rtdm_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace rtdm;

static const int NARGS = 23;

static void print_plan(const long long* v)
{
    SGMGeom g{};
    g.D = (int)v[0]; g.W1 = (int)v[2]; g.x0 = g.D; g.W = g.W1 + g.D; g.H = 16;
    SgmLimits lim{};
    lim.s2 = v[4] != 0; lim.sweep = v[5] != 0; lim.ring_words = (size_t)v[6];
    for (int i = 0; i < 12; ++i) (&lim.cap[0][0][0])[i] = (int)v[11 + i];
    sgm_wide_set_mode((int)v[7]);
    const SgmPlan p = plan_sgm(g, (int)v[1], (int)v[3], lim, SgmDone{(unsigned)v[8], v[9] != 0, v[10] != 0});
    static const char* const kinds[] = {"WIDE", "PATH_H", "VERT", "SWEEP", "ADD_S2", "VERT3"};
    static_assert(sizeof kinds / sizeof *kinds == (int)SgmStep::VERT3 + 1, "a name per SgmStep");
    for (int i = 0; i < p.npasses; ++i) {
        const SgmPass& q = p.pass[i];
        printf("%s %s (%d,%d) first=%d last=%d s2=%d", p.variant, kinds[(int)q.step], q.dx, q.dy, (int)q.first, (int)q.last, (int)q.s2);
        if (q.step == SgmStep::SWEEP) printf(" cols=%d strips=%d items=%d grid=%d", q.cols, q.strips, q.items, q.grid);
        if (q.step == SgmStep::WIDE) printf(" waves=%d", q.waves);
        printf("\n");
    }
    printf("end\n");
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
        fprintf(stderr, "usage: %s D paths W1 n s2 sweep ring_words wide_mode done_dirs s2_pending swept cap{12} | %s - < configurations\n", argv[0], argv[0]);
        return 2;
    }
    for (int k = 0; k < NARGS; ++k) v[k] = atoll(argv[1 + k]);
    print_plan(v);
    return 0;
}
