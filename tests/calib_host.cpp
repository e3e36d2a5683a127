// calib_host.cpp -- stand-alone host program around rt-depth-map_amd/csrc/rtdm_calib.h for tests/test_calib_cpu.py (built by
// tests/calib_hostbuild.py with g++, plainly and with -fsanitize=address,undefined).  Doubles are printed as hex floats.
//   calib_host parse   <intrinsics> <extrinsics>                    status, mask, every value read
//   calib_host rectify <intrinsics> <extrinsics> <flags> <alpha> [<new_width> <new_height>]
//   calib_host raw     <numbers> <flags> <alpha> [<new_width> <new_height>]     numbers: 58 doubles (M1 D1 M2 D2 R T) + W H
//   calib_host nulls                                                 the statuses of calls with null pointers
//   calib_host fuzz    <intrinsics> <extrinsics>                     every truncation and single-byte replacement of <extrinsics>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rtdm_calib.h"

using namespace rtdm;

static void row(const char* name, const double* v, int n)
{
    printf("%s", name);
    for (int i = 0; i < n; ++i) printf(" %a", v[i]);
    printf("\n");
}

static void print_calib(const Calib& c)
{
    row("M1", c.M1, 9); row("D1", c.D1, 14); row("M2", c.M2, 9); row("D2", c.D2, 14); row("R", c.R, 9); row("T", c.T, 3);
    printf("size %d %d\n", c.width, c.height);
}

static void print_rect(const Rectification& r)
{
    row("R1", r.R1, 9); row("R2", r.R2, 9); row("P1", r.P1, 12); row("P2", r.P2, 12); row("Q", r.Q, 16);
    printf("ROI1 %d %d %d %d\nROI2 %d %d %d %d\n", r.roi1.x, r.roi1.y, r.roi1.width, r.roi1.height, r.roi2.x, r.roi2.y,
           r.roi2.width, r.roi2.height);
}

static int rectify_and_print(const Calib& c, int argc, char** argv, int at)
{
    const int flags = atoi(argv[at]);
    const double alpha = strtod(argv[at + 1], nullptr);
    const int nw = argc > at + 3 ? atoi(argv[at + 2]) : 0, nh = argc > at + 3 ? atoi(argv[at + 3]) : 0;
    Rectification r;
    memset(&r, 0, sizeof r);
    const int st = calib_stereo_rectify(&c, flags, alpha, nw, nh, &r);
    printf("status %d\n", st);
    if (st == CB_OK) print_rect(r);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "parse" && argc == 4) {
        Calib c; Rectification r; unsigned mask = 0;
        memset(&c, 0, sizeof c); memset(&r, 0, sizeof r);
        const int st = calib_load(argv[2], argv[3], &c, &r, &mask);
        printf("status %d\nmask %u\n", st, mask);
        if (st == CB_OK) { print_calib(c); print_rect(r); }
        return 0;
    }
    if (mode == "rectify" && argc >= 6) {
        Calib c;
        const int st = calib_load(argv[2], argv[3], &c, nullptr, nullptr);
        if (st) { printf("status %d\n", st); return 0; }
        return rectify_and_print(c, argc, argv, 4);
    }
    if (mode == "raw" && argc >= 5) {
        std::string text;
        if (calib_read_file(argv[2], &text)) return 2;
        double v[60];
        const char* p = text.c_str();
        for (int i = 0; i < 60; ++i) {
            char* e = nullptr;
            v[i] = strtod(p, &e);
            if (e == p) return 2;
            p = e;
        }
        Calib c;
        memcpy(c.M1, v, 9 * 8); memcpy(c.D1, v + 9, 14 * 8); memcpy(c.M2, v + 23, 9 * 8); memcpy(c.D2, v + 32, 14 * 8);
        memcpy(c.R, v + 46, 9 * 8); memcpy(c.T, v + 55, 3 * 8);
        c.width = (int)v[58]; c.height = (int)v[59];
        return rectify_and_print(c, argc, argv, 3);
    }
    if (mode == "nulls") {
        Calib c; Rectification r; double ir[9];
        memset(&c, 0, sizeof c);
        printf("load %d %d %d\n", calib_load(nullptr, "x", &c, &r, nullptr), calib_load("x", nullptr, &c, &r, nullptr),
               calib_load("x", "x", nullptr, &r, nullptr));
        printf("rectify %d %d\n", calib_stereo_rectify(nullptr, 0, 0.0, 0, 0, &r), calib_stereo_rectify(&c, 0, 0.0, 0, 0, nullptr));
        printf("map %d %d\n", calib_rectmap_check(nullptr, c.D1, c.R, r.P1, 4, 4, ir), calib_rectmap_check(c.M1, c.D1, c.R, nullptr, 4, 4, ir));
        printf("missing %d\n", calib_load("/nonexistent/intrinsics.yml", "/nonexistent/extrinsics.yml", &c, &r, nullptr));
        return 0;
    }
    if (mode == "fuzz" && argc == 4) {
        std::string a, b;
        if (calib_read_file(argv[2], &a) || calib_read_file(argv[3], &b)) return 2;
        long counts[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cases = 0, rectified = 0;
        Calib c; Rectification r, o; unsigned mask;
        for (size_t cut = 0; cut <= b.size(); ++cut) {
            // an exact-size heap copy, so that a read past the end is a report and not a silent success
            char* buf = (char*)malloc(cut ? cut : 1);
            if (!buf) return 2;
            memcpy(buf, b.data(), cut);
            const int st = calib_parse_pair(a.data(), a.size(), buf, cut, &c, &r, &mask);
            free(buf);
            if (st > 0 || st < -8) return 3;
            ++counts[-st]; ++cases;
            if (st == CB_OK && calib_stereo_rectify(&c, CB_ZERO_DISPARITY, -1.0, 0, 0, &o) == CB_OK) ++rectified;
        }
        const char repl[4] = {'[', ']', ',', '\0'};
        char* buf = (char*)malloc(b.size());
        if (!buf) return 2;
        for (size_t at = 0; at < b.size(); ++at)
            for (int k = 0; k < 4; ++k) {
                memcpy(buf, b.data(), b.size());
                buf[at] = repl[k];
                const int st = calib_parse_pair(a.data(), a.size(), buf, b.size(), &c, &r, &mask);
                if (st > 0 || st < -8) return 3;
                ++counts[-st]; ++cases;
                if (st == CB_OK) {
                    const int s2 = calib_stereo_rectify(&c, CB_ZERO_DISPARITY, -1.0, 0, 0, &o);
                    if (s2 > 0 || s2 < -8) return 3;
                    if (s2 == CB_OK) ++rectified;
                }
            }
        free(buf);
        printf("cases %ld\nrectified %ld\n", cases, rectified);
        for (int i = 0; i < 9; ++i) printf("status %d %ld\n", -i, counts[i]);
        return 0;
    }
    return 2;
}
