// rtdm_calib.h -- rectification from the reference's calibration files (main.cpp:53-98): a reader for the subset of OpenCV
// FileStorage YAML 1.0 that intrinsics.yml / extrinsics.yml use, cv::stereoRectify restated as rules C1-C9 (DESIGN.md
// section 4.13) and the host half of initUndistortRectifyMap (the inverse of P[:3,:3] R).  Plain C++11: no HIP, no allocation
// beyond std::string / std::vector, so tests/calib_host.cpp compiles it alone with g++, under the host sanitizers too.
// Double arithmetic in the written order; float wherever a rule says float32.  The build must not fuse multiplies with adds.
#ifndef RTDM_CALIB_H_
#define RTDM_CALIB_H_

#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rtdm {

// status values of include/rtdm.h (this header stands alone so that the host harness needs nothing else)
enum { CB_OK = 0, CB_BAD_PARAM = -1, CB_BAD_SIZE = -2, CB_UNSUPPORTED = -6, CB_NULL = -7, CB_BAD_STREAM = -8 };
// presence bits of the optional keys (RTDM_CALIB_HAS_* in rtdm.h)
enum { CB_HAS_WIDTH = 1, CB_HAS_HEIGHT = 2, CB_HAS_ROI1 = 4, CB_HAS_ROI2 = 8, CB_HAS_R1 = 16, CB_HAS_R2 = 32, CB_HAS_P1 = 64,
       CB_HAS_P2 = 128, CB_HAS_Q = 256 };
static const int CB_ZERO_DISPARITY = 1024;          // cv::CALIB_ZERO_DISPARITY
static const size_t CB_MAX_FILE = 1u << 20;         // a calibration file is a few KB; anything longer is refused
static const int CB_MAX_DATA = 64;                  // entries of the largest matrix that is kept (Q: 16)

// the layouts of rtdm_calib / rtdm_rectification / rtdm_region (api_rectify.hip asserts the sizes)
struct CalibRegion { int x, y, width, height; };
struct Calib { double M1[9], D1[14], M2[9], D2[14], R[9], T[3]; int width, height; };
struct Rectification { double R1[9], R2[9], P1[12], P2[12], Q[16]; CalibRegion roi1, roi2; };

// ---- the YAML reader ---------------------------------------------------------------------------------------------------
// Top level: `%YAML:1.0`, `---` and `#` lines, then `name: value` with the name in column 0.  value: `!!opencv-matrix` followed
// by the indented rows / cols / dt / data fields, `[ a, b, ... ]` (integers) or a scalar.  Keys this project does not know are
// skipped, whatever their value holds.  The text is walked by a cursor that never passes `end`; numbers go through strtod on
// a NUL-terminated copy.
struct CalibCursor { const char* p; const char* end; };

inline bool cb_is_name(char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_'; }
inline void cb_skip_blank(CalibCursor& c) { while (c.p < c.end && (*c.p == ' ' || *c.p == '\t' || *c.p == '\r')) ++c.p; }
inline void cb_skip_space(CalibCursor& c) { while (c.p < c.end && (*c.p == ' ' || *c.p == '\t' || *c.p == '\r' || *c.p == '\n')) ++c.p; }
inline void cb_skip_line(CalibCursor& c) { while (c.p < c.end && *c.p != '\n') ++c.p; if (c.p < c.end) ++c.p; }
inline bool cb_at(const CalibCursor& c, const char* word)
{
    const size_t n = strlen(word);
    return (size_t)(c.end - c.p) >= n && memcmp(c.p, word, n) == 0;
}
inline std::string cb_name(CalibCursor& c)
{
    const char* b = c.p;
    while (c.p < c.end && cb_is_name(*c.p)) ++c.p;
    return std::string(b, c.p);
}
// one number; the buffer behind the cursor ends in a NUL, so strtod stops inside it
inline bool cb_number(CalibCursor& c, double* v)
{
    if (c.p >= c.end) return false;
    char* e = nullptr;
    *v = strtod(c.p, &e);
    if (e == c.p || e > c.end) return false;
    c.p = e;
    return true;
}
// `[ v, v, ... ]` from the cursor (which stands on the bracket): up to cap values are stored, all are counted
inline int cb_list(CalibCursor& c, double* out, int cap, int* count)
{
    if (c.p >= c.end || *c.p != '[') return CB_BAD_STREAM;
    ++c.p;
    int n = 0;
    cb_skip_space(c);
    if (c.p < c.end && *c.p == ']') { ++c.p; *count = 0; return CB_OK; }
    for (;;) {
        cb_skip_space(c);
        double v;
        if (!cb_number(c, &v)) return CB_BAD_STREAM;
        if (n < cap) out[n] = v;
        if (n < 0x7fffffff) ++n;
        cb_skip_space(c);
        if (c.p >= c.end) return CB_BAD_STREAM;
        if (*c.p == ',') { ++c.p; continue; }
        if (*c.p == ']') { ++c.p; break; }
        return CB_BAD_STREAM;
    }
    *count = n;
    return CB_OK;
}

struct CalibMatrix { int rows, cols, count; char dt; double data[CB_MAX_DATA]; };

// the four fields behind `!!opencv-matrix`, in any order, until all four have been seen
inline int cb_matrix(CalibCursor& c, CalibMatrix* m)
{
    m->rows = m->cols = m->count = -1; m->dt = 0;
    int seen = 0;
    while (seen != 15) {
        cb_skip_space(c);
        const std::string f = cb_name(c);
        if (f.empty() || c.p >= c.end || *c.p != ':') return CB_BAD_STREAM;
        ++c.p;
        cb_skip_space(c);
        if (f == "rows" || f == "cols") {
            double v;
            if (!cb_number(c, &v)) return CB_BAD_STREAM;
            if (!(v >= 0 && v <= 1e6) || v != floor(v)) return CB_BAD_PARAM;
            (f == "rows" ? m->rows : m->cols) = (int)v;
            seen |= f == "rows" ? 1 : 2;
        } else if (f == "dt") {
            const std::string t = cb_name(c);
            if (t.empty()) return CB_BAD_STREAM;
            m->dt = t.size() == 1 ? t[0] : '?';
            seen |= 4;
        } else if (f == "data") {
            const int st = cb_list(c, m->data, CB_MAX_DATA, &m->count);
            if (st) return st;
            seen |= 8;
        } else {
            return CB_BAD_STREAM;
        }
    }
    return CB_OK;
}

inline bool cb_finite(const double* v, int n)
{
    for (int i = 0; i < n; ++i) if (!(fabs(v[i]) <= 1.7976931348623157e308)) return false;
    return true;
}

struct CalibKeys { unsigned required; unsigned optional; };   // required: bit 0..5 = M1 D1 M2 D2 R T

// Parses one file's text into cal / stored and adds what it found to keys.  stored may be null.
inline int calib_parse(const char* text, size_t len, Calib* cal, Rectification* stored, CalibKeys* keys)
{
    if (!text || !cal || !keys) return CB_NULL;
    if (len > CB_MAX_FILE) return CB_BAD_STREAM;
    const std::string buf(text, len);                 // c_str(): the same bytes and a NUL behind them
    CalibCursor c{buf.c_str(), buf.c_str() + len};
    Rectification scratch;
    Rectification* rs = stored ? stored : &scratch;
    for (;;) {
        cb_skip_space(c);
        if (c.p >= c.end) break;
        if (*c.p == '%' || *c.p == '#' || cb_at(c, "---") || cb_at(c, "...")) { cb_skip_line(c); continue; }
        const std::string key = cb_name(c);
        if (key.empty() || c.p >= c.end || *c.p != ':') return CB_BAD_STREAM;
        ++c.p;
        cb_skip_blank(c);
        if (cb_at(c, "!!opencv-matrix")) {
            c.p += strlen("!!opencv-matrix");
            CalibMatrix m;
            const int st = cb_matrix(c, &m);
            if (st) return st;
            double* dst = nullptr; int rows = 0, cols = 0; unsigned req = 0, opt = 0;
            if (key == "M1") { dst = cal->M1; rows = cols = 3; req = 1; }
            else if (key == "D1") { dst = cal->D1; req = 2; }
            else if (key == "M2") { dst = cal->M2; rows = cols = 3; req = 4; }
            else if (key == "D2") { dst = cal->D2; req = 8; }
            else if (key == "R") { dst = cal->R; rows = cols = 3; req = 16; }
            else if (key == "T") { dst = cal->T; req = 32; }
            else if (key == "R1") { dst = rs->R1; rows = cols = 3; opt = CB_HAS_R1; }
            else if (key == "R2") { dst = rs->R2; rows = cols = 3; opt = CB_HAS_R2; }
            else if (key == "P1") { dst = rs->P1; rows = 3; cols = 4; opt = CB_HAS_P1; }
            else if (key == "P2") { dst = rs->P2; rows = 3; cols = 4; opt = CB_HAS_P2; }
            else if (key == "Q") { dst = rs->Q; rows = cols = 4; opt = CB_HAS_Q; }
            if (!dst) continue;                                      // a matrix of somebody else's
            if (m.dt != 'd') return CB_BAD_PARAM;
            if ((long long)m.rows * m.cols != m.count) return CB_BAD_PARAM;
            int n = rows * cols;
            if (req == 2 || req == 8) {                              // D: a row or a column of 4, 5, 8, 12 or 14
                n = m.count;
                if ((m.rows != 1 && m.cols != 1) || (n != 4 && n != 5 && n != 8 && n != 12 && n != 14)) return CB_BAD_PARAM;
                for (int i = 0; i < 14; ++i) dst[i] = 0.0;
            } else if (req == 32) {                                  // T: 3 x 1 or 1 x 3
                n = 3;
                if (m.count != 3 || (m.rows != 1 && m.cols != 1)) return CB_BAD_PARAM;
            } else if (m.rows != rows || m.cols != cols) {
                return CB_BAD_PARAM;
            }
            if (!cb_finite(m.data, n)) return CB_BAD_PARAM;
            for (int i = 0; i < n; ++i) dst[i] = m.data[i];
            keys->required |= req; keys->optional |= opt;
        } else if (c.p < c.end && *c.p == '[') {
            double v[4]; int n = 0;
            const int st = cb_list(c, v, 4, &n);
            if (st) return st;
            if (key != "ROI1" && key != "ROI2") continue;
            if (n != 4) return CB_BAD_PARAM;
            for (int i = 0; i < 4; ++i) if (!(fabs(v[i]) <= 1e9) || v[i] != floor(v[i])) return CB_BAD_PARAM;
            CalibRegion* r = key == "ROI1" ? &rs->roi1 : &rs->roi2;
            r->x = (int)v[0]; r->y = (int)v[1]; r->width = (int)v[2]; r->height = (int)v[3];
            keys->optional |= key == "ROI1" ? CB_HAS_ROI1 : CB_HAS_ROI2;
        } else if (c.p >= c.end || *c.p == '\n') {
            // a nested mapping of somebody else's: its lines are indented
            if (key == "Width" || key == "Height" || key == "ROI1" || key == "ROI2") return CB_BAD_STREAM;
            cb_skip_line(c);
            while (c.p < c.end && (*c.p == ' ' || *c.p == '\t')) cb_skip_line(c);
        } else if (key == "Width" || key == "Height") {
            double v;
            if (!cb_number(c, &v)) return CB_BAD_STREAM;
            cb_skip_blank(c);
            if (c.p < c.end && *c.p != '\n') return CB_BAD_STREAM;
            if (!(v >= 1 && v <= 32767) || v != floor(v)) return CB_BAD_PARAM;
            (key == "Width" ? cal->width : cal->height) = (int)v;
            keys->optional |= key == "Width" ? CB_HAS_WIDTH : CB_HAS_HEIGHT;
        } else {
            cb_skip_line(c);                                         // a scalar of somebody else's
        }
    }
    return CB_OK;
}

// the two files as texts (main.cpp:61-78 reads M1 D1 M2 D2 Width Height from the first, ROI1 ROI2 R T from the second; here
// either file may hold any key, the later one wins)
inline int calib_parse_pair(const char* intr, size_t intr_len, const char* extr, size_t extr_len, Calib* cal,
                            Rectification* stored, unsigned* stored_mask)
{
    if (!intr || !extr || !cal) return CB_NULL;
    Calib c;
    memset(&c, 0, sizeof c);
    Rectification r;
    memset(&r, 0, sizeof r);
    CalibKeys keys{0, 0};
    int st = calib_parse(intr, intr_len, &c, &r, &keys);
    if (st == CB_OK) st = calib_parse(extr, extr_len, &c, &r, &keys);
    if (st) return st;
    if (keys.required != 63) return CB_BAD_PARAM;
    *cal = c;
    if (stored) *stored = r;
    if (stored_mask) *stored_mask = keys.optional;
    return CB_OK;
}

inline int calib_read_file(const char* path, std::string* out)
{
    FILE* f = fopen(path, "rb");
    if (!f) return CB_BAD_STREAM;
    std::vector<char> chunk(65536);
    out->clear();
    size_t n;
    while ((n = fread(chunk.data(), 1, chunk.size(), f)) > 0) {
        out->append(chunk.data(), n);
        if (out->size() > CB_MAX_FILE) { fclose(f); return CB_BAD_STREAM; }
    }
    const bool bad = ferror(f) != 0;
    fclose(f);
    return bad ? CB_BAD_STREAM : CB_OK;
}

inline int calib_load(const char* intrinsics_path, const char* extrinsics_path, Calib* cal, Rectification* stored,
                      unsigned* stored_mask)
{
    if (!intrinsics_path || !extrinsics_path || !cal) return CB_NULL;
    std::string a, b;
    int st = calib_read_file(intrinsics_path, &a);
    if (st == CB_OK) st = calib_read_file(extrinsics_path, &b);
    if (st) return st;
    return calib_parse_pair(a.data(), a.size(), b.data(), b.size(), cal, stored, stored_mask);
}

// ---- stereoRectify: rules C1-C9 ----------------------------------------------------------------------------------------
inline void cb_matmul3(const double* A, const double* B, double* O)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
inline void cb_matvec3(const double* A, const double* v, double* o)
{
    for (int i = 0; i < 3; ++i) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}

// C1, matrix -> rotation vector, closed form
inline int cb_rodrigues_vec(const double* R, double* r)
{
    const double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : c < -1. ? -1. : c;
    const double theta = acos(c);
    if (s < 1e-5) {
        if (!(c > 0)) return CB_UNSUPPORTED;                         // a rotation by (nearly) pi: the axis is not in r
        r[0] = r[1] = r[2] = 0.0;
        return CB_OK;
    }
    double vth = 1 / (2 * s);
    vth *= theta;
    r[0] = rx * vth; r[1] = ry * vth; r[2] = rz * vth;
    return CB_OK;
}

// C1, rotation vector -> matrix: R = cos(theta) I + (1 - cos(theta)) r r^T + sin(theta) [r]x
inline void cb_rodrigues_mat(const double* rv, double* R)
{
    double x = rv[0], y = rv[1], z = rv[2];
    const double theta = sqrt(x * x + y * y + z * z);
    if (theta < 2.220446049250313e-16) {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1. - c, it = 1. / theta;
    x = x * it; y = y * it; z = z * it;
    const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
    const double rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    for (int i = 0; i < 9; ++i) R[i] = c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i] + s * rx[i];
}

// C8: one float point through the inverse of the 12-term model (five fixed-point iterations), then RR (null: identity)
inline void cb_undistort_point(float u, float v, const double* M, const double* k, const double* RR, float* ox, float* oy)
{
    const double fx = M[0], fy = M[4], cx = M[2], cy = M[5];
    const double ifx = 1. / fx, ify = 1. / fy;
    double x = ((double)u - cx) * ifx, y = ((double)v - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; ++j) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        const double dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* r = RR ? RR : I3;
    const double xx = r[0] * x + r[1] * y + r[2], yy = r[3] * x + r[4] * y + r[5];
    const double ww = 1. / (r[6] * x + r[7] * y + r[8]);
    *ox = (float)(xx * ww);
    *oy = (float)(yy * ww);
}

struct CalibRectF { float x, y, w, h; };

// C7: the inner and the outer rectangle of the undistorted 9 x 9 grid
inline void cb_rectangles(const double* M, const double* D, const double* R, const double* P, int W, int H, CalibRectF* inner,
                          CalibRectF* outer)
{
    const double A[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    double RR[9];
    cb_matmul3(A, R, RR);
    float ix0 = -3.402823466e38f, ix1 = 3.402823466e38f, iy0 = -3.402823466e38f, iy1 = 3.402823466e38f;
    float ox0 = 3.402823466e38f, ox1 = -3.402823466e38f, oy0 = 3.402823466e38f, oy1 = -3.402823466e38f;
    for (int y = 0; y < 9; ++y)
        for (int x = 0; x < 9; ++x) {
            const float gx = (float)x * (float)W / 8.0f, gy = (float)y * (float)H / 8.0f;
            float px, py;
            cb_undistort_point(gx, gy, M, D, RR, &px, &py);
            ox0 = px < ox0 ? px : ox0; ox1 = px > ox1 ? px : ox1;
            oy0 = py < oy0 ? py : oy0; oy1 = py > oy1 ? py : oy1;
            if (x == 0) ix0 = px > ix0 ? px : ix0;
            if (x == 8) ix1 = px < ix1 ? px : ix1;
            if (y == 0) iy0 = py > iy0 ? py : iy0;
            if (y == 8) iy1 = py < iy1 ? py : iy1;
        }
    const float iw = ix1 - ix0, ih = iy1 - iy0, ow = ox1 - ox0, oh = oy1 - oy0;
    *inner = CalibRectF{ix0, iy0, iw, ih};
    *outer = CalibRectF{ox0, oy0, ow, oh};
}

// C6: the four side ratios of one rectangle; x + w and y + h are float sums
inline void cb_sides(const CalibRectF& r, double cx0, double cy0, double cx, double cy, int W, int H, double* out)
{
    const float xr = r.x + r.w, yb = r.y + r.h;
    out[0] = cx / (cx0 - r.x);
    out[1] = cy / (cy0 - r.y);
    out[2] = (W - cx) / (xr - cx0);
    out[3] = (H - cy) / (yb - cy0);
}

// C9: Rect(ceil, ceil, floor, floor) & Rect(0, 0, W, H)
inline int cb_roi(const CalibRectF& r, double cx0, double cy0, double cx, double cy, double s, int W, int H, CalibRegion* out)
{
    const double a[4] = {ceil((r.x - cx0) * s + cx), ceil((r.y - cy0) * s + cy), floor(r.w * s), floor(r.h * s)};
    for (int i = 0; i < 4; ++i) if (!(fabs(a[i]) <= 1e9)) return CB_BAD_PARAM;
    const int rx = (int)a[0], ry = (int)a[1], rw = (int)a[2], rh = (int)a[3];
    const int x0 = rx > 0 ? rx : 0, y0 = ry > 0 ? ry : 0;
    const int x1 = rx + rw < W ? rx + rw : W, y1 = ry + rh < H ? ry + rh : H;
    if (x1 <= x0 || y1 <= y0) *out = CalibRegion{0, 0, 0, 0};
    else *out = CalibRegion{x0, y0, x1 - x0, y1 - y0};
    return CB_OK;
}

inline int calib_stereo_rectify(const Calib* cal, int flags, double alpha, int new_width, int new_height, Rectification* out)
{
    if (!cal || !out) return CB_NULL;
    const int W = cal->width, H = cal->height;
    if (W <= 0 || H <= 0 || W > 32767 || H > 32767 || new_width < 0 || new_height < 0) return CB_BAD_SIZE;
    if (flags != 0 && flags != CB_ZERO_DISPARITY) return CB_BAD_PARAM;
    if (!(alpha == alpha)) return CB_BAD_PARAM;
    if (!cb_finite(cal->M1, 9) || !cb_finite(cal->D1, 14) || !cb_finite(cal->M2, 9) || !cb_finite(cal->D2, 14) ||
        !cb_finite(cal->R, 9) || !cb_finite(cal->T, 3))
        return CB_BAD_PARAM;
    if (cal->M1[0] == 0 || cal->M1[4] == 0 || cal->M2[0] == 0 || cal->M2[4] == 0) return CB_BAD_PARAM;
    // scope limits: the new image size is the image size (the reference's call), no tilt
    if ((long long)new_width * new_height != 0 && (new_width != W || new_height != H)) return CB_UNSUPPORTED;
    if (cal->D1[12] != 0 || cal->D1[13] != 0 || cal->D2[12] != 0 || cal->D2[13] != 0) return CB_UNSUPPORTED;
    // R is a rotation: max row sum of |R^T R - I| <= 1e-6, determinant > 0
    const double* R = cal->R;
    for (int i = 0; i < 3; ++i) {
        double row = 0;
        for (int j = 0; j < 3; ++j) row += fabs(R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - (i == j ? 1.0 : 0.0));
        if (!(row <= 1e-6)) return CB_BAD_PARAM;
    }
    if (!(R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]) > 0))
        return CB_BAD_PARAM;

    // C1
    double om[3], r_r[9], t[3];
    int st = cb_rodrigues_vec(R, om);
    if (st) return st;
    for (int i = 0; i < 3; ++i) om[i] = om[i] * -0.5;
    cb_rodrigues_mat(om, r_r);
    cb_matvec3(r_r, cal->T, t);
    // C2
    const int idx = fabs(t[0]) > fabs(t[1]) ? 0 : 1;
    const double c = t[idx], nt = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    if (!(nt > 0) || c == 0) return CB_BAD_PARAM;
    double uu[3] = {0, 0, 0};
    uu[idx] = c > 0 ? 1 : -1;
    double ww[3] = {t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]};
    const double nw = sqrt(ww[0] * ww[0] + ww[1] * ww[1] + ww[2] * ww[2]);
    if (nw > 0.0) {
        const double sc = acos(fabs(c) / nt) / nw;
        for (int i = 0; i < 3; ++i) ww[i] = ww[i] * sc;
    }
    double wR[9], r_rT[9], Rk[2][9];
    cb_rodrigues_mat(ww, wR);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r_rT[3 * i + j] = r_r[3 * j + i];
    cb_matmul3(wR, r_rT, Rk[0]);
    cb_matmul3(wR, r_r, Rk[1]);
    cb_matvec3(Rk[1], cal->T, t);
    if (t[idx] == 0) return CB_BAD_PARAM;
    // C3
    const double* M[2] = {cal->M1, cal->M2};
    const double* D[2] = {cal->D1, cal->D2};
    double fc_new = 1.7976931348623157e308;
    for (int k = 0; k < 2; ++k) {
        double fc = M[k][4 * (idx ^ 1)];
        if (D[k][0] < 0) fc *= 1 + D[k][0] * (W * W + H * H) / (4 * fc * fc);
        fc_new = fc < fc_new ? fc : fc_new;
    }
    // C4
    double cc[2][2];
    for (int k = 0; k < 2; ++k) {
        double sx = 0, sy = 0;
        for (int i = 0; i < 4; ++i) {
            const float u = (float)((i % 2) * (W - 1)), v = (float)((i / 2) * (H - 1));
            float px, py;
            cb_undistort_point(u, v, M[k], D[k], nullptr, &px, &py);
            const double X = px, Y = py, Z = 1.0;
            const double* r = Rk[k];
            double x = r[0] * X + r[1] * Y + r[2] * Z, y = r[3] * X + r[4] * Y + r[5] * Z, z = r[6] * X + r[7] * Y + r[8] * Z;
            z = z ? 1. / z : 1;
            x *= z; y *= z;
            sx += (double)(float)(x * fc_new);
            sy += (double)(float)(y * fc_new);
        }
        cc[k][0] = (W - 1) / 2.0 - sx * 0.25;
        cc[k][1] = (H - 1) / 2.0 - sy * 0.25;
    }
    // C5
    if (flags & CB_ZERO_DISPARITY) {
        cc[0][0] = cc[1][0] = (cc[0][0] + cc[1][0]) * 0.5;
        cc[0][1] = cc[1][1] = (cc[0][1] + cc[1][1]) * 0.5;
    } else if (idx == 0) {
        cc[0][1] = cc[1][1] = (cc[0][1] + cc[1][1]) * 0.5;
    } else {
        cc[0][0] = cc[1][0] = (cc[0][0] + cc[1][0]) * 0.5;
    }
    double P[2][12];
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < 12; ++i) P[k][i] = 0.0;
        P[k][0] = P[k][5] = fc_new;
        P[k][2] = cc[k][0]; P[k][6] = cc[k][1]; P[k][10] = 1.0;
    }
    P[1][4 * idx + 3] = t[idx] * fc_new;
    // C6, C7
    alpha = alpha < 1. ? alpha : 1.;
    CalibRectF inner[2], outer[2];
    for (int k = 0; k < 2; ++k) cb_rectangles(M[k], D[k], Rk[k], P[k], W, H, &inner[k], &outer[k]);
    double c1[2][2];
    for (int k = 0; k < 2; ++k) { c1[k][0] = W * cc[k][0] / W; c1[k][1] = H * cc[k][1] / H; }
    double s = 1.;
    if (alpha >= 0) {
        double s0 = -1.7976931348623157e308, s1 = 1.7976931348623157e308, v[4];
        for (int k = 0; k < 2; ++k) {
            cb_sides(inner[k], cc[k][0], cc[k][1], c1[k][0], c1[k][1], W, H, v);
            for (int i = 0; i < 4; ++i) s0 = v[i] > s0 ? v[i] : s0;
            cb_sides(outer[k], cc[k][0], cc[k][1], c1[k][0], c1[k][1], W, H, v);
            for (int i = 0; i < 4; ++i) s1 = v[i] < s1 ? v[i] : s1;
        }
        s = s0 * (1 - alpha) + s1 * alpha;
    }
    fc_new *= s;
    for (int k = 0; k < 2; ++k) { P[k][0] = P[k][5] = fc_new; P[k][2] = c1[k][0]; P[k][6] = c1[k][1]; }
    P[1][4 * idx + 3] = s * P[1][4 * idx + 3];
    // C9
    Rectification o;
    memset(&o, 0, sizeof o);
    st = cb_roi(inner[0], cc[0][0], cc[0][1], c1[0][0], c1[0][1], s, W, H, &o.roi1);
    if (st == CB_OK) st = cb_roi(inner[1], cc[1][0], cc[1][1], c1[1][0], c1[1][1], s, W, H, &o.roi2);
    if (st) return st;
    for (int i = 0; i < 9; ++i) { o.R1[i] = Rk[0][i]; o.R2[i] = Rk[1][i]; }
    for (int i = 0; i < 12; ++i) { o.P1[i] = P[0][i]; o.P2[i] = P[1][i]; }
    o.Q[0] = o.Q[5] = 1.0;
    o.Q[3] = -c1[0][0]; o.Q[7] = -c1[0][1]; o.Q[11] = fc_new;
    o.Q[14] = -1. / t[idx];
    o.Q[15] = (c1[0][idx] - c1[1][idx]) / t[idx];
    if (!cb_finite(o.R1, 9) || !cb_finite(o.R2, 9) || !cb_finite(o.P1, 12) || !cb_finite(o.P2, 12) || !cb_finite(o.Q, 16))
        return CB_BAD_PARAM;
    *out = o;
    return CB_OK;
}

// ---- the host half of initUndistortRectifyMap ----------------------------------------------------------------------------
// ir = (P[:3,:3] R)^-1 by cofactors, in the order of orc_init_undistort_rectify_map.  CB_BAD_PARAM for a zero determinant.
inline int calib_rectmap_inverse(const double* R, const double* P, double* ir)
{
    double a[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) a[3 * r + c] = P[4 * r] * R[c] + P[4 * r + 1] * R[3 + c] + P[4 * r + 2] * R[6 + c];
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c0 + a[1] * c1 + a[2] * c2;
    if (det == 0.0 || !(det == det)) return CB_BAD_PARAM;
    const double id = 1.0 / det;
    ir[0] = c0 * id; ir[1] = (a[2] * a[7] - a[1] * a[8]) * id; ir[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    ir[3] = c1 * id; ir[4] = (a[0] * a[8] - a[2] * a[6]) * id; ir[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    ir[6] = c2 * id; ir[7] = (a[1] * a[6] - a[0] * a[7]) * id; ir[8] = (a[0] * a[4] - a[1] * a[3]) * id;
    return CB_OK;
}

// what rtdm_undistort_rectify_map checks before any device use
inline int calib_rectmap_check(const double* M, const double* D, const double* R, const double* P, int width, int height,
                               double* ir)
{
    if (!M || !D || !R || !P) return CB_NULL;
    if (width <= 0 || height <= 0 || width > 32767 || height > 32767) return CB_BAD_SIZE;
    if (!cb_finite(M, 9) || !cb_finite(D, 14) || !cb_finite(R, 9) || !cb_finite(P, 12)) return CB_BAD_PARAM;
    if (D[12] != 0 || D[13] != 0) return CB_UNSUPPORTED;
    return calib_rectmap_inverse(R, P, ir);
}

}  // namespace rtdm
#endif  // RTDM_CALIB_H_
