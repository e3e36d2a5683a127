// k_wls.hip -- the disparity post-filter after the matcher (estimator.cpp:57-70, ENABLE_POST_FILTER): the weighted-least-
// squares filter of cv::ximgproc, restated as rules W1-W8 (CPU restatement tests/wls_ref.py).
//
//   k_wls_rowmm    W3, row half: min / max / count of the valid values of dL and dR in a (2r+1) row window
//   k_wls_conf     W3 column half + W4: the two discontinuity maps, the left-right check, the confidence C and the two
//                  right-hand sides (C dL, C) of W7, one workgroup per ROI row
//   k_wls_rhs      use_confidence = 0: right-hand sides (dL, 1)
//   k_wls_weights  W5: the horizontal and vertical neighbour weights of the guide, once per frame
//   k_wls_solve    W6: (I + lambda L) u = f on every row or column segment of the ROI, both right-hand sides at once
//   k_wls_final    W7 / W8: F1 / F2, rint, saturation, invalid value outside the ROI, optional float and confidence planes
//
// All arithmetic of the solve is fp32; nothing is summed with atomics, so a run is bitwise repeatable.
#include "rtdm_kernels.h"

#include <algorithm>

namespace rtdm {

// ---- W3 row half ---------------------------------------------------------------------------------------------------
// One workgroup per (row, frame); both maps' rows are staged in LDS (int16, 2 W elements).
__global__ __launch_bounds__(256) void k_wls_rowmm(WlsDisp dl, WlsDisp dr, int W, int r, int invL, int invR, WlsMM* mmL,
                                                   WlsMM* mmR, size_t pitch, size_t frame)
{
    extern __shared__ int16_t srow[];
    const int y = blockIdx.x, f = blockIdx.y;
    const int16_t* pl = dl.base + (size_t)f * dl.frame_e + (size_t)y * dl.pitch_e;
    const int16_t* pr = dr.base + (size_t)f * dr.frame_e + (size_t)y * dr.pitch_e;
    for (int x = threadIdx.x; x < W; x += blockDim.x) { srow[x] = pl[x]; srow[W + x] = pr[x]; }
    __syncthreads();
    WlsMM* ol = mmL + (size_t)f * frame + (size_t)y * pitch;
    WlsMM* orr = mmR + (size_t)f * frame + (size_t)y * pitch;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const int x0 = max(0, x - r), x1 = min(W - 1, x + r);
        int mnL = 32767, mxL = -32768, cL = 0, mnR = 32767, mxR = -32768, cR = 0;
        for (int k = x0; k <= x1; ++k) {
            const int a = srow[k], b = srow[W + k];
            if (a != invL) { mnL = min(mnL, a); mxL = max(mxL, a); ++cL; }
            if (b != invR) { mnR = min(mnR, b); mxR = max(mxR, b); ++cR; }
        }
        ol[x] = WlsMM{(int16_t)mnL, (int16_t)mxL, (int16_t)cL, 0};
        orr[x] = WlsMM{(int16_t)mnR, (int16_t)mxR, (int16_t)cR, 0};
    }
}

// ---- W3 column half + W4 ---------------------------------------------------------------------------------------------
// One workgroup per (ROI row, frame).  disc = 1 unless the window holds two or more valid values whose range exceeds T.
// discL / discR of the whole row go to LDS (2 W bytes): the check reads discR at x' = x - dL/16 anywhere in the row.
__global__ __launch_bounds__(256) void k_wls_conf(WlsDisp dl, WlsDisp dr, const WlsMM* mmL, const WlsMM* mmR, int W, int H,
                                                  WlsGeom g, int r, int T, int invL, int invR, size_t pitch, size_t frame,
                                                  uint8_t* conf, float2* F)
{
    extern __shared__ uint8_t sdisc[];
    const int y = g.y0 + blockIdx.x, f = blockIdx.y;
    const int ya = max(0, y - r), yb = min(H - 1, y + r);
    const WlsMM* bl = mmL + (size_t)f * frame;
    const WlsMM* br = mmR + (size_t)f * frame;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        int mnL = 32767, mxL = -32768, cL = 0, mnR = 32767, mxR = -32768, cR = 0;
        for (int yy = ya; yy <= yb; ++yy) {
            const WlsMM a = bl[(size_t)yy * pitch + x], b = br[(size_t)yy * pitch + x];
            mnL = min(mnL, (int)a.mn); mxL = max(mxL, (int)a.mx); cL += a.cnt;
            mnR = min(mnR, (int)b.mn); mxR = max(mxR, (int)b.mx); cR += b.cnt;
        }
        sdisc[x] = (cL >= 2 && mxL - mnL > T) ? 0 : 1;
        sdisc[W + x] = (cR >= 2 && mxR - mnR > T) ? 0 : 1;
    }
    __syncthreads();
    const int16_t* pl = dl.base + (size_t)f * dl.frame_e + (size_t)y * dl.pitch_e;
    const int16_t* pr = dr.base + (size_t)f * dr.frame_e + (size_t)y * dr.pitch_e;
    uint8_t* oc = conf + (size_t)f * frame + (size_t)y * pitch;
    float2* of = F + (size_t)f * frame + (size_t)y * pitch;
    for (int x = g.x0 + threadIdx.x; x < g.x1; x += blockDim.x) {
        const int d = pl[x];
        int c = 0;
        if (d != invL) {
            const int xp = x - d / 16;                 // C++ division truncates toward zero, as W4 asks
            if (xp >= 0 && xp < W) {
                const int e = pr[xp];
                if (e != invR && abs(d + e) <= T) c = 255 * sdisc[x] * sdisc[W + xp];
            }
        }
        oc[x] = (uint8_t)c;
        of[x] = make_float2(c ? (float)(c * d) : 0.0f, (float)c);
    }
}

__global__ __launch_bounds__(256) void k_wls_rhs(WlsDisp dl, WlsGeom g, size_t pitch, size_t frame, float2* F)
{
    const int rw = g.x1 - g.x0;
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= rw * (g.y1 - g.y0)) return;
    const int y = g.y0 + i / rw, x = g.x0 + i % rw;
    F[(size_t)f * frame + (size_t)y * pitch + x] = make_float2((float)dl.base[(size_t)f * dl.frame_e + (size_t)y * dl.pitch_e + x], 1.0f);
}

// ---- W5 ------------------------------------------------------------------------------------------------------------------
// wh(y, x): weight between (y, x-1) and (y, x); wv(y, x): between (y-1, x) and (y, x); 0 on the ROI's first column / row (no
// coupling across the ROI edge).  The LUT (3 * 255^2 + 1 floats) is gathered from L2.
template <int CN>
__global__ __launch_bounds__(256) void k_wls_weights(WlsGuide G, WlsGeom g, const float* lut, size_t pitch, size_t frame,
                                                     float* wh, float* wv)
{
    const int rw = g.x1 - g.x0;
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= rw * (g.y1 - g.y0)) return;
    const int y = g.y0 + i / rw, x = g.x0 + i % rw;
    const uint8_t* p = G.base + (size_t)f * G.frame + (size_t)y * G.pitch + (size_t)x * CN;
    float a = 0.0f, b = 0.0f;
    if (x > g.x0) {
        int s = 0;
#pragma unroll
        for (int c = 0; c < CN; ++c) { const int t = (int)p[c] - (int)p[c - CN]; s += t * t; }
        a = lut[s];
    }
    if (y > g.y0) {
        int s = 0;
#pragma unroll
        for (int c = 0; c < CN; ++c) { const int t = (int)p[c] - (int)p[(ptrdiff_t)c - (ptrdiff_t)G.pitch]; s += t * t; }
        b = lut[s];
    }
    const size_t o = (size_t)f * frame + (size_t)y * pitch + x;
    wh[o] = a; wv[o] = b;
}

// ---- W6: one pass of (I + lambda L) u = f over every line (row or column segment of the ROI) -------------------------------
// Partitioned solve.  A wave holds 64 / NCH lines, NCH lanes per line; lane k owns the chunk [k CH, k CH + m) of its line.
//  1. Forward elimination of the chunk's interior [s, e-1) with u(s-1) kept as an unknown L (the spike y') and u(e-1) as an
//     unknown R: the interior solution is u_j = X_j + Y_j L + Z_j R.  (c', d1', d2', y') of every interior element go to LDS,
//     lane-private (element j at [j * 64 + lane]: no bank conflicts, no barrier).
//  2. A backward scan yields the expression of the chunk's first element; the row e-1 then gives one equation in
//     U(k-1), U(k), U(k+1) (U = last unknown of a chunk): a tridiagonal reduced system of NCH unknowns per line, diagonally
//     dominant like the original (a Schur complement of it), solved by cyclic reduction across the line's lanes (shuffles).
//  3. Back substitution of the chunk with the now known L and R, written in place.
// F, wt: planes with element (line, j) at origin + line * line_stride + j * elem_stride; wt(j) couples j-1 and j.
template <int NCH>
__global__ __launch_bounds__(64) void k_wls_solve(float2* F, const float* wt, size_t frame, size_t line_stride,
                                                  size_t elem_stride, int nlines, int len, int CH, float lambda)
{
    extern __shared__ float4 sc[];
    constexpr int LPW = 64 / NCH;
    const int lane = threadIdx.x, k = lane % NCH;
    const int line = blockIdx.x * LPW + lane / NCH;
    const bool live = line < nlines;
    const int s = k * CH;
    const int e = live ? min(s + CH, len) : s;
    const int m = e - s;                                    // may be <= 0: an empty chunk at the end of a short line
    float2* Fl = F + (size_t)blockIdx.y * frame + (size_t)(live ? line : 0) * line_stride;
    const float* Wl = wt + (size_t)blockIdx.y * frame + (size_t)(live ? line : 0) * line_stride;
    const auto w = [&](int j) -> float { return (j > 0 && j < len) ? Wl[(size_t)j * elem_stride] : 0.0f; };

    // 1. forward elimination of the interior
    float cp = 0.0f, d1 = 0.0f, d2 = 0.0f, yp = 0.0f;
    float wprev = m > 0 ? w(s) : 0.0f;
    for (int j = s; j < e - 1; ++j) {
        const float wn = w(j + 1);
        const float a = -lambda * wprev, c = -lambda * wn, b = 1.0f - a - c;
        const float2 fv = Fl[(size_t)j * elem_stride];
        const float inv = 1.0f / (b - a * cp);
        yp = -a * (j == s ? 1.0f : yp) * inv;
        cp = c * inv;
        d1 = (fv.x - a * d1) * inv;
        d2 = (fv.y - a * d2) * inv;
        sc[(j - s) * 64 + lane] = make_float4(cp, d1, d2, yp);
        wprev = wn;
    }
    // 2. the chunk's reduced equation
    float A = 0.0f, B = 1.0f, C = 0.0f, R1 = 0.0f, R2 = 0.0f;
    float fX1 = 0.0f, fX2 = 0.0f, fY = 0.0f, fZ = 1.0f;    // first element = X + Y L + Z R (m == 1: it is R itself)
    float lX1 = 0.0f, lX2 = 0.0f, lY = 1.0f, lZ = 0.0f;    // element e-2: (m == 1: it is L)
    if (m >= 2) {
        lX1 = d1; lX2 = d2; lY = yp; lZ = -cp;
        fX1 = d1; fX2 = d2; fY = yp; fZ = -cp;
        for (int j = e - 3; j >= s; --j) {
            const float4 v = sc[(j - s) * 64 + lane];
            fX1 = v.y - v.x * fX1; fX2 = v.z - v.x * fX2; fY = v.w - v.x * fY; fZ = -v.x * fZ;
        }
    }
    // the next chunk's first-element expression
    const int nx = min(lane + 1, 63);
    float nX1 = __shfl(fX1, nx), nX2 = __shfl(fX2, nx), nY = __shfl(fY, nx), nZ = __shfl(fZ, nx);
    if (k == NCH - 1) { nX1 = nX2 = nY = nZ = 0.0f; }
    if (m >= 1) {
        const float wn = w(e);
        const float a = -lambda * wprev, c = -lambda * wn, b = 1.0f - a - c;
        const float2 fv = Fl[(size_t)(e - 1) * elem_stride];
        A = a * lY;
        B = a * lZ + b + c * nY;
        C = c * nZ;
        R1 = fv.x - a * lX1 - c * nX1;
        R2 = fv.y - a * lX2 - c * nX2;
    }
    // cyclic reduction of the line's NCH equations
#pragma unroll
    for (int st = 1; st < NCH; st <<= 1) {
        const int lm = max(lane - st, 0), lp = min(lane + st, 63);
        float Am = __shfl(A, lm), Bm = __shfl(B, lm), Cm = __shfl(C, lm), R1m = __shfl(R1, lm), R2m = __shfl(R2, lm);
        float Ap = __shfl(A, lp), Bp = __shfl(B, lp), Cp = __shfl(C, lp), R1p = __shfl(R1, lp), R2p = __shfl(R2, lp);
        if (k < st) { Am = 0.0f; Bm = 1.0f; Cm = 0.0f; R1m = 0.0f; R2m = 0.0f; }
        if (k + st >= NCH) { Ap = 0.0f; Bp = 1.0f; Cp = 0.0f; R1p = 0.0f; R2p = 0.0f; }
        const float al = -A / Bm, ga = -C / Bp;
        const float nA = al * Am, nC = ga * Cp;
        const float nB = B + al * Cm + ga * Ap;
        R1 = R1 + al * R1m + ga * R1p;
        R2 = R2 + al * R2m + ga * R2p;
        A = nA; B = nB; C = nC;
    }
    const float U1 = R1 / B, U2 = R2 / B;
    const int pv = max(lane - 1, 0);
    float L1 = __shfl(U1, pv), L2 = __shfl(U2, pv);
    if (k == 0) { L1 = 0.0f; L2 = 0.0f; }
    // 3. back substitution
    if (m >= 1) {
        float u1 = U1, u2 = U2;
        Fl[(size_t)(e - 1) * elem_stride] = make_float2(u1, u2);
        for (int j = e - 2; j >= s; --j) {
            const float4 v = sc[(j - s) * 64 + lane];
            u1 = v.y + v.w * L1 - v.x * u1;
            u2 = v.z + v.w * L2 - v.x * u2;
            Fl[(size_t)j * elem_stride] = make_float2(u1, u2);
        }
    }
}

// ---- W7 / W8 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wls_final(const float2* F, const uint8_t* conf, WlsGeom g, int W, int H, int inv,
                                                   int use_conf, size_t pitch, size_t frame, WlsOut o)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= W * H) return;
    const int y = i / W, x = i - y * W;
    const bool in = x >= g.x0 && x < g.x1 && y >= g.y0 && y < g.y1;
    float v = (float)inv, c = 0.0f;
    if (in) {
        const size_t q = (size_t)f * frame + (size_t)y * pitch + x;
        const float2 t = F[q];
        if (!use_conf) v = t.x;
        else if (t.y != 0.0f) v = t.x / t.y;
        if (use_conf) c = (float)conf[q];
    }
    const int16_t d = (int16_t)fmaxf(-32768.0f, fminf(32767.0f, rintf(v)));     // W8: half to even, saturated
    o.out[(size_t)f * o.out_frame + (size_t)y * o.out_pitch + x] = d;
    if (o.filt) o.filt[(size_t)f * o.filt_frame + (size_t)y * o.filt_pitch + x] = v;
    if (o.conf) o.conf[(size_t)f * o.conf_frame + (size_t)y * o.conf_pitch + x] = c;
}

// Lines per wave for a line length: the most lines whose chunks stay <= 32 elements (LDS <= 32 KiB per wave); 1 line of up
// to 64-element chunks above 2048.
static int wls_nch(int len)
{
    for (int nch = 4; nch < 64; nch <<= 1)
        if ((len + nch - 1) / nch <= 32) return nch;
    return 64;
}

static void launch_solve(float2* F, const float* wt, size_t frame, size_t line_stride, size_t elem_stride, int nlines, int len,
                         float lambda, int n, hipStream_t s)
{
    const int nch = wls_nch(len), lpw = 64 / nch;
    const int CH = (len + nch - 1) / nch;
    const size_t lds = (size_t)std::max(CH - 1, 1) * 64 * sizeof(float4);
    const dim3 grid((nlines + lpw - 1) / lpw, n);
#define RTDM_WLS_SOLVE(N) hipLaunchKernelGGL(k_wls_solve<N>, grid, dim3(64), lds, s, F, wt, frame, line_stride, elem_stride, nlines, len, CH, lambda)
    switch (nch) {
        case 4: RTDM_WLS_SOLVE(4); break;
        case 8: RTDM_WLS_SOLVE(8); break;
        case 16: RTDM_WLS_SOLVE(16); break;
        case 32: RTDM_WLS_SOLVE(32); break;
        default: RTDM_WLS_SOLVE(64); break;
    }
#undef RTDM_WLS_SOLVE
}

void launch_wls(const WlsLaunch& L, int n, hipStream_t s)
{
    const WlsGeom& g = L.g;
    const int W = L.W, H = L.H;
    const bool roi = g.x1 > g.x0 && g.y1 > g.y0;
    if (roi) {
        const int rw = g.x1 - g.x0, rh = g.y1 - g.y0;
        const dim3 pg((rw * rh + 255) / 256, n);
        if (L.use_conf) {
            hipLaunchKernelGGL(k_wls_rowmm, dim3(H, n), dim3(256), (size_t)W * 4, s, L.dl, L.dr, W, L.r, L.invL, L.invR,
                               L.mmL, L.mmR, L.pitch, L.frame);
            hipLaunchKernelGGL(k_wls_conf, dim3(rh, n), dim3(256), (size_t)W * 2, s, L.dl, L.dr, L.mmL, L.mmR, W, H, g, L.r, L.T,
                               L.invL, L.invR, L.pitch, L.frame, L.conf, L.F);
        } else {
            hipLaunchKernelGGL(k_wls_rhs, pg, dim3(256), 0, s, L.dl, g, L.pitch, L.frame, L.F);
        }
        if (L.guide.cn == 3) hipLaunchKernelGGL(k_wls_weights<3>, pg, dim3(256), 0, s, L.guide, g, L.lut, L.pitch, L.frame, L.wh, L.wv);
        else hipLaunchKernelGGL(k_wls_weights<1>, pg, dim3(256), 0, s, L.guide, g, L.lut, L.pitch, L.frame, L.wh, L.wv);
        const size_t org = (size_t)g.y0 * L.pitch + g.x0;
        for (int t = 0; t < L.num_iter; ++t) {
            launch_solve(L.F + org, L.wh + org, L.frame, L.pitch, 1, rh, rw, L.lambda[t], n, s);   // rows
            launch_solve(L.F + org, L.wv + org, L.frame, 1, L.pitch, rw, rh, L.lambda[t], n, s);   // columns
        }
    }
    hipLaunchKernelGGL(k_wls_final, dim3((W * H + 255) / 256, n), dim3(256), 0, s, L.F, L.conf, g, W, H, L.invL, L.use_conf,
                       L.pitch, L.frame, L.out);
}

}  // namespace rtdm
