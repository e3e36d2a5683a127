// k_prefilter.hip -- the x-Sobel prefilter (K1) with the FILTERED frame fill and the plane copy, for gfx950: HBM-bound
// per-pixel stages.  The normalised-response prefilter: k_prefilter_norm.hip.
// Semantics: SURVEY.md Appendix A.3a (what cv::StereoBM does behind
// /root/reference/stereo-matcher/bm-sw.cpp:35); oracle: oracle/bm_oracle.c.
#include "rtdm_kernels.h"
#include "rtdm_device.h"

#include <cstdlib>

namespace rtdm {

// ---------------------------------------------------------------------------------------------
// K1 prefilter: x-Sobel, clip to +-cap, + cap.  Rows come in pairs; a trailing odd row is all
// `cap`; row -1 mirrors to 1, row H to H-2; columns 0 and W-1 are `cap`.
// Fast variant: one thread = 8 consecutive output bytes from three 8-byte loads per source row
// (needs 8-byte aligned base/pitch/frame); byte variant for arbitrary caller pitches.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int colsum3(unsigned long long a, unsigned long long c, unsigned long long b, int k)
{ return (int)((a >> (8 * k)) & 0xff) + 2 * (int)((c >> (8 * k)) & 0xff) + (int)((b >> (8 * k)) & 0xff); }

__global__ __launch_bounds__(256) void k_prefilter8(Plane8 L, Plane8 R, Plane8W Lp, Plane8W Rp,
                                                    int W, int H, int cap, int n, int nxb)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;        // over (row, 8-byte block)
    if (idx >= nxb * H) return;
    const int y = idx / nxb, xb = idx - y * nxb, x0 = xb * 8;
    int f = blockIdx.y;
    const bool right = f >= n;
    if (right) f -= n;
    const Plane8 S = right ? R : L;
    const Plane8W O = right ? Rp : Lp;
    const uint8_t* src = S.base + (size_t)f * S.frame;
    uint8_t* dst = O.base + (size_t)f * O.frame + (size_t)y * O.pitch + x0;
    const int npair = (H >= 2) ? (H & ~1) : 0;
    const int off = cap + PREFILTER_BIAS;
    unsigned long long out = (unsigned long long)off * 0x0101010101010101ull;
    if (y < npair) {
        const int ya = (y > 0) ? y - 1 : 1;
        const int yb = (y < H - 1) ? y + 1 : H - 2;
        const uint8_t* ra = src + (size_t)ya * S.pitch + x0;
        const uint8_t* rc = src + (size_t)y * S.pitch + x0;
        const uint8_t* rb = src + (size_t)yb * S.pitch + x0;
        const bool has_prev = x0 > 0, has_next = x0 + 16 <= (int)S.pitch;
        const unsigned long long a1 = *(const unsigned long long*)ra, c1 = *(const unsigned long long*)rc,
                                 b1 = *(const unsigned long long*)rb;
        const unsigned long long a0 = has_prev ? *(const unsigned long long*)(ra - 8) : 0ull,
                                 c0 = has_prev ? *(const unsigned long long*)(rc - 8) : 0ull,
                                 b0 = has_prev ? *(const unsigned long long*)(rb - 8) : 0ull;
        const unsigned long long a2 = has_next ? *(const unsigned long long*)(ra + 8) : 0ull,
                                 c2 = has_next ? *(const unsigned long long*)(rc + 8) : 0ull,
                                 b2 = has_next ? *(const unsigned long long*)(rb + 8) : 0ull;
        int s[10];                                          // column sums for x0-1 .. x0+8
        s[0] = colsum3(a0, c0, b0, 7);
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k + 1] = colsum3(a1, c1, b1, k);
        s[9] = colsum3(a2, c2, b2, 0);
        out = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int x = x0 + k;
            int g = s[k + 2] - s[k];
            g = g < -cap ? -cap : (g > cap ? cap : g);
            const int v = (x == 0 || x >= W - 1) ? off : g + off;
            out |= (unsigned long long)v << (8 * k);
        }
    }
    *(unsigned long long*)dst = out;                        // plane pitch is a multiple of 64: in bounds
}

// The unit of work of k_fill_frame (16 pixels of a row outside what the search writes, or one row's run count), also run by the
// extra workgroups of k_prefilter16<.., true>: a single frame is bound by its launches, not by its kernels.
struct FillArgs { Plane16W d; int cx0, cx1, vy0, vy1, value; int32_t* rowcnt; int first_block; };
// The fill's units in order: 16-pixel pieces of the rows above [0, u0) and below [u0, u1) the valid rows, of the columns left
// [u1, u2) and right [u2, u3) of the search's inside them, then (rowcnt != null) one unit per row: total() of them.
struct FillUnits {
    int nw, nl, nr, u0, u1, u2, u3, nrc;
    __host__ __device__ FillUnits(int W, int H, int cx0, int cx1, int vy0, int vy1, bool rowcnt)
        : nw((W + 15) / 16), nl((cx0 + 15) / 16), nr((W - cx1 + 15) / 16), u0(nw * vy0), u1(u0 + nw * (H - vy1)), u2(u1 + nl * (vy1 - vy0)),
          u3(u2 + nr * (vy1 - vy0)), nrc(rowcnt ? H : 0) {}
    __host__ __device__ int total() const { return u3 + nrc; }
};
__device__ __forceinline__ void fill_frame_units(Plane16W d, int W, int H, int cx0, int cx1, int vy0, int vy1, int value, int32_t* rowcnt, int idx, int frame)
{
    const FillUnits u(W, H, cx0, cx1, vy0, vy1, rowcnt != nullptr);
    if (idx >= u.u3) {
        idx -= u.u3;
        if (rowcnt && idx < H) rowcnt[frame * H + idx] = 0;
        return;
    }
    int y, xs, xe;
    if (idx < u.u0)      { y = idx / u.nw; xs = (idx - y * u.nw) * 16; xe = W; }
    else if (idx < u.u1) { idx -= u.u0; y = idx / u.nw; xs = (idx - y * u.nw) * 16; xe = W; y += vy1; }
    else if (idx < u.u2) { idx -= u.u1; y = idx / u.nl; xs = (idx - y * u.nl) * 16; xe = cx0; y += vy0; }
    else                 { idx -= u.u2; y = idx / u.nr; xs = cx1 + (idx - y * u.nr) * 16; xe = W; y += vy0; }
    int16_t* p = d.base + (size_t)frame * d.frame_e + (size_t)y * d.pitch_e;
    for (int x = xs; x < min(xs + 16, xe); ++x) p[x] = (int16_t)value;
}

// Strip variant for 16-byte aligned sources: one thread = 16 columns x RY rows.  Rows stream through registers (each
// source row is loaded once per strip as ONE 128-bit load; k_prefilter8 issues nine 64-bit loads per 8 output
// bytes and is bound by the load-issue rate), the bytes left and right of the 16 come from the neighbouring lanes.
template <int RY, bool FILL>
__global__ __launch_bounds__(256) void k_prefilter16(Plane8 L, Plane8 R, Plane8W Lp, Plane8W Rp,
                                                     int W, int H, int cap, int n, int nxb, FillArgs fa)
{
    if constexpr (FILL) {
        if ((int)blockIdx.x >= fa.first_block) {            // the extra workgroups: k_fill_frame's work for frame blockIdx.y
            if ((int)blockIdx.y < n)
                fill_frame_units(fa.d, W, H, fa.cx0, fa.cx1, fa.vy0, fa.vy1, fa.value, fa.rowcnt, ((int)blockIdx.x - fa.first_block) * 256 + threadIdx.x, blockIdx.y);
            return;
        }
    }
    const int nstrip = (H + RY - 1) / RY;
    const int idx = blockIdx.x * 256 + threadIdx.x;        // over (strip, 16-byte block)
    const bool inb = idx < nxb * nstrip;
    const int cidx = inb ? idx : 0;
    const int strip = cidx / nxb, x0 = (cidx - strip * nxb) * 16, ys = strip * RY;
    const int lane = threadIdx.x & 63;
    int f = blockIdx.y;
    const bool right = f >= n;
    if (right) f -= n;
    const Plane8 S = right ? R : L;
    const Plane8W O = right ? Rp : Lp;
    const uint8_t* src = S.base + (size_t)f * S.frame + x0;
    uint8_t* dst = O.base + (size_t)f * O.frame + (size_t)ys * O.pitch + x0;
    const int npair = (H >= 2) ? (H & ~1) : 0;
    const bool has_prev = x0 > 0, has_next = x0 + 16 < W;
    const uint32_t capb = (uint32_t)(cap + PREFILTER_BIAS) * 0x01010101u;   // what edge columns and an odd last row hold
    const uint4 capv = make_uint4(capb, capb, capb, capb);
    // Packed 16-bit arithmetic, two columns per instruction (the scalar form ran 27 VALU instructions per pixel and was
    // VALU bound at 87 % busy -- not HBM bound, as a prefilter should be): the 18 bytes b[0..17] = left neighbour, the 16
    // of this thread, right neighbour become nine pairs P[i] = (b[2i], b[2i+1]) by v_perm; hd pair i = P[i+1] - P[i] =
    // (b[2i+2] - b[2i], b[2i+3] - b[2i+1]), the x-differences of columns 2i and 2i+1.
    typedef short s2 __attribute__((ext_vector_type(2)));
    const auto pk = [](uint32_t v) { return __builtin_bit_cast(s2, v); };
    const auto un = [](s2 v) { return __builtin_bit_cast(uint32_t, v); };
    const s2 capp = pk((uint32_t)cap * 0x00010001u), ncapp = pk((uint32_t)(-cap & 0xffff) * 0x00010001u);
    const s2 offp = pk((uint32_t)(cap + PREFILTER_BIAS) * 0x00010001u);
    // bytes of the output that are the frame's first / last column (or padding): they hold `cap`
    uint32_t em[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int x = x0 + 4 * q + k; m |= (x == 0 || x >= W - 1) ? (0xffu << (8 * k)) : 0u; }
        em[q] = m;
    }
    // all RY + 2 source rows are requested before the first one is used: a wave that waits for each row before asking for
    // the next keeps 1 KB in flight, and the kernel then runs at what eight such waves per SIMD can pull (5 TB/s)
    uint4 qs[RY + 2];
    int le[RY + 2], re[RY + 2];                             // bytes across the wave's edges (lanes 0 and 63 only)
#pragma unroll
    for (int j = 0; j < RY + 2; ++j) {
        int yy = ys + j - 1;                                // source row of this step (mirrored at the frame edge)
        yy = yy < 0 ? 1 : (yy > H - 1 ? H - 2 : yy);
        if (H < 2) yy = 0;
        const uint8_t* rp = src + (size_t)yy * S.pitch;
        qs[j] = make_uint4(0, 0, 0, 0); le[j] = 0; re[j] = 0;
        if (inb) qs[j] = *(const uint4*)rp;
        if (inb && lane == 0 && has_prev) le[j] = rp[-1];
        if (inb && lane == 63 && has_next) re[j] = rp[16];
    }
    s2 hd[3][8];                                            // x-differences of the last three rows
#pragma unroll
    for (int j = 0; j < RY + 2; ++j) {
        const uint4 q = qs[j];
        int lb = __shfl_up((int)(q.w >> 24), 1), rb = __shfl_down((int)(q.x & 0xff), 1);
        if (lane == 0) lb = le[j];
        if (lane == 63) rb = re[j];
        uint32_t P[9];
        P[0] = __builtin_amdgcn_perm(q.x, (uint32_t)lb, 0x0c040c00u);
        P[1] = __builtin_amdgcn_perm(0u, q.x, 0x0c020c01u);
        P[2] = __builtin_amdgcn_perm(q.y, q.x, 0x0c040c03u);
        P[3] = __builtin_amdgcn_perm(0u, q.y, 0x0c020c01u);
        P[4] = __builtin_amdgcn_perm(q.z, q.y, 0x0c040c03u);
        P[5] = __builtin_amdgcn_perm(0u, q.z, 0x0c020c01u);
        P[6] = __builtin_amdgcn_perm(q.w, q.z, 0x0c040c03u);
        P[7] = __builtin_amdgcn_perm(0u, q.w, 0x0c020c01u);
        P[8] = __builtin_amdgcn_perm((uint32_t)rb, q.w, 0x0c040c03u);
#pragma unroll
        for (int i = 0; i < 8; ++i) hd[j % 3][i] = pk(P[i + 1]) - pk(P[i]);
        if (j >= 2) {
            const int y = ys + j - 2;                       // output row: rows (j-2, j-1, j) are (above, centre, below)
            if (inb && y < H) {
                uint4 o = capv;
                if (y < npair) {
                    uint32_t v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const s2 c = hd[(j - 1) % 3][i];
                        s2 g = hd[(j - 2) % 3][i] + hd[j % 3][i] + c + c;          // |g| <= 1020
                        g = __builtin_elementwise_min(__builtin_elementwise_max(g, ncapp), capp) + offp;
                        v[i] = un(g);
                    }
                    uint32_t w[4];
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd) {
                        const uint32_t by = __builtin_amdgcn_perm(v[2 * qd + 1], v[2 * qd], 0x06040200u);   // four low bytes of two pairs
                        w[qd] = (by & ~em[qd]) | (capb & em[qd]);
                    }
                    o = make_uint4(w[0], w[1], w[2], w[3]);
                }
                *(uint4*)(dst + (size_t)(j - 2) * O.pitch) = o;   // plane pitch is a multiple of 64: in bounds
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_prefilter1(Plane8 L, Plane8 R, Plane8W Lp, Plane8W Rp,
                                                    int W, int H, int cap, int n)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    int f = blockIdx.z;
    if (x >= W) return;
    const bool right = f >= n;
    if (right) f -= n;
    const Plane8 S = right ? R : L;
    const Plane8W O = right ? Rp : Lp;
    const uint8_t* src = S.base + (size_t)f * S.frame;
    const int npair = (H >= 2) ? (H & ~1) : 0;
    int v = cap + PREFILTER_BIAS;
    if (y < npair && x > 0 && x < W - 1) {
        const int ya = (y > 0) ? y - 1 : 1;
        const int yb = (y < H - 1) ? y + 1 : H - 2;
        const uint8_t* ra = src + (size_t)ya * S.pitch;
        const uint8_t* rc = src + (size_t)y * S.pitch;
        const uint8_t* rb = src + (size_t)yb * S.pitch;
        int g = ((int)ra[x + 1] - (int)ra[x - 1]) + 2 * ((int)rc[x + 1] - (int)rc[x - 1]) + ((int)rb[x + 1] - (int)rb[x - 1]);
        g = g < -cap ? -cap : (g > cap ? cap : g);
        v = g + cap + PREFILTER_BIAS;
    }
    O.base[(size_t)f * O.frame + (size_t)y * O.pitch + x] = (uint8_t)v;
}

// fill != null: the frame fill (launch_fill_frame's arguments) rides in the prefilter's grid where the strip kernel runs, and is a
// launch of its own before the other forms (and before the normalised-response prefilter, k_prefilter_norm.hip)
void launch_prefilter(Plane8 L, Plane8 R, Plane8W Lp, Plane8W Rp, int W, int H, int cap, int n,
                      hipStream_t stream, const FillJob* fill, int type, int ws)
{
    const auto fill_alone = [&] { if (fill) launch_fill_frame(fill->disp, W, H, fill->cx0, fill->cx1, fill->vy0, fill->vy1, n, fill->value, fill->rowcnt, stream); };
    if (type == 0) {                                        // RTDM_PREFILTER_NORMALIZED_RESPONSE
        fill_alone();
        launch_prefilter_norm(L, R, Lp, Rp, W, H, cap, ws, n, stream);
        return;
    }
    const auto al16 = [](const Plane8& p) { return (((size_t)p.base | p.pitch | p.frame) & 15) == 0; };
    const size_t w16 = (size_t)((W + 15) & ~15);
    if (al16(L) && al16(R) && L.pitch >= w16 && R.pitch >= w16 && ((size_t)Lp.base & 15) == 0 && ((size_t)Rp.base & 15) == 0) {
        constexpr int RY = 8;
        const int nxb = (W + 15) / 16;
        const int pblocks = (nxb * ((H + RY - 1) / RY) + 255) / 256;
        FillArgs fa{};
        // RTDM_FILL_IN_PREFILTER=0 (test hook): k_fill_frame as a launch of its own, as for frames the strip form cannot take
        static const int fuse_fill = env_int("RTDM_FILL_IN_PREFILTER", 1);
        if (fill && fuse_fill) {
            const int units = FillUnits(W, H, fill->cx0, fill->cx1, fill->vy0, fill->vy1, fill->rowcnt != nullptr).total();
            if (units > 0) {
                fa = FillArgs{fill->disp, fill->cx0, fill->cx1, fill->vy0, fill->vy1, fill->value, fill->rowcnt, pblocks};
                hipLaunchKernelGGL((k_prefilter16<RY, true>), dim3(pblocks + (units + 255) / 256, 2 * n), dim3(256), 0, stream, L, R, Lp, Rp, W, H, cap, n, nxb, fa);
                return;
            }
        } else fill_alone();
        hipLaunchKernelGGL((k_prefilter16<RY, false>), dim3(pblocks, 2 * n), dim3(256), 0, stream, L, R, Lp, Rp, W, H, cap, n, nxb, fa);
        return;
    }
    fill_alone();
    const auto al8 = [](const Plane8& p) { return (((size_t)p.base | p.pitch | p.frame) & 7) == 0; };
    if (al8(L) && al8(R) && L.pitch >= (size_t)((W + 7) & ~7) && R.pitch >= (size_t)((W + 7) & ~7)) {
        const int nxb = (W + 7) / 8;
        hipLaunchKernelGGL(k_prefilter8, dim3((nxb * H + 255) / 256, 2 * n), dim3(256), 0, stream, L, R, Lp, Rp, W, H, cap, n, nxb);
    } else {
        hipLaunchKernelGGL(k_prefilter1, dim3((W + 255) / 256, H, 2 * n), dim3(256), 0, stream, L, R, Lp, Rp, W, H, cap, n);
    }
}

// ---------------------------------------------------------------------------------------------
// FILTERED fill of a rectangle [x0,x1) x [y0,y1) of every frame (16 pixels per thread).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fill16(Plane16W d, int x0, int x1, int y0, int y1, int value)
{
    const int nxb = (x1 - x0 + 15) / 16;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nxb * (y1 - y0)) return;
    const int y = y0 + idx / nxb, xs = x0 + (idx % nxb) * 16;
    int16_t* p = d.base + (size_t)blockIdx.y * d.frame_e + (size_t)y * d.pitch_e;
    for (int x = xs; x < min(xs + 16, x1); ++x) p[x] = (int16_t)value;
}

// Everything of a frame the search does not write, in ONE launch (four launches + a memset cost a single frame 17 us): the
// rows above / below [vy0, vy1), the columns left / right of [cx0, cx1) inside them, and (rowcnt != null) the per-row run
// counts of the speckle filter, which the left-right check only writes for the valid rows.
__global__ __launch_bounds__(256) void k_fill_frame(Plane16W d, int W, int H, int cx0, int cx1, int vy0, int vy1, int value, int32_t* rowcnt)
{
    fill_frame_units(d, W, H, cx0, cx1, vy0, vy1, value, rowcnt, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

void launch_fill_frame(Plane16W disp, int W, int H, int cx0, int cx1, int vy0, int vy1, int n, int value, int32_t* rowcnt, hipStream_t stream)
{
    const int units = FillUnits(W, H, cx0, cx1, vy0, vy1, rowcnt != nullptr).total();
    if (units <= 0) return;
    hipLaunchKernelGGL(k_fill_frame, dim3((units + 255) / 256, n), dim3(256), 0, stream, disp, W, H, cx0, cx1, vy0, vy1, value, rowcnt);
}

__global__ __launch_bounds__(256) void k_copy16(Plane16W src, Plane16W dst, int W, int H)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W * H) return;
    const int y = idx / W, x = idx - y * W;
    dst.base[(size_t)blockIdx.y * dst.frame_e + (size_t)y * dst.pitch_e + x] = src.base[(size_t)blockIdx.y * src.frame_e + (size_t)y * src.pitch_e + x];
}

void launch_copy16(Plane16W src, Plane16W dst, int W, int H, int n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_copy16, dim3((W * H + 255) / 256, n), dim3(256), 0, stream, src, dst, W, H);
}

void launch_fill16(Plane16W disp, int x0, int x1, int y0, int y1, int n, int value, hipStream_t stream)
{
    if (x1 <= x0 || y1 <= y0) return;
    const int nxb = (x1 - x0 + 15) / 16;
    hipLaunchKernelGGL(k_fill16, dim3((nxb * (y1 - y0) + 255) / 256, n), dim3(256), 0, stream, disp, x0, x1, y0, y1, value);
}

}  // namespace rtdm
