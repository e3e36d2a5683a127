// k_prefilter_norm.hip -- K1 for preFilterType NORMALIZED_RESPONSE (cv::StereoBM's prefilterNorm) on gfx950.
// Rules N1-N6, DESIGN.md section 4.10 (restated from memory of OpenCV's stereobm.cpp: parity with the library is unpinned):
//   r = ws / 2, g = ws*ws/8, scale_s = (1024 + g) / (2 g), scale_g = g * scale_s
//   S(x, y) = box sum of the (2r+1)^2 source pixels around (x, y), row and column indices clamped to the frame
//   n       = 4 c + l + r' + u + d, the neighbours clamped to the frame as well (so column 0 sees 5 c + r' + u + d)
//   dst     = clamp((n * scale_g - S * scale_s) >> 10, -cap, cap) + cap            every row, every column
// ws >= 91 makes both scales 0 and the plane constant: that is a fill (k_prefilter_norm_const).
//
// The box sum is separable and never costs ws^2 per pixel.  One workgroup of 256 threads makes a tile of TX = 128 columns x
// RY = 32 rows:
//   1. the source tile with its halo, (RY + 2r) rows x (TX + 2 HP) columns (HP = r rounded up to 16), goes to LDS with every
//      clamp applied on the way in, so that nothing after this step knows about frame edges.  16-byte aligned sources come in
//      as 128-bit loads (a chunk left / right of the frame is the row's first / last byte repeated); every other caller
//      plane is gathered byte by byte (the slow form: same kernel, other loader);
//   2. one thread per tile column (TX + 2r of them) runs the vertical sum of 2r+1 rows down the tile: 2r+1 reads to start,
//      then one row in and one row out per output row; the RY x (TX + 2r) sums (<= 89 * 255, 16 bits) go to LDS;
//   3. one thread per 16 output bytes (8 per row, 32 rows) runs the horizontal window over those sums the same way (2r+1
//      reads, then 15 steps of one in / one out), takes c, l, r', u, d from the source tile, and stores 16 bytes.
// Per pixel that is (RY + 2r) / RY source bytes (the vertical halo; L2 serves most of it), 2 + (2r+1)/RY LDS reads in step 2
// and about 5 + (2r+1)/16 in step 3: linear in ws with a small slope, constant HBM traffic (1 byte in, 1 byte out).
// LDS: (RY + 2r) (TX + 2 HP) + 2 RY VP bytes = 15.7 KB at ws = 9, 41.3 KB at ws = 89 (VP: see below); dynamic, so small
// windows keep six and more workgroups per CU.
#include "rtdm_kernels.h"
#include "rtdm_device.h"

namespace rtdm {

namespace {
constexpr int NTX = 128, NRY = 32;

struct NormGeom {
    int W, H, cap, n;
    int r, HP, TW, TH;      // radius, halo columns (r rounded up to 16), tile width TX + 2 HP, tile height RY + 2r
    int VP;                 // pitch (elements) of the vertical-sum rows
    int scale_s, scale_g;
};
}

// VP = 2 (mod 16): step 3's lanes are 8 segments (32 bytes apart = 8 banks) x 8 rows; rows VP * 2 bytes apart then start
// one bank further each, and the 64 lanes of a wave hit 64 different banks.
// (and VP > TX + 2r: step 3's last window step reads one element past the sums it uses)
static inline int norm_vpitch(int r) { const int c = NTX + 2 * r + 1; return c + ((2 - c % 16) + 16) % 16; }

template <bool AL16>
__global__ __launch_bounds__(256) void k_prefilter_norm(Plane8 L, Plane8 R, Plane8W Lp, Plane8W Rp, NormGeom g)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* tile = lds;                                             // [TH][TW]
    uint16_t* vs = (uint16_t*)(lds + (size_t)g.TH * g.TW);           // [RY][VP]   (TH * TW is a multiple of 16)
    const int tid = threadIdx.x;
    const int xs = blockIdx.x * NTX, ys = blockIdx.y * NRY;
    int f = blockIdx.z;
    const bool right = f >= g.n;
    if (right) f -= g.n;
    const Plane8 S = right ? R : L;
    const Plane8W O = right ? Rp : Lp;
    const uint8_t* src = S.base + (size_t)f * S.frame;
    const int W = g.W, H = g.H, r = g.r, TW = g.TW, TH = g.TH;
    const int gx0 = xs - g.HP;                                       // frame column of tile column 0 (a multiple of 16)

    // ---- 1. the source tile, clamped ---------------------------------------------------------------------------------------
    if constexpr (AL16) {
        const int ncx = TW / 16;
        for (int i = tid; i < TH * ncx; i += 256) {
            const int j = i / ncx, k = i - j * ncx;
            const int y = min(max(ys - r + j, 0), H - 1);
            const uint8_t* row = src + (size_t)y * S.pitch;
            const int gx = gx0 + 16 * k;
            uint8_t* t = tile + j * TW + 16 * k;
            if (gx < 0 || gx >= W) {
                const uint32_t b = (uint32_t)row[gx < 0 ? 0 : W - 1] * 0x01010101u;
                *(uint4*)t = make_uint4(b, b, b, b);
            } else {
                *(uint4*)t = *(const uint4*)(row + gx);              // pitch >= W rounded up to 16: inside the row
                if (gx + 16 > W) {
                    const uint8_t last = row[W - 1];
                    for (int c = W - gx; c < 16; ++c) t[c] = last;
                }
            }
        }
    } else {
        for (int i = tid; i < TH * TW; i += 256) {
            const int j = i / TW, c = i - j * TW;
            const int y = min(max(ys - r + j, 0), H - 1), x = min(max(gx0 + c, 0), W - 1);
            tile[i] = src[(size_t)y * S.pitch + x];
        }
    }
    __syncthreads();

    // ---- 2. vertical sums of 2r+1 rows, running down the tile: vs[y][c] for tile column HP - r + c ------------------------
    const int nvc = NTX + 2 * r;                                     // <= 216 < 256
    if (tid < nvc) {
        const uint8_t* col = tile + (g.HP - r) + tid;
        int s = 0;
        for (int j = 0; j <= 2 * r; ++j) s += col[j * TW];
        for (int y = 0; y < NRY; ++y) {
            vs[y * g.VP + tid] = (uint16_t)s;                        // <= 89 * 255
            if (y + 1 < NRY) s += (int)col[(y + 2 * r + 1) * TW] - (int)col[y * TW];
        }
    }
    __syncthreads();

    // ---- 3. horizontal window, centre term, response: 16 bytes of one row per thread ----------------------------------------
    const int row = tid >> 3, seg = tid & 7;
    const int y = ys + row, x0 = xs + 16 * seg;
    if (y >= H || x0 >= W) return;
    const uint16_t* v = vs + row * g.VP + 16 * seg;                  // v[k + r] is the column sum of frame column x0 + k
    const uint8_t* tc = tile + (row + r) * TW + g.HP + 16 * seg;     // tc[k] is source pixel (x0 + k, y), clamped
    int s = 0;
    for (int k = 0; k <= 2 * r; ++k) s += v[k];
    const int off = g.cap + PREFILTER_BIAS;
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int k = 4 * q + b;
            const int c = tc[k];
            const int nn = 4 * c + tc[k - 1] + tc[k + 1] + tc[k - TW] + tc[k + TW];
            int val = (nn * g.scale_g - s * g.scale_s) >> 10;
            val = min(max(val, -g.cap), g.cap) + off;
            if (x0 + k >= W) val = off;                              // row padding: what the x-Sobel planes hold there
            w |= (uint32_t)val << (8 * b);
            s += (int)v[k + 2 * r + 1] - (int)v[k];                  // (the last step reads one element it does not use: inside VP)
        }
        o[q] = w;
    }
    *(uint4*)(O.base + (size_t)f * O.frame + (size_t)y * O.pitch + x0) = make_uint4(o[0], o[1], o[2], o[3]);   // plane pitch is a multiple of 64: in bounds
}

// ws >= 91: scale_s = scale_g = 0, every pixel is ftzero
__global__ __launch_bounds__(256) void k_prefilter_norm_const(Plane8W Lp, Plane8W Rp, int W, int H, int cap, int n, int nxb)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;                  // over (row, 16-byte block)
    if (idx >= nxb * H) return;
    const int y = idx / nxb, x0 = (idx - y * nxb) * 16;
    int f = blockIdx.y;
    const bool right = f >= n;
    if (right) f -= n;
    const Plane8W O = right ? Rp : Lp;
    const uint32_t b = (uint32_t)(cap + PREFILTER_BIAS) * 0x01010101u;
    *(uint4*)(O.base + (size_t)f * O.frame + (size_t)y * O.pitch + x0) = make_uint4(b, b, b, b);
}

void launch_prefilter_norm(Plane8 L, Plane8 R, Plane8W Lp, Plane8W Rp, int W, int H, int cap, int ws, int n, hipStream_t stream)
{
    const int gg = ws * ws / 8;
    const int scale_s = (1024 + gg) / (2 * gg), scale_g = gg * scale_s;          // N1
    if (scale_s == 0) {
        const int nxb = (W + 15) / 16;
        hipLaunchKernelGGL(k_prefilter_norm_const, dim3((nxb * H + 255) / 256, 2 * n), dim3(256), 0, stream, Lp, Rp, W, H, cap, n, nxb);
        return;
    }
    NormGeom g{};
    g.W = W; g.H = H; g.cap = cap; g.n = n;
    g.r = ws / 2; g.HP = (g.r + 15) & ~15; g.TW = NTX + 2 * g.HP; g.TH = NRY + 2 * g.r;
    g.VP = norm_vpitch(g.r);
    g.scale_s = scale_s; g.scale_g = scale_g;
    const size_t lds = (size_t)g.TH * g.TW + (size_t)NRY * g.VP * sizeof(uint16_t);   // <= 41.3 KB (ws = 89)
    const dim3 grid((W + NTX - 1) / NTX, (H + NRY - 1) / NRY, 2 * n);
    const auto al16 = [](const Plane8& p) { return (((size_t)p.base | p.pitch | p.frame) & 15) == 0; };
    const size_t w16 = (size_t)((W + 15) & ~15);
    if (al16(L) && al16(R) && L.pitch >= w16 && R.pitch >= w16)
        hipLaunchKernelGGL((k_prefilter_norm<true>), grid, dim3(256), lds, stream, L, R, Lp, Rp, g);
    else
        hipLaunchKernelGGL((k_prefilter_norm<false>), grid, dim3(256), lds, stream, L, R, Lp, Rp, g);
}

}  // namespace rtdm
