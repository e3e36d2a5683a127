// k_morph_general.hip -- K5g: erosion / dilation with ANY structuring element up to 63 x 63, and the chains of them that make
// cv::morphologyEx's operations (rules M1-M7).  It sits beside the fused 10x10 kernel of k_morph.hip,
// which keeps serving the default setting; api_morph.hip routes.
//
// ONE launch per erosion / dilation.  A workgroup owns a 64x32 output tile and stages it with the halo the element needs
// (anchor columns to the left, rounded up to a dword; width - 1 - anchor to the right; the same with rows) in LDS, neutral
// bytes (255 before an erosion, 0 before a dilation) standing in outside the image.  The element is a table of runs
// (row, first column, length): wave 0 expands it from the row bit masks in the kernel arguments while the tile is staged.
// Horizontal extrema by doubling: plane k holds the extrema of the windows [x, x + 2^k), k = 0 .. log2(longest run), plane
// k + 1 made from plane k and its copy shifted by 2^k.  A run of length L is then the extremum of TWO windows of the largest
// 2^k <= L, at its first column and at its last column + 1 - 2^k, whatever L is: two LDS reads (ds_read2_b32 of the aligned
// dword pair that holds the four bytes, shifted out by v_alignbyte) per run and four output pixels.  Bytes are widened to
// (u16, u16) pairs by v_perm so that one v_pk_min/max_u16 serves two pixels, as in k_morph.hip.
// GRADIENT / TOPHAT / BLACKHAT subtract in the epilogue of their last pass (a second, pointwise input; v_pk_sub_u16 clamp).
#include "rtdm_kernels.h"

#include <algorithm>

namespace rtdm {

static constexpr int GTW = 64, GTH = 32;        // output tile; 256 threads: thread t owns columns 4 (t % 16) .. + 3 of rows t / 16 and t / 16 + 16

typedef unsigned short gus2_t __attribute__((ext_vector_type(2)));

template <bool DILATE> __device__ __forceinline__ uint32_t gpm(uint32_t a, uint32_t b)
{
    const gus2_t x = __builtin_bit_cast(gus2_t, a), y = __builtin_bit_cast(gus2_t, b);
    return __builtin_bit_cast(uint32_t, DILATE ? __builtin_elementwise_max(x, y) : __builtin_elementwise_min(x, y));
}
// bytes 0, 1 / 2, 3 of d as a (u16, u16) pair
__device__ __forceinline__ uint32_t glo(uint32_t d) { return __builtin_amdgcn_perm(0u, d, 0x0c010c00u); }
__device__ __forceinline__ uint32_t ghi(uint32_t d) { return __builtin_amdgcn_perm(0u, d, 0x0c030c02u); }
__device__ __forceinline__ uint32_t gpack4(uint32_t p01, uint32_t p23) { return __builtin_amdgcn_perm(p23, p01, 0x06040200u); }
// the four bytes at row + c, row 4-byte aligned: the aligned dword pair around them, shifted
__device__ __forceinline__ uint32_t gld4(const uint8_t* row, int c)
{
    const uint32_t* q = (const uint32_t*)(row + (c & ~3));
    return __builtin_amdgcn_alignbyte(q[1], q[0], (uint32_t)(c & 3));
}

// What the launcher derives from the element and the frame: staged rows SH = GTH + h - 1, staged columns SW (a multiple of 4
// that covers axr + GTW + w - 1 - ax), plane row pitch SP = SW + 8 (every read of a dword pair stays inside its row's pitch
// or runs into bytes nobody needs), axr = ax rounded up to 4 (the staged columns start on a dword of an aligned source),
// table bytes TB (16-byte multiple) in front of the planes.
struct MorphGeom { int W, H, SW, SH, SP, axr, TB; };

// SUB: 0 = store the extremum; 1 = extremum - second; 2 = second - extremum (saturating; never negative by construction)
template <bool DILATE, int SUB>
__global__ __launch_bounds__(256) void k_morph_pass(Plane8 in, Plane8W out, Plane8 second, MorphGeom g, MorphBits el)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint32_t* tab = (uint32_t*)lds;               // run r: row | first staged column << 8 | second window's column << 16 | k << 24
    uint8_t* P = lds + g.TB;                      // planes 0 .. kmax, PL bytes each
    const int SP = g.SP, SH = g.SH, PL = SP * SH, W = g.W, H = g.H;
    const int tid = threadIdx.x, f = blockIdx.z;
    const int tx0 = blockIdx.x * GTW, ty0 = blockIdx.y * GTH;
    const int gx0 = tx0 - g.axr, gy0 = ty0 - el.ay;              // image coordinates of staged (0, 0)
    const int off = g.axr - el.ax;                                // element column j of output column x reads staged column x + j + off

    if (tid < 64) {                                               // wave 0: lane i expands row i behind the runs of the rows above
        int ofs = 0;
        unsigned long long mine = 0;
        for (int r = 0; r < el.h; ++r) {
            const unsigned long long m = el.rows[r];
            if (r < tid) ofs += __popcll(m & ~(m << 1));
            if (r == tid) mine = m;
        }
        while (mine) {
            const int j1 = __ffsll((long long)mine) - 1;
            const unsigned long long t = mine + (1ull << j1);     // bit 63 is never a member: no overflow
            const int L = __ffsll((long long)t) - 1 - j1, k = 31 - __clz(L), c1 = off + j1;
            tab[ofs++] = (uint32_t)tid | ((uint32_t)c1 << 8) | ((uint32_t)(c1 + L - (1 << k)) << 16) | ((uint32_t)k << 24);
            mine &= t;
        }
    }

    const uint8_t* src = in.base + (size_t)f * in.frame;
    const uint32_t neutral = DILATE ? 0u : 255u;
    const int SW = g.SW;
    const bool interior = gx0 >= 0 && gy0 >= 0 && gx0 + SW <= W && gy0 + SH <= H;
    if (interior && (((size_t)src | in.pitch) & 3) == 0) {        // gx0 is a multiple of 4 by construction
        const int nq = SW >> 2;
        for (int i = tid; i < SH * nq; i += 256) {
            const int y = i / nq, xq = i - y * nq;
            *(uint32_t*)(P + y * SP + 4 * xq) = *(const uint32_t*)(src + (size_t)(gy0 + y) * in.pitch + gx0 + 4 * xq);
        }
    } else {
        for (int i = tid; i < SH * SW; i += 256) {
            const int y = i / SW, x = i - y * SW;
            const int gx = gx0 + x, gy = gy0 + y;
            P[y * SP + x] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? src[(size_t)gy * in.pitch + gx] : (uint8_t)neutral;
        }
    }
    __syncthreads();

    // plane k from plane k - 1: [x, x + 2^k) = [x, x + 2^(k-1)) and [x + 2^(k-1), x + 2^k).  Groups near the end of a row
    // read on into the next row (after the last row: into the next plane or the slack behind the planes) and make bytes
    // that no run reads: a run's windows end inside the staged columns of their own row.  Reading on into the next plane means
    // reading the first bytes of plane k while other threads write them: formally an LDS data race, on purpose -- whatever
    // value such a read returns only ever goes into those unread bytes (at most 20 bytes past the end of plane k - 1).
    const int NG = SP >> 2;
    for (int k = 1; k <= el.kmax; ++k) {
        const int sh = 1 << (k - 1);
        const uint8_t* a = P + (k - 1) * PL;
        uint8_t* b = P + k * PL;
        for (int i = tid; i < SH * NG; i += 256) {
            const uint32_t* p = (const uint32_t*)(a + 4 * i);
            const uint32_t d0 = p[0];
            const uint32_t d1 = sh < 4 ? __builtin_amdgcn_alignbyte(p[1], d0, (uint32_t)sh) : p[sh >> 2];
            *(uint32_t*)(b + 4 * i) = gpack4(gpm<DILATE>(glo(d0), glo(d1)), gpm<DILATE>(ghi(d0), ghi(d1)));
        }
        __syncthreads();
    }

    const int x0 = 4 * (tid & 15), yA = tid >> 4;                 // rows yA and yA + 16 of the tile
    const uint32_t npair = DILATE ? 0u : 0x00ff00ffu;
    uint32_t a01 = npair, a23 = npair, b01 = npair, b23 = npair;
    const uint8_t* base = P + yA * SP + x0;
    for (int r = 0; r < el.nruns; ++r) {
        const uint32_t e = tab[r];
        const int c1 = (e >> 8) & 255, c2 = (e >> 16) & 255;
        const uint8_t* row = base + (e >> 24) * PL + (e & 255) * SP;
        const uint32_t va = gld4(row, c1), vb = gld4(row, c2);
        const uint32_t wa = gld4(row + 16 * SP, c1), wb = gld4(row + 16 * SP, c2);
        a01 = gpm<DILATE>(a01, gpm<DILATE>(glo(va), glo(vb))); a23 = gpm<DILATE>(a23, gpm<DILATE>(ghi(va), ghi(vb)));
        b01 = gpm<DILATE>(b01, gpm<DILATE>(glo(wa), glo(wb))); b23 = gpm<DILATE>(b23, gpm<DILATE>(ghi(wa), ghi(wb)));
    }

    uint8_t* dst = out.base + (size_t)f * out.frame;
    const uint8_t* sec = SUB ? second.base + (size_t)f * second.frame : nullptr;
    const bool al_out = (((size_t)dst | out.pitch) & 3) == 0;
    const bool al_sec = SUB && (((size_t)sec | second.pitch) & 3) == 0;
    const int gx = tx0 + x0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int gy = ty0 + yA + 16 * h;
        if (gx >= W || gy >= H) continue;
        uint32_t p01 = h ? b01 : a01, p23 = h ? b23 : a23;
        const bool full = gx + 3 < W;
        if (SUB) {
            const uint8_t* s = sec + (size_t)gy * second.pitch + gx;
            uint32_t sv = 0;
            if (full && al_sec) sv = *(const uint32_t*)s;
            else for (int k = 0; k < 4; ++k) if (gx + k < W) sv |= (uint32_t)s[k] << (8 * k);
            const gus2_t s01 = __builtin_bit_cast(gus2_t, glo(sv)), s23 = __builtin_bit_cast(gus2_t, ghi(sv));
            const gus2_t m01 = __builtin_bit_cast(gus2_t, p01), m23 = __builtin_bit_cast(gus2_t, p23);
            p01 = __builtin_bit_cast(uint32_t, SUB == 1 ? __builtin_elementwise_sub_sat(m01, s01) : __builtin_elementwise_sub_sat(s01, m01));
            p23 = __builtin_bit_cast(uint32_t, SUB == 1 ? __builtin_elementwise_sub_sat(m23, s23) : __builtin_elementwise_sub_sat(s23, m23));
        }
        const uint32_t res = gpack4(p01, p23);
        uint8_t* d = dst + (size_t)gy * out.pitch + gx;
        if (full && al_out) *(uint32_t*)d = res;
        else for (int k = 0; k < 4; ++k) if (gx + k < W) d[k] = (uint8_t)(res >> (8 * k));
    }
}

static MorphGeom morph_geom(const MorphBits& el, int W, int H)
{
    MorphGeom g;
    g.W = W; g.H = H;
    g.axr = (el.ax + 3) & ~3;
    g.SW = (g.axr + GTW + el.w - 1 - el.ax + 3) & ~3;
    g.SH = GTH + el.h - 1;
    g.SP = g.SW + 8;
    g.TB = (el.nruns * 4 + 15) & ~15;
    return g;
}
static size_t morph_lds_bytes(const MorphGeom& g, int kmax) { return (size_t)g.TB + (size_t)(kmax + 1) * g.SP * g.SH + 64; }
// the most any element asks for: 63 x 63 with 32 runs in every row, anchor column 61 .. 62
static constexpr size_t MORPH_LDS_MOST = 63 * 32 * 4 + 6 * (size_t)(64 + GTW + 4 + 8) * (GTH + 62) + 64;

struct MorphPass { bool dilate; bool identity; int sub; Plane8 in; Plane8W out; Plane8 second; };

template <bool DILATE, int SUB>
static hipError_t launch_pass(const MorphPass& p, const MorphBits& el, int W, int H, int n, hipStream_t stream)
{
    const MorphGeom g = morph_geom(el, W, H);
    const size_t lds = morph_lds_bytes(g, el.kmax);
    // Above the default limit the kernel has to ask for its dynamic LDS.  The attribute belongs to the device, so it is set
    // once per device and instantiation, always to the same value: the most any element needs, capped by what a CU has.
    static OncePerDevice once;
    if (lds > 48 * 1024 && once.first()) {
        int dev = 0, lds_max = 0;
        size_t want = MORPH_LDS_MOST;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess && lds_max > 0)
            want = std::min(want, (size_t)lds_max);
        (void)hipGetLastError();
        const hipError_t e = hipFuncSetAttribute((const void*)k_morph_pass<DILATE, SUB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((W + GTW - 1) / GTW, (H + GTH - 1) / GTH, n);
    hipLaunchKernelGGL((k_morph_pass<DILATE, SUB>), grid, dim3(256), lds, stream, p.in, p.out, p.second, g, el);
    return hipGetLastError();
}

static hipError_t launch_pass(const MorphPass& p, const MorphBits& el, const MorphBits& one, int W, int H, int n, hipStream_t s)
{
    const MorphBits& e = p.identity ? one : el;
    if (p.dilate) return p.sub == 1 ? launch_pass<true, 1>(p, e, W, H, n, s) : p.sub == 2 ? launch_pass<true, 2>(p, e, W, H, n, s)
                                                                                           : launch_pass<true, 0>(p, e, W, H, n, s);
    return p.sub == 1 ? launch_pass<false, 1>(p, e, W, H, n, s) : p.sub == 2 ? launch_pass<false, 2>(p, e, W, H, n, s)
                                                                             : launch_pass<false, 0>(p, e, W, H, n, s);
}

// The chain of passes of one operation.  No pass writes the plane it reads: a chain runs IN -> T0 -> T1 -> ... -> OUT, and
// where IN and OUT are one plane a chain of a single pass gets a copy pass (the 1x1 element) behind it.  The pointwise second
// input of a difference may be the plane its pass writes: a thread reads its four bytes before it stores them.
hipError_t launch_morph_general(int op, int iterations, const MorphBits& el, Plane8 in, Plane8W out, uint8_t* tmp0, uint8_t* tmp1,
                                int W, int H, int n, hipStream_t stream)
{
    const size_t tp = (size_t)W, tf = (size_t)W * H;
    const Plane8 IN = in, OUT{out.base, out.pitch, out.frame}, T0{tmp0, tp, tf}, T1{tmp1, tp, tf}, NONE{nullptr, 0, 0};
    const bool alias = in.base == out.base;
    const auto wr = [](const Plane8& p) { return Plane8W{(uint8_t*)p.base, p.pitch, p.frame}; };
    MorphBits one{};
    one.rows[0] = 1; one.w = one.h = 1; one.nruns = 1;
    std::vector<MorphPass> chain;
    const int it = iterations;
    // kinds[i]: pass i dilates; a linear chain ping-pongs between the scratch planes and ends in OUT
    const auto linear = [&](const std::vector<bool>& kinds, int sub, const Plane8& second) {
        Plane8 cur = IN;
        const int np = (int)kinds.size();
        const bool copy = np == 1 && alias;                                // the one pass would write what it reads
        for (int i = 0; i < np; ++i) {
            const bool last = i == np - 1 && !copy;
            const Plane8 dst = last ? OUT : (i & 1 ? T1 : T0);
            chain.push_back(MorphPass{kinds[i], false, last ? sub : 0, cur, wr(dst), last ? second : NONE});
            cur = dst;
        }
        if (copy) chain.push_back(MorphPass{false, true, sub, T0, wr(OUT), second});
    };
    std::vector<bool> kinds;
    const auto add = [&](bool dilate) { kinds.insert(kinds.end(), (size_t)it, dilate); };
    switch (op) {
    case 0: add(false); linear(kinds, 0, NONE); break;
    case 1: add(true); linear(kinds, 0, NONE); break;
    case 2: add(false); add(true); linear(kinds, 0, NONE); break;
    case 3: add(true); add(false); linear(kinds, 0, NONE); break;
    case 5: add(false); add(true); linear(kinds, 2, IN); break;            // src - open
    case 6: add(true); add(false); linear(kinds, 1, IN); break;            // close - src
    case 100: add(false); add(true); add(true); add(false); linear(kinds, 0, NONE); break;
    case 4: {                                                              // d^n - e^n
        Plane8 cur = IN, E = NONE;
        for (int i = 0; i < it; ++i) {                                     // e^n -> T0 or T1
            E = i & 1 ? T1 : T0;
            chain.push_back(MorphPass{false, false, 0, cur, wr(E), NONE});
            cur = E;
        }
        const Plane8 X = (it - 1) & 1 ? T0 : T1;                           // the other scratch plane
        cur = IN;
        bool done = false;
        for (int i = 0; i < it; ++i) {
            const bool last = i == it - 1;
            // apart: the last pass lands in OUT; one plane: IN is read by the first pass alone, which therefore writes X
            const bool to_out = alias ? (i & 1) : ((it - 1 - i) & 1) == 0;
            const Plane8 dst = to_out ? OUT : X;
            const bool sub = last && to_out;
            chain.push_back(MorphPass{true, false, sub ? 1 : 0, cur, wr(dst), sub ? E : NONE});
            done = sub;
            cur = dst;
        }
        if (!done) chain.push_back(MorphPass{false, true, 1, X, wr(OUT), E});
        break;
    }
    default: return hipErrorInvalidValue;
    }
    for (const MorphPass& p : chain) {
        const hipError_t e = launch_pass(p, el, one, W, H, n, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rtdm
