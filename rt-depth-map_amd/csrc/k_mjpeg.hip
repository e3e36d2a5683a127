// k_mjpeg.hip -- baseline MJPEG frames on the device (the reference's DecoderDevice; rules J1-J5):
//   k_mjpeg_huff   J1: entropy decoding, one lane per entropy segment (the stretch between two RSTn markers), one workgroup
//                  per frame; dequantised int16 coefficients, written sparsely into a zeroed buffer
//   k_mjpeg_huff_split  J1 for a frame that is ONE segment (no restart intervals): the segment cut among up to 1024 lanes
//   k_mjpeg_idct   J2: libjpeg's JDCT_ISLOW, one lane per 8 x 8 block, the block in registers; planar Y / Cb / Cr out
//   k_mjpeg_rgb    J3 + J4: fancy upsampling, YCbCr -> RGB, crop, interleaved RGB at the caller's pitch
// The per-segment loop itself is mjpeg_decode_segment in rtdm_mjpeg.h, which also runs on the CPU (tests/mjpeg_host.cpp); so
// does a lane's pass of the split form, mjpeg_split_pass (tests/mjpeg_split_host.cpp).
#include "rtdm_kernels.h"
#include "rtdm_mjpeg.h"

namespace rtdm {

__constant__ uint8_t c_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                                     13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
                                     52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the subsequences a frame is cut into when split_s bytes are asked for (0: none); fewer than 2 = the frame is k_mjpeg_huff's
__device__ __forceinline__ uint32_t split_plan(const MjpegDesc& d, const MjpegSeg* __restrict__ segs, uint32_t split_s, uint32_t* begin,
                                               uint32_t* end, uint32_t* sp)
{
    *begin = *end = *sp = 0;
    if (split_s == 0 || d.nseg != 1) return 0;
    const MjpegSeg sg = segs[d.seg_first];
    *end = sg.end < d.stream_len ? sg.end : d.stream_len;
    *begin = sg.begin < *end ? sg.begin : *end;
    return mjpeg_split_plan(*end - *begin, split_s, sp);
}

// One workgroup = one frame.  Its descriptor and the six decoding tables live in LDS (about 7.3 KB); lane t takes segments
// t, t + blockDim.x, ...  A frame of one segment (no restart intervals) is left to k_mjpeg_huff_split when split_s says so.
__global__ __launch_bounds__(256) void k_mjpeg_huff(const uint8_t* __restrict__ streams, const MjpegDesc* __restrict__ desc,
                                                    const MjpegSeg* __restrict__ segs, int16_t* __restrict__ coef,
                                                    size_t coef_frame_e, int* __restrict__ status, uint32_t split_s)
{
    __shared__ MjpegDesc sd;
    __shared__ MjpegHuff tabs[6];
    __shared__ uint8_t zz[64];
    static_assert(sizeof(MjpegDesc) % 4 == 0, "the descriptor is copied word by word");
    const uint32_t* src = (const uint32_t*)(desc + blockIdx.x);
    for (unsigned i = threadIdx.x; i < sizeof(MjpegDesc) / 4; i += blockDim.x) ((uint32_t*)&sd)[i] = src[i];
    if (threadIdx.x < 64) zz[threadIdx.x] = c_zigzag[threadIdx.x];
    __syncthreads();
    uint32_t begin, end, sp;
    if (split_plan(sd, segs, split_s, &begin, &end, &sp) >= 2) return;          // the whole workgroup: the other kernel's frame
    const int ncomp = sd.ncomp < 1 ? 1 : (sd.ncomp > 3 ? 3 : sd.ncomp);
    if ((int)threadIdx.x < 2 * ncomp) mjpeg_build_table(sd.bits[threadIdx.x], sd.vals[threadIdx.x], &tabs[threadIdx.x]);
    __syncthreads();
    const uint8_t* s = streams + sd.stream_off;
    int16_t* out = coef + (size_t)blockIdx.x * coef_frame_e;
    for (uint32_t seg = threadIdx.x; seg < sd.nseg; seg += blockDim.x) {
        const int st = mjpeg_decode_segment(s, sd, segs[sd.seg_first + seg], seg, tabs, zz, out);
        if (st != MJ_OK) atomicMin(&status[blockIdx.x], MJ_BAD_STREAM);
    }
}

// The exclusive scan over the lanes of a workgroup of what their passes counted: the blocks before lane i, and the DC walks of
// the lanes before it composed in order (they do not commute).  Within a wave by shuffles, across the waves through wt.
struct SplitSum { uint32_t blocks; MjpegClamp m0, m1, m2; };
__device__ __forceinline__ SplitSum split_then(const SplitSum& f, const SplitSum& g)
{
    SplitSum r;
    r.blocks = f.blocks + g.blocks;
    r.m0 = mjpeg_clamp_then(f.m0, g.m0); r.m1 = mjpeg_clamp_then(f.m1, g.m1); r.m2 = mjpeg_clamp_then(f.m2, g.m2);
    return r;
}
__device__ __forceinline__ MjpegClamp shfl_up_clamp(const MjpegClamp& f, int d)
{
    MjpegClamp r;
    r.a = __shfl_up(f.a, d); r.l = __shfl_up(f.l, d); r.h = __shfl_up(f.h, d);
    return r;
}
__device__ __forceinline__ SplitSum shfl_up_sum(const SplitSum& f, int d)
{
    SplitSum r;
    r.blocks = __shfl_up(f.blocks, d);
    r.m0 = shfl_up_clamp(f.m0, d); r.m1 = shfl_up_clamp(f.m1, d); r.m2 = shfl_up_clamp(f.m2, d);
    return r;
}
__device__ __forceinline__ SplitSum split_identity()
{
    SplitSum r;
    r.blocks = 0; r.m0 = r.m1 = r.m2 = mjpeg_clamp_id();
    return r;
}
// every lane of the workgroup calls this (it holds a barrier); wt: one entry per wave
__device__ __forceinline__ SplitSum split_scan_exclusive(SplitSum mine, SplitSum* wt)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const SplitSum o = shfl_up_sum(mine, d);
        if (lane >= d) mine = split_then(o, mine);
    }
    if (lane == 63) wt[wave] = mine;
    SplitSum before = shfl_up_sum(mine, 1);
    if (lane == 0) before = split_identity();
    __syncthreads();
    SplitSum waves = split_identity();
    for (int w = 0; w < wave; ++w) waves = split_then(waves, wt[w]);
    return split_then(waves, before);
}

// One workgroup = one frame of ONE segment, cut into nsub subsequences (mjpeg_split_plan), lane i on subsequence i; the
// algorithm is described in rtdm_mjpeg.h.  Rounds: each lane but the last decodes its subsequence from the state the lane before
// it arrived in (round 0: from its guess) without storing, and leaves the state it arrives in; states pass through LDS, double
// buffered, so that a round reads only what the round before wrote.  A lane whose start did not change sits the round out.  The
// rounds end when no lane arrived anywhere new (one vote of the workgroup) and after nsub - 1 of them at the latest, by when
// every lane the last one depends on is right.  Then the scan, then the pass that stores.  LDS: 7.3 KB of tables, 16 KB of
// states, 0.6 KB for the scan.  Nothing is shared between workgroups but the totals (vector atomics), so any grid is safe.
// tot[0] frames decoded here, tot[1] their subsequences; *tot_rounds the most rounds any of them took.
__global__ __launch_bounds__(1024) void k_mjpeg_huff_split(const uint8_t* __restrict__ streams, const MjpegDesc* __restrict__ desc,
                                                           const MjpegSeg* __restrict__ segs, int16_t* __restrict__ coef,
                                                           size_t coef_frame_e, int* __restrict__ status, uint32_t split_s,
                                                           unsigned long long* __restrict__ tot, int* __restrict__ tot_rounds)
{
    __shared__ MjpegDesc sd;
    __shared__ MjpegHuff tabs[6];
    __shared__ uint8_t zz[64];
    __shared__ MjpegState handed[2][MJ_SPLIT_LANES];
    __shared__ SplitSum wt[MJ_SPLIT_LANES / 64];
    const uint32_t* src = (const uint32_t*)(desc + blockIdx.x);
    for (unsigned i = threadIdx.x; i < sizeof(MjpegDesc) / 4; i += blockDim.x) ((uint32_t*)&sd)[i] = src[i];
    if (threadIdx.x < 64) zz[threadIdx.x] = c_zigzag[threadIdx.x];
    __syncthreads();
    uint32_t begin, end, sp;
    const uint32_t nsub = split_plan(sd, segs, split_s, &begin, &end, &sp);
    if (nsub < 2) return;                                                       // the whole workgroup: k_mjpeg_huff's frame
    if (nsub > blockDim.x || nsub > MJ_SPLIT_LANES || (uint32_t)sd.mcux * (uint32_t)sd.mcuy == 0) {      // cannot happen; the guard stays
        if (threadIdx.x == 0) atomicMin(&status[blockIdx.x], MJ_BAD_STREAM);
        return;
    }
    const int ncomp = sd.ncomp < 1 ? 1 : (sd.ncomp > 3 ? 3 : sd.ncomp);
    if ((int)threadIdx.x < 2 * ncomp) mjpeg_build_table(sd.bits[threadIdx.x], sd.vals[threadIdx.x], &tabs[threadIdx.x]);
    __syncthreads();
    const uint8_t* s = streams + sd.stream_off;
    const uint32_t i = threadIdx.x;
    const bool active = i < nsub, last = i + 1 == nsub;
    const uint32_t stop = active && !last ? begin + (i + 1) * sp : 0xFFFFFFFFu;
    MjpegState in = mjpeg_state_invalid(), ex = mjpeg_state_invalid();
    MjpegLane res;
    mjpeg_lane_clear(res);
    SplitSum mine = split_identity();
    int cur = 0, rounds = 0;
    for (uint32_t r = 0; r + 1 < nsub; ++r) {                                   // nsub is the workgroup's: every lane loops alike
        bool changed = r == 0;
        if (active) {
            const MjpegState ni = r == 0 ? mjpeg_split_guess(s, begin, end, sp, i) : (i > 0 ? handed[cur][i - 1] : in);
            if (r == 0 || !mjpeg_state_same(ni, in)) {
                in = ni;
                if (!last) {
                    mjpeg_split_pass(s, sd, end, tabs, zz, ni, stop, 0, 0, 0, 0, nullptr, &res);
                    changed = changed || !mjpeg_state_same(res.out, ex);
                    ex = res.out;
                    mine.blocks = res.blocks; mine.m0 = res.m0; mine.m1 = res.m1; mine.m2 = res.m2;
                }
            }
        }
        handed[cur ^ 1][i] = ex;
        cur ^= 1;
        ++rounds;
        if (__syncthreads_and(!changed)) break;
    }
    if (active && i > 0) in = handed[cur][i - 1];
    const SplitSum before = split_scan_exclusive(mine, wt);
    if (active) {
        const int st = mjpeg_split_pass(s, sd, end, tabs, zz, in, stop, before.blocks, mjpeg_clamp_apply(before.m0, 0),
                                        mjpeg_clamp_apply(before.m1, 0), mjpeg_clamp_apply(before.m2, 0),
                                        coef + (size_t)blockIdx.x * coef_frame_e, &res);
        if (st != MJ_OK) atomicMin(&status[blockIdx.x], MJ_BAD_STREAM);
    }
    if (i == 0) {
        atomicAdd(&tot[0], 1ull);
        atomicAdd(&tot[1], (unsigned long long)nsub);
        atomicMax(tot_rounds, rounds);
    }
}

// One ISLOW pass over eight values (jidctint's butterfly; CONST_BITS 13).  32-bit arithmetic holds every value a stream an
// encoder wrote can produce; the saturated coefficients of a damaged stream may wrap, which the GPU's integers do silently.
__device__ __forceinline__ void islow_pass(const int (&x)[8], int (&o)[8], int add, int shift)
{
    int z2 = x[2], z3 = x[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 - z3 * 15137;
    int tmp3 = z1 + z2 * 6270;
    int tmp0 = (x[0] + x[4]) * 8192;         // << CONST_BITS
    int tmp1 = (x[0] - x[4]) * 8192;
    const int t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
    tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    o[0] = (t10 + tmp3 + add) >> shift; o[7] = (t10 - tmp3 + add) >> shift;
    o[1] = (t11 + tmp2 + add) >> shift; o[6] = (t11 - tmp2 + add) >> shift;
    o[2] = (t12 + tmp1 + add) >> shift; o[5] = (t12 - tmp1 + add) >> shift;
    o[3] = (t13 + tmp0 + add) >> shift; o[4] = (t13 - tmp0 + add) >> shift;
}

struct MjpegGeom {        // what the frames of one launch share
    int W, H, ncomp, hs, vs, mcux, mcuy;
    uint32_t first[4];    // first block of component c inside a frame; first[ncomp] = blocks per frame
};

// lane = block `b` of frame blockIdx.y.  coef: 64 int16 per block, natural order; planes: per frame the padded Y plane, then Cb, Cr.
__global__ __launch_bounds__(256) void k_mjpeg_idct(const int16_t* __restrict__ coef, uint8_t* __restrict__ planes, MjpegGeom g)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x, nb = g.first[g.ncomp];
    if (b >= nb) return;
    const int c = (g.ncomp == 3 && b >= g.first[1]) ? (b >= g.first[2] ? 2 : 1) : 0;
    const uint32_t local = b - g.first[c];
    const uint32_t bw = (uint32_t)(g.mcux * (c == 0 ? g.hs : 1));
    const uint32_t by = local / bw, bx = local - by * bw;
    const int4* in = (const int4*)(coef + ((size_t)blockIdx.y * nb + b) * 64);
    int v[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int4 q = in[r];
        v[r][0] = (int16_t)(q.x & 0xFFFF); v[r][1] = q.x >> 16; v[r][2] = (int16_t)(q.y & 0xFFFF); v[r][3] = q.y >> 16;
        v[r][4] = (int16_t)(q.z & 0xFFFF); v[r][5] = q.z >> 16; v[r][6] = (int16_t)(q.w & 0xFFFF); v[r][7] = q.w >> 16;
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {             // columns first, descaled by CONST_BITS - PASS1_BITS = 11
        int x[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = v[r][col];
        islow_pass(x, o, 1024, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r][col] = o[r];
    }
    uint8_t* dst = planes + (size_t)blockIdx.y * nb * 64 + (size_t)g.first[c] * 64 + ((size_t)by * 8 * bw + bx) * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {                   // rows, descaled by CONST_BITS + PASS1_BITS + 3 = 18
        int o[8];
        islow_pass(v[r], o, 131072, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo |= (uint32_t)min(max(o[i] + 128, 0), 255) << (8 * i);
            hi |= (uint32_t)min(max(o[i + 4] + 128, 0), 255) << (8 * i);
        }
        *(uint2*)(dst + (size_t)r * bw * 8) = make_uint2(lo, hi);
    }
}

// J3 for the pixel (x, y) of a chroma plane sampled hs x vs coarser; n x m is the plane's TRUE size (not the padded one).
// As in libjpeg, planes of one or two columns are replicated, not interpolated.
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ pl, int pitch, int x, int y, int n, int m, int hs, int vs)
{
    if (hs == 1) return pl[(size_t)y * pitch + x];
    if (n <= 2) return pl[(size_t)(y >> (vs - 1)) * pitch + (x >> 1)];
    const int i = x >> 1, nb = (x & 1) ? min(i + 1, n - 1) : max(i - 1, 0);
    if (vs == 1) {
        const uint8_t* row = pl + (size_t)y * pitch;
        return (3 * row[i] + row[nb] + 1 + (x & 1)) >> 2;
    }
    const int r = y >> 1, fr = (y & 1) ? min(r + 1, m - 1) : max(r - 1, 0);
    const uint8_t* near = pl + (size_t)r * pitch;
    const uint8_t* far = pl + (size_t)fr * pitch;
    const int s = 3 * near[i] + far[i], sn = 3 * near[nb] + far[nb];
    return (3 * s + sn + 8 - (x & 1)) >> 4;
}

// lane = one output pixel of frame blockIdx.z
__global__ __launch_bounds__(256) void k_mjpeg_rgb(const uint8_t* __restrict__ planes, MjpegGeom g, uint8_t* __restrict__ rgb,
                                                   size_t pitch, size_t frame_stride)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const uint8_t* fp = planes + (size_t)blockIdx.z * g.first[g.ncomp] * 64;
    const int ypitch = g.mcux * g.hs * 8;
    const int Y = fp[(size_t)y * ypitch + x];
    int R = Y, G = Y, B = Y;
    if (g.ncomp == 3) {
        const int cpitch = g.mcux * 8, n = (g.W + g.hs - 1) / g.hs, m = (g.H + g.vs - 1) / g.vs;
        const int cb = chroma_at(fp + (size_t)g.first[1] * 64, cpitch, x, y, n, m, g.hs, g.vs) - 128;
        const int cr = chroma_at(fp + (size_t)g.first[2] * 64, cpitch, x, y, n, m, g.hs, g.vs) - 128;
        R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
        G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
        B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
    }
    uint8_t* o = rgb + (size_t)blockIdx.z * frame_stride + (size_t)y * pitch + (size_t)x * 3;
    o[0] = (uint8_t)R; o[1] = (uint8_t)G; o[2] = (uint8_t)B;
}

static MjpegGeom make_geom(const MjpegDesc& d)
{
    MjpegGeom g;
    g.W = d.W; g.H = d.H; g.ncomp = d.ncomp; g.hs = d.hs; g.vs = d.vs; g.mcux = d.mcux; g.mcuy = d.mcuy;
    for (int c = 0; c < 4; ++c) g.first[c] = mjpeg_comp_first_block(d, c < d.ncomp ? c : d.ncomp);
    return g;
}

void launch_mjpeg(const uint8_t* d_streams, const MjpegDesc* d_desc, const MjpegSeg* d_segs, int m, const MjpegDesc& shape,
                  unsigned max_nseg, const MjpegSplitCall& split, int16_t* d_coef, uint8_t* d_planes, uint8_t* d_rgb, size_t pitch,
                  size_t frame_stride, int* d_status, hipStream_t s)
{
    const MjpegGeom g = make_geom(shape);
    const size_t nb = g.first[g.ncomp];
    const unsigned lanes = max_nseg <= 64 ? 64u : (max_nseg <= 128 ? 128u : 256u);
    // both kernels get every frame of the call and each leaves the other's at once; a kernel that has no frame is not launched
    if (split.frames < m)
        hipLaunchKernelGGL(k_mjpeg_huff, dim3(m), dim3(lanes), 0, s, d_streams, d_desc, d_segs, d_coef, nb * 64, d_status,
                           split.frames ? split.bytes : 0u);
    if (split.frames > 0)
        hipLaunchKernelGGL(k_mjpeg_huff_split, dim3(m), dim3(mjpeg_split_lanes(split.max_nsub)), 0, s, d_streams, d_desc, d_segs, d_coef,
                           nb * 64, d_status, split.bytes, split.totals, split.max_rounds);
    hipLaunchKernelGGL(k_mjpeg_idct, dim3((unsigned)((nb + 255) / 256), m), dim3(256), 0, s, d_coef, d_planes, g);
    hipLaunchKernelGGL(k_mjpeg_rgb, dim3((g.W + 63) / 64, (g.H + 3) / 4, m), dim3(256), 0, s, d_planes, g, d_rgb, pitch, frame_stride);
}

}  // namespace rtdm
