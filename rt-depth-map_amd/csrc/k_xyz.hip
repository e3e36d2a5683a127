// k_xyz.hip -- reprojectImageTo3D on the device (estimator.cpp:76): the dense xyz map / Z plane and the compacted, coloured
// point cloud of the pixels calc_depth would keep (estimator.cpp:235).  Rules X1-X8, DESIGN.md section 4.11.
//
// A frame is walked as the linear pixel index p = y * W + x, so row-major order is index order and there is no row limit.
// W * H fits an int (rtdm_xyz_create), and so does the last index of the last tile, so p is 32-bit unsigned arithmetic.
// One workgroup of 256 lanes owns a tile of XYZ_TILE = 1024 consecutive pixels as four chunks of 256: lane t of chunk k
// holds pixel tile * 1024 + k * 256 + t, so every load and store of a chunk is lane-consecutive.
//
// The cloud never waits for another workgroup (X8):  k_xyz_count (kept pixels per tile)  ->  k_xyz_scan (one workgroup per
// frame: exclusive scan of the tile counts, total = counts[f])  ->  k_xyz_scatter (the predicate again; rank inside a wave
// from __ballot + v_mbcnt, wave offsets inside the tile through LDS, tile offset from the scan).  No atomic decides a
// position.  With handle_missing_values the per-frame minimum is a pass of its own in front (k_xyz_min); its atomicMin
// is an integer minimum, which is the same whatever order its workgroups (row groups, not tiles) arrive in.  It is the only
// frame-minimum kernel: calc_depth (k_depth.hip), the per-object depth (k_depth_objects.hip) and the measurements
// (k_measure.hip) call launch_xyz_min too.  Z (X3 + X4) and the Z part of the keep test (X6) are rtdm_xyz_point.h's, shared
// with k_measure.hip.
//
// Floating point (X2, X3): every multiply and add of the homogeneous point is a double operation rounded on its own, in
// the written order -- contraction is off inside xyz_h (rtdm_xyz_point.h) -- then one IEEE double division and one
// rounding to float.
#include "rtdm_kernels.h"
#include "rtdm_xyz_point.h"

namespace rtdm {

static const int XYZ_CHUNKS = XYZ_TILE / 256;
static const int XYZ_MIN_GROUPS = 64;               // row groups of a frame in k_xyz_min: more of them meet at one atomicMin

// X6
__device__ __forceinline__ bool xyz_keep(const XyzParams& P, int disp, float z, int maskbyte)
{
    return disp != P.invalid16 && xyz_keep_z(P, z) && maskbyte != 0;
}

__device__ __forceinline__ int xyz_lane_rank(unsigned long long ballot)   // set bits below this lane
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// X4: minimum key of every frame.  minkey[f] starts above every key (launch_xyz_min sets it).  grid: (row groups, frames): a
// workgroup walks the rows y = blockIdx.x, blockIdx.x + gridDim.x, ... of its frame, so no pixel index is formed and no
// frame size is too large; a wave's minimum by shuffles, the workgroup's through four words of LDS, one atomicMin.
__global__ __launch_bounds__(256) void k_xyz_min(XyzDisp D, int W, int H, int mode, int* minkey)
{
    __shared__ int red[4];
    const int16_t* disp = D.base + (size_t)blockIdx.y * D.frame_e;
    int m = 0x7fffffff;
    for (int y = blockIdx.x; y < H; y += gridDim.x)
        for (int x = threadIdx.x; x < W; x += 256) m = min(m, xyz_key(disp[(size_t)y * D.pitch_e + x], mode));
    for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMin(minkey + blockIdx.y, min(min(red[0], red[1]), min(red[2], red[3])));
}

// X5: the dense map.  xyz: 3 floats per pixel; zp: the Z plane; either may be null.
__global__ __launch_bounds__(256) void k_xyz_map(XyzDisp D, int W, unsigned WH, XyzParams P, const int* minkey, XyzMap O)
{
    const int f = blockIdx.y;
    const int16_t* disp = D.base + (size_t)f * D.frame_e;
    const int mk = P.hmv ? minkey[f] : 0;
#pragma unroll
    for (int k = 0; k < XYZ_CHUNKS; ++k) {
        const unsigned p = blockIdx.x * (unsigned)XYZ_TILE + k * 256 + threadIdx.x;
        if (p >= WH) continue;
        const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
        const int key = xyz_key(disp[(size_t)y * D.pitch_e + x], P.mode);
        const double d = xyz_d(key, P.mode), xd = (double)x, yd = (double)y;
        double h3;
        const float z = xyz_z(P, key, P.hmv, mk, xd, yd, d, &h3);
        if (O.xyz) {
            float* o = O.xyz + (size_t)f * O.xyz_frame + (size_t)y * O.xyz_pitch + 3 * (size_t)x;
            o[0] = (float)(xyz_h(P, 0, xd, yd, d) / h3);
            o[1] = (float)(xyz_h(P, 1, xd, yd, d) / h3);
            o[2] = z;
        }
        if (O.z) O.z[(size_t)f * O.z_frame + (size_t)y * O.z_pitch + x] = z;
    }
}

// the pixel of chunk k of this lane: position, key, Z, h_3 and the keep flag (X6)
struct XyzPix { int x, y, key; float z; double h3; bool keep; };

__device__ __forceinline__ XyzPix xyz_pixel(const XyzCloudIn& I, int f, int W, unsigned WH, const XyzParams& P, int mk, int k)
{
    XyzPix px{0, 0, 0, 0.0f, 0.0, false};
    const unsigned p = blockIdx.x * (unsigned)XYZ_TILE + k * 256 + threadIdx.x;
    if (p < WH) {
        px.y = (int)(p / (unsigned)W); px.x = (int)(p - (unsigned)px.y * (unsigned)W);
        const int disp = I.disp.base[(size_t)f * I.disp.frame_e + (size_t)px.y * I.disp.pitch_e + px.x];
        px.key = xyz_key(disp, P.mode);
        const double d = xyz_d(px.key, P.mode), xd = (double)px.x, yd = (double)px.y;
        px.z = xyz_z(P, px.key, P.hmv, mk, xd, yd, d, &px.h3);
        const int mb = I.mask ? I.mask[(size_t)f * I.mframe + (size_t)px.y * I.mpitch + px.x] : 1;
        px.keep = xyz_keep(P, disp, px.z, mb);
    }
    return px;
}

// X8, pass 1: kept pixels of every tile
__global__ __launch_bounds__(256) void k_xyz_count(XyzCloudIn I, int W, unsigned WH, XyzParams P, const int* minkey,
                                                   int* tile_cnt, int tiles)
{
    __shared__ int wsum[4];
    const int f = blockIdx.y;
    const int mk = P.hmv ? minkey[f] : 0;
    int c = 0;                                         // wave-uniform
#pragma unroll
    for (int k = 0; k < XYZ_CHUNKS; ++k) c += __popcll(__ballot(xyz_pixel(I, f, W, WH, P, mk, k).keep));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[(size_t)f * tiles + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// X8, pass 2: one workgroup per frame turns its tile counts into exclusive offsets, in place, and stores the total
__global__ __launch_bounds__(256) void k_xyz_scan(int* tile_cnt, int tiles, int* counts)
{
    __shared__ int sc[256];
    int* t = tile_cnt + (size_t)blockIdx.x * tiles;
    int carry = 0;
    for (int base = 0; base < tiles; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < tiles ? t[i] : 0;
        sc[threadIdx.x] = v;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {
            const int a = threadIdx.x >= s ? sc[threadIdx.x - s] : 0;
            __syncthreads();
            sc[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < tiles) t[i] = carry + sc[threadIdx.x] - v;
        carry += sc[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// X7 + X8, pass 3: the predicate again, then record number = tile offset + offset of (chunk, wave) inside the tile + rank
// inside the wave.  Records at or beyond `capacity` are not written.
__global__ __launch_bounds__(256) void k_xyz_scatter(XyzCloudIn I, int W, unsigned WH, XyzParams P, const int* minkey,
                                                     const int* tile_off, int tiles, XyzRec* points, size_t points_frame_b,
                                                     int capacity)
{
    __shared__ int wsum[XYZ_CHUNKS * 4];               // [chunk][wave] counts, then exclusive offsets
    const int f = blockIdx.y, wave = threadIdx.x >> 6;
    const int mk = P.hmv ? minkey[f] : 0;
    const int toff = tile_off[(size_t)f * tiles + blockIdx.x];
    if (toff >= capacity) return;                      // uniform: every record of this tile lies beyond the capacity
    XyzPix px[XYZ_CHUNKS];
    int rank[XYZ_CHUNKS];
#pragma unroll
    for (int k = 0; k < XYZ_CHUNKS; ++k) {
        px[k] = xyz_pixel(I, f, W, WH, P, mk, k);
        const unsigned long long b = __ballot(px[k].keep);
        rank[k] = xyz_lane_rank(b);
        if ((threadIdx.x & 63) == 0) wsum[k * 4 + wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < XYZ_CHUNKS * 4; ++i) { const int v = wsum[i]; wsum[i] = run; run += v; }
    }
    __syncthreads();
    XyzRec* out = (XyzRec*)((unsigned char*)points + (size_t)f * points_frame_b);
#pragma unroll
    for (int k = 0; k < XYZ_CHUNKS; ++k) {
        if (!px[k].keep) continue;
        const int pos = toff + wsum[k * 4 + wave] + rank[k];
        if (pos >= capacity) continue;
        const int x = px[k].x, y = px[k].y;
        const double d = xyz_d(px[k].key, P.mode), xd = (double)x, yd = (double)y;
        const double h3 = px[k].h3;
        XyzRec r;
        r.x = (float)(xyz_h(P, 0, xd, yd, d) / h3);
        r.y = (float)(xyz_h(P, 1, xd, yd, d) / h3);
        r.z = px[k].z;
        unsigned c = 0xff000000u;                      // a = 255; r = g = b = 0 without a guide
        if (I.cn == 1) {
            const unsigned g = I.guide[(size_t)f * I.gframe + (size_t)y * I.gpitch + x];
            c |= g | (g << 8) | (g << 16);
        } else if (I.cn == 3) {
            const uint8_t* g = I.guide + (size_t)f * I.gframe + (size_t)y * I.gpitch + 3 * (size_t)x;
            c |= (unsigned)g[0] | ((unsigned)g[1] << 8) | ((unsigned)g[2] << 16);
        }
        r.rgba = c;
        out[pos] = r;
    }
}

int xyz_tiles(int W, int H) { return (int)(((unsigned)W * (unsigned)H + XYZ_TILE - 1) / XYZ_TILE); }

// One memset and one kernel; one more kernel for every further 32768 frames (a grid's second dimension ends at 65535).
void launch_xyz_min(XyzDisp D, int n, int W, int H, int mode, int* minkey, hipStream_t stream)
{
    // the initial minimum is written on the device -- 0x7f7f7f7f is above every key (a key is at most an int16) --: an async
    // copy from a stack local would only be safe if the runtime staged pageable sources at enqueue time
    (void)hipMemsetAsync(minkey, 0x7f, (size_t)n * sizeof(int), stream);
    for (int f0 = 0; f0 < n; f0 += 32768)
        hipLaunchKernelGGL(k_xyz_min, dim3(std::min(H, XYZ_MIN_GROUPS), std::min(n - f0, 32768)), dim3(256), 0, stream,
                           XyzDisp{D.base + (size_t)f0 * D.frame_e, D.pitch_e, D.frame_e}, W, H, mode, minkey + f0);
}

void launch_xyz_map(XyzDisp D, int n, int W, int H, const XyzParams& P, int* minkey, XyzMap O, hipStream_t stream)
{
    if (P.hmv) launch_xyz_min(D, n, W, H, P.mode, minkey, stream);
    hipLaunchKernelGGL(k_xyz_map, dim3(xyz_tiles(W, H), n), dim3(256), 0, stream, D, W, (unsigned)W * (unsigned)H, P, minkey, O);
}

void launch_xyz_cloud(const XyzCloudIn& I, int n, int W, int H, const XyzParams& P, int* minkey, int* tile_cnt, XyzRec* points,
                      size_t points_frame_b, int capacity, int* counts, hipStream_t stream)
{
    const int tiles = xyz_tiles(W, H);
    const unsigned WH = (unsigned)W * (unsigned)H;
    if (P.hmv) launch_xyz_min(I.disp, n, W, H, P.mode, minkey, stream);
    hipLaunchKernelGGL(k_xyz_count, dim3(tiles, n), dim3(256), 0, stream, I, W, WH, P, minkey, tile_cnt, tiles);
    hipLaunchKernelGGL(k_xyz_scan, dim3(n), dim3(256), 0, stream, tile_cnt, tiles, counts);
    if (capacity > 0)
        hipLaunchKernelGGL(k_xyz_scatter, dim3(tiles, n), dim3(256), 0, stream, I, W, WH, P, minkey, tile_cnt, tiles, points,
                           points_frame_b, capacity);
}

}  // namespace rtdm
