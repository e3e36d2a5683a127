// k_objects.hip -- the object detection that produces the matcher's ROI, on the device:
//     cvtColor(BGR2HSV) + inRange                     (/root/reference/estimator.cpp:40-43)   -> k_hsv_inrange
//     [morphFilter->run: k_morph.hip]                 (estimator.cpp:45)
//     findContours(RETR_EXTERNAL) + boundingRect      (estimator.cpp:47, 167-174)             -> k_cc_*
// Semantics: oracle/objects_oracle.c.  Connected components by union-find over one label plane: foreground pixels
// are united 8-connected, background pixels 4-connected, background on the image border with a virtual frame node
// (index W*H).  Roots are the smallest index of a set = the component's first pixel in raster order, which is what
// decides both the contour order and (through the background left of it) whether the component is external.
// Frame batches and several colour classes per call: k_hsv_classes writes one mask plane per class,
// the labelling kernels take their plane from blockIdx.y, and k_cc_count / k_cc_scan / k_cc_scatter select and order the boxes
// on the device, where the single-frame path collects records in arbitrary order (k_cc_collect) for a host sort.
// Which pixels belong to which stored object: k_cc_scatter<true> leaves every root its object's id,
// k_cc_labels writes the label planes from them, run by run, and adds up the raw moments of every object's pixels.
#include <mutex>
#include "rtdm_kernels.h"
#include "rtdm_device.h"

namespace rtdm {

struct HsvTabs { int sdiv[256], hdiv[256]; };
static __device__ HsvTabs g_hsv;

__global__ void k_hsv_tabs()
{
    const int i = threadIdx.x;
    // round(255*4096 / i), round(180*4096 / (6 i)): exact in integers (no quotient is a tie)
    g_hsv.sdiv[i] = i ? ((255 << 12) * 2 + i) / (2 * i) : 0;
    g_hsv.hdiv[i] = i ? ((180 << 12) * 2 + 6 * i) / (12 * i) : 0;
}

__global__ __launch_bounds__(256) void k_hsv_inrange(const uint8_t* rgb, size_t pitch, int W, int H, int lh, int ls, int lv,
                                                     int hh, int hs, int hv, uint8_t* mask, size_t mpitch)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W * H) return;
    const int y = idx / W, x = idx - y * W;
    const uint8_t* p = rgb + (size_t)y * pitch + (size_t)x * 3;
    const int r = p[0], g = p[1], b = p[2];
    const int v = max(r, max(g, b)), vmin = min(r, min(g, b)), diff = v - vmin;
    const int s = (diff * g_hsv.sdiv[v] + (1 << 11)) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * g_hsv.hdiv[diff] + (1 << 11)) >> 12;
    if (h < 0) h += 180;
    h = min(max(h, 0), 255);
    const bool ok = h >= lh && h <= hh && s >= ls && s <= hs && v >= lv && v <= hv;
    mask[(size_t)y * mpitch + x] = ok ? 255 : 0;
}

__device__ __forceinline__ bool cc_fg(const uint8_t* mask, size_t mpitch, int W, int H, int x, int y, int zero_border)
{
    if (zero_border && (x == 0 || y == 0 || x == W - 1 || y == H - 1)) return false;
    return mask[(size_t)y * mpitch + x] != 0;
}

struct OpMax {
    static __device__ int id() { return 0; }
    static __device__ int f(int a, int b) { return max(a, b); }
};

// The planes of one labelling launch: plane i (blockIdx.y) has its mask at mask + i * mplane and its workspace at
// scratch + i * splane -- boxes first, then the labels at label_off (layout: cc_scratch_bytes).  Labels are indices inside
// their own plane.
struct CcPlanes { const uint8_t* mask; size_t mpitch, mplane; uint8_t* scratch; size_t splane, label_off; };
__device__ __forceinline__ const uint8_t* cc_mask(const CcPlanes& P) { return P.mask + (size_t)blockIdx.y * P.mplane; }
__device__ __forceinline__ int4* cc_box(const CcPlanes& P) { return (int4*)(P.scratch + (size_t)blockIdx.y * P.splane); }
__device__ __forceinline__ int32_t* cc_label(const CcPlanes& P) { return (int32_t*)(P.scratch + (size_t)blockIdx.y * P.splane + P.label_off); }

// One workgroup per row: every pixel's parent becomes the first pixel of its horizontal run of same-kind pixels
// (max-scan of "run starts here" flags), so no union is ever needed along a row.  count_off != 0: the plane's record
// counter of k_cc_collect, zeroed here.
__global__ __launch_bounds__(256) void k_cc_rows(CcPlanes P, int W, int H, int zero_border, size_t count_off)
{
    extern __shared__ int sc[];
    __shared__ int wsum[4];
    const uint8_t* mask = cc_mask(P);
    const size_t mpitch = P.mpitch;
    int32_t* label = cc_label(P);
    int4* box = cc_box(P);
    const int y = blockIdx.x;
    for (int x = threadIdx.x; x < W; x += 256) {
        const bool v = cc_fg(mask, mpitch, W, H, x, y, zero_border);
        const bool start = x == 0 || cc_fg(mask, mpitch, W, H, x - 1, y, zero_border) != v;
        sc[x] = start ? x + 1 : 0;
    }
    __syncthreads();
    row_scan<OpMax>(sc, W, wsum);
    for (int x = threadIdx.x; x < W; x += 256) {
        label[y * W + x] = y * W + sc[x] - 1;
        box[y * W + x] = make_int4(x, y, x, y);
    }
    if (y == 0 && threadIdx.x == 0) {
        label[W * H] = W * H;
        if (count_off) *(int*)(P.scratch + (size_t)blockIdx.y * P.splane + count_off) = 0;
    }
}

__global__ __launch_bounds__(256) void k_cc_merge(CcPlanes P, int W, int H, int zero_border)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= W * H) return;
    const uint8_t* mask = cc_mask(P);
    const size_t mpitch = P.mpitch;
    int32_t* label = cc_label(P);
    const int y = p / W, x = p - y * W;
    const bool v = cc_fg(mask, mpitch, W, H, x, y, zero_border);
    const bool hasL = x > 0, hasU = y > 0;
    const bool l = hasL && cc_fg(mask, mpitch, W, H, x - 1, y, zero_border) == v;            // left neighbour of my kind
    const bool u = hasU && cc_fg(mask, mpitch, W, H, x, y - 1, zero_border) == v;            // upper neighbour of my kind
    const bool ul = hasL && hasU && cc_fg(mask, mpitch, W, H, x - 1, y - 1, zero_border) == v;
    // a vertical contact needs one union per segment: if my left neighbour and the pixel above it are of my kind too,
    // they made the link for both runs (rows are already joined by k_cc_rows)
    if (u && !(l && ul)) uf_union(label, p, p - W);
    if (v) {
        // foreground is 8-connected; the diagonals matter only when the pixel above is background
        if (!u && ul) uf_union(label, p, p - W - 1);
        if (!u && hasU && x + 1 < W && cc_fg(mask, mpitch, W, H, x + 1, y - 1, zero_border)) uf_union(label, p, p - W + 1);
    } else if ((x == 0 || y == 0 || x == W - 1 || y == H - 1) && !(l && (y == 0 || y == H - 1)) && !(u && (x == 0 || x == W - 1))) {
        uf_union(label, p, W * H);                       // background on the image border hangs on the frame node (once per border run)
    }
}

// Boxes from the horizontal runs only: a run's first pixel reports (min x, min y, max y), its last pixel (max x).
// A blob of 100k pixels would otherwise serialise 400k atomics on the four words of its root.
__global__ __launch_bounds__(256) void k_cc_bbox(CcPlanes P, int W, int H, int zero_border)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= W * H) return;
    const uint8_t* mask = cc_mask(P);
    const size_t mpitch = P.mpitch;
    int32_t* label = cc_label(P);
    int4* box = cc_box(P);
    const int y = p / W, x = p - y * W;
    if (!cc_fg(mask, mpitch, W, H, x, y, zero_border)) return;
    const bool first = x == 0 || !cc_fg(mask, mpitch, W, H, x - 1, y, zero_border);
    const bool last = x == W - 1 || !cc_fg(mask, mpitch, W, H, x + 1, y, zero_border);
    if (!first && !last) return;
    const int r = uf_find(label, p);
    if (r == p) return;                                  // the root's own coordinates are its initial box
    int* b = (int*)&box[r];
    if (first) { atomicMin(b + 0, x); atomicMin(b + 1, y); atomicMax(b + 3, y); }
    if (last) atomicMax(b + 2, x);
}

// one record per foreground root: first pixel, box, external flag
__global__ __launch_bounds__(256) void k_cc_collect(const uint8_t* mask, size_t mpitch, int32_t* label, const int4* box, int W, int H,
                                                    int zero_border, int* count, int* records, int max_records)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= W * H) return;
    const int y = p / W, x = p - y * W;
    if (!cc_fg(mask, mpitch, W, H, x, y, zero_border) || ld_relaxed(&label[p]) != p) return;
    const bool external = x == 0 || uf_find(label, p - 1) == uf_find(label, W * H);
    const int slot = atomicAdd(count, 1);
    if (slot >= max_records) return;
    const int4 b = box[p];
    int* r = records + 6 * slot;
    r[0] = p; r[1] = b.x; r[2] = b.y; r[3] = b.z - b.x + 1; r[4] = b.w - b.y + 1; r[5] = external ? 1 : 0;
}

// ---- frame batches and colour classes (rules O1-O6) ------------------------------------------------
// O1: one conversion per pixel, every range tested, one mask byte per class plane (plane f * nclasses + c).  A lane owns four
// neighbouring pixels of a row: twelve colour bytes are three dwords and four mask bytes one, where the caller's strides keep
// them aligned (rgb4 / mask4); the last pixels of a row whose width is no multiple of four, and every other layout, go byte
// by byte.
struct HsvFrames { const uint8_t* rgb; size_t pitch, frame; uint8_t* mask; size_t mpitch, mplane; int rgb4, mask4; };

__device__ __forceinline__ unsigned hsv_class_bits(int r, int g, int b, const HsvClasses& C)
{
    const int v = max(r, max(g, b)), vmin = min(r, min(g, b)), diff = v - vmin;
    const int s = (diff * g_hsv.sdiv[v] + (1 << 11)) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * g_hsv.hdiv[diff] + (1 << 11)) >> 12;
    if (h < 0) h += 180;
    h = min(max(h, 0), 255);
    unsigned bits = 0;
    for (int i = 0; i < C.nranges; ++i) {
        const bool ok = h >= C.lo[i][0] && h <= C.hi[i][0] && s >= C.lo[i][1] && s <= C.hi[i][1] && v >= C.lo[i][2] && v <= C.hi[i][2];
        bits |= (ok ? 1u : 0u) << C.cls[i];
    }
    return bits;
}

__global__ __launch_bounds__(256) void k_hsv_classes(HsvFrames F, int W, int H, int quads, HsvClasses C)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= quads * H) return;
    const int f = blockIdx.y;
    const int y = q / quads, x0 = (q - y * quads) * 4;
    const int npx = min(4, W - x0);
    const uint8_t* p = F.rgb + (size_t)f * F.frame + (size_t)y * F.pitch + (size_t)x0 * 3;
    unsigned b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    if (F.rgb4 && npx == 4) {
        const uint32_t* d = (const uint32_t*)p;
        const uint32_t u = d[0], v = d[1], w = d[2];
        b0 = hsv_class_bits(u & 255, (u >> 8) & 255, (u >> 16) & 255, C);
        b1 = hsv_class_bits(u >> 24, v & 255, (v >> 8) & 255, C);
        b2 = hsv_class_bits((v >> 16) & 255, v >> 24, w & 255, C);
        b3 = hsv_class_bits((w >> 8) & 255, (w >> 16) & 255, w >> 24, C);
    } else {
        b0 = hsv_class_bits(p[0], p[1], p[2], C);
        if (npx > 1) b1 = hsv_class_bits(p[3], p[4], p[5], C);
        if (npx > 2) b2 = hsv_class_bits(p[6], p[7], p[8], C);
        if (npx > 3) b3 = hsv_class_bits(p[9], p[10], p[11], C);
    }
    uint8_t* m = F.mask + (size_t)f * C.nclasses * F.mplane + (size_t)y * F.mpitch + x0;
    for (int c = 0; c < C.nclasses; ++c, m += F.mplane) {
        const unsigned m0 = ((b0 >> c) & 1) * 255u, m1 = ((b1 >> c) & 1) * 255u, m2 = ((b2 >> c) & 1) * 255u, m3 = ((b3 >> c) & 1) * 255u;
        if (F.mask4 && npx == 4) {
            *(uint32_t*)m = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
        } else {
            m[0] = (uint8_t)m0;
            if (npx > 1) m[1] = (uint8_t)m1;
            if (npx > 2) m[2] = (uint8_t)m2;
            if (npx > 3) m[3] = (uint8_t)m3;
        }
    }
}

// O3 + O4 without a sort: the kept records of a plane are its foreground roots (= first pixels) that are external and whose
// box passes min_area, and their order is the descending order of those pixels.  k_cc_count (kept roots per chunk of 256
// pixels) -> k_cc_scan (one workgroup per frame: the chunk counts of every class plane become exclusive offsets in place,
// the plane totals the counts and the class offsets) -> k_cc_scatter (the predicate again; rank = chunk offset + wave offset
// + lanes below, position = class offset + kept of the plane - 1 - rank).  No atomic decides a position and no workgroup
// waits for another.  The union box is an integer min / max, the same in whatever order the waves arrive; it is gathered in
// roi[f] as (min x, min y, max x, max y) and turned into (x, y, w, h) by k_cc_roi.
// Behind a plane's chunk counts (cnt_off, `chunks` ints) lie its two totals: {kept, class offset}.
struct CcSelect { int W, H, zero_border, min_area, nclasses, chunks; size_t cnt_off; };
__device__ __forceinline__ int* cc_cnt(const CcPlanes& P, const CcSelect& S, int plane)
{ return (int*)(P.scratch + (size_t)plane * P.splane + S.cnt_off); }

__device__ __forceinline__ bool cc_keep(const CcPlanes& P, const CcSelect& S, int p, int4* b)
{
    const int W = S.W, H = S.H;
    if (p >= W * H) return false;
    const uint8_t* mask = cc_mask(P);
    int32_t* label = cc_label(P);
    const int y = p / W, x = p - y * W;
    if (!cc_fg(mask, P.mpitch, W, H, x, y, S.zero_border) || ld_relaxed(&label[p]) != p) return false;
    if (x != 0 && uf_find(label, p - 1) != uf_find(label, W * H)) return false;            // enclosed by another component
    *b = cc_box(P)[p];
    return (b->z - b->x + 1) * (b->w - b->y + 1) >= S.min_area;
}

__device__ __forceinline__ int cc_lane_rank(unsigned long long ballot)   // set bits below this lane
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

__global__ __launch_bounds__(256) void k_cc_count(CcPlanes P, CcSelect S)
{
    __shared__ int wsum[4];
    int4 b;
    const int c = __popcll(__ballot(cc_keep(P, S, blockIdx.x * 256 + threadIdx.x, &b)));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cc_cnt(P, S, blockIdx.y)[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void k_cc_scan(CcPlanes P, CcSelect S, int* counts, int* roi)
{
    __shared__ int sc[256];
    const int f = blockIdx.x;
    int class_off = 0;
    for (int c = 0; c < S.nclasses; ++c) {
        int* t = cc_cnt(P, S, f * S.nclasses + c);
        int carry = 0;
        for (int base = 0; base < S.chunks; base += 256) {
            const int i = base + threadIdx.x;
            const int v = i < S.chunks ? t[i] : 0;
            sc[threadIdx.x] = v;
            __syncthreads();
            for (int s = 1; s < 256; s <<= 1) {
                const int a = threadIdx.x >= s ? sc[threadIdx.x - s] : 0;
                __syncthreads();
                sc[threadIdx.x] += a;
                __syncthreads();
            }
            if (i < S.chunks) t[i] = carry + sc[threadIdx.x] - v;
            carry += sc[255];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            t[S.chunks] = carry; t[S.chunks + 1] = class_off;
            counts[f * S.nclasses + c] = carry;
        }
        class_off += carry;
    }
    if (threadIdx.x == 0) { roi[4 * f] = 1000000; roi[4 * f + 1] = 1000000; roi[4 * f + 2] = -1000000; roi[4 * f + 3] = -1000000; }
}

// IDS (labels or stats are wanted, rule L1): every foreground root also gets its object's id in the first word of its own box
// entry, written by the lane that has just read that entry -- 1 + position for a stored object, 0 for a root that is not kept
// or lies beyond the capacity -- and a stored object's moments start at zero.  k_cc_labels reads the id from there.
template <bool IDS>
__global__ __launch_bounds__(256) void k_cc_scatter(CcPlanes P, CcSelect S, CcObject* objects, int capacity, int* roi, CcStats* stats)
{
    __shared__ int wsum[4];
    const int plane = blockIdx.y, f = plane / S.nclasses, cls = plane - f * S.nclasses, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * 256 + threadIdx.x;
    int4 b = make_int4(0, 0, 0, 0);
    const bool keep = cc_keep(P, S, p, &b);
    if (IDS && !keep && p < S.W * S.H && cc_fg(cc_mask(P), P.mpitch, S.W, S.H, p % S.W, p / S.W, S.zero_border) &&
        ld_relaxed(&cc_label(P)[p]) == p)
        cc_box(P)[p].x = 0;
    const unsigned long long bal = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    if (bal == 0) return;                                                   // wave-uniform, behind the only barrier
    int below = 0;
    for (int q = 0; q < wave; ++q) below += wsum[q];
    const int* t = cc_cnt(P, S, plane);
    const int rank = t[blockIdx.x] + below + cc_lane_rank(bal);
    const int pos = t[S.chunks + 1] + t[S.chunks] - 1 - rank;
    if (keep && pos < capacity) {
        CcObject* o = objects + (size_t)f * capacity + pos;          // member stores: the caller's array only has int alignment
        o->x = b.x; o->y = b.y; o->w = b.z - b.x + 1; o->h = b.w - b.y + 1;
        o->cls = cls; o->first_pixel = p; o->reserved[0] = 0; o->reserved[1] = 0;
    }
    if (IDS && keep) {
        const bool stored = pos < capacity;
        cc_box(P)[p].x = stored ? pos + 1 : 0;
        if (stored && stats) stats[(size_t)f * capacity + pos] = CcStats{0, 0, 0, 0, 0, 0};
    }
    int x0 = keep ? b.x : 1000000, y0 = keep ? b.y : 1000000, x1 = keep ? b.z + 1 : -1000000, y1 = keep ? b.w + 1 : -1000000;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o)); y0 = min(y0, __shfl_xor(y0, o));
        x1 = max(x1, __shfl_xor(x1, o)); y1 = max(y1, __shfl_xor(y1, o));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(roi + 4 * f, x0); atomicMin(roi + 4 * f + 1, y0); atomicMax(roi + 4 * f + 2, x1); atomicMax(roi + 4 * f + 3, y1);
    }
}

// L1 / L2: one workgroup per row of a plane, run-based like k_cc_rows.  The max-scan gives every pixel the start of its run;
// the LAST pixel of a foreground run [a, x] finds the root from a, reads the id k_cc_scatter left there and leaves it at
// sc[a], where no other run reads or writes.  Then the row goes out from LDS, lane after lane: whole waves of neighbouring
// dwords, or of 16-byte quads where base, pitch and plane stride allow (vec4).  No atomic decides a label.
// Moments: a run's closed-form sums (n, sum x, sum x^2; the other three follow from the row's y) are first combined per id
// inside the row, in a table of CC_ROW_IDS entries in LDS (open addressing, CC_ROW_PROBES tries), and one lane per used entry
// adds the row's share to the object's six words with 64-bit integer atomics -- the same sum in any order.  A run that
// finds no entry adds its own share directly.  (Per-run atomics on the words of one object cost 4.5 ms on a 934x404 frame
// of 60 % noise, whose largest component has some 60000 runs: profiles/objects_labels_time.txt.)
#define CC_ROW_IDS 64
#define CC_ROW_PROBES 8
__device__ __forceinline__ void cc_add_moments(CcStats* s, long long y, unsigned long long n, unsigned long long sx, unsigned long long sxx)
{
    unsigned long long* m = (unsigned long long*)s;
    atomicAdd(m + 0, n); atomicAdd(m + 1, sx); atomicAdd(m + 2, n * y);
    atomicAdd(m + 3, sxx); atomicAdd(m + 4, sx * y); atomicAdd(m + 5, n * y * y);
}

__global__ __launch_bounds__(256) void k_cc_labels(CcPlanes P, int W, int H, int zero_border, int nclasses, int capacity, CcLabelsOut O,
                                                   int vec4)
{
    extern __shared__ int sc[];
    __shared__ int wsum[4];
    __shared__ int row_id[CC_ROW_IDS];
    __shared__ unsigned long long row_sum[CC_ROW_IDS][3];
    const uint8_t* mask = cc_mask(P);
    const size_t mpitch = P.mpitch;
    const int y = blockIdx.x;
    CcStats* stats = O.stats ? O.stats + (size_t)(blockIdx.y / nclasses) * capacity : nullptr;
    if (threadIdx.x < CC_ROW_IDS) {
        row_id[threadIdx.x] = 0;
        row_sum[threadIdx.x][0] = 0; row_sum[threadIdx.x][1] = 0; row_sum[threadIdx.x][2] = 0;
    }
    for (int x = threadIdx.x; x < W; x += 256) {
        const bool v = cc_fg(mask, mpitch, W, H, x, y, zero_border);
        const bool start = x == 0 || cc_fg(mask, mpitch, W, H, x - 1, y, zero_border) != v;
        sc[x] = start ? x + 1 : 0;
    }
    __syncthreads();
    row_scan<OpMax>(sc, W, wsum);
    for (int x = threadIdx.x; x < W; x += 256) {
        if (!cc_fg(mask, mpitch, W, H, x, y, zero_border)) continue;
        if (x != W - 1 && cc_fg(mask, mpitch, W, H, x + 1, y, zero_border)) continue;
        const int a = sc[x] - 1;
        const int id = cc_box(P)[uf_find(cc_label(P), y * W + a)].x;
        sc[a] = id;
        if (!stats || id <= 0 || id > capacity) continue;
        const long long n = x - a + 1, sx = (long long)(a + x) * n / 2;
        const long long lo = a - 1, hi = x, sxx = hi * (hi + 1) * (2 * hi + 1) / 6 - lo * (lo + 1) * (2 * lo + 1) / 6;
        bool placed = false;
        for (int k = 0; k < CC_ROW_PROBES && !placed; ++k) {
            const int e = (id + k) & (CC_ROW_IDS - 1);
            const int old = atomicCAS(&row_id[e], 0, id);
            if (old != 0 && old != id) continue;
            atomicAdd(&row_sum[e][0], (unsigned long long)n); atomicAdd(&row_sum[e][1], (unsigned long long)sx);
            atomicAdd(&row_sum[e][2], (unsigned long long)sxx);
            placed = true;
        }
        if (!placed) cc_add_moments(stats + (id - 1), y, n, sx, sxx);
    }
    __syncthreads();
    if (stats && threadIdx.x < CC_ROW_IDS && row_id[threadIdx.x] != 0)
        cc_add_moments(stats + (row_id[threadIdx.x] - 1), y, row_sum[threadIdx.x][0], row_sum[threadIdx.x][1], row_sum[threadIdx.x][2]);
    if (!O.labels) return;
    int32_t* row = (int32_t*)((uint8_t*)O.labels + (size_t)blockIdx.y * O.lplane + (size_t)y * O.lpitch);
    const auto id_at = [&](int x) {
        if (!cc_fg(mask, mpitch, W, H, x, y, zero_border)) return 0;
        const int t = sc[x];                              // a run's first pixel holds the id, the others the run's start + 1
        return (x == 0 || !cc_fg(mask, mpitch, W, H, x - 1, y, zero_border)) ? t : sc[t - 1];
    };
    const int quads = vec4 ? W / 4 : 0;
    for (int q = threadIdx.x; q < quads; q += 256)
        ((int4*)row)[q] = make_int4(id_at(4 * q), id_at(4 * q + 1), id_at(4 * q + 2), id_at(4 * q + 3));
    for (int x = 4 * quads + threadIdx.x; x < W; x += 256) row[x] = id_at(x);
}

__global__ void k_cc_roi(int* roi, int n)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    roi[4 * f + 2] -= roi[4 * f];
    roi[4 * f + 3] -= roi[4 * f + 1];
}

// the tables live in device globals: filled once per device, and finished before any thread's launch can use them
// (std::call_once holds later callers back until the first has synchronised)
void hsv_tables_ready(hipStream_t stream)
{
    static std::once_flag tabs[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    const auto fill = [&] {
        hipLaunchKernelGGL(k_hsv_tabs, dim3(1), dim3(256), 0, stream);
        (void)hipStreamSynchronize(stream);
    };
    if (dev >= 0 && dev < 64) std::call_once(tabs[dev], fill);
    else fill();
}

void launch_hsv_inrange(const uint8_t* rgb, size_t pitch, int W, int H, const int lo[3], const int hi[3], uint8_t* mask,
                        size_t mpitch, hipStream_t stream)
{
    hsv_tables_ready(stream);
    hipLaunchKernelGGL(k_hsv_inrange, dim3((W * H + 255) / 256), dim3(256), 0, stream, rgb, pitch, W, H, lo[0], lo[1], lo[2],
                       hi[0], hi[1], hi[2], mask, mpitch);
}

void launch_hsv_classes(const uint8_t* rgb, size_t pitch, size_t frame, int n, int W, int H, const HsvClasses& C, uint8_t* mask,
                        size_t mpitch, size_t mplane, hipStream_t stream)
{
    hsv_tables_ready(stream);
    HsvFrames F{rgb, pitch, frame, mask, mpitch, mplane, 0, 0};
    F.rgb4 = ((size_t)rgb | pitch | frame) % 4 == 0;
    F.mask4 = ((size_t)mask | mpitch | mplane) % 4 == 0;
    const int quads = (W + 3) / 4;
    hipLaunchKernelGGL(k_hsv_classes, dim3((quads * H + 255) / 256, n), dim3(256), 0, stream, F, W, H, quads, C);
}

size_t cc_scratch_bytes(int W, int H, int max_records)
{ return ((size_t)W * H + 1) * 4 + 64 + (size_t)W * H * 16 + 64 + (size_t)max_records * 24 + 64; }

// The workspace of one plane: box: W*H int4, label: W*H+1 ints, records: max_records x 6 ints, count: 1 int -- in this order.
struct CcLayout { size_t label_off, rec_off, count_off; };
static CcLayout cc_layout(int W, int H, int max_records)
{
    const size_t N = (size_t)W * H;
    CcLayout L;
    L.label_off = N * 16 + 64;
    L.rec_off = L.label_off + (((N + 1) * 4 + 63) & ~(size_t)63);
    L.count_off = L.rec_off + (size_t)max_records * 24;
    return L;
}

// On return the kernels are enqueued; *d_count / *d_records point at the results inside scratch.
void launch_cc_boxes(const uint8_t* mask, size_t mpitch, int W, int H, int zero_border, void* scratch, int max_records,
                     int** d_count, int** d_records, hipStream_t stream)
{
    const int N = W * H;
    const CcLayout L = cc_layout(W, H, max_records);
    uint8_t* s = (uint8_t*)scratch;
    const CcPlanes P{mask, mpitch, 0, s, 0, L.label_off};
    int* records = (int*)(s + L.rec_off);
    int* count = (int*)(s + L.count_off);
    const dim3 grid((N + 1 + 255) / 256), block(256);
    hipLaunchKernelGGL(k_cc_rows, dim3(H), block, (size_t)W * sizeof(int), stream, P, W, H, zero_border, L.count_off);
    hipLaunchKernelGGL(k_cc_merge, grid, block, 0, stream, P, W, H, zero_border);
    hipLaunchKernelGGL(k_cc_bbox, grid, block, 0, stream, P, W, H, zero_border);
    hipLaunchKernelGGL(k_cc_collect, grid, block, 0, stream, mask, mpitch, (int32_t*)(s + L.label_off), (const int4*)s, W, H, zero_border,
                       count, records, max_records);
    *d_count = count; *d_records = records;
}

size_t cc_plane_bytes(int W, int H, int max_records) { return (cc_scratch_bytes(W, H, max_records) + 63) & ~(size_t)63; }

// n frames x nclasses planes, each with cc_plane_bytes of `scratch`.  The chunk counts and the two totals of a plane lie
// where launch_cc_boxes keeps its records: (chunks + 2) ints, less than the 24 bytes per possible record there.
void launch_cc_objects(const uint8_t* mask, size_t mpitch, size_t mplane, int n, int nclasses, int W, int H, int zero_border,
                       int min_area, void* scratch, int max_records, CcObject* objects, int capacity, int* counts, int* rois,
                       hipStream_t stream, const CcLabelsOut& out)
{
    const int N = W * H, planes = n * nclasses;
    const CcLayout L = cc_layout(W, H, max_records);
    const CcPlanes P{mask, mpitch, mplane, (uint8_t*)scratch, cc_plane_bytes(W, H, max_records), L.label_off};
    const CcSelect S{W, H, zero_border, min_area, nclasses, (N + 255) / 256, L.rec_off};
    const dim3 grid((N + 1 + 255) / 256, planes), chunks(S.chunks, planes), block(256);
    hipLaunchKernelGGL(k_cc_rows, dim3(H, planes), block, (size_t)W * sizeof(int), stream, P, W, H, zero_border, (size_t)0);
    hipLaunchKernelGGL(k_cc_merge, grid, block, 0, stream, P, W, H, zero_border);
    hipLaunchKernelGGL(k_cc_bbox, grid, block, 0, stream, P, W, H, zero_border);
    hipLaunchKernelGGL(k_cc_count, chunks, block, 0, stream, P, S);
    hipLaunchKernelGGL(k_cc_scan, dim3(n), block, 0, stream, P, S, counts, rois);
    const bool ids = out.labels || out.stats;
    if (ids) hipLaunchKernelGGL(k_cc_scatter<true>, chunks, block, 0, stream, P, S, objects, capacity, rois, out.stats);
    else hipLaunchKernelGGL(k_cc_scatter<false>, chunks, block, 0, stream, P, S, objects, capacity, rois, (CcStats*)nullptr);
    hipLaunchKernelGGL(k_cc_roi, dim3((n + 63) / 64), dim3(64), 0, stream, rois, n);
    if (!ids) return;
    const int vec4 = ((size_t)out.labels | out.lpitch | out.lplane) % 16 == 0;
    hipLaunchKernelGGL(k_cc_labels, dim3(H, planes), block, (size_t)W * sizeof(int), stream, P, W, H, zero_border, nclasses, capacity,
                       out, vec4);
}

}  // namespace rtdm
