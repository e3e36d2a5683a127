// k_measure.hip -- per-object measurements from the detector's device lists (rules G1-G10): for every
// stored object the Z quantiles, the extent and the centre of its kept pixels in camera coordinates.  Where the objects lie,
// which pixels they cover and the walk of a box are k_depth_objects.hip's too (rtdm_objslot.h); the point of a pixel, its Z and
// the keep test are k_xyz.hip's too (rtdm_xyz_point.h).
//
//   launch_xyz_min   the frame's smallest disparity key (X4), either key mode
//   k_meas_bands     one wave per (frame, slot, band of DOBJ_BAND rows), rtdm_objslot.h's walk: sums of X, Y, Z in D3's order, the
//                    two counts and the six extreme keys of the band -> workspace.  No atomics.
//   k_meas_final     one lane per slot: the bands in ascending order -> every field of the record but the quantiles of a
//                    non-empty object
//   k_meas_select    one workgroup per slot: a most-significant-digit-first radix select (8-bit digits) over the Z keys that
//                    follows all requested ranks at once; Z is recomputed in every pass, no per-pixel key is stored
// No kernel waits for another workgroup and no grid depends on a count the host does not know.
#include "rtdm_kernels.h"
#include "rtdm_objslot.h"
#include "rtdm_xyz_point.h"

namespace rtdm {

struct MeasBand { double s[3]; unsigned lo[3], hi[3]; int npix, nplane; };     // one band's partial, 56 bytes

// G5: the float's bits as a key whose unsigned order is the order of the values (-0.0 below +0.0), and back
__device__ __forceinline__ unsigned meas_key(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float meas_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }

struct MeasMin { __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return min(a, b); } };
struct MeasMax { __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return max(a, b); } };

// G2-G4 over rtdm_objslot.h's walk: the plane first (nplane counts what it passes), then Z and the keep test, then X and Y
template <bool LABELS>
__global__ __launch_bounds__(256) void k_meas_bands(DepthObjects a, XyzParams P, const int* minkey, MeasBand* part)
{
    dobj_for_bands(a, [&](const DobjItem& t) {
        const int mk = minkey[t.f];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        int c = 0, cp = 0;
        unsigned lo0 = ~0u, lo1 = ~0u, lo2 = ~0u, hi0 = 0u, hi1 = 0u, hi2 = 0u;
        dobj_for_pixels(t, [&](int x, int y) {
            if (!dobj_plane<LABELS>(t.mp, a.mpitch, x, y, t.i)) return;
            ++cp;
            const int key = xyz_key(t.dp[(size_t)y * a.dpitch_e + x], P.mode);
            const double d = xyz_d(key, P.mode), xd = (double)x, yd = (double)y;
            double h3;
            const float Z = xyz_z(P, key, true, mk, xd, yd, d, &h3);
            if (!xyz_keep_z(P, Z)) return;
            const float X = (float)(xyz_h(P, 0, xd, yd, d) / h3), Y = (float)(xyz_h(P, 1, xd, yd, d) / h3);
            s0 += (double)X; s1 += (double)Y; s2 += (double)Z; ++c;
            const unsigned k0 = meas_key(X), k1 = meas_key(Y), k2 = meas_key(Z);
            lo0 = min(lo0, k0); lo1 = min(lo1, k1); lo2 = min(lo2, k2);
            hi0 = max(hi0, k0); hi1 = max(hi1, k1); hi2 = max(hi2, k2);
        });
        s0 = dobj_fold(s0, DobjAdd()); s1 = dobj_fold(s1, DobjAdd()); s2 = dobj_fold(s2, DobjAdd());
        c = dobj_fold(c, DobjAdd()); cp = dobj_fold(cp, DobjAdd());
        lo0 = dobj_fold(lo0, MeasMin()); lo1 = dobj_fold(lo1, MeasMin()); lo2 = dobj_fold(lo2, MeasMin());
        hi0 = dobj_fold(hi0, MeasMax()); hi1 = dobj_fold(hi1, MeasMax()); hi2 = dobj_fold(hi2, MeasMax());
        if ((threadIdx.x & 63) == 0) {
            MeasBand* o = part + (size_t)t.slot * a.nb + t.band;
            o->s[0] = s0; o->s[1] = s1; o->s[2] = s2;
            o->lo[0] = lo0; o->lo[1] = lo1; o->lo[2] = lo2; o->hi[0] = hi0; o->hi[1] = hi1; o->hi[2] = hi2;
            o->npix = c; o->nplane = cp;
        }
    });
}

// one lane = one object slot: its bands in ascending order.  Writes G8's zeros, and the quantiles nobody asked for as zeros.
__global__ __launch_bounds__(256) void k_meas_final(DepthObjects a, int nquant, const MeasBand* part, MeasRecord* out)
{
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= (long long)a.n * a.cap) return;
    DobjBox b;
    if (!dobj_slot(a, (int)(slot / a.cap), (int)(slot % a.cap), &b)) return;
    const int bands = dobj_box_bands(b);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int c = 0, cp = 0;
    unsigned lo0 = ~0u, lo1 = ~0u, lo2 = ~0u, hi0 = 0u, hi1 = 0u, hi2 = 0u;
    for (int k = 0; k < bands; ++k) {
        const MeasBand* p = part + (size_t)slot * a.nb + k;
        s0 += p->s[0]; s1 += p->s[1]; s2 += p->s[2];
        c += p->npix; cp += p->nplane;
        lo0 = min(lo0, p->lo[0]); lo1 = min(lo1, p->lo[1]); lo2 = min(lo2, p->lo[2]);
        hi0 = max(hi0, p->hi[0]); hi1 = max(hi1, p->hi[1]); hi2 = max(hi2, p->hi[2]);
    }
    MeasRecord* o = out + slot;
    o->npix = c; o->nplane = cp;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (c == 0 || k >= nquant) o->zq[k] = 0.0f;
    const bool any = c > 0;
    o->lo[0] = any ? meas_unkey(lo0) : 0.0f; o->lo[1] = any ? meas_unkey(lo1) : 0.0f; o->lo[2] = any ? meas_unkey(lo2) : 0.0f;
    o->hi[0] = any ? meas_unkey(hi0) : 0.0f; o->hi[1] = any ? meas_unkey(hi1) : 0.0f; o->hi[2] = any ? meas_unkey(hi2) : 0.0f;
    o->mean[0] = any ? s0 / c : 0.0; o->mean[1] = any ? s1 / c : 0.0; o->mean[2] = any ? s2 / c : 0.0;
}

// G5.  One workgroup = one object slot, its four waves over row groups of the clipped box in the lane layout of the bands.
// A rank is followed as (prefix, rem): the key bits settled so far and the rank among the keys that carry them.  Ranks with
// equal prefixes share the histogram of the smallest of them (their leader), so a pixel adds to one bin at most.  Pass
// `shift` counts the digit (key >> shift) & 255 of the keys that carry a leader's prefix; then one wave per rank finds the bin
// that holds the rank -- four bins per lane, a wave scan over the lane sums.  Integer histograms in LDS: the same whatever
// order the adds arrive in.  Passes whose digit is the same for every kept key of the object -- known from lo[2] / hi[2] of
// k_meas_final -- are skipped: one exponent for the whole object skips the first, a constant Z all four.
// ROUNDED maps give an object a handful of Z values, and the leading digit of FIXED16 maps is hardly ever more than one: most
// lanes of a wave then want one bin, so a wave first adds the bin of its first live lane once for all lanes that want it,
// twice over, and only what is left goes lane by lane.
#define MEAS_PEEL 2
template <bool LABELS>
__global__ __launch_bounds__(256) void k_meas_select(DepthObjects a, XyzParams P, MeasQuant mq, const int* minkey, MeasRecord* out)
{
    __shared__ unsigned hist[8 * 256];
    __shared__ unsigned prefix[8], rem[8];
    __shared__ int leader[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long slots = (long long)a.n * a.cap;
    for (long long slot = blockIdx.x; slot < slots; slot += gridDim.x) {          // (everything about a slot is workgroup-uniform)
        const int i = (int)(slot % a.cap), f = (int)(slot / a.cap);
        DobjBox b;
        if (!dobj_slot(a, f, i, &b)) continue;
        MeasRecord* o = out + slot;
        const int npix = o->npix;                                                  // k_meas_final's
        if (npix <= 0) continue;
        const unsigned klo = meas_key(o->lo[2]), diff = klo ^ meas_key(o->hi[2]);
        const int cw = b.x1 - b.x0, ch = b.y1 - b.y0;
        const DobjLanes L = dobj_lanes(cw, lane);
        const int lw = L.lw, col = L.col, rof = L.rof, rstep = L.rstep;
        const int16_t* dp = a.disp + (size_t)f * a.dframe_e;
        const uint8_t* mp = a.mask + ((size_t)f * a.K + b.cls) * a.mplane;
        const int mk = minkey[f];
        __syncthreads();                                                           // the slot before has read its prefixes
        if (tid < 8) {
            prefix[tid] = 0;
            rem[tid] = tid < mq.nquant ? (unsigned)(((long long)(npix - 1) * mq.permille[tid]) / 1000) : 0u;
        }
        for (int shift = 24; shift >= 0; shift -= 8) {
            if ((diff >> shift) == 0) {                                            // every kept key has klo's digit here
                if (tid < 8) prefix[tid] |= klo & (0xffu << shift);
                continue;
            }
            __syncthreads();
            for (int k = tid; k < 8 * 256; k += 256) hist[k] = 0;
            if (tid < 8) {
                int l = tid;
                for (int j = tid - 1; j >= 0; --j)
                    if (prefix[j] == prefix[tid]) l = j;
                leader[tid] = tid < mq.nquant ? l : -1;
            }
            __syncthreads();
            const unsigned above = shift == 24 ? 0u : ~0u << (shift + 8);           // the bits the prefixes have settled
            unsigned pre[8];
            bool lead[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { pre[k] = prefix[k]; lead[k] = leader[k] == k; }
            for (int rb = 0; rb < ch; rb += 4 * rstep) {
                const int r = rb + wave * rstep + rof;
                for (int xb = 0; xb < cw; xb += lw) {
                    int bin = -1;
                    if (r < ch && xb + col < cw) {
                        const int x = b.x0 + xb + col, y = b.y0 + r;
                        if (dobj_plane<LABELS>(mp, a.mpitch, x, y, i)) {
                            const int dkey = xyz_key(dp[(size_t)y * a.dpitch_e + x], P.mode);
                            double h3;
                            const float Z = xyz_z(P, dkey, true, mk, (double)x, (double)y, xyz_d(dkey, P.mode), &h3);
                            if (xyz_keep_z(P, Z)) {
                                const unsigned key = meas_key(Z);
#pragma unroll
                                for (int k = 0; k < 8; ++k)
                                    if (lead[k] && ((key ^ pre[k]) & above) == 0) bin = k * 256 + (int)((key >> shift) & 255u);
                            }
                        }
                    }
#pragma unroll
                    for (int round = 0; round < MEAS_PEEL; ++round) {              // (the wave is whole here: the loops are uniform)
                        const unsigned long long live = __ballot(bin >= 0);
                        if (live == 0) break;
                        const int first = __ffsll((long long)live) - 1;
                        const int fb = __shfl(bin, first);
                        const unsigned long long same = __ballot(bin == fb);
                        if (lane == first) atomicAdd(&hist[fb], (unsigned)__popcll(same));
                        if (bin == fb) bin = -1;
                    }
                    if (bin >= 0) atomicAdd(&hist[bin], 1u);
                }
            }
            __syncthreads();
            for (int k = wave; k < mq.nquant; k += 4) {                            // one wave per rank
                const unsigned* h = hist + leader[k] * 256 + 4 * lane;
                const unsigned c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3], tot = c0 + c1 + c2 + c3;
                unsigned inc = tot;
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned v = __shfl_up(inc, off);
                    if (lane >= off) inc += v;
                }
                const unsigned want = rem[k];
                unsigned cum = inc - tot;
                if (want >= cum && want < inc) {                                   // one lane: its four bins hold the rank
                    int dgt = 4 * lane;
                    if (want >= cum + c0) {
                        cum += c0; ++dgt;
                        if (want >= cum + c1) {
                            cum += c1; ++dgt;
                            if (want >= cum + c2) { cum += c2; ++dgt; }
                        }
                    }
                    prefix[k] |= (unsigned)dgt << shift;
                    rem[k] = want - cum;
                }
            }
        }
        __syncthreads();
        if (tid < mq.nquant) o->zq[tid] = meas_unkey(prefix[tid]);
    }
}

// workspace layout, from its address rounded up to 8 (the 64 bytes on top pay for that):
// [n minimum keys, padded to 64 bytes | n * cap * bands(H) MeasBand].  The histograms of the selection live in LDS, so nquant
// adds nothing.
size_t measure_bytes(int n, int cap, int H, int nquant)
{
    (void)nquant;
    return 64 + dobj_min_bytes(n) + (size_t)std::max(n, 0) * std::max(cap, 0) * dobj_bands(H) * sizeof(MeasBand);
}

void launch_measure(DepthObjects a, const XyzParams& P, const MeasQuant& mq, void* workspace, MeasRecord* out, hipStream_t stream,
                    bool labels)
{
    static_assert(sizeof(MeasBand) == 56 && sizeof(MeasRecord) == 88, "the layouts the workspace size and the ABI state");
    if (a.n <= 0) return;
    a.nb = (int)dobj_bands(a.H);
    unsigned char* p;
    int* minkey = dobj_carve_min(workspace, a.n, &p);
    MeasBand* part = (MeasBand*)p;
    launch_xyz_min(XyzDisp{a.disp, a.dpitch_e, a.dframe_e}, a.n, a.W, a.H, P.mode, minkey, stream);
    if (a.cap <= 0) return;
    const size_t slots = (size_t)a.n * a.cap, parts = slots * a.nb;
    const unsigned blocks = (unsigned)std::min<size_t>((parts + 3) / 4, (size_t)1 << 16);
    if (labels) hipLaunchKernelGGL(k_meas_bands<true>, dim3(blocks), dim3(256), 0, stream, a, P, minkey, part);
    else hipLaunchKernelGGL(k_meas_bands<false>, dim3(blocks), dim3(256), 0, stream, a, P, minkey, part);
    hipLaunchKernelGGL(k_meas_final, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, a, mq.nquant, part, out);
    if (mq.nquant <= 0) return;
    const unsigned groups = (unsigned)std::min<size_t>(slots, (size_t)1 << 20);
    if (labels) hipLaunchKernelGGL(k_meas_select<true>, dim3(groups), dim3(256), 0, stream, a, P, mq, minkey, out);
    else hipLaunchKernelGGL(k_meas_select<false>, dim3(groups), dim3(256), 0, stream, a, P, mq, minkey, out);
}

}  // namespace rtdm
