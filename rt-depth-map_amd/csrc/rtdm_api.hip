// rtdm_api.hip -- the C ABI declared in include/rtdm.h: handle management, parameter validation
// (the checks cv::StereoBM::compute performs), geometry, staging copies and
// the launch sequence  K1 prefilter -> K2 search -> K3 left-right check -> K4 speckle filter.
// There is no CPU fallback anywhere in this file: every entry point needs a HIP device.
#include "../../include/rtdm.h"
#include "rtdm_kernels.h"
#include "rtdm_calib.h"
#include "rtdm_mjpeg.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

using namespace rtdm;

static thread_local std::string g_hip_err;

#define HIPC(expr)                                                                               \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            g_hip_err = std::string(#expr) + ": " + hipGetErrorString(e_);                       \
            return RTDM_ERR_HIP;                                                                 \
        }                                                                                        \
    } while (0)

struct StageEvent { hipEvent_t a, b; int stage; int frames; };

// Host entry points hand the caller's (possibly page-locked) planes to async copies: whatever way they leave, nothing may
// still be in flight from / to those planes.  Success paths synchronise themselves and disarm the guard.
struct DrainOnError {
    hipStream_t s;
    bool armed = true;
    ~DrainOnError()
    {
        if (!armed) return;
        const std::string first = g_hip_err;
        (void)hipStreamSynchronize(s); (void)hipGetLastError();
        g_hip_err = first;
    }
};

// Shape of a batched search launch, compared field by field (tune_strips).
struct TuneKey {
    int W, H, n, ncols, nrows, fuse;
    bool operator==(const TuneKey& o) const { return W == o.W && H == o.H && n == o.n && ncols == o.ncols && nrows == o.nrows && fuse == o.fuse; }
};
struct TuneEntry { TuneKey key; int strips; };   // strips: 0 = seen once, not measured yet; -1 = measuring failed

struct rtdm_bm {
    rtdm_bm_params p;
    int prefilter_type, prefilter_size;   // rtdm_bm_set_prefilter: cv::StereoBM's preFilterType / preFilterSize (XSOBEL, 9)
    int maxW, maxH, maxB, device;
    int roi1[4], roi2[4];
    hipStream_t stream;
    hipStream_t sBorder;           // batches: the border-column search runs here, next to the tile search
    hipStream_t sSpare[2];         // idle: they keep the runtime's stream-to-queue layout (rtdm_bm_create)
    hipEvent_t evFork, evJoin;     // ... behind this event of the compute stream, which then waits for that one
    hipEvent_t evBand[2];          // rtdm_bm_compute: one per band of the result on its way back
    hipStream_t sIn, sOut;         // rtdm_bm_compute_batch: copies in / out beside the compute stream
    hipEvent_t evH2D[2], evComp[2], evD2H[2];   // ... one set per half of the staging planes
    size_t ppitch;                 // pitch of the internal 8-bit planes
    uint8_t *dLp, *dRp;            // prefiltered planes   [maxB][maxH][ppitch]
    uint8_t *dInL, *dInR;          // staging for the host entry points
    int16_t* dOut;                 // internal disparity plane [maxB][maxH][Ws] (Ws = maxW rounded up to 8)
    std::vector<TuneEntry> tuned;  // measured strip counts per work shape, least recently used first (<= 16 entries)
    long tune_shapes, tune_launches;   // rtdm_bm_get_tuner_stats
    int32_t *dCost, *dLabel, *dSize, *dRowCnt;
    uint32_t* dRuns;
    int16_t* dHead;
    uint8_t* dMask;                // staging for rtdm_bm_compute_depth: mask plane + reduction scratch
    void* dDepth;
    uint8_t* hStage;               // page-locked staging for the single-frame host entry point
    size_t hStageBytes;
    bool profiling;
    std::vector<StageEvent> pending;
    double stage_ms[RTDM_NUM_STAGES];
    long stage_launches[RTDM_NUM_STAGES], stage_frames[RTDM_NUM_STAGES];
    std::string variant;
};

struct rtdm_morph {
    int W, H, maxB, device;
    hipStream_t stream;
    uint8_t *hIn, *hOut;           // page-locked host buffers handed to the application
    uint8_t *dIn, *dOut, *dT0, *dT1;
};

extern "C" {

const char* rtdm_strerror(int s)
{
    switch (s) {
        case RTDM_OK: return "ok";
        case RTDM_ERR_BAD_PARAM: return "invalid StereoBM parameter";
        case RTDM_ERR_BAD_SIZE: return "invalid frame size or pitch";
        case RTDM_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
        case RTDM_ERR_HIP: return "HIP runtime error";
        case RTDM_ERR_NOMEM: return "out of memory";
        case RTDM_ERR_UNSUPPORTED: return "configuration not supported by this build";
        case RTDM_ERR_NULL: return "null pointer";
        case RTDM_ERR_BAD_STREAM: return "damaged or incomplete JPEG stream";
        default: return "unknown rtdm status";
    }
}

const char* rtdm_last_hip_error(void) { return g_hip_err.c_str(); }
int rtdm_abi_version(void) { return RTDM_ABI_VERSION; }

int rtdm_device_count(int* count)
{
    if (!count) return RTDM_ERR_NULL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return n > 0 ? RTDM_OK : RTDM_ERR_NO_DEVICE;
}

void rtdm_bm_default_params(rtdm_bm_params* p, int numDisparities)
{
    if (!p) return;
    p->preFilterCap = 31; p->blockSize = 13; p->minDisparity = 0; p->numDisparities = numDisparities;
    p->textureThreshold = 10; p->uniquenessRatio = 10; p->speckleWindowSize = 100; p->speckleRange = 32;
    p->disp12MaxDiff = 1; p->legacy_right_clamp = 0;
}

static int validate_params(const rtdm_bm_params& p)
{
    if (p.preFilterCap < 1 || p.preFilterCap > 63) return RTDM_ERR_BAD_PARAM;
    if (p.blockSize < 5 || p.blockSize > 255 || (p.blockSize & 1) == 0) return RTDM_ERR_BAD_PARAM;
    if (p.numDisparities <= 0 || p.numDisparities % 16 != 0) return RTDM_ERR_BAD_PARAM;
    if (p.textureThreshold < 0 || p.uniquenessRatio < 0) return RTDM_ERR_BAD_PARAM;
    // the x16 fixed-point output is 16 bits wide: (minDisparity - 1) * 16 .. (minDisparity + numDisparities) * 16 must fit
    if (p.minDisparity < -2047 || (long)p.minDisparity + p.numDisparities > 2047) return RTDM_ERR_BAD_PARAM;
    if (p.legacy_right_clamp != 0 && p.legacy_right_clamp != 1) return RTDM_ERR_BAD_PARAM;
    return RTDM_OK;
}

static int use_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RTDM_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return RTDM_ERR_NO_DEVICE;
    HIPC(hipSetDevice(device));
    return RTDM_OK;
}

int rtdm_bm_create(const rtdm_bm_params* params, int max_width, int max_height, int max_batch,
                   int device, rtdm_bm** out)
{
    if (!params || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    int rc = validate_params(*params);
    if (rc) return rc;
    if (max_width <= 0 || max_height <= 0 || max_batch <= 0 || max_width > 32767 || max_height > 32767)
        return RTDM_ERR_BAD_SIZE;
    if ((long)max_batch * max_width * max_height >= (1L << 31)) return RTDM_ERR_BAD_SIZE;
    if (max_width > 4096) return RTDM_ERR_UNSUPPORTED;   // row kernels keep whole rows in LDS
    rc = use_device(device);
    if (rc) return rc;
    rtdm_bm* bm = new (std::nothrow) rtdm_bm();
    if (!bm) return RTDM_ERR_NOMEM;
    bm->p = *params; bm->prefilter_type = RTDM_PREFILTER_XSOBEL; bm->prefilter_size = 9;
    bm->maxW = max_width; bm->maxH = max_height; bm->maxB = max_batch; bm->device = device;
    for (int i = 0; i < 4; ++i) bm->roi1[i] = bm->roi2[i] = 0;
    bm->profiling = false;
    bm->tune_shapes = bm->tune_launches = 0;
    for (int i = 0; i < RTDM_NUM_STAGES; ++i) { bm->stage_ms[i] = 0; bm->stage_launches[i] = 0; bm->stage_frames[i] = 0; }
    bm->ppitch = ((size_t)max_width + 63) & ~(size_t)63;
    const size_t plane = bm->ppitch * max_height * (size_t)max_batch;
    // per-pixel workspace and the internal disparity plane use rows of Ws = max_width rounded up to 8 elements
    const size_t px = (size_t)((max_width + 7) & ~7) * max_height * max_batch;
    hipError_t e = hipStreamCreateWithFlags(&bm->stream, hipStreamNonBlocking);
    // + slack: the search kernels stage whole dwords of whole tiles and may read past the last row's end
    // (one allocation, the right planes behind the left ones: k_search_ring addresses both from the left plane's rows)
    const size_t plane_al = (plane + 1024 + 255) & ~(size_t)255;
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dLp, 2 * plane_al);
    if (e == hipSuccess) bm->dRp = bm->dLp + plane_al;
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dInL, plane);
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dInR, plane);
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dOut, px * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dCost, px * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dLabel, px * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dSize, px * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dRuns, px * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dHead, px * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dMask, (size_t)max_width * max_height);
    if (e == hipSuccess) e = hipMalloc(&bm->dDepth, depth_scratch_bytes(RTDM_MAX_REGIONS, max_height));
    bm->hStageBytes = 2 * bm->ppitch * (size_t)max_height + (size_t)((max_width + 7) & ~7) * max_height * (sizeof(int16_t) + 1) + 1024;
    if (e == hipSuccess) e = hipHostMalloc((void**)&bm->hStage, bm->hStageBytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&bm->dRowCnt, (size_t)max_batch * max_height * sizeof(int32_t));
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_bm_create: ") + hipGetErrorString(e);
        rtdm_bm_destroy(bm);
        return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
    }
    for (auto& e : bm->evBand) HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPC(hipStreamCreateWithFlags(&bm->sIn, hipStreamNonBlocking));
    HIPC(hipStreamCreateWithFlags(&bm->sOut, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k) {
        HIPC(hipEventCreateWithFlags(&bm->evH2D[k], hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&bm->evComp[k], hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&bm->evD2H[k], hipEventDisableTiming));
    }
    // The runtime maps streams onto its few hardware queues in creation order, and which queue the border side stream shares
    // shows in the search stage (~1 % at the headline).  The streams are therefore created in the order the handle has always
    // created them: sSpare are the two idle streams of the retired two-lane layout.
    HIPC(hipStreamCreateWithFlags(&bm->sSpare[0], hipStreamNonBlocking));
    HIPC(hipStreamCreateWithFlags(&bm->sBorder, hipStreamNonBlocking));
    HIPC(hipStreamCreateWithFlags(&bm->sSpare[1], hipStreamNonBlocking));
    HIPC(hipEventCreateWithFlags(&bm->evFork, hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&bm->evJoin, hipEventDisableTiming));
    *out = bm;
    return RTDM_OK;
}

void rtdm_bm_destroy(rtdm_bm* bm)
{
    if (!bm) return;
    (void)hipSetDevice(bm->device);
    if (bm->stream) (void)hipStreamSynchronize(bm->stream);
    if (bm->sBorder) { (void)hipStreamSynchronize(bm->sBorder); (void)hipStreamDestroy(bm->sBorder); }
    for (auto& q : bm->sSpare) if (q) (void)hipStreamDestroy(q);
    if (bm->evFork) (void)hipEventDestroy(bm->evFork);
    if (bm->evJoin) (void)hipEventDestroy(bm->evJoin);
    for (auto& e : bm->evBand) if (e) (void)hipEventDestroy(e);
    if (bm->sIn) { (void)hipStreamSynchronize(bm->sIn); (void)hipStreamDestroy(bm->sIn); }
    if (bm->sOut) { (void)hipStreamSynchronize(bm->sOut); (void)hipStreamDestroy(bm->sOut); }
    for (int k = 0; k < 2; ++k) {
        if (bm->evH2D[k]) (void)hipEventDestroy(bm->evH2D[k]);
        if (bm->evComp[k]) (void)hipEventDestroy(bm->evComp[k]);
        if (bm->evD2H[k]) (void)hipEventDestroy(bm->evD2H[k]);
    }
    for (auto& ev : bm->pending) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    void* bufs[] = {bm->dLp, bm->dInL, bm->dInR, bm->dOut, bm->dCost, bm->dLabel, bm->dSize, bm->dRuns, bm->dRowCnt, bm->dHead, bm->dMask, bm->dDepth};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (bm->hStage) (void)hipHostFree(bm->hStage);
    if (bm->stream) (void)hipStreamDestroy(bm->stream);
    delete bm;
}

int rtdm_bm_set_roi(rtdm_bm* bm, int which, int x, int y, int width, int height)
{
    if (!bm) return RTDM_ERR_NULL;
    if (which != 1 && which != 2) return RTDM_ERR_BAD_PARAM;
    int* r = which == 1 ? bm->roi1 : bm->roi2;
    r[0] = x; r[1] = y; r[2] = width; r[3] = height;
    return RTDM_OK;
}

int rtdm_bm_get_params(const rtdm_bm* bm, rtdm_bm_params* out)
{
    if (!bm || !out) return RTDM_ERR_NULL;
    *out = bm->p;
    return RTDM_OK;
}

int rtdm_bm_set_prefilter(rtdm_bm* bm, int preFilterType, int preFilterSize)
{
    if (!bm) return RTDM_ERR_NULL;
    if (preFilterType != RTDM_PREFILTER_NORMALIZED_RESPONSE && preFilterType != RTDM_PREFILTER_XSOBEL) return RTDM_ERR_BAD_PARAM;
    // (cv::StereoBM::compute checks the size whatever the type)
    if (preFilterSize < 5 || preFilterSize > 255 || (preFilterSize & 1) == 0) return RTDM_ERR_BAD_PARAM;
    bm->prefilter_type = preFilterType; bm->prefilter_size = preFilterSize;
    return RTDM_OK;
}

int rtdm_bm_get_prefilter(const rtdm_bm* bm, int* preFilterType, int* preFilterSize)
{
    if (!bm || !preFilterType || !preFilterSize) return RTDM_ERR_NULL;
    *preFilterType = bm->prefilter_type; *preFilterSize = bm->prefilter_size;
    return RTDM_OK;
}

// offsets, valid rectangle (getValidDisparityROI, clipped to the image and
// to rows that have a full window).  Returns false when the whole frame is FILTERED.
static bool make_geom(const rtdm_bm* bm, int W, int H, BMGeom* g)
{
    const rtdm_bm_params& p = bm->p;
    g->W = W; g->H = H; g->Ws = (W + 7) & ~7; g->D = p.numDisparities; g->minD = p.minDisparity;
    g->w = p.blockSize; g->r = p.blockSize / 2;
    g->cap = p.preFilterCap; g->tex = p.textureThreshold; g->uniq = p.uniquenessRatio;
    g->lofs = std::max(g->D - 1 + g->minD, 0);
    g->rofs = -std::min(g->D - 1 + g->minD, 0);
    g->width1 = W - g->rofs - g->D + 1;
    g->filtered = (g->minD - 1) * 16;
    g->want_cost = p.disp12MaxDiff >= 0;
    g->cost16 = 2L * p.preFilterCap * p.blockSize * p.blockSize < 65536;
    g->mask_cols = p.disp12MaxDiff < 0;
    g->legacy = p.legacy_right_clamp;
    int r1[4] = {0, 0, W, H}, r2[4] = {0, 0, W, H};
    if (bm->roi1[2] > 0 && bm->roi1[3] > 0) std::copy(bm->roi1, bm->roi1 + 4, r1);
    if (bm->roi2[2] > 0 && bm->roi2[3] > 0) std::copy(bm->roi2, bm->roi2 + 4, r2);
    const int maxD = g->minD + g->D - 1;
    int xmin = std::max(r1[0], r2[0] + maxD) + g->r;
    int xmax = std::min(r1[0] + r1[2], r2[0] + r2[2] - g->minD) - g->r;
    int ymin = std::max(r1[1], r2[1]) + g->r;
    int ymax = std::min(r1[1] + r1[3], r2[1] + r2[3]) - g->r;
    xmin = std::max(xmin, 0); xmax = std::min(xmax, W);
    ymin = std::max(ymin, g->r); ymax = std::min(ymax, H - g->r);
    g->vx0 = xmin; g->vx1 = xmax; g->vy0 = ymin; g->vy1 = ymax;
    // Columns worth searching (estimator.cpp:54 shrinks the rectangle every frame with setROI1):
    // validateDisparity lets column x vote for x - round(d/16) in [x - maxD - 1, x - minD + 1] and
    // reads the votes of x - floor/ceil(d/16), so a valid column depends on searched columns at
    // most D + |minD| + 2 away.  Everything else is masked to FILTERED anyway.
    const int reach = (p.disp12MaxDiff >= 0) ? g->D + std::abs(g->minD) + 2 : 0;
    g->cx0 = std::max(g->lofs, xmin - reach);
    g->cx1 = std::min(std::min(W, g->lofs + g->width1), xmax + reach);
    if (g->lofs >= W || g->rofs >= W || g->width1 < 1) return false;
    return xmax > xmin && ymax > ymin;
}

static void stage_begin(rtdm_bm* bm, int stage, int frames, hipStream_t s, StageEvent* ev)
{
    if (!bm->profiling) return;
    ev->stage = stage; ev->frames = frames;
    (void)hipEventCreate(&ev->a); (void)hipEventCreate(&ev->b);
    (void)hipEventRecord(ev->a, s);
}
static void stage_end(rtdm_bm* bm, hipStream_t s, StageEvent* ev)
{
    if (!bm->profiling) return;
    (void)hipEventRecord(ev->b, s);
    bm->pending.push_back(*ev);
}

static int chunk_front(rtdm_bm* bm, int n, Plane8 L, Plane8 R, int W, int H, Plane16W disp, hipStream_t s, BMGeom* gout,
                       bool* anyout);
static int chunk_back(rtdm_bm* bm, int n, int W, int H, Plane16W disp, const BMGeom& g, hipStream_t s);

// Row strips per frame for the fast search of a batch, chosen by measurement and remembered in the handle: the model
// (fast_strips_model) is right on average, but neighbouring strip counts differ by up to 5 % through scheduling effects it
// cannot see (profiles/r01_xcd_mapping_sweep.txt).  The search only writes its own outputs, so timing it a few times on
// the caller's data is harmless.  The key is the SHAPE of the work (frame size, batch, searched columns and rows as
// counts, not positions): a caller that moves a same-sized ROI around (estimator.cpp:53-54) keeps its entry.  A shape is
// measured the SECOND time it is seen -- a caller whose ROI changes size every call never pays the ~30 extra launches and
// the stream synchronisation -- and the table is a 16-entry LRU.  Small batches keep the model.  RTDM_AUTOTUNE=0: off.
static int tune_strips(rtdm_bm* bm, Plane8 Lpr, Plane8 Rpr, Plane16W disp, const BMGeom& g, int n, hipStream_t s, bool fuse, bool ring)
{
    const auto launch = [&](int c) {
        if (ring) launch_search_ring(Lpr, Rpr, disp, bm->dCost, g, n, s, c, fuse);
        else launch_search_fast(Lpr, Rpr, disp, bm->dCost, g, n, s, fuse, c);
    };
    static const bool enabled = env_int("RTDM_AUTOTUNE", 1) != 0 && getenv("RTDM_FAST_WGS") == nullptr;
    if (!enabled || n < 16) return 0;
    TuneKey key{g.W, g.H, n, g.cx1 - g.cx0, g.vy1 - g.vy0, (fuse ? 1 : 0) | (ring ? ring_lanes_per_pixel(g) : 0)};
    for (size_t i = 0; i < bm->tuned.size(); ++i) {
        if (!(bm->tuned[i].key == key)) continue;
        TuneEntry e = bm->tuned[i];
        bm->tuned.erase(bm->tuned.begin() + (long)i);              // most recently used goes to the back
        if (e.strips == 0) {
            e.strips = -1;                                          // being measured: a failure below leaves the model in charge
            ++bm->tune_shapes;
            const int model = ring ? ring_strips_model(g, n) : fast_strips_model(g, n), cap = (g.vy1 - g.vy0 + 15) / 16;
            int best = model;
            float best_ms = 1e30f;
            hipEvent_t a, b;
            if (hipEventCreate(&a) == hipSuccess) {
                if (hipEventCreate(&b) == hipSuccess) {
                    static const float f[] = {0.6f, 0.7f, 0.8f, 0.9f, 1.0f, 1.1f, 1.2f, 1.35f, 1.5f, 1.75f};
                    int seen[10], nseen = 0;
                    for (float fk : f) {
                        const int c = std::max(1, std::min(cap, (int)(model * fk + 0.5f)));
                        bool dup = false;
                        for (int k = 0; k < nseen; ++k) dup |= seen[k] == c;
                        if (dup) continue;
                        seen[nseen++] = c;
                        launch(c);          // warm
                        bm->tune_launches += 3;
                        float ms = 1e30f;
                        for (int rep = 0; rep < 2; ++rep) {
                            (void)hipEventRecord(a, s);
                            launch(c);
                            (void)hipEventRecord(b, s);
                            float t = 0.f;
                            if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&t, a, b) == hipSuccess) ms = std::min(ms, t);
                        }
                        if (ms < best_ms) { best_ms = ms; best = c; }
                    }
                    e.strips = best;
                    (void)hipEventDestroy(b);
                }
                (void)hipEventDestroy(a);
            }
        }
        bm->tuned.push_back(e);
        return e.strips > 0 ? e.strips : 0;
    }
    if (bm->tuned.size() >= 16) bm->tuned.erase(bm->tuned.begin());  // least recently used
    bm->tuned.push_back(TuneEntry{key, 0});                           // first sighting: remember, keep the model
    return 0;
}

// One chunk (n <= maxB) of device-resident frames, enqueued on `s`.  The row kernels move 8 columns per 128-bit
// access and let a ragged last chunk spill into the row padding, so they need 16-byte aligned rows of at least
// W rounded up to 8 elements whose padding is ours to write.  A caller's plane qualifies only if W % 8 == 0 and it
// is aligned; anything else (the reference's own crops are 233, 534 and 934 columns wide) runs on the handle's
// internal plane and is copied out at the end.
static int run_chunk(rtdm_bm* bm, int n, Plane8 L, Plane8 R, int W, int H, Plane16W out, hipStream_t s)
{
    const size_t Ws = (size_t)((W + 7) & ~7);
    // (the handle's own plane, or a frame-aligned part of it: rows of Ws elements whose padding is ours)
    const bool internal = out.pitch_e == Ws && out.base >= bm->dOut && out.base < bm->dOut + (size_t)bm->maxB * Ws * (size_t)H &&
                          (size_t)(out.base - bm->dOut) % (Ws * (size_t)H) == 0;
    const bool direct = internal || ((W & 7) == 0 && (((size_t)out.base | (out.pitch_e * 2) | (out.frame_e * 2)) & 15) == 0);
    const Plane16W disp = direct ? out : Plane16W{bm->dOut, Ws, Ws * (size_t)H};
    BMGeom g;
    bool any = false;
    int rc = chunk_front(bm, n, L, R, W, H, disp, s, &g, &any);
    if (rc) return rc;
    if (any) { rc = chunk_back(bm, n, W, H, disp, g, s); if (rc) return rc; }
    if (!direct) launch_copy16(disp, out, W, H, n, s);
    HIPC(hipGetLastError());
    return RTDM_OK;
}

// Fill + prefilter + SAD search of a chunk (VALU bound); *any = false: the whole frame is FILTERED, nothing follows.
static int chunk_front(rtdm_bm* bm, int n, Plane8 L, Plane8 R, int W, int H, Plane16W disp, hipStream_t s, BMGeom* gout,
                       bool* anyout)
{
    const rtdm_bm_params& p = bm->p;
    BMGeom& g = *gout;
    const bool any = make_geom(bm, W, H, &g);
    *anyout = any;
    if (!any) { launch_fill16(disp, 0, W, 0, H, n, g.filtered, s); return RTDM_OK; }
    // the search kernels write columns [cx0, cx1) of the valid rows; everything else is FILTERED
    // (+ the speckle filter's run counts = 0); the fill rides in the prefilter's launch
    const FillJob fill{disp, g.cx0, g.cx1, g.vy0, g.vy1, g.filtered, (p.speckleRange >= 0 && p.speckleWindowSize > 0) ? bm->dRowCnt : nullptr};
    StageEvent ev;
    bool u16 = false;
    // what k_search_generic cannot hold in LDS (D > 256, large windows at large D) -- or everything, when
    // rtdm_debug_disparity_slice forces it -- is searched by the disparity-sliced kernel over the whole range
    const bool dslice = !generic_search_supported(g, &u16) || dslice_forced();
    const bool fast = !dslice && fast_search_supported(g);
    {
        const bool ring = fast && ring_search_supported(g);
        const int lpp = ring ? ring_lanes_per_pixel(g) : 0;
        bm->variant = dslice ? (u16 ? "generic_dslice_u16" : "generic_dslice_u32")
                    : ring ? (lpp == 16 ? "fast_ring16_qsad" : lpp == 8 ? "fast_ring8_qsad" : lpp == 4 ? "fast_ring4_qsad" : "fast_ring_qsad") : fast ? "fast_qsad" : (u16 ? "generic_u16" : "generic_u32");
        Plane8W Lp{bm->dLp, bm->ppitch, bm->ppitch * (size_t)H}, Rp{bm->dRp, bm->ppitch, bm->ppitch * (size_t)H};
        stage_begin(bm, RTDM_STAGE_PREFILTER, n, s, &ev);
        launch_prefilter(L, R, Lp, Rp, W, H, p.preFilterCap, n, s, &fill, bm->prefilter_type, bm->prefilter_size);
        stage_end(bm, s, &ev);
        Plane8 Lpr{bm->dLp, Lp.pitch, Lp.frame}, Rpr{bm->dRp, Rp.pitch, Rp.frame};
        stage_begin(bm, RTDM_STAGE_SEARCH, n, s, &ev);
        if (fast) {
            int lx0, lx1, rx0, rx1;
            fast_border_ranges(g, &lx0, &lx1, &rx0, &rx1);
            // Batches of 16 or more: the border columns run as a kernel of their own on a side stream, concurrently with the
            // tile kernel.  Its waves need 37-72 VGPRs and fit NEXT to the four tile waves of a SIMD, whereas inside the tile
            // kernel's grid a border workgroup takes a tile workgroup's slot for the length of its latency-bound walk
            // (search -2 %).  Smaller batches keep the fused launch (one kernel less).
            const bool side = border_search_supported(g) && n >= 16;
            // (the 3.x clamp exists in the stand-alone border kernel only: the fused forms keep their register budget)
            const bool fuse = border_search_supported(g) && !side && !g.legacy;   // border workgroups inside the tile kernel's grid
            // (measured, if at all, before the side stream forks: nothing else runs beside the timed launches)
            const int strips = tune_strips(bm, Lpr, Rpr, disp, g, n, s, fuse, ring);
            if (side) {
                HIPC(hipEventRecord(bm->evFork, s));
                HIPC(hipStreamWaitEvent(bm->sBorder, bm->evFork, 0));
                launch_search_border(Lpr, Rpr, disp, bm->dCost, g, n, bm->sBorder, lx0, lx1, rx0, rx1);
                HIPC(hipEventRecord(bm->evJoin, bm->sBorder));
            }
            bool fused = fuse;
            if (ring) fused = launch_search_ring(Lpr, Rpr, disp, bm->dCost, g, n, s, strips, fuse);
            else launch_search_fast(Lpr, Rpr, disp, bm->dCost, g, n, s, fuse, strips);
            if (side) {
                HIPC(hipStreamWaitEvent(s, bm->evJoin, 0));
            } else if (fused) {
            } else if (border_search_supported(g)) {
                launch_search_border(Lpr, Rpr, disp, bm->dCost, g, n, s, lx0, lx1, rx0, rx1);
            } else {
                launch_search_generic(Lpr, Rpr, disp, bm->dCost, g, n, s, lx0, lx1);
                launch_search_generic(Lpr, Rpr, disp, bm->dCost, g, n, s, rx0, rx1);
            }
        } else if (dslice) {
            launch_search_dslice(Lpr, Rpr, disp, bm->dCost, g, n, s, g.cx0 - g.lofs, g.cx1 - g.lofs);
        } else {
            launch_search_generic(Lpr, Rpr, disp, bm->dCost, g, n, s, g.cx0 - g.lofs, g.cx1 - g.lofs);
        }
        stage_end(bm, s, &ev);
    }
    HIPC(hipGetLastError());
    return RTDM_OK;
}

// Left-right check + speckle filter of a chunk, in place on `disp` (latency bound).
static int chunk_back(rtdm_bm* bm, int n, int W, int H, Plane16W disp, const BMGeom& g, hipStream_t s)
{
    const rtdm_bm_params& p = bm->p;
    StageEvent ev;
    const bool speckle = p.speckleRange >= 0 && p.speckleWindowSize > 0;
    const bool lr = p.disp12MaxDiff >= 0;
    int compact_rows = 0;                // > 0: k_lrcheck_vec wrote per-chunk head records and merged blocks of that many rows
    if (lr) {
        stage_begin(bm, RTDM_STAGE_LRCHECK, n, s, &ev);
        if (speckle) compact_rows = launch_lrcheck(disp, bm->dCost, g, p.disp12MaxDiff, n, s, bm->dLabel, bm->dSize, bm->dRuns, bm->dRowCnt, bm->dHead,
                                                   p.speckleRange);
        else         launch_lrcheck(disp, bm->dCost, g, p.disp12MaxDiff, n, s);
        stage_end(bm, s, &ev);
    }
    if (speckle) {
        stage_begin(bm, RTDM_STAGE_SPECKLE, n, s, &ev);
        launch_speckle(disp, bm->dLabel, bm->dSize, bm->dRuns, bm->dRowCnt, bm->dHead, W, g.Ws, H, n, g.filtered, p.speckleWindowSize,
                       p.speckleRange, lr, std::max(compact_rows, 1), g.vy0, g.vy1, s, compact_rows > 0);
        stage_end(bm, s, &ev);
    }
    HIPC(hipGetLastError());
    return RTDM_OK;
}

// host memory the GPU can DMA from / to directly (hipHostMalloc, hipHostRegister)?
static bool page_locked(const void* q)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }   // plain malloc memory: an error, not a fault
    return a.type == hipMemoryTypeHost;
}

static int check_frame(const rtdm_bm* bm, int W, int H)
{
    if (W <= 0 || H <= 0 || W > bm->maxW || H > bm->maxH) return RTDM_ERR_BAD_SIZE;
    if (bm->p.blockSize >= std::min(W, H)) return RTDM_ERR_BAD_PARAM;   // cv::StereoBM::compute's check
    return RTDM_OK;
}

int rtdm_bm_compute_device(rtdm_bm* bm, int n, const uint8_t* d_left, const uint8_t* d_right,
                           size_t pitch, size_t frame_stride, int width, int height,
                           int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride, void* hip_stream)
{
    if (!bm || !d_left || !d_right || !d_disp) return RTDM_ERR_NULL;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    int rc = check_frame(bm, width, height);
    if (rc) return rc;
    if (pitch < (size_t)width || disp_pitch < (size_t)width * 2 || (disp_pitch & 1) || (disp_frame_stride & 1))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = (hipStream_t)hip_stream;          // NULL = the HIP null stream (what torch's default stream is)
    for (int i0 = 0; i0 < n; i0 += bm->maxB) {
        const int m = std::min(bm->maxB, n - i0);
        Plane8 L{d_left + (size_t)i0 * frame_stride, pitch, frame_stride};
        Plane8 R{d_right + (size_t)i0 * frame_stride, pitch, frame_stride};
        Plane16W O{d_disp + (size_t)i0 * (disp_frame_stride / 2), disp_pitch / 2, disp_frame_stride / 2};
        rc = run_chunk(bm, m, L, R, width, height, O, s);
        if (rc) return rc;
    }
    return RTDM_OK;
}

static int compute_batch_enqueue(rtdm_bm* bm, int n, const uint8_t* left, const uint8_t* right, size_t pitch, size_t frame_stride,
                                 int width, int height, int16_t* disp, size_t disp_pitch, size_t disp_frame_stride);

int rtdm_bm_compute_batch(rtdm_bm* bm, int n, const uint8_t* left, const uint8_t* right,
                          size_t pitch, size_t frame_stride, int width, int height,
                          int16_t* disp, size_t disp_pitch, size_t disp_frame_stride)
{
    if (!bm || !left || !right || !disp) return RTDM_ERR_NULL;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    int rc = check_frame(bm, width, height);
    if (rc) return rc;
    if (pitch < (size_t)width || disp_pitch < (size_t)width * 2) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    rc = compute_batch_enqueue(bm, n, left, right, pitch, frame_stride, width, height, disp, disp_pitch, disp_frame_stride);
    if (rc) {
        // an error exit must not leave DMA in flight from / to the caller's buffers: it is free to release them once we return
        const std::string first = g_hip_err;
        (void)hipStreamSynchronize(bm->sIn); (void)hipStreamSynchronize(bm->stream); (void)hipStreamSynchronize(bm->sOut);
        (void)hipGetLastError();
        g_hip_err = first;
    }
    return rc;
}

static int compute_batch_enqueue(rtdm_bm* bm, int n, const uint8_t* left, const uint8_t* right, size_t pitch, size_t frame_stride,
                                 int width, int height, int16_t* disp, size_t disp_pitch, size_t disp_frame_stride)
{
    int rc = RTDM_OK;
    hipStream_t s = bm->stream;
    const size_t dpitch = bm->ppitch, dframe = bm->ppitch * (size_t)height;
    const size_t Ws = (size_t)((width + 7) & ~7);                      // the handle's internal plane (see run_chunk)
    const size_t opitch = Ws * 2, oframe = opitch * (size_t)height;
    // Three streams, two halves of the staging planes: while chunk k is computed, chunk k+1 comes in over PCIe and chunk
    // k-1 goes out (both directions of the bus at once).  It pays for page-locked caller memory (hipHostMalloc /
    // hipHostRegister: the copies are true DMA); pageable frames are staged by the runtime inside the copy call.
    // Measured (tools/host_batch_rate.py, 256 x 720p): page-locked 11.6 k -> 21.1 k pairs/s (78 GB/s over PCIe, both ways),
    // pageable 11.2 k -> 10.5 k: so only for page-locked callers.
    const int half = std::max(1, bm->maxB / 2);
    const bool two = bm->maxB >= 2 && page_locked(left) && page_locked(right) && page_locked(disp);
    const int chunk = two ? half : bm->maxB;
    int k = 0;
    for (int i0 = 0; i0 < n; i0 += chunk, ++k) {
        const int m = std::min(chunk, n - i0), b = two ? (k & 1) : 0;
        const size_t fo = (size_t)b * (size_t)half;                    // first staging frame of this half
        hipStream_t si = two ? bm->sIn : s, so = two ? bm->sOut : s;
        if (two && k >= 2) HIPC(hipStreamWaitEvent(si, bm->evComp[b], 0));      // the half's previous chunk has been consumed
        uint8_t *dl = bm->dInL + fo * dframe, *dr = bm->dInR + fo * dframe;
        if (pitch == dpitch && frame_stride == dframe) {               // the caller's frames have the staging layout: one copy per image
            // (up to the last pixel of the last row: a view that starts at x > 0 of its parent plane ends before the row's pitch does)
            const size_t nbytes = (size_t)m * dframe - (dpitch - (size_t)width);
            HIPC(hipMemcpyAsync(dl, left + (size_t)i0 * frame_stride, nbytes, hipMemcpyHostToDevice, si));
            HIPC(hipMemcpyAsync(dr, right + (size_t)i0 * frame_stride, nbytes, hipMemcpyHostToDevice, si));
        } else {
            for (int i = 0; i < m; ++i) {
                HIPC(hipMemcpy2DAsync(dl + i * dframe, dpitch, left + (size_t)(i0 + i) * frame_stride, pitch, width, height, hipMemcpyHostToDevice, si));
                HIPC(hipMemcpy2DAsync(dr + i * dframe, dpitch, right + (size_t)(i0 + i) * frame_stride, pitch, width, height, hipMemcpyHostToDevice, si));
            }
        }
        if (two) {
            HIPC(hipEventRecord(bm->evH2D[b], si));
            HIPC(hipStreamWaitEvent(s, bm->evH2D[b], 0));
            if (k >= 2) HIPC(hipStreamWaitEvent(s, bm->evD2H[b], 0));   // ... and its previous result has left
        }
        Plane8 L{dl, dpitch, dframe}, R{dr, dpitch, dframe};
        int16_t* dout = bm->dOut + fo * Ws * (size_t)height;
        Plane16W O{dout, Ws, Ws * (size_t)height};
        rc = run_chunk(bm, m, L, R, width, height, O, s);
        if (rc) return rc;
        if (two) { HIPC(hipEventRecord(bm->evComp[b], s)); HIPC(hipStreamWaitEvent(so, bm->evComp[b], 0)); }
        // one linear copy only when the internal rows carry no padding: with width < Ws it would write the pad columns
        // [width, Ws) of the caller's rows, which are not part of the view
        if ((size_t)width == Ws && disp_pitch == opitch && disp_frame_stride == oframe) {
            HIPC(hipMemcpyAsync((uint8_t*)disp + (size_t)i0 * disp_frame_stride, dout, (size_t)m * oframe, hipMemcpyDeviceToHost, so));
        } else {
            for (int i = 0; i < m; ++i)
                HIPC(hipMemcpy2DAsync((uint8_t*)disp + (size_t)(i0 + i) * disp_frame_stride, disp_pitch,
                                      (uint8_t*)dout + i * oframe, opitch, (size_t)width * 2, height, hipMemcpyDeviceToHost, so));
        }
        if (two) HIPC(hipEventRecord(bm->evD2H[b], so));
        else HIPC(hipStreamSynchronize(s));                            // staging buffers are reused by the next chunk
    }
    if (two) { HIPC(hipStreamSynchronize(bm->sOut)); HIPC(hipStreamSynchronize(s)); HIPC(hipStreamSynchronize(bm->sIn)); }
    return RTDM_OK;
}

int rtdm_bm_compute(rtdm_bm* bm, const uint8_t* left, size_t left_pitch, const uint8_t* right,
                    size_t right_pitch, int width, int height, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !left || !right || !disp) return RTDM_ERR_NULL;
    int rc = check_frame(bm, width, height);
    if (rc) return rc;
    if (left_pitch < (size_t)width || right_pitch < (size_t)width || disp_pitch < (size_t)width * 2)
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    DrainOnError drain{s};
    const size_t dpitch = bm->ppitch, dframe = bm->ppitch * (size_t)height;
    // The caller's Mats are pageable ROI views (estimator.cpp:33,36): the rows are gathered into the page-locked staging
    // area on the host and go over in linear async copies -- in two BANDS of rows per direction, so that the host gathers
    // band 1 while band 0 is on the bus, and scatters band 0 of the result while band 1 arrives.  720p pair, host to host:
    // 0.363 ms with one copy per plane and row-by-row gathers, 0.347 with one band, 0.325 with two, 0.375 with four (every
    // further async copy costs more in the runtime than its overlap hides).  Rows that are contiguous in the caller's plane
    // move as one memcpy.
    const size_t Wsd = (size_t)((width + 7) & ~7);
    if (page_locked(left) && page_locked(right) && page_locked(disp)) {
        // the caller's planes are page-locked: DMA straight from and to them, no gathers on the host
        HIPC(hipMemcpy2DAsync(bm->dInL, dpitch, left, left_pitch, (size_t)width, height, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpy2DAsync(bm->dInR, dpitch, right, right_pitch, (size_t)width, height, hipMemcpyHostToDevice, s));
        Plane8 Ld{bm->dInL, dpitch, dframe}, Rd{bm->dInR, dpitch, dframe};
        Plane16W Od{bm->dOut, Wsd, Wsd * (size_t)height};
        rc = run_chunk(bm, 1, Ld, Rd, width, height, Od, s);
        if (rc) return rc;
        HIPC(hipMemcpy2DAsync(disp, disp_pitch, bm->dOut, Wsd * sizeof(int16_t), (size_t)width * sizeof(int16_t), height, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        drain.armed = false;
        return RTDM_OK;
    }
    uint8_t* hL = bm->hStage;
    uint8_t* hR = hL + dframe;
    int16_t* hD = (int16_t*)(bm->hStage + 2 * bm->ppitch * (size_t)bm->maxH);
    const int nb = height >= 256 ? 2 : 1, bh = (height + nb - 1) / nb;
    const auto gather = [&](uint8_t* dst, const uint8_t* src, size_t spitch, int y0, int y1) {
        if (spitch == dpitch) { memcpy(dst + (size_t)y0 * dpitch, src + (size_t)y0 * spitch, (size_t)(y1 - y0 - 1) * dpitch + (size_t)width); return; }
        for (int y = y0; y < y1; ++y) memcpy(dst + (size_t)y * dpitch, src + (size_t)y * spitch, (size_t)width);
    };
    for (int b = 0; b < nb; ++b) {
        const int y0 = b * bh, y1 = std::min(height, y0 + bh);
        if (y0 >= y1) break;
        gather(hL, left, left_pitch, y0, y1);
        HIPC(hipMemcpyAsync(bm->dInL + (size_t)y0 * dpitch, hL + (size_t)y0 * dpitch, (size_t)(y1 - y0) * dpitch, hipMemcpyHostToDevice, s));
        gather(hR, right, right_pitch, y0, y1);
        HIPC(hipMemcpyAsync(bm->dInR + (size_t)y0 * dpitch, hR + (size_t)y0 * dpitch, (size_t)(y1 - y0) * dpitch, hipMemcpyHostToDevice, s));
    }
    Plane8 L{bm->dInL, dpitch, dframe}, R{bm->dInR, dpitch, dframe};
    const size_t Ws = (size_t)((width + 7) & ~7);                      // the handle's internal plane (see run_chunk)
    Plane16W O{bm->dOut, Ws, Ws * (size_t)height};
    rc = run_chunk(bm, 1, L, R, width, height, O, s);
    if (rc) return rc;
    int nbo = 0;
    for (int b = 0; b < nb; ++b, ++nbo) {
        const int y0 = b * bh, y1 = std::min(height, y0 + bh);
        if (y0 >= y1) break;
        HIPC(hipMemcpyAsync(hD + (size_t)y0 * Ws, bm->dOut + (size_t)y0 * Ws, (size_t)(y1 - y0) * Ws * sizeof(int16_t), hipMemcpyDeviceToHost, s));
        HIPC(hipEventRecord(bm->evBand[b], s));
    }
    for (int b = 0; b < nbo; ++b) {
        const int y0 = b * bh, y1 = std::min(height, y0 + bh);
        HIPC(hipEventSynchronize(bm->evBand[b]));
        if ((size_t)width == Ws && disp_pitch == Ws * sizeof(int16_t)) {   // no pad columns between the rows: one copy per band
            memcpy((uint8_t*)disp + (size_t)y0 * disp_pitch, hD + (size_t)y0 * Ws, (size_t)(y1 - y0 - 1) * disp_pitch + (size_t)width * sizeof(int16_t));
        } else {
            for (int y = y0; y < y1; ++y)
                memcpy((uint8_t*)disp + (size_t)y * disp_pitch, hD + (size_t)y * Ws, (size_t)width * sizeof(int16_t));
        }
    }
    drain.armed = false;
    return RTDM_OK;
}

int rtdm_bm_synchronize(rtdm_bm* bm)
{
    if (!bm) return RTDM_ERR_NULL;
    HIPC(hipSetDevice(bm->device));
    HIPC(hipStreamSynchronize(bm->stream));
    return RTDM_OK;
}

int rtdm_bm_set_profiling(rtdm_bm* bm, int enabled)
{
    if (!bm) return RTDM_ERR_NULL;
    bm->profiling = enabled != 0;
    return RTDM_OK;
}

static int drain_events(rtdm_bm* bm)
{
    for (auto& ev : bm->pending) {
        HIPC(hipEventSynchronize(ev.b));
        float ms = 0.f;
        HIPC(hipEventElapsedTime(&ms, ev.a, ev.b));
        bm->stage_ms[ev.stage] += ms;
        bm->stage_launches[ev.stage] += 1;
        bm->stage_frames[ev.stage] += ev.frames;
        (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b);
    }
    bm->pending.clear();
    return RTDM_OK;
}

int rtdm_bm_get_stage_time(rtdm_bm* bm, int stage, double* total_ms, long* launches, long* frames)
{
    if (!bm) return RTDM_ERR_NULL;
    if (stage < 0 || stage >= RTDM_NUM_STAGES) return RTDM_ERR_BAD_PARAM;
    HIPC(hipSetDevice(bm->device));
    int rc = drain_events(bm);
    if (rc) return rc;
    if (total_ms) *total_ms = bm->stage_ms[stage];
    if (launches) *launches = bm->stage_launches[stage];
    if (frames) *frames = bm->stage_frames[stage];
    return RTDM_OK;
}

int rtdm_bm_reset_stage_times(rtdm_bm* bm)
{
    if (!bm) return RTDM_ERR_NULL;
    HIPC(hipSetDevice(bm->device));
    int rc = drain_events(bm);
    if (rc) return rc;
    for (int i = 0; i < RTDM_NUM_STAGES; ++i) { bm->stage_ms[i] = 0; bm->stage_launches[i] = 0; bm->stage_frames[i] = 0; }
    return RTDM_OK;
}

const char* rtdm_bm_search_variant(const rtdm_bm* bm) { return bm ? bm->variant.c_str() : ""; }
int rtdm_bm_get_tuner_stats(const rtdm_bm* bm, long* shapes_measured, long* timing_launches)
{
    if (!bm) return RTDM_ERR_NULL;
    if (shapes_measured) *shapes_measured = bm->tune_shapes;
    if (timing_launches) *timing_launches = bm->tune_launches;
    return RTDM_OK;
}
void rtdm_debug_search_kernel(int mode) { ring_set_mode(mode); }
void rtdm_debug_disparity_slice(int dt) { dslice_set_width(dt); }

// ---- VideoFilterDevice ---------------------------------------------------------------------
int rtdm_morph_create(int width, int height, int max_batch, int device, rtdm_morph** out)
{
    if (!out) return RTDM_ERR_NULL;
    *out = nullptr;
    if (width <= 0 || height <= 0 || max_batch <= 0) return RTDM_ERR_BAD_SIZE;
    int rc = use_device(device);
    if (rc) return rc;
    rtdm_morph* mf = new (std::nothrow) rtdm_morph();
    if (!mf) return RTDM_ERR_NOMEM;
    mf->W = width; mf->H = height; mf->maxB = max_batch; mf->device = device;
    const size_t px = (size_t)width * height, all = px * max_batch;
    hipError_t e = hipStreamCreateWithFlags(&mf->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void**)&mf->hIn, px, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&mf->hOut, px, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&mf->dIn, all);
    if (e == hipSuccess) e = hipMalloc((void**)&mf->dOut, all);
    if (e == hipSuccess) e = hipMalloc((void**)&mf->dT0, all);
    if (e == hipSuccess) e = hipMalloc((void**)&mf->dT1, all);
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_morph_create: ") + hipGetErrorString(e);
        rtdm_morph_destroy(mf);
        return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
    }
    *out = mf;
    return RTDM_OK;
}

void rtdm_morph_destroy(rtdm_morph* mf)
{
    if (!mf) return;
    (void)hipSetDevice(mf->device);
    if (mf->stream) (void)hipStreamSynchronize(mf->stream);
    if (mf->hIn) (void)hipHostFree(mf->hIn);
    if (mf->hOut) (void)hipHostFree(mf->hOut);
    void* bufs[] = {mf->dIn, mf->dOut, mf->dT0, mf->dT1};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (mf->stream) (void)hipStreamDestroy(mf->stream);
    delete mf;
}

uint8_t* rtdm_morph_in_buffer(rtdm_morph* mf) { return mf ? mf->hIn : nullptr; }
uint8_t* rtdm_morph_out_buffer(rtdm_morph* mf) { return mf ? mf->hOut : nullptr; }

int rtdm_morph_run_device(rtdm_morph* mf, int n, const uint8_t* d_in, size_t in_pitch, size_t in_frame_stride,
                          uint8_t* d_out, size_t out_pitch, size_t out_frame_stride, int width, int height,
                          void* hip_stream)
{
    if (!mf || !d_in || !d_out) return RTDM_ERR_NULL;
    if (n <= 0 || width <= 0 || height <= 0 || (size_t)width * height > (size_t)mf->W * mf->H) return RTDM_ERR_BAD_SIZE;
    if (in_pitch < (size_t)width || out_pitch < (size_t)width) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(mf->device));
    hipStream_t s = (hipStream_t)hip_stream;          // NULL = the HIP null stream
    for (int i0 = 0; i0 < n; i0 += mf->maxB) {
        const int m = std::min(mf->maxB, n - i0);
        Plane8 in{d_in + (size_t)i0 * in_frame_stride, in_pitch, in_frame_stride};
        Plane8W out{d_out + (size_t)i0 * out_frame_stride, out_pitch, out_frame_stride};
        launch_morph_open_close(in, out, mf->dT0, mf->dT1, width, height, m, s);
    }
    HIPC(hipGetLastError());
    return RTDM_OK;
}

int rtdm_morph_run(rtdm_morph* mf, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_pitch,
                   int width, int height)
{
    if (!mf || !in || !out) return RTDM_ERR_NULL;
    if (width <= 0 || height <= 0 || (size_t)width * height > (size_t)mf->W * mf->H) return RTDM_ERR_BAD_SIZE;
    if (in_pitch < (size_t)width || out_pitch < (size_t)width) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(mf->device));
    hipStream_t s = mf->stream;
    HIPC(hipMemcpy2DAsync(mf->dIn, width, in, in_pitch, width, height, hipMemcpyHostToDevice, s));
    int rc = rtdm_morph_run_device(mf, 1, mf->dIn, width, (size_t)width * height, mf->dOut, width,
                                   (size_t)width * height, width, height, s);
    if (rc) return rc;
    HIPC(hipMemcpy2DAsync(out, out_pitch, mf->dOut, width, width, height, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return RTDM_OK;
}

// ---- the step after the matcher ---------------------------------------------------------------
static int check_regions(const rtdm_region* regions, int n, int W, int H, int* flat, int* maxh)
{
    if (n < 0 || n > RTDM_MAX_REGIONS || (n > 0 && !regions)) return RTDM_ERR_BAD_SIZE;
    *maxh = 1;
    for (int i = 0; i < n; ++i) {
        const rtdm_region& r = regions[i];
        if (r.x < 0 || r.y < 0 || r.width < 0 || r.height < 0 || r.x + r.width > W || r.y + r.height > H) return RTDM_ERR_BAD_SIZE;
        flat[4 * i] = r.x; flat[4 * i + 1] = r.y; flat[4 * i + 2] = r.width; flat[4 * i + 3] = r.height;
        *maxh = std::max(*maxh, r.height);
    }
    return RTDM_OK;
}

int rtdm_depth_stats_device(int device, const int16_t* d_disp, size_t disp_pitch, int width, int height, const double* Q,
                            const uint8_t* d_mask, size_t mask_pitch, const rtdm_region* regions, int nregions,
                            double calibration_unit, double* mean_cm, int* counts, void* hip_stream)
{
    if (!d_disp || !Q || !d_mask || !mean_cm || !counts) return RTDM_ERR_NULL;
    if (width <= 0 || height <= 0 || disp_pitch < (size_t)width * 2 || (disp_pitch & 1) || mask_pitch < (size_t)width) return RTDM_ERR_BAD_SIZE;
    int flat[4 * RTDM_MAX_REGIONS], maxh = 1;
    int rc = check_regions(regions, nregions, width, height, flat, &maxh);
    if (rc) return rc;
    rc = use_device(device);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    void* scratch = nullptr;
    HIPC(hipMalloc(&scratch, depth_scratch_bytes(std::max(nregions, 1), maxh)));
    DepthQ q; std::copy(Q, Q + 16, q.q);
    launch_depth_stats(d_disp, disp_pitch / 2, width, height, q, d_mask, mask_pitch, flat, nregions, maxh, calibration_unit,
                       scratch, mean_cm, counts, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    HIPC(e);
    return RTDM_OK;
}

int rtdm_bm_compute_depth(rtdm_bm* bm, const uint8_t* left, size_t left_pitch, const uint8_t* right, size_t right_pitch,
                          int width, int height, const double* Q, const uint8_t* mask, size_t mask_pitch,
                          const rtdm_region* regions, int nregions, double calibration_unit,
                          double* mean_cm, int* counts, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !left || !right || !Q || !mask || !mean_cm || !counts) return RTDM_ERR_NULL;
    int rc = check_frame(bm, width, height);
    if (rc) return rc;
    if (left_pitch < (size_t)width || right_pitch < (size_t)width || mask_pitch < (size_t)width) return RTDM_ERR_BAD_SIZE;
    if (disp && disp_pitch < (size_t)width * 2) return RTDM_ERR_BAD_SIZE;
    int flat[4 * RTDM_MAX_REGIONS], maxh = 1;
    rc = check_regions(regions, nregions, width, height, flat, &maxh);
    if (rc) return rc;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    const size_t dpitch = bm->ppitch, dframe = bm->ppitch * (size_t)height;
    uint8_t* hL = bm->hStage;
    uint8_t* hR = hL + dframe;
    int16_t* hD = (int16_t*)(bm->hStage + 2 * bm->ppitch * (size_t)bm->maxH);
    uint8_t* hM = (uint8_t*)(hD + (size_t)((bm->maxW + 7) & ~7) * bm->maxH);
    for (int y = 0; y < height; ++y) {
        memcpy(hL + (size_t)y * dpitch, left + (size_t)y * left_pitch, (size_t)width);
        memcpy(hR + (size_t)y * dpitch, right + (size_t)y * right_pitch, (size_t)width);
        memcpy(hM + (size_t)y * width, mask + (size_t)y * mask_pitch, (size_t)width);
    }
    HIPC(hipMemcpyAsync(bm->dInL, hL, dframe, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(bm->dInR, hR, dframe, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(bm->dMask, hM, (size_t)width * height, hipMemcpyHostToDevice, s));
    Plane8 L{bm->dInL, dpitch, dframe}, R{bm->dInR, dpitch, dframe};
    const size_t Ws = (size_t)((width + 7) & ~7);                      // the handle's internal plane (see run_chunk)
    Plane16W O{bm->dOut, Ws, Ws * (size_t)height};
    rc = run_chunk(bm, 1, L, R, width, height, O, s);
    if (rc) return rc;
    DepthQ q; std::copy(Q, Q + 16, q.q);
    launch_depth_stats(bm->dOut, Ws, width, height, q, bm->dMask, (size_t)width, flat, nregions, bm->maxH,
                       calibration_unit, bm->dDepth, mean_cm, counts, s);
    if (disp) HIPC(hipMemcpyAsync(hD, bm->dOut, Ws * height * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    if (disp)
        for (int y = 0; y < height; ++y)
            memcpy((uint8_t*)disp + (size_t)y * disp_pitch, hD + (size_t)y * Ws, (size_t)width * sizeof(int16_t));
    return RTDM_OK;
}

// ---- SWSemiGlobalMatcher counterpart -------------------------------------------------------
struct rtdm_sgm {
    rtdm_sgm_params p;
    int maxW, maxH, maxB, device;
    hipStream_t stream;
    uint8_t *dInL, *dInR;
    uint8_t *dInL3, *dInR3;        // colour staging of rtdm_sgm_compute_cn (allocated by the first colour call)
    int16_t* dOut;
    SGMBuffers b;
    int prefilter_cap;             // rtdm_sgm_set_prefilter_cap: R1's ftzero = max(preFilterCap, 15) | 1
    int cost_limit;                // of the current call, > 0 where a block cost + P2 can pass 32767: a block cost above it would
                                   // wrap the library's 16-bit path costs (sgm_cost_limit)
    int32_t* hOvf;                 // page-locked copy of b.ovf
    uint32_t sweep_epoch;          // launches of k_sgm_sweep (tags of its edge ring)
    int sweep_cap[36];             // workgroups the device holds at once, per instantiation (0 = not asked yet)
    bool sweep_reported;           // a give-up of the sweep has been returned to the caller
    const char* path_variant;      // the path-pass form of the last call (launch_sgm), "" before the first
};

// The row-synchronous sweep waits on its neighbours with a bound; a pass that gave up has produced garbage and has said so in a
// page-locked flag.  The call that finds the flag returns an error ONCE; from then on the handle runs one pass per direction.
static int sgm_sweep_check(rtdm_sgm* sg)
{
    if (!sg->b.abortf || !*sg->b.abortf || sg->sweep_reported) return RTDM_OK;
    sg->sweep_reported = true;
    g_hip_err = "StereoSGBM: a row-synchronous sweep gave up waiting for a neighbouring strip; the output of that call is invalid "
                "(this handle runs one pass per direction from now on)";
    return RTDM_ERR_HIP;
}

// R1 generalised (oracle rule restated for colour in tests/sgm_cn_ref.py): a pixel cost is at most M = cn (2 ftzero + 63), a
// block cost at most M blockSize^2; where that + P2 can pass 32767 the block costs are checked against 32767 - P2
static int sgm_ftzero(const rtdm_sgm* sg) { return std::max(sg->prefilter_cap, 15) | 1; }
static int sgm_cost_limit(const rtdm_sgm* sg, int cn)
{
    const long M = (long)cn * (2 * sgm_ftzero(sg) + 63);
    return M * sg->p.blockSize * sg->p.blockSize + sg->p.P2 > 32767 ? 32767 - sg->p.P2 : 0;
}

// colour frames: the 24-byte bounds records (and, for the host entry point, the staging of the interleaved input)
static int sgm_colour_buffers(rtdm_sgm* sg, bool host)
{
    const size_t px = (size_t)sg->maxW * sg->maxH * sg->maxB;
    void** ptrs[] = {(void**)&sg->b.cl, (void**)&sg->b.cr, (void**)&sg->dInL3, (void**)&sg->dInR3};
    const size_t sizes[] = {px * 24, px * 24, (size_t)sg->maxW * sg->maxH * 3, (size_t)sg->maxW * sg->maxH * 3};
    for (int i = 0; i < (host ? 4 : 2); ++i) {
        if (*ptrs[i]) continue;
        const hipError_t e = hipMalloc(ptrs[i], sizes[i]);
        if (e != hipSuccess) {
            *ptrs[i] = nullptr;
            (void)hipGetLastError();
            g_hip_err = std::string("StereoSGBM colour buffers: ") + hipGetErrorString(e);
            return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
        }
    }
    return RTDM_OK;
}

// windows whose block cost + P2 can pass 32767: the frame is refused if it does (what is not restated is the wrap-around)
static int sgm_overflow_check(rtdm_sgm* sg, hipStream_t s)
{
    if (!sg->cost_limit) return RTDM_OK;
    HIPC(hipMemcpyAsync(sg->hOvf, sg->b.ovf, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (!*sg->hOvf) return RTDM_OK;
    HIPC(hipMemsetAsync(sg->b.ovf, 0, sizeof(int32_t), s));
    g_hip_err = "StereoSGBM: a block cost + P2 exceeds 32767 in this frame (the library's 16-bit costs would wrap)";
    return RTDM_ERR_UNSUPPORTED;
}

void rtdm_sgm_default_params(rtdm_sgm_params* p, int numDisparities, int blockSize)
{
    if (!p) return;
    p->blockSize = blockSize; p->minDisparity = 0; p->numDisparities = numDisparities; p->P1 = 600; p->P2 = 2400;
    p->uniquenessRatio = 10; p->speckleWindowSize = 100; p->speckleRange = 32; p->disp12MaxDiff = 1; p->paths = 8;
}

int rtdm_sgm_create(const rtdm_sgm_params* params, int max_width, int max_height, int max_batch, int device, rtdm_sgm** out)
{
    if (!params || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    rtdm_sgm_params p = *params;
    if (p.numDisparities <= 0 || p.numDisparities % 16 != 0 || p.blockSize < 1) return RTDM_ERR_BAD_PARAM;
    if (p.uniquenessRatio > 100) return RTDM_ERR_BAD_PARAM;
    // cv::StereoSGBM's modes by their direction count: 5 MODE_SGBM, 8 MODE_HH, 4 MODE_HH4 (R4'); 3 is MODE_SGBM_3WAY, which the
    // library serves and this build does not
    if (p.paths == 3) return RTDM_ERR_UNSUPPORTED;
    if (p.paths != 4 && p.paths != 5 && p.paths != 8) return RTDM_ERR_BAD_PARAM;
    // cv::StereoSGBM never checks the parity of blockSize: its window is SADWindowSize / 2 either side, an even size runs as
    // the next odd one (sgbm-sw.cpp:15 hands the caller's blockSize straight through)
    p.blockSize = p.blockSize / 2 * 2 + 1;
    // what cv::StereoSGBM does with out-of-range knobs (oracle/sgm_oracle.c R6, R9, R12): it coerces them
    if (p.P1 <= 0) p.P1 = 2;
    p.P2 = std::max(p.P2 > 0 ? p.P2 : 5, p.P1 + 1);
    if (p.uniquenessRatio < 0) p.uniquenessRatio = 10;
    if (p.disp12MaxDiff <= 0) p.disp12MaxDiff = 1;         // the library's left-right check cannot be switched off
    if (max_width <= 0 || max_height <= 0 || max_batch <= 0) return RTDM_ERR_BAD_SIZE;
    if (max_width > 4096) return RTDM_ERR_UNSUPPORTED;
    // 16-bit costs: a path cost is at most block cost + P2 (pixel cost <= M = cn (2 ftzero + 63), 93 for gray at preFilterCap
    // 0); above 32767 the library's short arithmetic wraps, which is not restated: windows that CAN get there (gray at preFilterCap
    // 0: > 17 at P2 = 2400) run with a check of the block costs and refuse the frame that does (RTDM_ERR_UNSUPPORTED from the
    // compute call; it takes nearly every pixel of a window at the maximum pixel cost).  The limit is set per call
    // (sgm_cost_limit): preFilterCap and the channel count change M.
    if (p.blockSize > 255 || p.P2 > 32000) return RTDM_ERR_UNSUPPORTED;
    int rc = use_device(device);
    if (rc) return rc;
    rtdm_sgm* sg = new (std::nothrow) rtdm_sgm();
    if (!sg) return RTDM_ERR_NOMEM;
    sg->p = p; sg->maxW = max_width; sg->maxH = max_height; sg->maxB = max_batch; sg->device = device;
    sg->path_variant = "";
    const size_t px = (size_t)max_width * max_height * max_batch;
    // D <= 256: volumes on max_width columns, as always.  D > 256 (the wide path pass): on the widest column domain a frame can
    // have, W1max = max_width + min(minD, 0) - max(minD + D, 0) -- at D = 4080 on 4096 columns that is 16 columns instead of
    // 4096 -- and no S2 (the side-by-side horizontal passes are off there); W1max <= 0: every frame is all-invalid, no volumes.
    const bool wide = p.numDisparities > 256;
    const long w1max = (long)max_width + std::min(p.minDisparity, 0) - std::max(p.minDisparity + p.numDisparities, 0);
    const size_t vol = wide ? (w1max > 0 ? (size_t)w1max * max_height * max_batch * p.numDisparities : 0) : px * p.numDisparities;
    hipError_t e = hipStreamCreateWithFlags(&sg->stream, hipStreamNonBlocking);
    void** ptrs[] = {(void**)&sg->dInL, (void**)&sg->dInR, (void**)&sg->dOut, (void**)&sg->b.gl, (void**)&sg->b.gr,
                     (void**)&sg->b.pix, (void**)&sg->b.C, (void**)&sg->b.S, (void**)&sg->b.label, (void**)&sg->b.size,
                     (void**)&sg->b.runs, (void**)&sg->b.rowcnt, (void**)&sg->b.headmap};
    const size_t sizes[] = {px, px, px * 2, px * 8, px * 8, vol, vol * 2, vol * 2, px * 4, px * 4, px * 4,
                            (size_t)max_batch * max_height * 4, px * 2};
    for (int i = 0; i < 13 && e == hipSuccess; ++i) if (sizes[i]) e = hipMalloc(ptrs[i], sizes[i]);
    if (e == hipSuccess) e = hipMalloc((void**)&sg->b.ovf, sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(sg->b.ovf, 0, sizeof(int32_t));
    if (e == hipSuccess) e = hipHostMalloc((void**)&sg->hOvf, sizeof(int32_t), hipHostMallocDefault);
    // (MODE_HH4 never runs a row-synchronous sweep: no edge ring)
    sg->b.ring_words = p.paths == 4 ? 0 : sgm_ring_words(max_width, p.numDisparities, max_batch);
    if (e == hipSuccess && sg->b.ring_words) e = hipMalloc((void**)&sg->b.ring, sg->b.ring_words * sizeof(unsigned long long));
    if (e == hipSuccess && sg->b.ring_words) e = hipMemset(sg->b.ring, 0, sg->b.ring_words * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipHostMalloc((void**)&sg->b.abortf, sizeof(int32_t), hipHostMallocMapped);
    // (C, S and S2 are whole allocations, so at least 256-byte aligned: the path passes' packed loads and stores need 16 bytes)
    if (e == hipSuccess && !wide && hipMalloc((void**)&sg->b.S2, vol * 2) != hipSuccess) { (void)hipGetLastError(); sg->b.S2 = nullptr; }   // (optional: without it the horizontal passes run one after the other)
    if (e == hipSuccess) *sg->b.abortf = 0;
    sg->b.epoch = &sg->sweep_epoch; sg->b.sweep_cap = sg->sweep_cap;
    if (e == hipSuccess) e = hipEventCreateWithFlags((hipEvent_t*)&sg->b.ev_in, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags((hipEvent_t*)&sg->b.ev_out, hipEventDisableTiming);
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_sgm_create: ") + hipGetErrorString(e);
        rtdm_sgm_destroy(sg);
        return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
    }
    *out = sg;
    return RTDM_OK;
}

void rtdm_sgm_destroy(rtdm_sgm* sg)
{
    if (!sg) return;
    (void)hipSetDevice(sg->device);
    if (sg->stream) (void)hipStreamSynchronize(sg->stream);
    void* bufs[] = {sg->dInL, sg->dInR, sg->dOut, sg->b.gl, sg->b.gr, sg->b.pix, sg->b.C, sg->b.S, sg->b.label, sg->b.size,
                    sg->b.runs, sg->b.rowcnt, sg->b.headmap, sg->b.cl, sg->b.cr, sg->dInL3, sg->dInR3};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (sg->b.ovf) (void)hipFree(sg->b.ovf);
    if (sg->b.ring) (void)hipFree(sg->b.ring);
    if (sg->b.S2) (void)hipFree(sg->b.S2);
    if (sg->b.abortf) (void)hipHostFree(sg->b.abortf);
    if (sg->b.ev_in) (void)hipEventDestroy((hipEvent_t)sg->b.ev_in);
    if (sg->b.ev_out) (void)hipEventDestroy((hipEvent_t)sg->b.ev_out);
    if (sg->hOvf) (void)hipHostFree(sg->hOvf);
    if (sg->stream) (void)hipStreamDestroy(sg->stream);
    delete sg;
}

static int sgm_chunk(rtdm_sgm* sg, int n, int cn, Plane8 L, Plane8 R, int W, int H, Plane16W disp, hipStream_t s)
{
    const rtdm_sgm_params& p = sg->p;
    SGMGeom g;
    g.W = W; g.H = H; g.D = p.numDisparities; g.minD = p.minDisparity;
    g.x0 = std::max(g.minD + g.D, 0);
    g.W1 = (W + std::min(g.minD, 0)) - g.x0;
    if (g.W1 <= 0) { launch_fill16(disp, 0, W, 0, H, n, (g.minD - 1) * 16, s); return RTDM_OK; }
    sg->path_variant = launch_sgm(L, R, disp, g, sg->b, p.blockSize, p.P1, p.P2, p.uniquenessRatio, p.disp12MaxDiff,
                                  p.speckleWindowSize, p.speckleRange, p.paths, n, s, sg->cost_limit, cn, sgm_ftzero(sg));
    HIPC(hipGetLastError());
    return RTDM_OK;
}

int rtdm_sgm_compute_device_cn(rtdm_sgm* sg, int channels, int n, const uint8_t* d_left, const uint8_t* d_right, size_t pitch,
                               size_t frame_stride, int width, int height, int16_t* d_disp, size_t disp_pitch,
                               size_t disp_frame_stride, void* hip_stream)
{
    if (!sg || !d_left || !d_right || !d_disp) return RTDM_ERR_NULL;
    if (channels != 1 && channels != 3) return RTDM_ERR_BAD_PARAM;
    if (n <= 0 || width <= 0 || height <= 0 || width > sg->maxW || height > sg->maxH) return RTDM_ERR_BAD_SIZE;
    if (pitch < (size_t)width * channels || disp_pitch < (size_t)width * 2 || (disp_pitch & 1) || (disp_frame_stride & 1)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(sg->device));
    if (channels == 3) { const int rc = sgm_colour_buffers(sg, false); if (rc) return rc; }
    sg->cost_limit = sgm_cost_limit(sg, channels);
    hipStream_t s = (hipStream_t)hip_stream;          // NULL = the HIP null stream
    for (int i0 = 0; i0 < n; i0 += sg->maxB) {
        const int m = std::min(sg->maxB, n - i0);
        Plane8 L{d_left + (size_t)i0 * frame_stride, pitch, frame_stride}, R{d_right + (size_t)i0 * frame_stride, pitch, frame_stride};
        Plane16W O{d_disp + (size_t)i0 * (disp_frame_stride / 2), disp_pitch / 2, disp_frame_stride / 2};
        int rc = sgm_chunk(sg, m, channels, L, R, width, height, O, s);
        if (rc) return rc;
    }
    int rc = sgm_overflow_check(sg, s);                // (where a block cost can overflow: this call then synchronises the stream)
    return rc ? rc : sgm_sweep_check(sg);              // (asynchronous call: a give-up of this call's sweep shows in the next call)
}

int rtdm_sgm_compute_device(rtdm_sgm* sg, int n, const uint8_t* d_left, const uint8_t* d_right, size_t pitch,
                            size_t frame_stride, int width, int height, int16_t* d_disp, size_t disp_pitch,
                            size_t disp_frame_stride, void* hip_stream)
{
    return rtdm_sgm_compute_device_cn(sg, 1, n, d_left, d_right, pitch, frame_stride, width, height, d_disp, disp_pitch,
                                      disp_frame_stride, hip_stream);
}

int rtdm_sgm_compute_cn(rtdm_sgm* sg, int channels, const uint8_t* left, size_t left_pitch, const uint8_t* right,
                        size_t right_pitch, int width, int height, int16_t* disp, size_t disp_pitch)
{
    if (!sg || !left || !right || !disp) return RTDM_ERR_NULL;
    if (channels != 1 && channels != 3) return RTDM_ERR_BAD_PARAM;
    if (width <= 0 || height <= 0 || width > sg->maxW || height > sg->maxH) return RTDM_ERR_BAD_SIZE;
    const size_t row = (size_t)width * channels;
    if (left_pitch < row || right_pitch < row || disp_pitch < (size_t)width * 2) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(sg->device));
    if (channels == 3) { const int rc = sgm_colour_buffers(sg, true); if (rc) return rc; }
    sg->cost_limit = sgm_cost_limit(sg, channels);
    hipStream_t s = sg->stream;
    uint8_t* inL = channels == 3 ? sg->dInL3 : sg->dInL;
    uint8_t* inR = channels == 3 ? sg->dInR3 : sg->dInR;
    HIPC(hipMemcpy2DAsync(inL, row, left, left_pitch, row, height, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpy2DAsync(inR, row, right, right_pitch, row, height, hipMemcpyHostToDevice, s));
    Plane8 L{inL, row, row * height}, R{inR, row, row * height};
    Plane16W O{sg->dOut, (size_t)width, (size_t)width * height};
    int rc = sgm_chunk(sg, 1, channels, L, R, width, height, O, s);
    if (rc) return rc;
    HIPC(hipMemcpy2DAsync(disp, disp_pitch, sg->dOut, (size_t)width * 2, (size_t)width * 2, height, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    rc = sgm_overflow_check(sg, s);
    return rc ? rc : sgm_sweep_check(sg);
}

int rtdm_sgm_compute(rtdm_sgm* sg, const uint8_t* left, size_t left_pitch, const uint8_t* right, size_t right_pitch,
                     int width, int height, int16_t* disp, size_t disp_pitch)
{
    return rtdm_sgm_compute_cn(sg, 1, left, left_pitch, right, right_pitch, width, height, disp, disp_pitch);
}

int rtdm_sgm_set_prefilter_cap(rtdm_sgm* sg, int preFilterCap)
{
    if (!sg) return RTDM_ERR_NULL;
    if (preFilterCap >= 128) return RTDM_ERR_UNSUPPORTED;      // the library's 8-bit clip table wraps from here on
    sg->prefilter_cap = preFilterCap;
    return RTDM_OK;
}

int rtdm_sgm_get_pass_stats(const rtdm_sgm* sg, long* sweeps, int* gave_up)
{
    if (!sg) return RTDM_ERR_NULL;
    if (sweeps) *sweeps = (long)sg->sweep_epoch;
    if (gave_up) *gave_up = sg->b.abortf && *sg->b.abortf ? 1 : 0;
    return RTDM_OK;
}

const char* rtdm_sgm_path_variant(const rtdm_sgm* sg) { return sg ? sg->path_variant : ""; }
void rtdm_debug_sgm_wide_paths(int lines_per_wave_or_waves) { sgm_wide_set_mode(lines_per_wave_or_waves); }
void rtdm_debug_sgm_cost16(int on) { sgm_cost16_set(on); }

// ---- rectification in front of the matcher (estimator.cpp:29-39) ----------------------------------------------
struct rtdm_rectify {
    int W, H, rx, ry, rw, rh, maxB, device;
    int16_t* dMap1[2];            // roi part of the maps: rh x rw x 2
    uint16_t* dMap2[2];           // rh x rw
    uint8_t* dRgb[2];             // staging for host frames: H x W x 3 (+ padding)
    uint8_t* dOut;                // staging for host outputs: rh x rw x 3
    uint8_t* dGray[2];            // rectified gray pair for the chained matcher call: rh x pitch
    size_t gpitch;
    uint8_t* hStage;              // pinned: 2 RGB frames in, rh x rw x 3 out
    hipStream_t stream;
};

void rtdm_rectify_destroy(rtdm_rectify* rc)
{
    if (!rc) return;
    (void)hipSetDevice(rc->device);
    if (rc->stream) (void)hipStreamSynchronize(rc->stream);
    void* bufs[] = {rc->dMap1[0], rc->dMap1[1], rc->dMap2[0], rc->dMap2[1], rc->dRgb[0], rc->dRgb[1], rc->dOut, rc->dGray[0], rc->dGray[1]};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (rc->hStage) (void)hipHostFree(rc->hStage);
    if (rc->stream) (void)hipStreamDestroy(rc->stream);
    delete rc;
}

// stream, device buffers and the pinned staging area of a handle whose geometry is set
static hipError_t rectify_alloc(rtdm_rectify* rc)
{
    const size_t npx = (size_t)rc->rw * rc->rh, fbytes = (size_t)rc->W * rc->H * 3;
    hipError_t e = hipStreamCreateWithFlags(&rc->stream, hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = hipMalloc((void**)&rc->dMap1[k], npx * 4);
        if (e == hipSuccess) e = hipMalloc((void**)&rc->dMap2[k], npx * 2);
        if (e == hipSuccess) e = hipMalloc((void**)&rc->dRgb[k], fbytes + 16);
        if (e == hipSuccess) e = hipMalloc((void**)&rc->dGray[k], rc->gpitch * rc->rh * (size_t)rc->maxB);
    }
    if (e == hipSuccess) e = hipMalloc((void**)&rc->dOut, npx * 3);
    if (e == hipSuccess) e = hipHostMalloc((void**)&rc->hStage, 2 * fbytes + npx * 3 + 128 * (size_t)rc->rh, hipHostMallocDefault);
    return e;
}

static int rectify_check_geometry(int width, int height, int roi_x, int roi_y, int roi_width, int roi_height, int max_batch)
{
    if (width <= 0 || height <= 0 || width > 32767 || height > 32767 || max_batch <= 0) return RTDM_ERR_BAD_SIZE;
    if (roi_x < 0 || roi_y < 0 || roi_width <= 0 || roi_height <= 0 || roi_x + roi_width > width || roi_y + roi_height > height)
        return RTDM_ERR_BAD_SIZE;
    return RTDM_OK;
}

static rtdm_rectify* rectify_new(int width, int height, int roi_x, int roi_y, int roi_width, int roi_height, int max_batch, int device)
{
    rtdm_rectify* rc = new (std::nothrow) rtdm_rectify();
    if (!rc) return nullptr;
    rc->W = width; rc->H = height; rc->rx = roi_x; rc->ry = roi_y; rc->rw = roi_width; rc->rh = roi_height;
    rc->maxB = max_batch; rc->device = device;
    rc->gpitch = ((size_t)roi_width + 63) & ~(size_t)63;
    return rc;
}

static int rectify_create_failed(rtdm_rectify* rc, const char* where, hipError_t e)
{
    g_hip_err = std::string(where) + ": " + hipGetErrorString(e);
    rtdm_rectify_destroy(rc);
    return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
}

int rtdm_rectify_create(const int16_t* map1_left, const uint16_t* map2_left, const int16_t* map1_right,
                        const uint16_t* map2_right, int width, int height, int roi_x, int roi_y, int roi_width,
                        int roi_height, int max_batch, int device, rtdm_rectify** out)
{
    if (!map1_left || !map2_left || !map1_right || !map2_right || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    int st = rectify_check_geometry(width, height, roi_x, roi_y, roi_width, roi_height, max_batch);
    if (st) return st;
    st = use_device(device);
    if (st) return st;
    rtdm_rectify* rc = rectify_new(width, height, roi_x, roi_y, roi_width, roi_height, max_batch, device);
    if (!rc) return RTDM_ERR_NOMEM;
    const size_t npx = (size_t)roi_width * roi_height;
    hipError_t e = rectify_alloc(rc);
    if (e == hipSuccess) {
        // crop the maps on the host (through the pinned area), one linear copy each
        for (int k = 0; k < 2 && e == hipSuccess; ++k) {
            const int16_t* m1 = k ? map1_right : map1_left;
            const uint16_t* m2 = k ? map2_right : map2_left;
            int16_t* h1 = (int16_t*)rc->hStage;
            uint16_t* h2 = (uint16_t*)(rc->hStage + npx * 4);
            for (int y = 0; y < roi_height; ++y) {
                memcpy(h1 + (size_t)y * roi_width * 2, m1 + ((size_t)(roi_y + y) * width + roi_x) * 2, (size_t)roi_width * 4);
                memcpy(h2 + (size_t)y * roi_width, m2 + (size_t)(roi_y + y) * width + roi_x, (size_t)roi_width * 2);
            }
            e = hipMemcpy(rc->dMap1[k], h1, npx * 4, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(rc->dMap2[k], h2, npx * 2, hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) return rectify_create_failed(rc, "rtdm_rectify_create", e);
    *out = rc;
    return RTDM_OK;
}

// ---- rectification from the calibration files (main.cpp:53-98; rtdm_calib.h, k_rectmap.hip) -------------------------------------
static_assert(sizeof(rtdm_calib) == sizeof(Calib) && sizeof(rtdm_rectification) == sizeof(Rectification) &&
              sizeof(rtdm_region) == sizeof(CalibRegion), "rtdm_calib.h restates the layouts of rtdm.h");

int rtdm_calib_load(const char* intrinsics_path, const char* extrinsics_path, rtdm_calib* calib, rtdm_rectification* stored,
                    unsigned* stored_mask)
{
    if (!intrinsics_path || !extrinsics_path || !calib) return RTDM_ERR_NULL;
    Calib c;
    Rectification r;
    unsigned mask = 0;
    const int st = calib_load(intrinsics_path, extrinsics_path, &c, &r, &mask);
    if (st) return st;
    memcpy(calib, &c, sizeof c);
    if (stored) memcpy(stored, &r, sizeof r);
    if (stored_mask) *stored_mask = mask;
    return RTDM_OK;
}

int rtdm_stereo_rectify(const rtdm_calib* calib, int flags, double alpha, int new_width, int new_height, rtdm_rectification* out)
{
    if (!calib || !out) return RTDM_ERR_NULL;
    Calib c;
    Rectification r;
    memcpy(&c, calib, sizeof c);
    const int st = calib_stereo_rectify(&c, flags, alpha, new_width, new_height, &r);
    if (st) return st;
    memcpy(out, &r, sizeof r);
    return RTDM_OK;
}

static int rectmap_params(const double* M, const double* D, const double* R, const double* P, int width, int height, RectMapParams* o)
{
    const int st = calib_rectmap_check(M, D, R, P, width, height, o->ir);
    if (st) return st;
    o->fx = M[0]; o->fy = M[4]; o->u0 = M[2]; o->v0 = M[5];
    for (int i = 0; i < 12; ++i) o->k[i] = D[i];
    return RTDM_OK;
}

// the full maps of one camera into device memory; returns when they are complete
static int rectmap_full(const RectMapParams& P, int width, int height, int16_t* d_map1, uint16_t* d_map2, hipStream_t s)
{
    double* ckpt = nullptr;
    HIPC(hipMalloc((void**)&ckpt, rectmap_scratch_bytes(0, width, height)));
    launch_rectmap(P, 0, 0, width, height, ckpt, d_map1, d_map2, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(ckpt);
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_undistort_rectify_map: ") + hipGetErrorString(e);
        return RTDM_ERR_HIP;
    }
    return RTDM_OK;
}

int rtdm_undistort_rectify_map_device(const double* M, const double* D, const double* R, const double* P, int width, int height,
                                      int device, int16_t* d_map1, uint16_t* d_map2, void* hip_stream)
{
    if (!M || !D || !R || !P || !d_map1 || !d_map2) return RTDM_ERR_NULL;
    RectMapParams prm;
    int st = rectmap_params(M, D, R, P, width, height, &prm);
    if (st) return st;
    if (((uintptr_t)d_map1 & 3) || ((uintptr_t)d_map2 & 1)) return RTDM_ERR_BAD_SIZE;
    st = use_device(device);
    if (st) return st;
    return rectmap_full(prm, width, height, d_map1, d_map2, (hipStream_t)hip_stream);
}

int rtdm_undistort_rectify_map(const double* M, const double* D, const double* R, const double* P, int width, int height,
                               int device, int16_t* map1, uint16_t* map2)
{
    if (!M || !D || !R || !P || !map1 || !map2) return RTDM_ERR_NULL;
    RectMapParams prm;
    int st = rectmap_params(M, D, R, P, width, height, &prm);
    if (st) return st;
    st = use_device(device);
    if (st) return st;
    const size_t npx = (size_t)width * height;
    int16_t* d1 = nullptr;
    HIPC(hipMalloc((void**)&d1, npx * 6));                   // map1, then map2 behind it
    uint16_t* d2 = (uint16_t*)(d1 + npx * 2);
    st = rectmap_full(prm, width, height, d1, d2, nullptr);
    hipError_t e = hipSuccess;
    if (st == RTDM_OK) e = hipMemcpy(map1, d1, npx * 4, hipMemcpyDeviceToHost);
    if (st == RTDM_OK && e == hipSuccess) e = hipMemcpy(map2, d2, npx * 2, hipMemcpyDeviceToHost);
    (void)hipFree(d1);
    if (st) return st;
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_undistort_rectify_map: ") + hipGetErrorString(e);
        return RTDM_ERR_HIP;
    }
    return RTDM_OK;
}

int rtdm_rectify_create_calib(const rtdm_calib* calib, const rtdm_rectification* rect, int roi_x, int roi_y, int roi_width,
                              int roi_height, int max_batch, int device, rtdm_rectify** out)
{
    if (!calib || !rect || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    const int width = calib->width, height = calib->height;
    int st = rectify_check_geometry(width, height, roi_x, roi_y, roi_width, roi_height, max_batch);
    if (st) return st;
    RectMapParams prm[2];
    st = rectmap_params(calib->M1, calib->D1, rect->R1, rect->P1, width, height, &prm[0]);
    if (st == RTDM_OK) st = rectmap_params(calib->M2, calib->D2, rect->R2, rect->P2, width, height, &prm[1]);
    if (st) return st;
    st = use_device(device);
    if (st) return st;
    rtdm_rectify* rc = rectify_new(width, height, roi_x, roi_y, roi_width, roi_height, max_batch, device);
    if (!rc) return RTDM_ERR_NOMEM;
    hipError_t e = rectify_alloc(rc);
    double* ckpt = nullptr;
    const size_t cbytes = rectmap_scratch_bytes(roi_x, roi_width, roi_height);
    if (e == hipSuccess) e = hipMalloc((void**)&ckpt, 2 * cbytes);
    if (e == hipSuccess) {
        for (int k = 0; k < 2; ++k)
            launch_rectmap(prm[k], roi_x, roi_y, roi_width, roi_height, ckpt + k * (cbytes / sizeof(double)), rc->dMap1[k], rc->dMap2[k],
                           rc->stream);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(rc->stream);
    }
    if (ckpt) (void)hipFree(ckpt);
    if (e != hipSuccess) return rectify_create_failed(rc, "rtdm_rectify_create_calib", e);
    *out = rc;
    return RTDM_OK;
}

// host RGB frames -> dRgb[0/1] through the pinned staging area
static int rectify_upload(rtdm_rectify* rc, const uint8_t* a, size_t apitch, const uint8_t* b, size_t bpitch, hipStream_t s)
{
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H;
    const uint8_t* src[2] = {a, b};
    const size_t pit[2] = {apitch, bpitch};
    for (int k = 0; k < 2; ++k) {
        if (!src[k]) continue;
        uint8_t* h = rc->hStage + k * fbytes;
        if (pit[k] == row) memcpy(h, src[k], fbytes);
        else for (int y = 0; y < rc->H; ++y) memcpy(h + (size_t)y * row, src[k] + (size_t)y * pit[k], row);
        HIPC(hipMemcpyAsync(rc->dRgb[k], h, fbytes, hipMemcpyHostToDevice, s));
    }
    return RTDM_OK;
}

static void rectify_gray_launch(rtdm_rectify* rc, const uint8_t* dl, const uint8_t* dr, int n, Plane8W ol, Plane8W orr, hipStream_t s)
{
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H;
    RectifySrc L{dl, row, fbytes}, R{dr, row, fbytes};
    launch_rectify_gray(L, R, rc->dMap1[0], rc->dMap2[0], rc->dMap1[1], rc->dMap2[1], rc->W, rc->H, rc->rw, rc->rh, ol, orr, n, s);
}

int rtdm_rectify_gray(rtdm_rectify* rc, const uint8_t* rgb_left, size_t left_pitch, const uint8_t* rgb_right,
                      size_t right_pitch, uint8_t* left_rect, size_t left_rect_pitch, uint8_t* right_rect,
                      size_t right_rect_pitch)
{
    if (!rc || !rgb_left || !rgb_right || !left_rect || !right_rect) return RTDM_ERR_NULL;
    const size_t row = (size_t)rc->W * 3;
    if (left_pitch < row || right_pitch < row || left_rect_pitch < (size_t)rc->rw || right_rect_pitch < (size_t)rc->rw) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(rc->device));
    hipStream_t s = rc->stream;
    int st = rectify_upload(rc, rgb_left, left_pitch, rgb_right, right_pitch, s);
    if (st) return st;
    const size_t gframe = rc->gpitch * rc->rh;
    rectify_gray_launch(rc, rc->dRgb[0], rc->dRgb[1], 1, Plane8W{rc->dGray[0], rc->gpitch, gframe}, Plane8W{rc->dGray[1], rc->gpitch, gframe}, s);
    HIPC(hipGetLastError());
    // back through the page-locked area (2-D copies into pageable memory take the slow path)
    uint8_t* hl = rc->hStage + 2 * (size_t)rc->W * rc->H * 3;
    uint8_t* hr = hl + gframe;
    HIPC(hipMemcpyAsync(hl, rc->dGray[0], gframe, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(hr, rc->dGray[1], gframe, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (int y = 0; y < rc->rh; ++y) {
        memcpy(left_rect + (size_t)y * left_rect_pitch, hl + (size_t)y * rc->gpitch, (size_t)rc->rw);
        memcpy(right_rect + (size_t)y * right_rect_pitch, hr + (size_t)y * rc->gpitch, (size_t)rc->rw);
    }
    return RTDM_OK;
}

int rtdm_rectify_rgb(rtdm_rectify* rc, int which, const uint8_t* rgb, size_t pitch, uint8_t* out, size_t out_pitch)
{
    if (!rc || !rgb || !out) return RTDM_ERR_NULL;
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H;
    if ((which != 0 && which != 1) || pitch < row || out_pitch < (size_t)rc->rw * 3) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(rc->device));
    hipStream_t s = rc->stream;
    int st = rectify_upload(rc, rgb, pitch, nullptr, 0, s);
    if (st) return st;
    launch_rectify_rgb(RectifySrc{rc->dRgb[0], row, fbytes}, rc->dMap1[which], rc->dMap2[which], rc->W, rc->H, rc->rw, rc->rh,
                       Plane8W{rc->dOut, (size_t)rc->rw * 3, (size_t)rc->rw * 3 * rc->rh}, 1, s);
    HIPC(hipGetLastError());
    uint8_t* ho = rc->hStage + 2 * fbytes;
    HIPC(hipMemcpyAsync(ho, rc->dOut, (size_t)rc->rw * 3 * rc->rh, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (int y = 0; y < rc->rh; ++y) memcpy(out + (size_t)y * out_pitch, ho + (size_t)y * rc->rw * 3, (size_t)rc->rw * 3);
    return RTDM_OK;
}

int rtdm_rectify_gray_device(rtdm_rectify* rc, int n, const uint8_t* d_rgb_left, const uint8_t* d_rgb_right,
                             uint8_t* d_left_rect, uint8_t* d_right_rect, void* hip_stream)
{
    if (!rc || !d_rgb_left || !d_rgb_right || !d_left_rect || !d_right_rect) return RTDM_ERR_NULL;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(rc->device));
    const size_t oframe = (size_t)rc->rw * rc->rh;
    rectify_gray_launch(rc, d_rgb_left, d_rgb_right, n, Plane8W{d_left_rect, (size_t)rc->rw, oframe},
                        Plane8W{d_right_rect, (size_t)rc->rw, oframe}, (hipStream_t)hip_stream);
    HIPC(hipGetLastError());
    return RTDM_OK;
}

// gray + remap + crop of n device frames into the rectifier's planes, then the matcher, chunk by chunk
static int rgb_chunks(rtdm_bm* bm, rtdm_rectify* rc, int n, const uint8_t* dl, const uint8_t* dr, Plane16W out, hipStream_t s)
{
    const size_t fbytes = (size_t)rc->W * rc->H * 3, gframe = rc->gpitch * rc->rh;
    const int chunk = std::min(bm->maxB, rc->maxB);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        rectify_gray_launch(rc, dl + (size_t)i0 * fbytes, dr + (size_t)i0 * fbytes, m,
                            Plane8W{rc->dGray[0], rc->gpitch, gframe}, Plane8W{rc->dGray[1], rc->gpitch, gframe}, s);
        HIPC(hipGetLastError());
        const int st = run_chunk(bm, m, Plane8{rc->dGray[0], rc->gpitch, gframe}, Plane8{rc->dGray[1], rc->gpitch, gframe},
                                 rc->rw, rc->rh, Plane16W{out.base + (size_t)i0 * out.frame_e, out.pitch_e, out.frame_e}, s);
        if (st) return st;
    }
    return RTDM_OK;
}

int rtdm_bm_compute_rgb_device(rtdm_bm* bm, rtdm_rectify* rc, int n, const uint8_t* d_rgb_left,
                               const uint8_t* d_rgb_right, int16_t* d_disp, void* hip_stream)
{
    if (!bm || !rc || !d_rgb_left || !d_rgb_right || !d_disp) return RTDM_ERR_NULL;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    if (bm->device != rc->device) return RTDM_ERR_BAD_PARAM;
    int st = check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    HIPC(hipSetDevice(bm->device));
    const size_t oframe = (size_t)rc->rw * rc->rh;
    return rgb_chunks(bm, rc, n, d_rgb_left, d_rgb_right, Plane16W{d_disp, (size_t)rc->rw, oframe}, (hipStream_t)hip_stream);
}

int rtdm_bm_compute_rgb(rtdm_bm* bm, rtdm_rectify* rc, const uint8_t* rgb_left, size_t left_pitch,
                        const uint8_t* rgb_right, size_t right_pitch, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !rc || !rgb_left || !rgb_right || !disp) return RTDM_ERR_NULL;
    if (bm->device != rc->device) return RTDM_ERR_BAD_PARAM;
    int st = check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    const size_t row = (size_t)rc->W * 3;
    if (left_pitch < row || right_pitch < row || disp_pitch < (size_t)rc->rw * 2) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    st = rectify_upload(rc, rgb_left, left_pitch, rgb_right, right_pitch, s);
    if (st) return st;
    const size_t Ws = (size_t)((rc->rw + 7) & ~7);                     // the handle's internal plane (see run_chunk)
    st = rgb_chunks(bm, rc, 1, rc->dRgb[0], rc->dRgb[1], Plane16W{bm->dOut, Ws, Ws * (size_t)rc->rh}, s);
    if (st) return st;
    int16_t* hD = (int16_t*)(bm->hStage + 2 * bm->ppitch * (size_t)bm->maxH);
    HIPC(hipMemcpyAsync(hD, bm->dOut, Ws * rc->rh * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (int y = 0; y < rc->rh; ++y)
        memcpy((uint8_t*)disp + (size_t)y * disp_pitch, hD + (size_t)y * Ws, (size_t)rc->rw * sizeof(int16_t));
    return RTDM_OK;
}

// ---- object detection -> ROI (estimator.cpp:40-53) and the whole per-frame chain ---------------------------------
struct rtdm_objects {
    int W, H, device, maxRec;
    uint8_t *dRgb, *dMaskIn, *dMaskOut, *dT0, *dT1;
    void* dScratch;
    int* hRec;                    // pinned: [0] = count, then the first HEAD records
    std::vector<int> all;         // host copy of every record when there are more than HEAD
    hipStream_t stream;
};
static const int OBJ_HEAD = 512;  // records fetched together with the count

void rtdm_objects_destroy(rtdm_objects* ob)
{
    if (!ob) return;
    (void)hipSetDevice(ob->device);
    if (ob->stream) (void)hipStreamSynchronize(ob->stream);
    void* bufs[] = {ob->dRgb, ob->dMaskIn, ob->dMaskOut, ob->dT0, ob->dT1, ob->dScratch};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (ob->hRec) (void)hipHostFree(ob->hRec);
    if (ob->stream) (void)hipStreamDestroy(ob->stream);
    delete ob;
}

int rtdm_objects_create(int width, int height, int device, rtdm_objects** out)
{
    if (!out) return RTDM_ERR_NULL;
    *out = nullptr;
    if (width <= 0 || height <= 0 || width > 32767 || height > 32767 || (long)width * height >= (1L << 30)) return RTDM_ERR_BAD_SIZE;
    if (width > 8192) return RTDM_ERR_UNSUPPORTED;      // the component labelling keeps one row of ints in LDS
    int st = use_device(device);
    if (st) return st;
    rtdm_objects* ob = new (std::nothrow) rtdm_objects();
    if (!ob) return RTDM_ERR_NOMEM;
    ob->W = width; ob->H = height; ob->device = device;
    ob->maxRec = ((width + 1) / 2 + 1) * ((height + 1) / 2 + 1);          // more 8-connected components cannot exist
    const size_t px = (size_t)width * height;
    hipError_t e = hipStreamCreateWithFlags(&ob->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&ob->dRgb, px * 3 + 16);
    if (e == hipSuccess) e = hipMalloc((void**)&ob->dMaskIn, px);
    if (e == hipSuccess) e = hipMalloc((void**)&ob->dMaskOut, px);
    if (e == hipSuccess) e = hipMalloc((void**)&ob->dT0, px);
    if (e == hipSuccess) e = hipMalloc((void**)&ob->dT1, px);
    if (e == hipSuccess) e = hipMalloc(&ob->dScratch, cc_scratch_bytes(width, height, ob->maxRec));
    if (e == hipSuccess) e = hipHostMalloc((void**)&ob->hRec, (size_t)(1 + 6 * OBJ_HEAD) * sizeof(int) + px * 3, hipHostMallocDefault);
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_objects_create: ") + hipGetErrorString(e);
        rtdm_objects_destroy(ob);
        return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
    }
    *out = ob;
    return RTDM_OK;
}

// dRgb (crop, pitch 3W) -> mask -> morphology -> component boxes; synchronises `s` to read the boxes back.
static int objects_run(rtdm_objects* ob, const rtdm_hsv_range* range, int min_area, int zero_border, rtdm_region* boxes,
                       int max_boxes, int* nboxes, rtdm_region* roi, hipStream_t s)
{
    const int W = ob->W, H = ob->H;
    launch_hsv_inrange(ob->dRgb, (size_t)W * 3, W, H, range->low, range->high, ob->dMaskIn, (size_t)W, s);
    launch_morph_open_close(Plane8{ob->dMaskIn, (size_t)W, (size_t)W * H}, Plane8W{ob->dMaskOut, (size_t)W, (size_t)W * H},
                            ob->dT0, ob->dT1, W, H, 1, s);
    int *dCount = nullptr, *dRec = nullptr;
    launch_cc_boxes(ob->dMaskOut, (size_t)W, W, H, zero_border, ob->dScratch, ob->maxRec, &dCount, &dRec, s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(ob->hRec, dCount, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(ob->hRec + 1, dRec, (size_t)6 * std::min(OBJ_HEAD, ob->maxRec) * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    const int nrec = std::min(ob->hRec[0], ob->maxRec);
    const int* rec = ob->hRec + 1;
    if (nrec > OBJ_HEAD) {
        ob->all.resize((size_t)6 * nrec);
        HIPC(hipMemcpy(ob->all.data(), dRec, (size_t)6 * nrec * sizeof(int), hipMemcpyDeviceToHost));
        rec = ob->all.data();
    }
    // reverse discovery order = descending first-pixel index; external components with area >= min_area only
    std::vector<const int*> keep;
    for (int i = 0; i < nrec; ++i) {
        const int* r = rec + 6 * i;
        if (r[5] && r[3] * r[4] >= min_area) keep.push_back(r);
    }
    std::sort(keep.begin(), keep.end(), [](const int* a, const int* b) { return a[0] > b[0]; });
    int max_x = -1000000, max_y = -1000000, min_x = 1000000, min_y = 1000000;
    for (size_t i = 0; i < keep.size(); ++i) {
        const int* r = keep[i];
        if ((int)i < max_boxes && boxes) { boxes[i].x = r[1]; boxes[i].y = r[2]; boxes[i].width = r[3]; boxes[i].height = r[4]; }
        min_x = std::min(min_x, r[1]); min_y = std::min(min_y, r[2]);
        max_x = std::max(max_x, r[1] + r[3]); max_y = std::max(max_y, r[2] + r[4]);
    }
    *nboxes = (int)keep.size();
    if (roi) { roi->x = min_x; roi->y = min_y; roi->width = max_x - min_x; roi->height = max_y - min_y; }
    return RTDM_OK;
}

int rtdm_objects_detect(rtdm_objects* ob, const uint8_t* rgb, size_t pitch, const rtdm_hsv_range* range, int min_area,
                        int zero_border, uint8_t* mask_out, size_t mask_pitch, rtdm_region* boxes, int max_boxes,
                        int* nboxes, rtdm_region* roi)
{
    if (!ob || !rgb || !range || !nboxes || (max_boxes > 0 && !boxes)) return RTDM_ERR_NULL;
    const size_t row = (size_t)ob->W * 3;
    if (pitch < row || max_boxes < 0 || (mask_out && mask_pitch < (size_t)ob->W)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(ob->device));
    hipStream_t s = ob->stream;
    uint8_t* h = (uint8_t*)(ob->hRec + 1 + 6 * OBJ_HEAD);
    for (int y = 0; y < ob->H; ++y) memcpy(h + (size_t)y * row, rgb + (size_t)y * pitch, row);
    HIPC(hipMemcpyAsync(ob->dRgb, h, row * ob->H, hipMemcpyHostToDevice, s));
    int st = objects_run(ob, range, min_area, zero_border, boxes, max_boxes, nboxes, roi, s);
    if (st) return st;
    if (mask_out) {                                     // through the page-locked area (the upload is long done)
        HIPC(hipMemcpyAsync(h, ob->dMaskOut, (size_t)ob->W * ob->H, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        for (int y = 0; y < ob->H; ++y) memcpy(mask_out + (size_t)y * mask_pitch, h + (size_t)y * ob->W, (size_t)ob->W);
    }
    return RTDM_OK;
}

int rtdm_estimate_frame(rtdm_bm* bm, rtdm_rectify* rc, rtdm_objects* ob, const uint8_t* rgb_left, size_t left_pitch,
                        const uint8_t* rgb_right, size_t right_pitch, const double* Q, const rtdm_hsv_range* range,
                        int min_area, int zero_border, double calibration_unit, rtdm_region* boxes, double* mean_cm,
                        int* counts, int max_boxes, int* nboxes, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !rc || !ob || !rgb_left || !rgb_right || !Q || !range || !boxes || !mean_cm || !counts || !nboxes) return RTDM_ERR_NULL;
    if (bm->device != rc->device || bm->device != ob->device) return RTDM_ERR_BAD_PARAM;
    if (ob->W != rc->rw || ob->H != rc->rh || max_boxes <= 0) return RTDM_ERR_BAD_SIZE;
    int st = check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    const int W = rc->rw, H = rc->rh;
    const size_t row = (size_t)rc->W * 3, fbytes = row * rc->H;
    if (left_pitch < row || right_pitch < row || (disp && disp_pitch < (size_t)W * 2)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    st = rectify_upload(rc, rgb_left, left_pitch, rgb_right, right_pitch, s);
    if (st) return st;
    // estimator.cpp:29-39: both gray crops and the colour crop of the left frame
    const size_t gframe = rc->gpitch * H;
    rectify_gray_launch(rc, rc->dRgb[0], rc->dRgb[1], 1, Plane8W{rc->dGray[0], rc->gpitch, gframe}, Plane8W{rc->dGray[1], rc->gpitch, gframe}, s);
    launch_rectify_rgb(RectifySrc{rc->dRgb[0], row, fbytes}, rc->dMap1[0], rc->dMap2[0], rc->W, rc->H, W, H,
                       Plane8W{ob->dRgb, (size_t)W * 3, (size_t)W * 3 * H}, 1, s);
    // estimator.cpp:40-53
    rtdm_region roi;
    st = objects_run(ob, range, min_area, zero_border, boxes, max_boxes, nboxes, &roi, s);
    if (st) return st;
    if (*nboxes == 0) return RTDM_OK;                     // estimator.cpp:48: nothing to measure in this frame
    const int nreg = std::min(std::min(*nboxes, max_boxes), RTDM_MAX_REGIONS);
    // estimator.cpp:54-56
    st = rtdm_bm_set_roi(bm, 1, roi.x, roi.y, roi.width, roi.height);
    if (st) return st;
    const size_t Ws = (size_t)((W + 7) & ~7);
    st = run_chunk(bm, 1, Plane8{rc->dGray[0], rc->gpitch, gframe}, Plane8{rc->dGray[1], rc->gpitch, gframe}, W, H,
                   Plane16W{bm->dOut, Ws, Ws * (size_t)H}, s);
    if (st) return st;
    // estimator.cpp:75-77
    int flat[4 * RTDM_MAX_REGIONS], maxh = 1;
    st = check_regions(boxes, nreg, W, H, flat, &maxh);
    if (st) return st;
    DepthQ q; std::copy(Q, Q + 16, q.q);
    launch_depth_stats(bm->dOut, Ws, W, H, q, ob->dMaskOut, (size_t)W, flat, nreg, bm->maxH, calibration_unit, bm->dDepth,
                       mean_cm, counts, s);
    int16_t* hD = (int16_t*)(bm->hStage + 2 * bm->ppitch * (size_t)bm->maxH);
    if (disp) HIPC(hipMemcpyAsync(hD, bm->dOut, Ws * H * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    if (disp)
        for (int y = 0; y < H; ++y) memcpy((uint8_t*)disp + (size_t)y * disp_pitch, hD + (size_t)y * Ws, (size_t)W * sizeof(int16_t));
    return RTDM_OK;
}

// ---- synthetic stream ------------------------------------------------------------------------
int rtdm_synth_pairs_device(uint64_t seed, int first_frame, int n, int width, int height, int numDisparities,
                            uint8_t* d_left, uint8_t* d_right, size_t pitch, size_t frame_stride, int device,
                            void* hip_stream)
{
    if (!d_left || !d_right) return RTDM_ERR_NULL;
    if (n <= 0 || width <= 0 || height <= 0 || pitch < (size_t)width) return RTDM_ERR_BAD_SIZE;
    int rc = use_device(device);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    void* scratch = nullptr;
    HIPC(hipMalloc(&scratch, synth_scratch_bytes(n)));
    Plane8W L{d_left, pitch, frame_stride}, R{d_right, pitch, frame_stride};
    launch_synth(seed, first_frame, n, width, height, numDisparities, L, R, scratch, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    HIPC(e);
    return RTDM_OK;
}

// ---- disparity WLS post-filter (ENABLE_POST_FILTER, estimator.cpp:57-70; rules W1-W8) ----------------
struct rtdm_wls {
    rtdm_wls_params p;
    int maxW, maxH, maxB, device;
    hipStream_t stream;
    float* dLut;                   // W5: lut[k] = exp(-sqrt(k) / sigma), k = 0 .. 3 * 255^2
    float2* dF;                    // [maxB][maxH][maxW] the two right-hand sides / solutions
    float *dWh, *dWv;              // neighbour weights
    uint8_t* dConf;                // C in {0, 255}
    WlsMM *dMML, *dMMR;            // W3 row windows
    int16_t *dInL, *dInR, *dOut;   // single-frame staging of the host entry points
    uint8_t *dGuide, *dImgR;
    float *dConfOut, *dFilt;
};

static const int WLS_LUT_N = 3 * 255 * 255 + 1;

static int wls_validate(const rtdm_wls_params& p)
{
    if (!(p.lambda >= 0.0) || !(p.sigma_color > 0.0) || p.lrc_thresh < 0 || p.depth_discontinuity_radius < 0) return RTDM_ERR_BAD_PARAM;
    if (p.roi_left < 0 || p.roi_right < 0 || p.roi_top < 0 || p.roi_bottom < 0) return RTDM_ERR_BAD_PARAM;
    if (p.num_iter < 1 || p.num_iter > RTDM_WLS_MAX_ITER || !(p.attenuation > 0.0 && p.attenuation <= 1.0)) return RTDM_ERR_BAD_PARAM;
    if (p.use_confidence != 0 && p.use_confidence != 1) return RTDM_ERR_BAD_PARAM;
    // both invalid values, (minD - 1) * 16 and -(minD + numD) * 16, are int16 (the matchers' own bound)
    if (p.num_disparities <= 0 || p.min_disparity < -2047 || (long)p.min_disparity + p.num_disparities > 2047) return RTDM_ERR_BAD_PARAM;
    return RTDM_OK;
}

// W5: computed in double, rounded to float, values below FLT_MIN flushed to 0 (tests/wls_ref.py builds the same table)
static int wls_upload_lut(rtdm_wls* h)
{
    std::vector<float> lut(WLS_LUT_N);
    for (int k = 0; k < WLS_LUT_N; ++k) {
        const float v = (float)std::exp(-std::sqrt((double)k) / h->p.sigma_color);
        lut[k] = v < FLT_MIN ? 0.0f : v;
    }
    HIPC(hipMemcpy(h->dLut, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
    return RTDM_OK;
}

static WlsGeom wls_geom(const rtdm_wls_params& p, int W, int H)
{
    WlsGeom g{p.roi_left, W - p.roi_right, p.roi_top, H - p.roi_bottom};
    if (g.x1 <= g.x0 || g.y1 <= g.y0) g = WlsGeom{0, 0, 0, 0};     // empty ROI: the whole output is invalid
    return g;
}

int rtdm_wls_params_for_bm(const rtdm_bm_params* left, rtdm_wls_params* out)
{
    if (!left || !out) return RTDM_ERR_NULL;
    const int w = left->blockSize, minD = left->minDisparity, numD = left->numDisparities;
    out->lambda = 8000.0; out->sigma_color = 1.5; out->lrc_thresh = 24; out->num_iter = 3; out->attenuation = 0.25;
    out->use_confidence = 1;
    out->depth_discontinuity_radius = (int)std::ceil(0.33 * w);
    out->min_disparity = minD; out->num_disparities = numD;
    out->roi_left = std::max(0, minD + numD) + w / 2;
    out->roi_right = std::max(0, -minD) + w / 2;
    out->roi_top = w / 2; out->roi_bottom = w / 2;
    return RTDM_OK;
}

int rtdm_wls_params_for_sgm(const rtdm_sgm_params* left, rtdm_wls_params* out)
{
    if (!left || !out) return RTDM_ERR_NULL;
    const int w = left->blockSize, minD = left->minDisparity, numD = left->numDisparities;
    out->lambda = 8000.0; out->sigma_color = 1.5; out->lrc_thresh = 24; out->num_iter = 3; out->attenuation = 0.25;
    out->use_confidence = 1;
    out->depth_discontinuity_radius = (int)std::ceil(0.5 * w);
    out->min_disparity = minD; out->num_disparities = numD;
    out->roi_left = std::max(0, minD + numD);
    out->roi_right = std::max(0, -minD);
    out->roi_top = 0; out->roi_bottom = 0;
    return RTDM_OK;
}

int rtdm_bm_right_params(const rtdm_bm_params* left, rtdm_bm_params* right)
{
    if (!left || !right) return RTDM_ERR_NULL;
    *right = *left;                // numDisparities, blockSize, preFilterCap (and the border rule) carry over
    right->minDisparity = -(left->minDisparity + left->numDisparities) + 1;
    right->textureThreshold = 0; right->uniquenessRatio = 0; right->speckleWindowSize = 0; right->disp12MaxDiff = 1000000;
    return RTDM_OK;
}

int rtdm_sgm_right_params(const rtdm_sgm_params* left, rtdm_sgm_params* right)
{
    if (!left || !right) return RTDM_ERR_NULL;
    *right = *left;                // numDisparities, blockSize, P1, P2, paths carry over; preFilterCap is the caller's to copy
    right->minDisparity = -(left->minDisparity + left->numDisparities) + 1;
    right->uniquenessRatio = 0; right->speckleWindowSize = 0; right->disp12MaxDiff = 1000000;
    return RTDM_OK;
}

void rtdm_wls_destroy(rtdm_wls* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    void* bufs[] = {h->dLut, h->dF, h->dWh, h->dWv, h->dConf, h->dMML, h->dMMR, h->dInL, h->dInR, h->dOut, h->dGuide, h->dImgR,
                    h->dConfOut, h->dFilt};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int rtdm_wls_create(const rtdm_wls_params* params, int max_width, int max_height, int max_batch, int device, rtdm_wls** out)
{
    if (!params || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    int rc = wls_validate(*params);
    if (rc) return rc;
    if (max_width <= 0 || max_height <= 0 || max_batch <= 0) return RTDM_ERR_BAD_SIZE;
    if (max_width > 4096 || max_height > 4096) return RTDM_ERR_UNSUPPORTED;   // one wave solves a whole row / column segment
    if ((long)max_batch * max_width * max_height >= (1L << 31)) return RTDM_ERR_BAD_SIZE;
    rc = use_device(device);
    if (rc) return rc;
    rtdm_wls* h = new (std::nothrow) rtdm_wls();
    if (!h) return RTDM_ERR_NOMEM;
    h->p = *params; h->maxW = max_width; h->maxH = max_height; h->maxB = max_batch; h->device = device;
    const size_t px = (size_t)max_width * max_height * max_batch, fr = (size_t)max_width * max_height;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    void** ptrs[] = {(void**)&h->dLut, (void**)&h->dF, (void**)&h->dWh, (void**)&h->dWv, (void**)&h->dConf, (void**)&h->dMML,
                     (void**)&h->dMMR, (void**)&h->dInL, (void**)&h->dInR, (void**)&h->dOut, (void**)&h->dGuide, (void**)&h->dImgR,
                     (void**)&h->dConfOut, (void**)&h->dFilt};
    const size_t sizes[] = {WLS_LUT_N * sizeof(float), px * sizeof(float2), px * 4, px * 4, px, px * sizeof(WlsMM), px * sizeof(WlsMM),
                            fr * 2, fr * 2, fr * 2, fr * 3, fr, fr * 4, fr * 4};
    for (int i = 0; i < 14 && e == hipSuccess; ++i) e = hipMalloc(ptrs[i], sizes[i]);
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_wls_create: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        rtdm_wls_destroy(h);
        return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
    }
    rc = wls_upload_lut(h);
    if (rc) { rtdm_wls_destroy(h); return rc; }
    *out = h;
    return RTDM_OK;
}

int rtdm_wls_set_params(rtdm_wls* h, const rtdm_wls_params* params)
{
    if (!h || !params) return RTDM_ERR_NULL;
    const int rc = wls_validate(*params);
    if (rc) return rc;
    const bool lut = params->sigma_color != h->p.sigma_color;
    h->p = *params;
    if (!lut) return RTDM_OK;
    HIPC(hipSetDevice(h->device));
    HIPC(hipDeviceSynchronize());  // a filter call in flight on any stream may still read the old table
    return wls_upload_lut(h);
}

int rtdm_wls_get_params(const rtdm_wls* h, rtdm_wls_params* out)
{
    if (!h || !out) return RTDM_ERR_NULL;
    *out = h->p;
    return RTDM_OK;
}

// one chunk of <= maxB frames through the launch sequence of k_wls.hip
static int wls_chunk(rtdm_wls* h, int n, WlsDisp dl, WlsDisp dr, WlsGuide G, WlsOut o, int W, int H, hipStream_t s)
{
    const rtdm_wls_params& p = h->p;
    WlsLaunch L{};
    L.dl = dl; L.dr = dr; L.guide = G; L.out = o;
    L.g = wls_geom(p, W, H);
    L.W = W; L.H = H; L.r = p.depth_discontinuity_radius; L.T = p.lrc_thresh;
    L.invL = (p.min_disparity - 1) * 16;
    L.invR = -(p.min_disparity + p.num_disparities) * 16;       // (minDR - 1) * 16, minDR = -(minD + numD) + 1
    L.use_conf = p.use_confidence; L.num_iter = p.num_iter;
    // W6: lambda_0 = 1.5 lambda 4^(T-1) / (4^T - 1), then * attenuation per iteration (double, rounded once per pass)
    double lam = 1.5 * p.lambda * std::pow(4.0, p.num_iter - 1) / (std::pow(4.0, p.num_iter) - 1.0);
    for (int t = 0; t < p.num_iter; ++t) { L.lambda[t] = (float)lam; lam *= p.attenuation; }
    L.lut = h->dLut;
    L.pitch = (size_t)h->maxW; L.frame = (size_t)h->maxW * h->maxH;
    L.F = h->dF; L.wh = h->dWh; L.wv = h->dWv; L.conf = h->dConf; L.mmL = h->dMML; L.mmR = h->dMMR;
    launch_wls(L, n, s);
    HIPC(hipGetLastError());
    return RTDM_OK;
}

static int wls_check(const rtdm_wls* h, int channels, int W, int H)
{
    if (channels != 1 && channels != 3) return RTDM_ERR_BAD_PARAM;
    if (W <= 0 || H <= 0 || W > h->maxW || H > h->maxH) return RTDM_ERR_BAD_SIZE;
    return RTDM_OK;
}

int rtdm_wls_filter_device(rtdm_wls* h, int n, const int16_t* d_left, size_t left_pitch, size_t left_frame_stride,
                           const int16_t* d_right, size_t right_pitch, size_t right_frame_stride, const uint8_t* d_guide,
                           size_t guide_pitch, size_t guide_frame_stride, int channels, int width, int height,
                           int16_t* d_out, size_t out_pitch, size_t out_frame_stride, float* d_conf, size_t conf_pitch,
                           size_t conf_frame_stride, float* d_filtered, size_t filtered_pitch, size_t filtered_frame_stride,
                           void* hip_stream)
{
    if (!h || !d_left || !d_guide || !d_out || (h->p.use_confidence && !d_right)) return RTDM_ERR_NULL;
    int rc = wls_check(h, channels, width, height);
    if (rc) return rc;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    const size_t W = (size_t)width;
    const bool cr = h->p.use_confidence;
    if (left_pitch < 2 * W || ((left_pitch | left_frame_stride) & 1) || guide_pitch < W * channels ||
        out_pitch < 2 * W || ((out_pitch | out_frame_stride) & 1) ||
        (cr && (right_pitch < 2 * W || ((right_pitch | right_frame_stride) & 1))) ||
        (d_conf && (conf_pitch < 4 * W || ((conf_pitch | conf_frame_stride) & 3))) ||
        (d_filtered && (filtered_pitch < 4 * W || ((filtered_pitch | filtered_frame_stride) & 3))))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    for (int i0 = 0; i0 < n; i0 += h->maxB) {
        const int m = std::min(h->maxB, n - i0);
        WlsDisp dl{d_left + (size_t)i0 * (left_frame_stride / 2), left_pitch / 2, left_frame_stride / 2};
        WlsDisp dr{cr ? d_right + (size_t)i0 * (right_frame_stride / 2) : d_left, cr ? right_pitch / 2 : 0, cr ? right_frame_stride / 2 : 0};
        WlsGuide G{d_guide + (size_t)i0 * guide_frame_stride, guide_pitch, guide_frame_stride, channels};
        WlsOut o{d_out + (size_t)i0 * (out_frame_stride / 2), out_pitch / 2, out_frame_stride / 2,
                 d_filtered ? d_filtered + (size_t)i0 * (filtered_frame_stride / 4) : nullptr, filtered_pitch / 4, filtered_frame_stride / 4,
                 d_conf ? d_conf + (size_t)i0 * (conf_frame_stride / 4) : nullptr, conf_pitch / 4, conf_frame_stride / 4};
        rc = wls_chunk(h, m, dl, dr, G, o, width, height, s);
        if (rc) return rc;
    }
    return RTDM_OK;
}

// the outputs of one staged frame back to the caller's planes
static int wls_download(rtdm_wls* h, int W, int H, int16_t* out, size_t out_pitch, float* conf, size_t conf_pitch,
                        float* filtered, size_t filtered_pitch, hipStream_t s)
{
    HIPC(hipMemcpy2DAsync(out, out_pitch, h->dOut, (size_t)W * 2, (size_t)W * 2, H, hipMemcpyDeviceToHost, s));
    if (conf) HIPC(hipMemcpy2DAsync(conf, conf_pitch, h->dConfOut, (size_t)W * 4, (size_t)W * 4, H, hipMemcpyDeviceToHost, s));
    if (filtered) HIPC(hipMemcpy2DAsync(filtered, filtered_pitch, h->dFilt, (size_t)W * 4, (size_t)W * 4, H, hipMemcpyDeviceToHost, s));
    return RTDM_OK;
}

int rtdm_wls_filter(rtdm_wls* h, const int16_t* disp_left, size_t left_pitch, const int16_t* disp_right, size_t right_pitch,
                    const uint8_t* guide, size_t guide_pitch, int channels, int width, int height, int16_t* out,
                    size_t out_pitch, float* conf, size_t conf_pitch, float* filtered, size_t filtered_pitch)
{
    if (!h || !disp_left || !guide || !out || (h->p.use_confidence && !disp_right)) return RTDM_ERR_NULL;
    int rc = wls_check(h, channels, width, height);
    if (rc) return rc;
    const size_t W = (size_t)width;
    const bool cr = h->p.use_confidence;
    if (left_pitch < 2 * W || (cr && right_pitch < 2 * W) || guide_pitch < W * channels || out_pitch < 2 * W ||
        (conf && conf_pitch < 4 * W) || (filtered && filtered_pitch < 4 * W))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(h->dInL, W * 2, disp_left, left_pitch, W * 2, height, hipMemcpyHostToDevice, s));
    if (cr) HIPC(hipMemcpy2DAsync(h->dInR, W * 2, disp_right, right_pitch, W * 2, height, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpy2DAsync(h->dGuide, W * channels, guide, guide_pitch, W * channels, height, hipMemcpyHostToDevice, s));
    const size_t fr = W * height;
    WlsDisp dl{h->dInL, W, fr}, dr{h->dInR, W, fr};
    WlsGuide G{h->dGuide, W * channels, fr * channels, channels};
    WlsOut o{h->dOut, W, fr, filtered ? h->dFilt : nullptr, W, fr, conf ? h->dConfOut : nullptr, W, fr};
    rc = wls_chunk(h, 1, dl, dr, G, o, width, height, s);
    if (rc) return rc;
    rc = wls_download(h, width, height, out, out_pitch, conf, conf_pitch, filtered, filtered_pitch, s);
    if (rc) return rc;
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    return RTDM_OK;
}

int rtdm_bm_compute_filtered(rtdm_bm* left_bm, rtdm_bm* right_bm, rtdm_wls* wls, const uint8_t* left, size_t left_pitch,
                             const uint8_t* right, size_t right_pitch, int width, int height, int16_t* out, size_t out_pitch,
                             int16_t* raw_left, size_t raw_left_pitch)
{
    if (!left_bm || !wls || !left || !right || !out || (wls->p.use_confidence && !right_bm)) return RTDM_ERR_NULL;
    const bool cr = wls->p.use_confidence;
    if (left_bm->device != wls->device || (cr && right_bm->device != wls->device)) return RTDM_ERR_BAD_PARAM;
    int rc = wls_check(wls, 1, width, height);
    if (rc) return rc;
    const size_t W = (size_t)width, fr = W * height;
    if (left_pitch < W || right_pitch < W || out_pitch < 2 * W || (raw_left && raw_left_pitch < 2 * W)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(wls->device));
    hipStream_t s = wls->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(wls->dGuide, W, left, left_pitch, W, height, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpy2DAsync(wls->dImgR, W, right, right_pitch, W, height, hipMemcpyHostToDevice, s));
    rc = rtdm_bm_compute_device(left_bm, 1, wls->dGuide, wls->dImgR, W, fr, width, height, wls->dInL, W * 2, fr * 2, s);
    if (rc) return rc;
    if (cr) {                      // createRightMatcher's handle, called as compute(right, left)
        rc = rtdm_bm_compute_device(right_bm, 1, wls->dImgR, wls->dGuide, W, fr, width, height, wls->dInR, W * 2, fr * 2, s);
        if (rc) return rc;
    }
    HIPC(hipSetDevice(wls->device));
    WlsDisp dl{wls->dInL, W, fr}, dr{wls->dInR, W, fr};
    WlsGuide G{wls->dGuide, W, fr, 1};
    WlsOut o{wls->dOut, W, fr, nullptr, W, fr, nullptr, W, fr};
    rc = wls_chunk(wls, 1, dl, dr, G, o, width, height, s);
    if (rc) return rc;
    rc = wls_download(wls, width, height, out, out_pitch, nullptr, 0, nullptr, 0, s);
    if (rc) return rc;
    if (raw_left) HIPC(hipMemcpy2DAsync(raw_left, raw_left_pitch, wls->dInL, W * 2, W * 2, height, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    return RTDM_OK;
}

// ---- reprojectImageTo3D and the point cloud (estimator.cpp:75-77, :235; rules X1-X8) ----------------
static_assert(sizeof(rtdm_point) == 16 && sizeof(XyzRec) == 16, "rtdm_point is a 16-byte record");

struct rtdm_xyz {
    rtdm_xyz_params p;
    int maxW, maxH, maxB, device;
    hipStream_t stream;
    int *dMin, *dTile, *dCounts;   // [maxB] frame minima, [maxB][tiles of maxW x maxH] tile counts, [maxB] counts of a host call
    // single-frame staging of the host entry points
    int16_t* dDisp;
    uint8_t *dGuide, *dMask, *dImgL, *dImgR;
    float *dXYZ, *dZ;
    XyzRec* dPts;
};

static int xyz_validate(const rtdm_xyz_params& p)
{
    if (p.disparity_mode != RTDM_XYZ_FIXED16 && p.disparity_mode != RTDM_XYZ_ROUNDED) return RTDM_ERR_BAD_PARAM;
    if (p.handle_missing_values != 0 && p.handle_missing_values != 1) return RTDM_ERR_BAD_PARAM;
    for (int i = 0; i < 16; ++i) if (!std::isfinite(p.Q[i])) return RTDM_ERR_BAD_PARAM;
    if (!(p.max_z > 0.0)) return RTDM_ERR_BAD_PARAM;
    return RTDM_OK;
}

static XyzParams xyz_kernel_params(const rtdm_xyz_params& p)
{
    XyzParams P;
    std::copy(p.Q, p.Q + 16, P.q);
    P.max_z = p.max_z; P.mode = p.disparity_mode; P.hmv = p.handle_missing_values;
    // (min_disparity - 1) * 16 as the int the 16-bit map is compared with; outside int16 no pixel carries it
    const long inv = ((long)p.min_disparity - 1) * 16;
    P.invalid16 = inv >= INT16_MIN && inv <= INT16_MAX ? (int)inv : INT32_MIN;
    return P;
}

void rtdm_xyz_default_params(rtdm_xyz_params* p, const double* Q, int min_disparity)
{
    if (!p) return;
    for (int i = 0; i < 16; ++i) p->Q[i] = Q ? Q[i] : (i % 5 == 0 ? 1.0 : 0.0);
    p->disparity_mode = RTDM_XYZ_ROUNDED; p->handle_missing_values = 1; p->min_disparity = min_disparity; p->max_z = 10000.0;
}

void rtdm_xyz_destroy(rtdm_xyz* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    void* bufs[] = {h->dMin, h->dTile, h->dCounts, h->dDisp, h->dGuide, h->dMask, h->dImgL, h->dImgR, h->dXYZ, h->dZ, h->dPts};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int rtdm_xyz_create(const rtdm_xyz_params* params, int max_width, int max_height, int max_batch, int device, rtdm_xyz** out)
{
    if (!params || !out) return RTDM_ERR_NULL;
    *out = nullptr;
    int rc = xyz_validate(*params);
    if (rc) return rc;
    if (max_width <= 0 || max_height <= 0 || max_batch <= 0 || max_batch > 65535) return RTDM_ERR_BAD_SIZE;
    if ((long)max_width * max_height > (long)INT32_MAX) return RTDM_ERR_UNSUPPORTED;   // counts and record numbers are ints
    rc = use_device(device);
    if (rc) return rc;
    rtdm_xyz* h = new (std::nothrow) rtdm_xyz();
    if (!h) return RTDM_ERR_NOMEM;
    h->p = *params; h->maxW = max_width; h->maxH = max_height; h->maxB = max_batch; h->device = device;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dMin, (size_t)max_batch * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&h->dTile, (size_t)max_batch * xyz_tiles(max_width, max_height) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&h->dCounts, (size_t)max_batch * sizeof(int));
    // single-frame staging of the host entry points: 40 bytes per pixel of max_width x max_height
    void** stage[] = {(void**)&h->dDisp, (void**)&h->dGuide, (void**)&h->dMask, (void**)&h->dImgL, (void**)&h->dImgR,
                      (void**)&h->dXYZ, (void**)&h->dZ, (void**)&h->dPts};
    const size_t elem[] = {2, 3, 1, 1, 1, 12, 4, sizeof(XyzRec)};
    for (int i = 0; i < 8 && e == hipSuccess; ++i) e = hipMalloc(stage[i], (size_t)max_width * max_height * elem[i]);
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_xyz_create: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        rtdm_xyz_destroy(h);
        return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
    }
    *out = h;
    return RTDM_OK;
}

int rtdm_xyz_set_params(rtdm_xyz* h, const rtdm_xyz_params* params)
{
    if (!h || !params) return RTDM_ERR_NULL;
    const int rc = xyz_validate(*params);
    if (rc) return rc;
    h->p = *params;                // kernels take the parameters by value: calls already enqueued keep theirs
    return RTDM_OK;
}

int rtdm_xyz_get_params(const rtdm_xyz* h, rtdm_xyz_params* out)
{
    if (!h || !out) return RTDM_ERR_NULL;
    *out = h->p;
    return RTDM_OK;
}

static int xyz_check(const rtdm_xyz* h, int W, int H)
{
    if (W <= 0 || H <= 0 || W > h->maxW || H > h->maxH) return RTDM_ERR_BAD_SIZE;
    return RTDM_OK;
}

int rtdm_xyz_map_device(rtdm_xyz* h, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride, int width,
                        int height, float* d_xyz, size_t xyz_pitch, size_t xyz_frame_stride, float* d_z, size_t z_pitch,
                        size_t z_frame_stride, void* hip_stream)
{
    if (!h || !d_disp) return RTDM_ERR_NULL;
    int rc = xyz_check(h, width, height);
    if (rc) return rc;
    if (n <= 0 || (!d_xyz && !d_z)) return RTDM_ERR_BAD_SIZE;
    const size_t W = (size_t)width;
    if (disp_pitch < 2 * W || ((disp_pitch | disp_frame_stride) & 1) ||
        (d_xyz && (xyz_pitch < 12 * W || ((xyz_pitch | xyz_frame_stride) & 3))) ||
        (d_z && (z_pitch < 4 * W || ((z_pitch | z_frame_stride) & 3))))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    const XyzParams P = xyz_kernel_params(h->p);
    for (int i0 = 0; i0 < n; i0 += h->maxB) {
        const int m = std::min(h->maxB, n - i0);
        XyzDisp D{d_disp + (size_t)i0 * (disp_frame_stride / 2), disp_pitch / 2, disp_frame_stride / 2};
        XyzMap O{d_xyz ? d_xyz + (size_t)i0 * (xyz_frame_stride / 4) : nullptr, xyz_pitch / 4, xyz_frame_stride / 4,
                 d_z ? d_z + (size_t)i0 * (z_frame_stride / 4) : nullptr, z_pitch / 4, z_frame_stride / 4};
        launch_xyz_map(D, m, width, height, P, h->dMin, O, s);
        HIPC(hipGetLastError());
    }
    return RTDM_OK;
}

int rtdm_xyz_map(rtdm_xyz* h, const int16_t* disp, size_t disp_pitch, int width, int height, float* xyz, size_t xyz_pitch,
                 float* z, size_t z_pitch)
{
    if (!h || !disp) return RTDM_ERR_NULL;
    int rc = xyz_check(h, width, height);
    if (rc) return rc;
    const size_t W = (size_t)width, fr = W * height;
    if ((!xyz && !z) || disp_pitch < 2 * W || (xyz && xyz_pitch < 12 * W) || (z && z_pitch < 4 * W)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(h->dDisp, W * 2, disp, disp_pitch, W * 2, height, hipMemcpyHostToDevice, s));
    XyzDisp D{h->dDisp, W, fr};
    XyzMap O{xyz ? h->dXYZ : nullptr, 3 * W, 3 * fr, z ? h->dZ : nullptr, W, fr};
    launch_xyz_map(D, 1, width, height, xyz_kernel_params(h->p), h->dMin, O, s);
    HIPC(hipGetLastError());
    if (xyz) HIPC(hipMemcpy2DAsync(xyz, xyz_pitch, h->dXYZ, W * 12, W * 12, height, hipMemcpyDeviceToHost, s));
    if (z) HIPC(hipMemcpy2DAsync(z, z_pitch, h->dZ, W * 4, W * 4, height, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    return RTDM_OK;
}

// what both cloud entries check of the optional planes, before any device use
static int xyz_cloud_check(const rtdm_xyz* h, const void* disp, const void* guide, int channels, int width, int height,
                           const void* points, int capacity, const void* count)
{
    if (!h || !disp || !count || (channels != 0 && !guide) || (capacity > 0 && !points)) return RTDM_ERR_NULL;
    if ((channels != 0 && channels != 1 && channels != 3) || capacity < 0) return RTDM_ERR_BAD_PARAM;
    return xyz_check(h, width, height);
}

int rtdm_xyz_cloud_device(rtdm_xyz* h, int n, const int16_t* d_disp, size_t disp_pitch, size_t disp_frame_stride,
                          const uint8_t* d_guide, size_t guide_pitch, size_t guide_frame_stride, int channels,
                          const uint8_t* d_mask, size_t mask_pitch, size_t mask_frame_stride, int width, int height,
                          rtdm_point* d_points, size_t points_frame_stride, int capacity, int* d_counts, void* hip_stream)
{
    int rc = xyz_cloud_check(h, d_disp, d_guide, channels, width, height, d_points, capacity, d_counts);
    if (rc) return rc;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    const size_t W = (size_t)width;
    if (disp_pitch < 2 * W || ((disp_pitch | disp_frame_stride) & 1) || (channels && guide_pitch < W * channels) ||
        (d_mask && mask_pitch < W) ||
        (capacity > 0 && (((uintptr_t)d_points | points_frame_stride) & 3)) ||
        (capacity > 0 && n > 1 && points_frame_stride < (size_t)capacity * sizeof(rtdm_point)))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    const XyzParams P = xyz_kernel_params(h->p);
    for (int i0 = 0; i0 < n; i0 += h->maxB) {
        const int m = std::min(h->maxB, n - i0);
        XyzCloudIn I{};
        I.disp = XyzDisp{d_disp + (size_t)i0 * (disp_frame_stride / 2), disp_pitch / 2, disp_frame_stride / 2};
        I.cn = channels;
        if (channels) { I.guide = d_guide + (size_t)i0 * guide_frame_stride; I.gpitch = guide_pitch; I.gframe = guide_frame_stride; }
        if (d_mask) { I.mask = d_mask + (size_t)i0 * mask_frame_stride; I.mpitch = mask_pitch; I.mframe = mask_frame_stride; }
        XyzRec* pts = capacity > 0 ? (XyzRec*)((unsigned char*)d_points + (size_t)i0 * points_frame_stride) : nullptr;
        launch_xyz_cloud(I, m, width, height, P, h->dMin, h->dTile, pts, points_frame_stride, capacity, d_counts + i0, s);
        HIPC(hipGetLastError());
    }
    return RTDM_OK;
}

// the staged disparity map (and guide / mask) of one frame -> count and the first min(count, capacity) records, synchronous
static int xyz_cloud_staged(rtdm_xyz* h, int channels, bool mask, int width, int height, rtdm_point* points, int capacity,
                            int* count, hipStream_t s)
{
    const size_t W = (size_t)width, fr = W * height;
    const int cap = (int)std::min((size_t)capacity, fr);        // a frame has at most W * H records
    XyzCloudIn I{};
    I.disp = XyzDisp{h->dDisp, W, fr};
    I.cn = channels;
    if (channels) { I.guide = h->dGuide; I.gpitch = W * channels; I.gframe = fr * channels; }
    if (mask) { I.mask = h->dMask; I.mpitch = W; I.mframe = fr; }
    launch_xyz_cloud(I, 1, width, height, xyz_kernel_params(h->p), h->dMin, h->dTile, h->dPts, 0, cap, h->dCounts, s);
    HIPC(hipGetLastError());
    int c = 0;
    HIPC(hipMemcpyAsync(&c, h->dCounts, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    const int wr = std::min(c, cap);
    if (wr > 0) {
        HIPC(hipMemcpyAsync(points, h->dPts, (size_t)wr * sizeof(rtdm_point), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
    }
    *count = c;
    return RTDM_OK;
}

int rtdm_xyz_cloud(rtdm_xyz* h, const int16_t* disp, size_t disp_pitch, const uint8_t* guide, size_t guide_pitch, int channels,
                   const uint8_t* mask, size_t mask_pitch, int width, int height, rtdm_point* points, int capacity, int* count)
{
    int rc = xyz_cloud_check(h, disp, guide, channels, width, height, points, capacity, count);
    if (rc) return rc;
    const size_t W = (size_t)width;
    if (disp_pitch < 2 * W || (channels && guide_pitch < W * channels) || (mask && mask_pitch < W)) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(h->dDisp, W * 2, disp, disp_pitch, W * 2, height, hipMemcpyHostToDevice, s));
    if (channels) HIPC(hipMemcpy2DAsync(h->dGuide, W * channels, guide, guide_pitch, W * channels, height, hipMemcpyHostToDevice, s));
    if (mask) HIPC(hipMemcpy2DAsync(h->dMask, W, mask, mask_pitch, W, height, hipMemcpyHostToDevice, s));
    rc = xyz_cloud_staged(h, channels, mask != nullptr, width, height, points, capacity, count, s);
    if (rc) return rc;
    drain.armed = false;
    return RTDM_OK;
}

int rtdm_bm_compute_cloud(rtdm_bm* bm, rtdm_xyz* h, const uint8_t* left, size_t left_pitch, const uint8_t* right,
                          size_t right_pitch, int width, int height, const uint8_t* guide, size_t guide_pitch, int channels,
                          const uint8_t* mask, size_t mask_pitch, rtdm_point* points, int capacity, int* count, int16_t* disp,
                          size_t disp_pitch)
{
    if (!bm || !left || !right) return RTDM_ERR_NULL;
    int rc = xyz_cloud_check(h, left, guide, channels, width, height, points, capacity, count);
    if (rc) return rc;
    if (bm->device != h->device || bm->p.minDisparity != h->p.min_disparity) return RTDM_ERR_BAD_PARAM;
    rc = check_frame(bm, width, height);
    if (rc) return rc;
    const size_t W = (size_t)width, fr = W * height;
    if (left_pitch < W || right_pitch < W || (channels && guide_pitch < W * channels) || (mask && mask_pitch < W) ||
        (disp && disp_pitch < 2 * W))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(h->dImgL, W, left, left_pitch, W, height, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpy2DAsync(h->dImgR, W, right, right_pitch, W, height, hipMemcpyHostToDevice, s));
    if (channels) HIPC(hipMemcpy2DAsync(h->dGuide, W * channels, guide, guide_pitch, W * channels, height, hipMemcpyHostToDevice, s));
    if (mask) HIPC(hipMemcpy2DAsync(h->dMask, W, mask, mask_pitch, W, height, hipMemcpyHostToDevice, s));
    rc = rtdm_bm_compute_device(bm, 1, h->dImgL, h->dImgR, W, fr, width, height, h->dDisp, W * 2, fr * 2, s);
    if (rc) return rc;
    HIPC(hipSetDevice(h->device));
    rc = xyz_cloud_staged(h, channels, mask != nullptr, width, height, points, capacity, count, s);
    if (rc) return rc;
    if (disp) {
        HIPC(hipMemcpy2DAsync(disp, disp_pitch, h->dDisp, W * 2, W * 2, height, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
    }
    drain.armed = false;
    return RTDM_OK;
}

// ---- DecoderDevice: baseline MJPEG frames (estimator.cpp:24-27; rules J1-J5) ------------------------
static_assert(sizeof(rtdm_mjpeg_info) == sizeof(MjpegInfo), "rtdm_mjpeg_info and MjpegInfo are one layout");
static_assert(MJ_BAD_STREAM == RTDM_ERR_BAD_STREAM && MJ_UNSUPPORTED == RTDM_ERR_UNSUPPORTED && MJ_BAD_SIZE == RTDM_ERR_BAD_SIZE &&
              MJ_NULL == RTDM_ERR_NULL, "rtdm_mjpeg.h restates the status values");

struct rtdm_mjpeg {
    int maxW, maxH, maxB, device;
    size_t maxBytes, slot;         // longest stream served; its slot in the staging area (maxBytes rounded up to 16)
    size_t maxSegs, maxBlocks;     // per frame: entropy segments (one MCU each at worst), 8 x 8 blocks of three full planes
    hipStream_t stream;
    hipEvent_t evStaged;           // the staging area is on its way to the device up to here ...
    bool staged;                   // ... and must not be overwritten before
    uint8_t* hStreams; MjpegDesc* hDesc; MjpegSeg* hSegs; int* hStatus;     // page-locked
    uint8_t* dStreams; MjpegDesc* dDesc; MjpegSeg* dSegs;
    int16_t* dCoef;                // [maxB][blocks][64] dequantised coefficients
    uint8_t* dPlanes;              // [maxB] planar Y, Cb, Cr at their own (padded) resolutions
    uint8_t* dRgb;                 // one frame for the host entry point
    int* dStatus;                  // [maxB + 1]
};

int rtdm_mjpeg_probe(const uint8_t* stream, size_t len, rtdm_mjpeg_info* out)
{
    if (!stream || !out) return RTDM_ERR_NULL;
    MjpegDesc d;
    return mjpeg_parse(stream, len, &d, (MjpegInfo*)out, nullptr, 0);
}

void rtdm_mjpeg_destroy(rtdm_mjpeg* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->staged) (void)hipEventSynchronize(h->evStaged);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    void* dev[] = {h->dStreams, h->dDesc, h->dSegs, h->dCoef, h->dPlanes, h->dRgb, h->dStatus};
    for (void* b : dev) if (b) (void)hipFree(b);
    void* host[] = {h->hStreams, h->hDesc, h->hSegs, h->hStatus};
    for (void* b : host) if (b) (void)hipHostFree(b);
    if (h->evStaged) (void)hipEventDestroy(h->evStaged);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int rtdm_mjpeg_create(int max_width, int max_height, int max_batch, size_t max_stream_bytes, int device, rtdm_mjpeg** out)
{
    if (!out) return RTDM_ERR_NULL;
    *out = nullptr;
    if (max_width <= 0 || max_height <= 0 || max_width > 65535 || max_height > 65535 || max_batch <= 0 || max_batch > 65535)
        return RTDM_ERR_BAD_SIZE;
    if (max_stream_bytes < 4 || max_stream_bytes > (size_t)1 << 30) return RTDM_ERR_BAD_SIZE;
    const size_t slot = (max_stream_bytes + 15) & ~(size_t)15;
    if (slot * (size_t)max_batch > 0xFFFFFFFFu) return RTDM_ERR_BAD_SIZE;     // stream offsets are 32 bits wide
    int rc = use_device(device);
    if (rc) return rc;
    rtdm_mjpeg* h = new (std::nothrow) rtdm_mjpeg();
    if (!h) return RTDM_ERR_NOMEM;
    h->maxW = max_width; h->maxH = max_height; h->maxB = max_batch; h->device = device;
    h->maxBytes = max_stream_bytes; h->slot = slot;
    h->maxSegs = (size_t)((max_width + 7) / 8) * ((max_height + 7) / 8);
    h->maxBlocks = 3 * (size_t)((max_width + 15) / 16 * 2) * ((max_height + 15) / 16 * 2);
    const size_t B = (size_t)max_batch;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->evStaged, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->hStreams, slot * B, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->hDesc, sizeof(MjpegDesc) * B, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->hSegs, sizeof(MjpegSeg) * h->maxSegs * B, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->hStatus, sizeof(int) * 2, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dStreams, slot * B);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dDesc, sizeof(MjpegDesc) * B);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dSegs, sizeof(MjpegSeg) * h->maxSegs * B);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dCoef, h->maxBlocks * 128 * B);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dPlanes, h->maxBlocks * 64 * B);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dRgb, (size_t)max_width * max_height * 3);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dStatus, sizeof(int) * (B + 1));
    if (e != hipSuccess) {
        g_hip_err = std::string("rtdm_mjpeg_create: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        rtdm_mjpeg_destroy(h);
        return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
    }
    *out = h;
    return RTDM_OK;
}

// what a frame of a call must be besides parseable: the call's size, within the handle, the sampling of the call's first frame
static int mjpeg_fits(const rtdm_mjpeg* h, const MjpegDesc& d, int W, int H, const MjpegDesc* first)
{
    if (d.W != W || d.H != H || W > h->maxW || H > h->maxH || d.stream_len > h->maxBytes) return RTDM_ERR_BAD_SIZE;
    if (first && (first->ncomp != d.ncomp || first->hs != d.hs || first->vs != d.vs)) return RTDM_ERR_BAD_SIZE;
    return RTDM_OK;
}

// m <= maxB frames: parse and stage on the host, then copies, the zeroing of coefficients and status words, and the three
// kernels on s.  *shape: the first frame of the CALL (ncomp 0 before it); d_status: m ints on the device.
static int mjpeg_chunk(rtdm_mjpeg* h, int m, const uint8_t* const* streams, const size_t* lens, int W, int H, uint8_t* d_rgb,
                       size_t pitch, size_t frame_stride, int* d_status, hipStream_t s, MjpegDesc* shape)
{
    if (h->staged) { HIPC(hipEventSynchronize(h->evStaged)); h->staged = false; }
    size_t nsegs = 0, bytes = 0;
    unsigned max_nseg = 1;
    for (int k = 0; k < m; ++k) {
        if (!streams[k]) return RTDM_ERR_NULL;
        MjpegDesc& d = h->hDesc[k];
        MjpegInfo info;
        int st = mjpeg_parse(streams[k], lens[k], &d, &info, h->hSegs + nsegs, h->maxSegs);
        if (st) return st;
        st = mjpeg_fits(h, d, W, H, shape->ncomp ? shape : nullptr);
        if (st) return st;
        if (!shape->ncomp) *shape = d;
        d.stream_off = (uint32_t)bytes; d.seg_first = (uint32_t)nsegs;
        memcpy(h->hStreams + bytes, streams[k], d.stream_len);
        bytes += ((size_t)d.stream_len + 15) & ~(size_t)15;
        nsegs += d.nseg;
        max_nseg = std::max(max_nseg, (unsigned)d.nseg);
    }
    const size_t nb = mjpeg_frame_blocks(*shape);
    HIPC(hipMemcpyAsync(h->dStreams, h->hStreams, bytes, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(h->dDesc, h->hDesc, sizeof(MjpegDesc) * m, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(h->dSegs, h->hSegs, sizeof(MjpegSeg) * nsegs, hipMemcpyHostToDevice, s));
    HIPC(hipEventRecord(h->evStaged, s));
    h->staged = true;
    HIPC(hipMemsetAsync(h->dCoef, 0, nb * 128 * m, s));
    HIPC(hipMemsetAsync(d_status, 0, sizeof(int) * m, s));
    launch_mjpeg(h->dStreams, h->dDesc, h->dSegs, m, *shape, max_nseg, h->dCoef, h->dPlanes, d_rgb, pitch, frame_stride, d_status, s);
    HIPC(hipGetLastError());
    return RTDM_OK;
}

int rtdm_mjpeg_decode_batch_device(rtdm_mjpeg* h, int n, const uint8_t* const* streams, const size_t* lens, int width, int height,
                                   uint8_t* d_rgb, size_t pitch, size_t frame_stride, int* d_status, void* hip_stream)
{
    if (!h || !streams || !lens || !d_rgb) return RTDM_ERR_NULL;
    if (n <= 0 || width <= 0 || height <= 0 || width > h->maxW || height > h->maxH) return RTDM_ERR_BAD_SIZE;
    if (pitch < (size_t)width * 3 || (n > 1 && frame_stride < pitch * (size_t)height)) return RTDM_ERR_BAD_SIZE;
    MjpegDesc shape;
    shape.ncomp = 0;
    if (n > h->maxB) {
        // a call in chunks: every frame is checked before the first chunk reaches the device
        MjpegDesc d, first;
        MjpegInfo info;
        first.ncomp = 0;
        for (int k = 0; k < n; ++k) {
            if (!streams[k]) return RTDM_ERR_NULL;
            int st = mjpeg_parse(streams[k], lens[k], &d, &info, nullptr, 0);
            if (st) return st;
            if (d.nseg > h->maxSegs) return RTDM_ERR_BAD_SIZE;
            st = mjpeg_fits(h, d, width, height, first.ncomp ? &first : nullptr);
            if (st) return st;
            if (!first.ncomp) first = d;
        }
    }
    HIPC(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    for (int i0 = 0; i0 < n; i0 += h->maxB) {
        const int m = std::min(h->maxB, n - i0);
        const int st = mjpeg_chunk(h, m, streams + i0, lens + i0, width, height, d_rgb + (size_t)i0 * frame_stride, pitch,
                                   frame_stride, d_status ? d_status + i0 : h->dStatus, s, &shape);
        if (st) return st;
    }
    return RTDM_OK;
}

int rtdm_mjpeg_decode(rtdm_mjpeg* h, const uint8_t* stream, size_t len, int width, int height, uint8_t* rgb, size_t pitch)
{
    if (!h || !stream || !rgb) return RTDM_ERR_NULL;
    if (width <= 0 || height <= 0 || width > h->maxW || height > h->maxH || pitch < (size_t)width * 3) return RTDM_ERR_BAD_SIZE;
    MjpegDesc shape;
    shape.ncomp = 0;
    // refusals come first: the device is not touched for a frame that is not served
    {
        MjpegDesc d;
        MjpegInfo info;
        int st = mjpeg_parse(stream, len, &d, &info, nullptr, 0);
        if (st) return st;
        st = mjpeg_fits(h, d, width, height, nullptr);
        if (st) return st;
    }
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    const size_t row = (size_t)width * 3;
    int st = mjpeg_chunk(h, 1, &stream, &len, width, height, h->dRgb, row, row * height, h->dStatus, s, &shape);
    if (st) return st;
    HIPC(hipMemcpy2DAsync(rgb, pitch, h->dRgb, row, row, height, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h->hStatus, h->dStatus, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    return h->hStatus[0] ? RTDM_ERR_BAD_STREAM : RTDM_OK;
}

int rtdm_bm_compute_mjpeg(rtdm_bm* bm, rtdm_rectify* rc, rtdm_mjpeg* dec, const uint8_t* left, size_t left_len,
                          const uint8_t* right, size_t right_len, int width, int height, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !rc || !dec || !left || !right || !disp) return RTDM_ERR_NULL;
    if (bm->device != rc->device || bm->device != dec->device) return RTDM_ERR_BAD_PARAM;
    if (width != rc->W || height != rc->H || width > dec->maxW || height > dec->maxH) return RTDM_ERR_BAD_SIZE;
    int st = check_frame(bm, rc->rw, rc->rh);
    if (st) return st;
    if (disp_pitch < (size_t)rc->rw * 2) return RTDM_ERR_BAD_SIZE;
    const uint8_t* src[2] = {left, right};
    const size_t len[2] = {left_len, right_len};
    for (int k = 0; k < 2; ++k) {                    // refusals before any device use
        MjpegDesc d;
        MjpegInfo info;
        st = mjpeg_parse(src[k], len[k], &d, &info, nullptr, 0);
        if (st) return st;
        st = mjpeg_fits(dec, d, width, height, nullptr);
        if (st) return st;
    }
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    DrainOnError drain{s};
    const size_t row = (size_t)width * 3;
    for (int k = 0; k < 2; ++k) {                    // the two cameras may differ in sampling: one chunk each
        MjpegDesc shape;
        shape.ncomp = 0;
        st = mjpeg_chunk(dec, 1, src + k, len + k, width, height, rc->dRgb[k], row, row * height, dec->dStatus + k, s, &shape);
        if (st) return st;
    }
    HIPC(hipMemcpyAsync(dec->hStatus, dec->dStatus, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    const size_t Ws = (size_t)((rc->rw + 7) & ~7);                     // the handle's internal plane (see run_chunk)
    st = rgb_chunks(bm, rc, 1, rc->dRgb[0], rc->dRgb[1], Plane16W{bm->dOut, Ws, Ws * (size_t)rc->rh}, s);
    if (st) return st;
    int16_t* hD = (int16_t*)(bm->hStage + 2 * bm->ppitch * (size_t)bm->maxH);
    HIPC(hipMemcpyAsync(hD, bm->dOut, Ws * rc->rh * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    if (dec->hStatus[0] || dec->hStatus[1]) return RTDM_ERR_BAD_STREAM;
    for (int y = 0; y < rc->rh; ++y)
        memcpy((uint8_t*)disp + (size_t)y * disp_pitch, hD + (size_t)y * Ws, (size_t)rc->rw * sizeof(int16_t));
    return RTDM_OK;
}

}  // extern "C"
