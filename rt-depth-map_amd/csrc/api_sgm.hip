// api_sgm.hip -- rtdm_sgm, the SWSemiGlobalMatcher (cv::StereoSGBM) counterpart.
#include "rtdm_handles.h"
#include "rtdm_sgm_stripes.h"

using namespace rtdm;

struct rtdm_sgm {
    rtdm_sgm_params p;
    int maxW, maxH, maxB, device;
    hipStream_t stream;
    uint8_t *dInL, *dInR;
    uint8_t *dInL3, *dInR3;        // colour staging of rtdm_sgm_compute_cn (allocated by the first colour call)
    int16_t* dOut;
    SGMBuffers b;
    size_t pix_bytes;              // of b.pix
    uint16_t* dWarm;               // MODE_SGBM_3WAY's warm-up costs C' where b.pix cannot hold them (allocated by the first such call)
    int prefilter_cap;             // rtdm_sgm_set_prefilter_cap: R1's ftzero = max(preFilterCap, 15) | 1
    SgmCostKind cost;              // rtdm_sgm_set_cost: the pixel cost of the next call (R1, or census descriptors: N1-N5)
    int cost_limit;                // of the current call, > 0 where a block cost + P2 can pass 32767: a block cost above it would
                                   // wrap the library's 16-bit path costs (sgm_block_cost_limit, rtdm_sgm_cost_plan.h)
    int32_t* hOvf;                 // page-locked copy of b.ovf
    uint32_t sweep_epoch;          // launches of k_sgm_sweep (tags of its edge ring)
    SgmLimits lim;                 // cap: workgroups the device holds at once per sweep form, asked by the first call (caps_asked)
    bool caps_asked;
    bool sweep_reported;           // a give-up of the sweep has been returned to the caller
    const char* path_variant;      // the path-pass form of the last call (launch_sgm), "" before the first
    AllocList mem;                 // every device and page-locked buffer above, the colour buffers from their first call on
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

static_assert(SGM_COST_BT == RTDM_SGM_COST_BT && SGM_COST_CENSUS == RTDM_SGM_COST_CENSUS, "the kernels' names for rtdm.h's values");
static int sgm_ftzero(const rtdm_sgm* sg) { return std::max(sg->prefilter_cap, 15) | 1; }
static int sgm_cost_limit(const rtdm_sgm* sg, int cn) { return sgm_block_cost_limit(sg->cost, cn, sgm_ftzero(sg), sg->p.blockSize, sg->p.P2); }

// colour frames: the 24-byte bounds records (and, for the host entry point, the staging of the interleaved input)
static int sgm_colour_buffers(rtdm_sgm* sg, bool host)
{
    const size_t fr = (size_t)sg->maxW * sg->maxH, px = fr * sg->maxB;
    AllocList& m = sg->mem;
    if (!sg->b.cl) m.dev(&sg->b.cl, px * 24);
    if (!sg->b.cr) m.dev(&sg->b.cr, px * 24);
    if (host && !sg->dInL3) m.dev(&sg->dInL3, fr * 3);
    if (host && !sg->dInR3) m.dev(&sg->dInR3, fr * 3);
    if (m.err == hipSuccess) return RTDM_OK;
    return create_failed("StereoSGBM colour buffers", std::exchange(m.err, hipSuccess));     // (the next colour call asks again)
}

// MODE_SGBM_3WAY (T3): where the n frames' warm-up block costs C' go -- 3 stripes x min(blockSize / 2, H) rows of W1 x D u16 per
// frame.  b.pix is dead once C exists and holds them where about 6 (blockSize / 2) <= H; a frame too low for that gets a buffer
// of exactly the handle's largest such call, and a failed allocation is an error, never a silent other route.
static int sgm_warm_buffer(rtdm_sgm* sg, const SGMGeom& g, int n)
{
    const size_t need = (size_t)n * (SGM3_STRIPES - 1) * sgm3_warm_rows(sg->p.blockSize, g.H) * g.W1 * g.D * sizeof(uint16_t);
    if (need <= sg->pix_bytes) { sg->b.Cw = (uint16_t*)sg->b.pix; return RTDM_OK; }
    if (!sg->dWarm) {
        const long w1max = (long)sg->maxW + std::min(sg->p.minDisparity, 0) - std::max(sg->p.minDisparity + sg->p.numDisparities, 0);
        const size_t most = (size_t)sg->maxB * (SGM3_STRIPES - 1) * sgm3_warm_rows(sg->p.blockSize, sg->maxH) * (size_t)w1max *
                            sg->p.numDisparities * sizeof(uint16_t);
        AllocList& m = sg->mem;
        if (!m.dev(&sg->dWarm, most)) return create_failed("StereoSGBM MODE_SGBM_3WAY warm-up costs", std::exchange(m.err, hipSuccess));
    }
    sg->b.Cw = sg->dWarm;
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
    // cv::StereoSGBM's modes by their direction count: 5 MODE_SGBM, 8 MODE_HH, 4 MODE_HH4 (R4'); 3 is MODE_SGBM_3WAY, which this
    // door keeps refusing: it is served through rtdm_sgm_set_mode on a live handle (DESIGN.md section 4.21 and "Known limits")
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
    sg->cost = SgmCostKind{SGM_COST_BT, 9, 7};
    const size_t px = (size_t)max_width * max_height * max_batch;
    // D <= 256: volumes on max_width columns, as always.  D > 256 (the wide path pass): on the widest column domain a frame can
    // have, W1max = max_width + min(minD, 0) - max(minD + D, 0) -- at D = 4080 on 4096 columns that is 16 columns instead of
    // 4096 -- and no S2 (the side-by-side horizontal passes are off there); W1max <= 0: every frame is all-invalid, no volumes.
    const bool wide = p.numDisparities > 256;
    const long w1max = (long)max_width + std::min(p.minDisparity, 0) - std::max(p.minDisparity + p.numDisparities, 0);
    const size_t vol = wide ? (w1max > 0 ? (size_t)w1max * max_height * max_batch * p.numDisparities : 0) : px * p.numDisparities;
    AllocList& m = sg->mem;
    hipError_t& e = m.err;
    e = hipStreamCreateWithFlags(&sg->stream, hipStreamNonBlocking);
    m.dev(&sg->dInL, px); m.dev(&sg->dInR, px); m.dev(&sg->dOut, px * 2);
    m.dev(&sg->b.gl, px * 8); m.dev(&sg->b.gr, px * 8);
    sg->pix_bytes = vol;
    m.dev(&sg->b.pix, vol); m.dev(&sg->b.C, vol * 2); m.dev(&sg->b.S, vol * 2);          // (vol == 0: skipped)
    m.dev(&sg->b.label, px * 4); m.dev(&sg->b.size, px * 4); m.dev(&sg->b.runs, px * 4);
    m.dev(&sg->b.rowcnt, (size_t)max_batch * max_height * 4); m.dev(&sg->b.headmap, px * 2);
    if (m.dev(&sg->b.ovf, sizeof(int32_t))) e = hipMemset(sg->b.ovf, 0, sizeof(int32_t));
    m.host(&sg->hOvf, sizeof(int32_t));
    // (MODE_HH4 never runs a row-synchronous sweep: no edge ring)
    sg->b.ring_words = p.paths == 4 ? 0 : sgm_ring_words(max_width, p.numDisparities, max_batch);
    const size_t ring_bytes = sg->b.ring_words * sizeof(unsigned long long);
    if (m.dev(&sg->b.ring, ring_bytes) && ring_bytes) e = hipMemset(sg->b.ring, 0, ring_bytes);
    m.host(&sg->b.abortf, sizeof(int32_t), hipHostMallocMapped);
    // (C, S and S2 are whole allocations, so at least 256-byte aligned: the path passes' packed loads and stores need 16 bytes;
    // S2 is optional: without it the horizontal passes run one after the other)
    if (e == hipSuccess && !wide && !m.dev(&sg->b.S2, vol * 2)) { (void)hipGetLastError(); e = hipSuccess; }
    if (e == hipSuccess) *sg->b.abortf = 0;
    sg->b.epoch = &sg->sweep_epoch;
    if (e == hipSuccess) e = hipEventCreateWithFlags((hipEvent_t*)&sg->b.ev_in, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags((hipEvent_t*)&sg->b.ev_out, hipEventDisableTiming);
    if (e != hipSuccess) { const hipError_t first = e; rtdm_sgm_destroy(sg); return create_failed("rtdm_sgm_create", first); }
    *out = sg;
    return RTDM_OK;
}

void rtdm_sgm_destroy(rtdm_sgm* sg)
{
    if (!sg) return;
    (void)hipSetDevice(sg->device);
    if (sg->stream) (void)hipStreamSynchronize(sg->stream);
    sg->mem.release();
    if (sg->b.ev_in) (void)hipEventDestroy((hipEvent_t)sg->b.ev_in);
    if (sg->b.ev_out) (void)hipEventDestroy((hipEvent_t)sg->b.ev_out);
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
    if (p.paths == 3) { const int rc = sgm_warm_buffer(sg, g, n); if (rc) return rc; }
    const SGMBuffers& b = sg->b;
    if (!sg->caps_asked) { sgm_sweep_caps(g.D, p.paths, b.S2 != nullptr, sg->lim.cap); sg->caps_asked = true; }
    sg->lim.sweep = b.ring && b.ev_in && b.ev_out && b.abortf && *b.abortf == 0;
    sg->lim.s2 = b.S2 != nullptr;
    sg->lim.ring_words = b.ring_words;
    sg->path_variant = launch_sgm(L, R, disp, g, b, sg->lim, p.paths, n, s,
                                  SgmParams{p.blockSize, p.P1, p.P2, p.uniquenessRatio, p.disp12MaxDiff, p.speckleWindowSize,
                                            p.speckleRange, cn, sgm_ftzero(sg), sg->cost});
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
    if (channels == 3 && sg->cost.kind == SGM_COST_CENSUS) return RTDM_ERR_UNSUPPORTED;      // N5: the census cost is gray only
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
    if (channels == 3 && sg->cost.kind == SGM_COST_CENSUS) return RTDM_ERR_UNSUPPORTED;      // N5
    HIPC(hipSetDevice(sg->device));
    if (channels == 3) { const int rc = sgm_colour_buffers(sg, true); if (rc) return rc; }
    sg->cost_limit = sgm_cost_limit(sg, channels);
    hipStream_t s = sg->stream;
    DrainOnError drain{s};
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
    if (rc == RTDM_OK) drain.armed = false;
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

// No allocation, no synchronisation: the descriptors live where the bounds do (b.gl / b.gr), and a call in flight has read the
// handle's setting when it was issued
int rtdm_sgm_set_cost(rtdm_sgm* sg, int cost, int census_width, int census_height)
{
    if (!sg) return RTDM_ERR_NULL;
    if (cost == RTDM_SGM_COST_BT) { sg->cost.kind = SGM_COST_BT; return RTDM_OK; }      // (the two sizes are ignored)
    if (cost != RTDM_SGM_COST_CENSUS) return RTDM_ERR_BAD_PARAM;
    const bool wok = census_width == 3 || census_width == 5 || census_width == 7 || census_width == 9;
    const bool hok = census_height == 3 || census_height == 5 || census_height == 7;
    if (!wok || !hok) return RTDM_ERR_BAD_PARAM;
    sg->cost = SgmCostKind{SGM_COST_CENSUS, census_width, census_height};
    return RTDM_OK;
}

int rtdm_sgm_get_cost(const rtdm_sgm* sg, int* cost, int* census_width, int* census_height)
{
    if (!sg) return RTDM_ERR_NULL;
    if (cost) *cost = sg->cost.kind;
    if (census_width) *census_width = sg->cost.cw;
    if (census_height) *census_height = sg->cost.ch;
    return RTDM_OK;
}

// cv::StereoSGBM::setMode on a live handle: the direction count of the next call's plan.  Nothing is allocated or freed and the
// device is not used; the sweep capacities belong to the mode and are asked again by the next call.
static_assert(RTDM_SGM_MODE_SGBM == 0 && RTDM_SGM_MODE_HH == 1 && RTDM_SGM_MODE_SGBM_3WAY == 2 && RTDM_SGM_MODE_HH4 == 3, "cv::StereoSGBM's values");
int rtdm_sgm_set_mode(rtdm_sgm* sg, int mode)
{
    if (!sg) return RTDM_ERR_NULL;
    if (mode < RTDM_SGM_MODE_SGBM || mode > RTDM_SGM_MODE_HH4) return RTDM_ERR_BAD_PARAM;
    // (k_sgm_vert3 holds a line of at most 256 disparities; there is no wide form of it)
    if (mode == RTDM_SGM_MODE_SGBM_3WAY && sg->p.numDisparities > 256) return RTDM_ERR_UNSUPPORTED;
    static const int paths[4] = {5, 8, 3, 4};
    if (sg->p.paths != paths[mode]) { sg->p.paths = paths[mode]; sg->caps_asked = false; }
    return RTDM_OK;
}

int rtdm_sgm_get_mode(const rtdm_sgm* sg, int* mode)
{
    if (!sg || !mode) return RTDM_ERR_NULL;
    *mode = sg->p.paths == 5 ? RTDM_SGM_MODE_SGBM : (sg->p.paths == 8 ? RTDM_SGM_MODE_HH : (sg->p.paths == 3 ? RTDM_SGM_MODE_SGBM_3WAY : RTDM_SGM_MODE_HH4));
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
