// api_bm.hip -- rtdm_bm, the StereoBM counterpart: parameter validation (cv::StereoBM::compute's checks, SURVEY.md Appendix
// A.1), geometry, staging copies and the launches  K1 prefilter -> K2 search -> K3 left-right check -> K4 speckle filter.
#include "rtdm_handles.h"
#include "rtdm_bm_geom.h"

using namespace rtdm;

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
    rtdm_bm* bm = new (std::nothrow) rtdm_bm();            // (value-initialised: ROIs, counters, streams and events start as zero)
    if (!bm) return RTDM_ERR_NOMEM;
    bm->p = *params; bm->prefilter_type = RTDM_PREFILTER_XSOBEL; bm->prefilter_size = 9;
    bm->maxW = max_width; bm->maxH = max_height; bm->maxB = max_batch; bm->device = device;
    bm->ppitch = ((size_t)max_width + 63) & ~(size_t)63;
    const size_t plane = bm->ppitch * max_height * (size_t)max_batch;
    // per-pixel workspace and the internal disparity plane use rows of Ws = max_width rounded up to 8 elements
    const size_t px = bm_ws(max_width) * max_height * max_batch;
    AllocList& m = bm->mem;
    m.err = hipStreamCreateWithFlags(&bm->stream, hipStreamNonBlocking);
    // + slack: the search kernels stage whole dwords of whole tiles and may read past the last row's end
    // (one allocation, the right planes behind the left ones: k_search_ring addresses both from the left plane's rows)
    // ... and, in front, up to three bytes before the first row's start: the paired form of k_search_ring starts a wave's copy
    // three bytes left of its first window (256 bytes of slack keep the planes' alignment; the list frees what it allocated)
    const size_t plane_al = (plane + 1024 + 255) & ~(size_t)255, front = 256;
    if (m.dev(&bm->dLp, front + 2 * plane_al)) { bm->dLp += front; bm->dRp = bm->dLp + plane_al; }
    m.dev(&bm->dInL, plane); m.dev(&bm->dInR, plane); m.dev(&bm->dOut, px * sizeof(int16_t));
    m.dev(&bm->dCost, px * sizeof(int32_t)); m.dev(&bm->dLabel, px * sizeof(int32_t)); m.dev(&bm->dSize, px * sizeof(int32_t));
    m.dev(&bm->dRuns, px * sizeof(uint32_t)); m.dev(&bm->dHead, px * sizeof(int16_t));
    m.dev(&bm->dMask, (size_t)max_width * max_height); m.dev(&bm->dDepth, depth_scratch_bytes(RTDM_MAX_REGIONS, max_height));
    // the staging area: two input planes of ppitch x max_height | hD, the internal plane of one frame | hM, its mask | slack
    const size_t hplanes = 2 * bm->ppitch * (size_t)max_height, hpx = bm_ws(max_width) * max_height;
    m.host(&bm->hStage, hplanes + hpx * (sizeof(int16_t) + 1) + 1024);
    if (bm->hStage) { bm->hD = (int16_t*)(bm->hStage + hplanes); bm->hM = (uint8_t*)(bm->hD + hpx); }
    m.dev(&bm->dRowCnt, (size_t)max_batch * max_height * sizeof(int32_t));
    // events and the side streams join the same chain: whatever fails, the handle goes through rtdm_bm_destroy
    hipError_t e = m.err;
    const auto new_event = [&e](hipEvent_t* ev) { if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming); };
    const auto new_stream = [&e](hipStream_t* q) { if (e == hipSuccess) e = hipStreamCreateWithFlags(q, hipStreamNonBlocking); };
    for (auto& ev : bm->evBand) new_event(&ev);
    new_stream(&bm->sIn); new_stream(&bm->sOut);
    for (int k = 0; k < 2; ++k) { new_event(&bm->evH2D[k]); new_event(&bm->evComp[k]); new_event(&bm->evD2H[k]); }
    // The runtime maps streams onto its few hardware queues in creation order, and which queue the border side stream shares
    // shows in the search stage (~1 % at the headline).  The streams are therefore created in the order the handle has always
    // created them: sSpare are the two idle streams of the retired two-lane layout.
    new_stream(&bm->sSpare[0]); new_stream(&bm->sBorder); new_stream(&bm->sSpare[1]);
    new_event(&bm->evFork); new_event(&bm->evJoin);
    if (e != hipSuccess) { rtdm_bm_destroy(bm); return create_failed("rtdm_bm_create", e); }
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
    for (hipEvent_t e : {bm->evFork, bm->evJoin, bm->evBand[0], bm->evBand[1]}) if (e) (void)hipEventDestroy(e);
    if (bm->sIn) { (void)hipStreamSynchronize(bm->sIn); (void)hipStreamDestroy(bm->sIn); }
    if (bm->sOut) { (void)hipStreamSynchronize(bm->sOut); (void)hipStreamDestroy(bm->sOut); }
    for (int k = 0; k < 2; ++k)
        for (hipEvent_t e : {bm->evH2D[k], bm->evComp[k], bm->evD2H[k]}) if (e) (void)hipEventDestroy(e);
    for (auto& ev : bm->pending) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    bm->mem.release();
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

// what the rectangles of a frame depend on besides ROI1 (rtdm_bm_geom.h)
static BMRoiGeom roi_geom(const rtdm_bm* bm, int W, int H)
{
    const rtdm_bm_params& p = bm->p;
    return BMRoiGeom{W, H, p.numDisparities, p.minDisparity, p.blockSize / 2, p.disp12MaxDiff >= 0,
                     {bm->roi2[0], bm->roi2[1], bm->roi2[2], bm->roi2[3]}};
}

// offsets, valid rectangle (getValidDisparityROI, clipped to the image and
// to rows that have a full window).  Returns false when the whole frame is FILTERED.
// roi1: the handle's (bm->roi1).  envelope: the rectangle that holds every ROI1's, what rtdm_bm_compute_device_rois searches.
static bool make_geom(const rtdm_bm* bm, int W, int H, BMGeom* g, const int* roi1, bool envelope = false)
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
    // the valid rectangle and the columns worth searching: rtdm_bm_geom.h, shared with the kernels of the per-frame ROIs
    const BMRoiRect q = bm_roi_rect(roi_geom(bm, W, H), roi1, envelope);
    g->vx0 = q.vx0; g->vx1 = q.vx1; g->vy0 = q.vy0; g->vy1 = q.vy1;
    g->cx0 = q.cx0; g->cx1 = q.cx1;
    return q.any != 0;
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

// Fill + prefilter + SAD search of a chunk (VALU bound); *any = false: the whole frame is FILTERED, nothing follows.
// g, any: make_geom's, under the handle's ROI1 or (rtdm_bm_compute_device_rois) the envelope of all of them.
static int chunk_front(rtdm_bm* bm, int n, Plane8 L, Plane8 R, int W, int H, Plane16W disp, hipStream_t s, const BMGeom& g, bool any)
{
    const rtdm_bm_params& p = bm->p;
    if (!any) { launch_fill16(disp, 0, W, 0, H, n, g.filtered, s); return RTDM_OK; }
    // the search kernels write columns [cx0, cx1) of the valid rows; everything else is FILTERED
    // (+ the speckle filter's run counts = 0); the fill rides in the prefilter's launch
    const FillJob fill{disp, g.cx0, g.cx1, g.vy0, g.vy1, g.filtered, (p.speckleRange >= 0 && p.speckleWindowSize > 0) ? bm->dRowCnt : nullptr};
    StageEvent ev;
    Plane8W Lp{bm->dLp, bm->ppitch, bm->ppitch * (size_t)H}, Rp{bm->dRp, bm->ppitch, bm->ppitch * (size_t)H};
    stage_begin(bm, RTDM_STAGE_PREFILTER, n, s, &ev);
    launch_prefilter(L, R, Lp, Rp, W, H, p.preFilterCap, n, s, &fill, bm->prefilter_type, bm->prefilter_size);
    stage_end(bm, s, &ev);
    Plane8 Lpr{bm->dLp, Lp.pitch, Lp.frame}, Rpr{bm->dRp, Rp.pitch, Rp.frame};
    stage_begin(bm, RTDM_STAGE_SEARCH, n, s, &ev);
    // (the two planes share their strides; rtdm_bm_create puts the right ones behind the left ones in one allocation)
    const SearchPlan plan = plan_search(g, n, bm->dRp > bm->dLp && (size_t)(bm->dRp - bm->dLp) < ((size_t)1 << 32) - ((size_t)1 << 20));
    bm->variant = plan.variant;
    HIPC(launch_search(plan, Lpr, Rpr, disp, bm->dCost, g, n, s, SearchSide{bm->sBorder, bm->evFork, bm->evJoin}, &bm->tuner));
    stage_end(bm, s, &ev);
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
    const SpkBuffers wk = speckle ? SpkBuffers{bm->dLabel, bm->dSize, bm->dRuns, bm->dRowCnt, bm->dHead} : SpkBuffers{};
    SpkHeads heads = SpkHeads::NONE;     // what the check leaves for the filter; off: the filter initialises its rows itself
    int block_rows = 1;
    if (lr) {
        stage_begin(bm, RTDM_STAGE_LRCHECK, n, s, &ev);
        const LrPlan lp = plan_lrcheck(g, p.disp12MaxDiff, speckle ? p.speckleRange : 0, n, speckle, rows_aligned(disp, bm->dCost, wk.headmap, W));
        launch_lrcheck(lp, disp, bm->dCost, g, wk, s);
        heads = lp.heads; block_rows = lp.block_rows;
        stage_end(bm, s, &ev);
    }
    if (speckle) {
        stage_begin(bm, RTDM_STAGE_SPECKLE, n, s, &ev);
        const SpkPlan sp = plan_speckle(W, g.Ws, H, n, heads, block_rows, g.vy0, g.vy1, rows_aligned(disp, nullptr, nullptr, W));
        launch_speckle(sp, disp, wk, g.filtered, p.speckleWindowSize, p.speckleRange, s);
        stage_end(bm, s, &ev);
    }
    HIPC(hipGetLastError());
    return RTDM_OK;
}

// One chunk (n <= maxB) of device-resident frames, enqueued on `s`.  The row kernels move 8 columns per 128-bit
// access and let a ragged last chunk spill into the row padding, so they need 16-byte aligned rows of at least
// W rounded up to 8 elements whose padding is ours to write.  A caller's plane qualifies only if W % 8 == 0 and it
// is aligned; anything else (the reference's own crops are 233, 534 and 934 columns wide) runs on the handle's
// internal plane and is copied out at the end.
int rtdm::bm_run_chunk(rtdm_bm* bm, int n, Plane8 L, Plane8 R, int W, int H, Plane16W out, hipStream_t s)
{
    const size_t Ws = bm_ws(W);
    // (the handle's own plane, or a frame-aligned part of it: rows of Ws elements whose padding is ours)
    const bool internal = out.pitch_e == Ws && out.base >= bm->dOut && out.base < bm->dOut + (size_t)bm->maxB * Ws * (size_t)H &&
                          (size_t)(out.base - bm->dOut) % (Ws * (size_t)H) == 0;
    const bool direct = internal || ((W & 7) == 0 && (((size_t)out.base | (out.pitch_e * 2) | (out.frame_e * 2)) & 15) == 0);
    const Plane16W disp = direct ? out : bm_internal_plane(bm, W, H);
    BMGeom g;
    const bool any = make_geom(bm, W, H, &g, bm->roi1);
    int rc = chunk_front(bm, n, L, R, W, H, disp, s, g, any);
    if (rc) return rc;
    if (any) { rc = chunk_back(bm, n, W, H, disp, g, s); if (rc) return rc; }
    if (!direct) launch_copy16(disp, out, W, H, n, s);
    HIPC(hipGetLastError());
    return RTDM_OK;
}

// bm_run_chunk with frame f under ROI1 = d_rois[f] (device memory; w <= 0 or h <= 0: the frame is skipped), rules B1-B4 of
// DESIGN.md section 4.19.  The handle's ROI1 is not read.  Always on the handle's internal plane, where the results stay;
// out.base != null: the planes of the frames that are not skipped are copied there.  The route:
//   front    fill, prefilter and search ONCE for the chunk under the envelope of every ROI1 (make_geom): the search is per
//            pixel, so further searched columns and rows change no searched value
//   mask     SEARCHED: every frame gets the state its own restricted search leaves -- FILTERED outside its searched columns
//            and valid rows, so that exactly the columns vote that vote there
//   check    the left-right check with the envelope's valid rectangle, without the speckle init (its run heads would be stale
//            after the next mask)
//   mask     VALID: the frame's own valid rectangle (inside it the check has seen what the restricted path's sees)
//   speckle  from SpkHeads::NONE, as where the check is off: FILTERED pixels join no component
// With the check off the two masks are one (BOTH).  The masks' launches count as the left-right stage for the stage times.
int rtdm::bm_run_chunk_rois(rtdm_bm* bm, int n, Plane8 L, Plane8 R, int W, int H, const int* d_rois, Plane16W out, hipStream_t s)
{
    const rtdm_bm_params& p = bm->p;
    const Plane16W disp = bm_internal_plane(bm, W, H);
    BMGeom g;
    const bool any = make_geom(bm, W, H, &g, nullptr, true);
    int rc = chunk_front(bm, n, L, R, W, H, disp, s, g, any);
    if (rc) return rc;
    if (any) {
        const BMRoiGeom G = roi_geom(bm, W, H);
        const bool speckle = p.speckleRange >= 0 && p.speckleWindowSize > 0;
        const bool lr = p.disp12MaxDiff >= 0;
        StageEvent ev;
        stage_begin(bm, RTDM_STAGE_LRCHECK, n, s, &ev);
        launch_roi_mask(lr ? RoiMask::SEARCHED : RoiMask::BOTH, disp, G, d_rois, n, g.filtered, s);
        if (lr) {
            const LrPlan lp = plan_lrcheck(g, p.disp12MaxDiff, 0, n, false, rows_aligned(disp, bm->dCost, nullptr, W));
            launch_lrcheck(lp, disp, bm->dCost, g, SpkBuffers{}, s);
            launch_roi_mask(RoiMask::VALID, disp, G, d_rois, n, g.filtered, s);
        }
        stage_end(bm, s, &ev);
        if (speckle) {
            const SpkBuffers wk{bm->dLabel, bm->dSize, bm->dRuns, bm->dRowCnt, bm->dHead};
            stage_begin(bm, RTDM_STAGE_SPECKLE, n, s, &ev);
            const SpkPlan sp = plan_speckle(W, g.Ws, H, n, SpkHeads::NONE, 1, g.vy0, g.vy1, rows_aligned(disp, nullptr, nullptr, W));
            launch_speckle(sp, disp, wk, g.filtered, p.speckleWindowSize, p.speckleRange, s);
            stage_end(bm, s, &ev);
        }
    }
    if (out.base) launch_copy16_rois(disp, out, W, H, n, d_rois, s);
    HIPC(hipGetLastError());
    return RTDM_OK;
}

int rtdm::bm_check_frame(const rtdm_bm* bm, int W, int H)
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
    int rc = bm_check_frame(bm, width, height);
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
        rc = bm_run_chunk(bm, m, L, R, width, height, O, s);
        if (rc) return rc;
    }
    return RTDM_OK;
}

int rtdm_bm_compute_device_rois(rtdm_bm* bm, int n, const uint8_t* d_left, const uint8_t* d_right, size_t pitch,
                                size_t frame_stride, int width, int height, const int* d_roi1, int16_t* d_disp, size_t disp_pitch,
                                size_t disp_frame_stride, void* hip_stream)
{
    if (!bm || !d_left || !d_right || !d_roi1 || !d_disp) return RTDM_ERR_NULL;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    int rc = bm_check_frame(bm, width, height);
    if (rc) return rc;
    if (pitch < (size_t)width || disp_pitch < (size_t)width * 2 || (disp_pitch & 1) || (disp_frame_stride & 1))
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = (hipStream_t)hip_stream;
    for (int i0 = 0; i0 < n; i0 += bm->maxB) {
        const int m = std::min(bm->maxB, n - i0);
        Plane8 L{d_left + (size_t)i0 * frame_stride, pitch, frame_stride};
        Plane8 R{d_right + (size_t)i0 * frame_stride, pitch, frame_stride};
        Plane16W O{d_disp + (size_t)i0 * (disp_frame_stride / 2), disp_pitch / 2, disp_frame_stride / 2};
        rc = bm_run_chunk_rois(bm, m, L, R, width, height, d_roi1 + 4 * (size_t)i0, O, s);
        if (rc) return rc;
    }
    return RTDM_OK;
}

int rtdm_bm_compute_batch(rtdm_bm* bm, int n, const uint8_t* left, const uint8_t* right,
                          size_t pitch, size_t frame_stride, int width, int height,
                          int16_t* disp, size_t disp_pitch, size_t disp_frame_stride)
{
    if (!bm || !left || !right || !disp) return RTDM_ERR_NULL;
    if (n <= 0) return RTDM_ERR_BAD_SIZE;
    int rc = bm_check_frame(bm, width, height);
    if (rc) return rc;
    if (pitch < (size_t)width || disp_pitch < (size_t)width * 2) return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    DrainOnError drain(bm->sIn, s, bm->sOut);   // (an error exit leaves no DMA in flight from / to the caller's buffers)
    const size_t dpitch = bm->ppitch, dframe = bm->ppitch * (size_t)height;
    const size_t Ws = bm_ws(width);                                    // the handle's internal plane (see bm_run_chunk)
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
        rc = bm_run_chunk(bm, m, L, R, width, height, O, s);
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
    drain.armed = false;
    return RTDM_OK;
}

// The caller's Mats are pageable ROI views (estimator.cpp:33,36): the rows are gathered into the page-locked staging
// area on the host and go over in linear async copies -- in two BANDS of rows per direction, so that the host gathers
// band 1 while band 0 is on the bus, and scatters band 0 of the result while band 1 arrives.  720p pair, host to host:
// 0.363 ms with one copy per plane and row-by-row gathers, 0.347 with one band, 0.325 with two, 0.375 with four (every
// further async copy costs more in the runtime than its overlap hides).  Rows that are contiguous in the caller's plane
// move as one memcpy.
static int bm_band_rows(int height) { return height >= 256 ? (height + 1) / 2 : height; }

int rtdm::bm_upload_gray(rtdm_bm* bm, const uint8_t* left, size_t left_pitch, const uint8_t* right, size_t right_pitch, int width, int height,
                         hipStream_t s)
{
    const size_t dpitch = bm->ppitch, dframe = dpitch * (size_t)height;
    const uint8_t* src[2] = {left, right};
    const size_t spitch[2] = {left_pitch, right_pitch};
    uint8_t* dIn[2] = {bm->dInL, bm->dInR};
    for (int y0 = 0, bh = bm_band_rows(height); y0 < height; y0 += bh) {
        const int rows = std::min(bh, height - y0);
        for (int k = 0; k < 2; ++k) {
            uint8_t* h = bm->hStage + k * dframe + (size_t)y0 * dpitch;
            copy_rows(h, dpitch, src[k] + (size_t)y0 * spitch[k], spitch[k], (size_t)width, rows, RowPad::OURS);
            HIPC(hipMemcpyAsync(dIn[k] + (size_t)y0 * dpitch, h, (size_t)rows * dpitch, hipMemcpyHostToDevice, s));
        }
    }
    return RTDM_OK;
}

int rtdm_bm_compute(rtdm_bm* bm, const uint8_t* left, size_t left_pitch, const uint8_t* right,
                    size_t right_pitch, int width, int height, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !left || !right || !disp) return RTDM_ERR_NULL;
    int rc = bm_check_frame(bm, width, height);
    if (rc) return rc;
    if (left_pitch < (size_t)width || right_pitch < (size_t)width || disp_pitch < (size_t)width * 2)
        return RTDM_ERR_BAD_SIZE;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    DrainOnError drain{s};
    const size_t dpitch = bm->ppitch, dframe = bm->ppitch * (size_t)height;
    const Plane16W O = bm_internal_plane(bm, width, height);
    const size_t Ws = O.pitch_e;
    if (page_locked(left) && page_locked(right) && page_locked(disp)) {
        // the caller's planes are page-locked: DMA straight from and to them, no gathers on the host
        HIPC(hipMemcpy2DAsync(bm->dInL, dpitch, left, left_pitch, (size_t)width, height, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpy2DAsync(bm->dInR, dpitch, right, right_pitch, (size_t)width, height, hipMemcpyHostToDevice, s));
        Plane8 Ld{bm->dInL, dpitch, dframe}, Rd{bm->dInR, dpitch, dframe};
        rc = bm_run_chunk(bm, 1, Ld, Rd, width, height, O, s);
        if (rc) return rc;
        HIPC(hipMemcpy2DAsync(disp, disp_pitch, bm->dOut, Ws * sizeof(int16_t), (size_t)width * sizeof(int16_t), height, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        drain.armed = false;
        return RTDM_OK;
    }
    rc = bm_upload_gray(bm, left, left_pitch, right, right_pitch, width, height, s);
    if (rc) return rc;
    Plane8 L{bm->dInL, dpitch, dframe}, R{bm->dInR, dpitch, dframe};
    rc = bm_run_chunk(bm, 1, L, R, width, height, O, s);
    if (rc) return rc;
    const int bh = bm_band_rows(height);                 // back in the same bands: band 0 is scattered while band 1 arrives
    for (int y0 = 0, b = 0; y0 < height; y0 += bh, ++b) {
        HIPC(hipMemcpyAsync(bm->hD + (size_t)y0 * Ws, bm->dOut + (size_t)y0 * Ws, (size_t)std::min(bh, height - y0) * Ws * sizeof(int16_t), hipMemcpyDeviceToHost, s));
        HIPC(hipEventRecord(bm->evBand[b], s));
    }
    for (int y0 = 0, b = 0; y0 < height; y0 += bh, ++b) {
        HIPC(hipEventSynchronize(bm->evBand[b]));
        copy_rows((uint8_t*)disp + (size_t)y0 * disp_pitch, disp_pitch, bm->hD + (size_t)y0 * Ws, Ws * sizeof(int16_t), (size_t)width * sizeof(int16_t),
                  std::min(bh, height - y0), RowPad::KEEP);
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
    if (shapes_measured) *shapes_measured = bm->tuner.shapes;
    if (timing_launches) *timing_launches = bm->tuner.launches;
    return RTDM_OK;
}
void rtdm_debug_search_kernel(int mode) { ring_set_mode(mode); }
void rtdm_debug_disparity_slice(int dt) { dslice_set_width(dt); }

int rtdm_bm_compute_depth(rtdm_bm* bm, const uint8_t* left, size_t left_pitch, const uint8_t* right, size_t right_pitch,
                          int width, int height, const double* Q, const uint8_t* mask, size_t mask_pitch,
                          const rtdm_region* regions, int nregions, double calibration_unit,
                          double* mean_cm, int* counts, int16_t* disp, size_t disp_pitch)
{
    if (!bm || !left || !right || !Q || !mask || !mean_cm || !counts) return RTDM_ERR_NULL;
    int rc = bm_check_frame(bm, width, height);
    if (rc) return rc;
    if (left_pitch < (size_t)width || right_pitch < (size_t)width || mask_pitch < (size_t)width) return RTDM_ERR_BAD_SIZE;
    if (disp && disp_pitch < (size_t)width * 2) return RTDM_ERR_BAD_SIZE;
    int flat[4 * RTDM_MAX_REGIONS], maxh = 1;
    rc = depth_check_regions(regions, nregions, width, height, flat, &maxh);
    if (rc) return rc;
    HIPC(hipSetDevice(bm->device));
    hipStream_t s = bm->stream;
    DrainOnError drain{s};
    const size_t dpitch = bm->ppitch, dframe = bm->ppitch * (size_t)height;
    rc = bm_upload_gray(bm, left, left_pitch, right, right_pitch, width, height, s);
    if (rc) return rc;
    copy_rows(bm->hM, (size_t)width, mask, mask_pitch, (size_t)width, height, RowPad::OURS);
    HIPC(hipMemcpyAsync(bm->dMask, bm->hM, (size_t)width * height, hipMemcpyHostToDevice, s));
    Plane8 L{bm->dInL, dpitch, dframe}, R{bm->dInR, dpitch, dframe};
    const Plane16W O = bm_internal_plane(bm, width, height);
    rc = bm_run_chunk(bm, 1, L, R, width, height, O, s);
    if (rc) return rc;
    DepthQ q; std::copy(Q, Q + 16, q.q);
    launch_depth_stats(bm->dOut, O.pitch_e, width, height, q, bm->dMask, (size_t)width, flat, nregions, bm->maxH,
                       calibration_unit, bm->dDepth, mean_cm, counts, s);
    if (disp) { rc = bm_download_disp(bm, width, height, s); if (rc) return rc; }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    if (disp) bm_scatter_disp(bm, width, height, disp, disp_pitch);
    return RTDM_OK;
}

int rtdm::bm_download_disp(rtdm_bm* bm, int W, int H, hipStream_t s)
{
    HIPC(hipMemcpyAsync(bm->hD, bm->dOut, bm_internal_plane(bm, W, H).frame_e * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    return RTDM_OK;
}

void rtdm::bm_scatter_disp(const rtdm_bm* bm, int W, int H, int16_t* disp, size_t disp_pitch)
{
    const size_t Ws = bm_ws(W);
    copy_rows(disp, disp_pitch, bm->hD, Ws * sizeof(int16_t), (size_t)W * sizeof(int16_t), H, RowPad::KEEP);
}
