// api_objects.hip -- rtdm_objects: object detection -> boxes and ROI (estimator.cpp:40-53).
#include "rtdm_handles.h"

using namespace rtdm;

static const int OBJ_HEAD = 512;  // records fetched together with the count
static const int OBJ_MAX_BATCH = 64;

void rtdm_objects_destroy(rtdm_objects* ob)
{
    if (!ob) return;
    (void)hipSetDevice(ob->device);
    if (ob->stream) (void)hipStreamSynchronize(ob->stream);
    ob->mem.release();
    if (ob->dObj) (void)hipFree(ob->dObj);
    if (ob->dLab) (void)hipFree(ob->dLab);
    if (ob->dStats) (void)hipFree(ob->dStats);
    if (ob->stream) (void)hipStreamDestroy(ob->stream);
    delete ob;
}

int rtdm_objects_create_batch(int width, int height, int max_batch, int max_classes, int device, rtdm_objects** out)
{
    static_assert(sizeof(rtdm_object) == 32 && sizeof(CcObject) == sizeof(rtdm_object), "one record layout");
    static_assert(sizeof(rtdm_object_stats) == 48 && sizeof(CcStats) == sizeof(rtdm_object_stats), "one moments layout");
    static_assert(HSV_MAX_RANGES == RTDM_MAX_HSV_RANGES && HSV_MAX_CLASSES == RTDM_MAX_CLASSES, "one limit");
    if (!out) return RTDM_ERR_NULL;
    *out = nullptr;
    if (width <= 0 || height <= 0 || width > 32767 || height > 32767 || (long)width * height >= (1L << 30)) return RTDM_ERR_BAD_SIZE;
    if (max_batch < 1 || max_batch > OBJ_MAX_BATCH) return RTDM_ERR_BAD_SIZE;
    if (max_classes < 1 || max_classes > RTDM_MAX_CLASSES) return RTDM_ERR_BAD_PARAM;
    if (width > 8192) return RTDM_ERR_UNSUPPORTED;      // the component labelling keeps one row of ints in LDS
    int st = use_device(device);
    if (st) return st;
    rtdm_objects* ob = new (std::nothrow) rtdm_objects();
    if (!ob) return RTDM_ERR_NOMEM;
    ob->W = width; ob->H = height; ob->device = device; ob->maxB = max_batch; ob->maxC = max_classes;
    morph_setting_default(&ob->morph);
    ob->maxRec = ((width + 1) / 2 + 1) * ((height + 1) / 2 + 1);          // more 8-connected components cannot exist
    ob->mpitch = ((size_t)width + 3) & ~(size_t)3;
    const size_t px = (size_t)width * height, planes = (size_t)max_batch * max_classes;
    AllocList& m = ob->mem;
    m.err = hipStreamCreateWithFlags(&ob->stream, hipStreamNonBlocking);
    m.dev(&ob->dRgb, max_batch * objects_rgb_pitch(ob) * height + 16);
    m.dev(&ob->dMaskIn, planes * ob->mpitch * height); m.dev(&ob->dMaskOut, planes * ob->mpitch * height);
    m.dev(&ob->dT0, planes * px); m.dev(&ob->dT1, planes * px);
    m.dev(&ob->dScratch, planes * cc_plane_bytes(width, height, ob->maxRec));
    m.dev(&ob->dMeta, (planes + 4 * (size_t)max_batch) * sizeof(int));
    m.host(&ob->hRec, (size_t)(1 + 6 * OBJ_HEAD) * sizeof(int) + px * 3);
    if (m.err != hipSuccess) { const hipError_t e = m.err; rtdm_objects_destroy(ob); return create_failed("rtdm_objects_create", e); }
    hsv_tables_ready(ob->stream);                       // so that no later call has to wait for them
    *out = ob;
    return RTDM_OK;
}

int rtdm_objects_create(int width, int height, int device, rtdm_objects** out)
{
    return rtdm_objects_create_batch(width, height, 1, 1, device, out);
}

int rtdm_objects_set_morph(rtdm_objects* ob, int op, int iterations, const rtdm_morph_element* el)
{
    const int rc = morph_setting_check(op, iterations, el);
    if (rc) return rc;
    if (!ob) return RTDM_ERR_NULL;
    morph_setting_store(&ob->morph, op, iterations, el);
    return RTDM_OK;
}

int rtdm_objects_get_morph(const rtdm_objects* ob, int* op, int* iterations, rtdm_morph_element* el)
{
    if (!ob) return RTDM_ERR_NULL;
    morph_setting_get(ob->morph, op, iterations, el);
    return RTDM_OK;
}

// dRgb (crop, pitch 3W) -> mask -> morphology -> component boxes; synchronises `s` to read the boxes back.
int rtdm::objects_run(rtdm_objects* ob, const rtdm_hsv_range* range, int min_area, int zero_border, rtdm_region* boxes, int max_boxes,
                      int* nboxes, rtdm_region* roi, hipStream_t s)
{
    const int W = ob->W, H = ob->H;
    launch_hsv_inrange(ob->dRgb, (size_t)W * 3, W, H, range->low, range->high, ob->dMaskIn, (size_t)W, s);
    const int mrc = morph_run(ob->morph, Plane8{ob->dMaskIn, (size_t)W, (size_t)W * H}, Plane8W{ob->dMaskOut, (size_t)W, (size_t)W * H},
                              ob->dT0, ob->dT1, W, H, 1, s);
    if (mrc) return mrc;
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
    DrainOnError drain{s};
    uint8_t* h = (uint8_t*)(ob->hRec + 1 + 6 * OBJ_HEAD);
    copy_rows(h, row, rgb, pitch, row, ob->H, RowPad::OURS);
    HIPC(hipMemcpyAsync(ob->dRgb, h, row * ob->H, hipMemcpyHostToDevice, s));
    int st = objects_run(ob, range, min_area, zero_border, boxes, max_boxes, nboxes, roi, s);
    if (st) return st;
    if (mask_out) {                                     // through the page-locked area (the upload is long done)
        HIPC(hipMemcpyAsync(h, ob->dMaskOut, (size_t)ob->W * ob->H, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        copy_rows(mask_out, mask_pitch, h, (size_t)ob->W, (size_t)ob->W, ob->H, RowPad::KEEP);
    }
    drain.armed = false;                                // (objects_run has synchronised)
    return RTDM_OK;
}

// ---- frame batches and colour classes (rules O1-O6) ----------------------------------------------------------------------
// the handle's colour staging for the batched calls: rows (and so frames) start on dwords, k_hsv_classes reads three per lane
size_t rtdm::objects_rgb_pitch(const rtdm_objects* ob) { return ((size_t)ob->W * 3 + 3) & ~(size_t)3; }

// O1 / O6: the ranges and their classes as the kernel takes them; needs no handle
int rtdm::objects_classes_check(const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, HsvClasses* C)
{
    if (!ranges || !range_class) return RTDM_ERR_NULL;
    if (nranges < 1 || nranges > RTDM_MAX_HSV_RANGES || nclasses < 1 || nclasses > RTDM_MAX_CLASSES) return RTDM_ERR_BAD_PARAM;
    memset(C, 0, sizeof *C);
    C->nranges = nranges; C->nclasses = nclasses;
    unsigned owned = 0;
    for (int i = 0; i < nranges; ++i) {
        if (range_class[i] < 0 || range_class[i] >= nclasses) return RTDM_ERR_BAD_PARAM;
        owned |= 1u << range_class[i];
        C->cls[i] = range_class[i];
        for (int k = 0; k < 3; ++k) { C->lo[i][k] = ranges[i].low[k]; C->hi[i][k] = ranges[i].high[k]; }
    }
    return owned == (1u << nclasses) - 1 ? RTDM_OK : RTDM_ERR_BAD_PARAM;       // every class owns a range
}

// The refusals of the two batched entry points, in the order include/rtdm.h gives: what needs no handle comes first.
static int objects_batch_check(const rtdm_objects* ob, int n, const void* rgb, size_t pitch, size_t frame_stride,
                               const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, const void* masks,
                               size_t mask_pitch, size_t mask_plane_stride, const void* objects, int capacity, const void* counts,
                               const void* rois, HsvClasses* C)
{
    if (!rgb || !counts || !rois || (capacity > 0 && !objects)) return RTDM_ERR_NULL;
    const int rc = objects_classes_check(ranges, range_class, nranges, nclasses, C);
    if (rc) return rc;
    if (n < 0 || capacity < 0) return RTDM_ERR_BAD_SIZE;
    if (!ob) return RTDM_ERR_NULL;
    if (nclasses > ob->maxC) return RTDM_ERR_BAD_PARAM;
    if (pitch < (size_t)ob->W * 3 || (masks && mask_pitch < (size_t)ob->W)) return RTDM_ERR_BAD_SIZE;
    if (n > 1 && frame_stride < pitch * ob->H) return RTDM_ERR_BAD_SIZE;
    if (masks && (size_t)n * nclasses > 1 && mask_plane_stride < mask_pitch * ob->H) return RTDM_ERR_BAD_SIZE;
    return RTDM_OK;
}

// L8: what the labels form of a call refuses on top, in the order include/rtdm.h gives.  W, H: the handle's (L2: the largest
// moment, below W * H * max(W, H)^2, must fit int64).  planes: how many label planes the call writes or reads.
static int labels_check(const void* labels, size_t label_pitch, size_t label_plane_stride, const void* stats, int W, int H, size_t planes)
{
    if (labels) {
        if (label_pitch < (size_t)W * 4 || label_pitch % 4) return RTDM_ERR_BAD_SIZE;
        if (label_plane_stride % 4 || (planes > 1 && label_plane_stride < label_pitch * H)) return RTDM_ERR_BAD_SIZE;
        if ((size_t)labels % 4) return RTDM_ERR_BAD_SIZE;
    }
    if (stats && (size_t)stats % 8) return RTDM_ERR_BAD_SIZE;
    if (labels || stats) {
        const unsigned __int128 side = (unsigned)std::max(W, H), top = (unsigned __int128)W * H * side * side;
        if (top > (unsigned __int128)INT64_MAX) return RTDM_ERR_UNSUPPORTED;
    }
    return RTDM_OK;
}

// One chunk (m <= maxB frames) on s: class masks -> filter -> labelling -> selection.  d_masks == null: the filtered planes
// stay in the handle (dMaskOut, rows of ob->mpitch).  lab: the chunk's label planes and moments, each may be null.
int rtdm::objects_run_chunk(rtdm_objects* ob, int m, const uint8_t* d_rgb, size_t pitch, size_t frame_stride, const HsvClasses& C,
                            int min_area, int zero_border, uint8_t* d_masks, size_t mask_pitch, size_t mask_plane_stride,
                            CcObject* d_objects, int capacity, int* d_counts, int* d_rois, hipStream_t s, const CcLabelsOut& lab)
{
    const int W = ob->W, H = ob->H, planes = m * C.nclasses;
    const size_t ip = ob->mpitch, iplane = ip * H;
    launch_hsv_classes(d_rgb, pitch, frame_stride, m, W, H, C, ob->dMaskIn, ip, iplane, s);
    const Plane8W out = d_masks ? Plane8W{d_masks, mask_pitch, mask_plane_stride} : Plane8W{ob->dMaskOut, ip, iplane};
    const int rc = morph_run(ob->morph, Plane8{ob->dMaskIn, ip, iplane}, out, ob->dT0, ob->dT1, W, H, planes, s);
    if (rc) return rc;
    launch_cc_objects(out.base, out.pitch, out.frame, m, C.nclasses, W, H, zero_border, min_area, ob->dScratch, ob->maxRec, d_objects,
                      capacity, d_counts, d_rois, s, lab);
    HIPC(hipGetLastError());
    return RTDM_OK;
}

int rtdm_objects_detect_labels_device(rtdm_objects* ob, int n, const uint8_t* d_rgb, size_t pitch, size_t frame_stride,
                                      const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses,
                                      int min_area, int zero_border, uint8_t* d_masks, size_t mask_pitch,
                                      size_t mask_plane_stride, rtdm_object* d_objects, int capacity, int* d_counts,
                                      rtdm_region* d_rois, int32_t* d_labels, size_t label_pitch, size_t label_plane_stride,
                                      rtdm_object_stats* d_stats, void* hip_stream)
{
    HsvClasses C;
    int rc = objects_batch_check(ob, n, d_rgb, pitch, frame_stride, ranges, range_class, nranges, nclasses, d_masks, mask_pitch,
                                 mask_plane_stride, d_objects, capacity, d_counts, d_rois, &C);
    if (rc) return rc;
    rc = labels_check(d_labels, label_pitch, label_plane_stride, d_stats, ob->W, ob->H, (size_t)n * nclasses);
    if (rc) return rc;
    if (n == 0) return RTDM_OK;
    HIPC(hipSetDevice(ob->device));
    hipStream_t s = (hipStream_t)hip_stream;          // NULL = the HIP null stream
    for (int i0 = 0; i0 < n; i0 += ob->maxB) {
        const int m = std::min(ob->maxB, n - i0);
        const int st = objects_run_chunk(ob, m, d_rgb + (size_t)i0 * frame_stride, pitch, frame_stride, C, min_area, zero_border,
                                         d_masks ? d_masks + (size_t)i0 * nclasses * mask_plane_stride : nullptr, mask_pitch,
                                         mask_plane_stride, (CcObject*)d_objects + (size_t)i0 * capacity, capacity,
                                         d_counts + (size_t)i0 * nclasses, (int*)(d_rois + i0), s,
                                         CcLabelsOut{d_labels ? (int32_t*)((uint8_t*)d_labels + (size_t)i0 * nclasses * label_plane_stride) : nullptr,
                                                     label_pitch, label_plane_stride, d_stats ? (CcStats*)d_stats + (size_t)i0 * capacity : nullptr});
        if (st) return st;
    }
    return RTDM_OK;
}

int rtdm_objects_detect_device(rtdm_objects* ob, int n, const uint8_t* d_rgb, size_t pitch, size_t frame_stride,
                               const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, int min_area,
                               int zero_border, uint8_t* d_masks, size_t mask_pitch, size_t mask_plane_stride,
                               rtdm_object* d_objects, int capacity, int* d_counts, rtdm_region* d_rois, void* hip_stream)
{
    return rtdm_objects_detect_labels_device(ob, n, d_rgb, pitch, frame_stride, ranges, range_class, nranges, nclasses, min_area, zero_border,
                                             d_masks, mask_pitch, mask_plane_stride, d_objects, capacity, d_counts, d_rois, nullptr, 0, 0,
                                             nullptr, hip_stream);
}

// room for `entries` records in the handle's device staging of the host entry points
int rtdm::objects_stage(rtdm_objects* ob, size_t entries)
{
    if (entries <= ob->objCap) return RTDM_OK;
    if (ob->dObj) { HIPC(hipStreamSynchronize(ob->stream)); HIPC(hipFree(ob->dObj)); }
    ob->dObj = nullptr; ob->objCap = 0;
    HIPC(hipMalloc(&ob->dObj, entries * sizeof(CcObject)));
    ob->objCap = entries;
    return RTDM_OK;
}

// room for a chunk's label planes / moments in the handle's device staging of the host entry point
static int objects_stage_labels(rtdm_objects* ob, size_t label_bytes, size_t stat_entries)
{
    if (label_bytes > ob->labBytes) {
        if (ob->dLab) { HIPC(hipStreamSynchronize(ob->stream)); HIPC(hipFree(ob->dLab)); }
        ob->dLab = nullptr; ob->labBytes = 0;
        HIPC(hipMalloc(&ob->dLab, label_bytes));
        ob->labBytes = label_bytes;
    }
    if (stat_entries > ob->statCap) {
        if (ob->dStats) { HIPC(hipStreamSynchronize(ob->stream)); HIPC(hipFree(ob->dStats)); }
        ob->dStats = nullptr; ob->statCap = 0;
        HIPC(hipMalloc(&ob->dStats, stat_entries * sizeof(CcStats)));
        ob->statCap = stat_entries;
    }
    return RTDM_OK;
}

int rtdm_objects_detect_labels_batch(rtdm_objects* ob, int n, const uint8_t* rgb, size_t pitch, size_t frame_stride,
                                     const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses,
                                     int min_area, int zero_border, uint8_t* masks, size_t mask_pitch, size_t mask_plane_stride,
                                     rtdm_object* objects, int capacity, int* counts, rtdm_region* rois, int32_t* labels,
                                     size_t label_pitch, size_t label_plane_stride, rtdm_object_stats* stats)
{
    HsvClasses C;
    int rc = objects_batch_check(ob, n, rgb, pitch, frame_stride, ranges, range_class, nranges, nclasses, masks, mask_pitch,
                                 mask_plane_stride, objects, capacity, counts, rois, &C);
    if (rc) return rc;
    rc = labels_check(labels, label_pitch, label_plane_stride, stats, ob->W, ob->H, (size_t)n * nclasses);
    if (rc) return rc;
    if (n == 0) return RTDM_OK;
    HIPC(hipSetDevice(ob->device));
    hipStream_t s = ob->stream;
    DrainOnError drain{s};
    const int W = ob->W, H = ob->H, K = nclasses;
    const size_t rp = objects_rgb_pitch(ob), rf = rp * H, ip = ob->mpitch, iplane = ip * H;
    // a frame never has more than K * maxRec objects: the staging need not follow a larger capacity
    const int cap = (int)std::min((size_t)capacity, (size_t)K * ob->maxRec);
    rc = objects_stage(ob, (size_t)std::min(ob->maxB, n) * cap);
    if (rc) return rc;
    const size_t lp = (size_t)W * 4, lplane = lp * H;                        // the staged label planes: dense rows
    rc = objects_stage_labels(ob, labels ? (size_t)std::min(ob->maxB, n) * K * lplane : 0, stats ? (size_t)std::min(ob->maxB, n) * cap : 0);
    if (rc) return rc;
    int* dCounts = ob->dMeta;
    int* dRois = ob->dMeta + (size_t)ob->maxB * ob->maxC;
    for (int i0 = 0; i0 < n; i0 += ob->maxB) {
        const int m = std::min(ob->maxB, n - i0);
        for (int j = 0; j < m; ++j)
            HIPC(hipMemcpy2DAsync(ob->dRgb + j * rf, rp, rgb + (size_t)(i0 + j) * frame_stride, pitch, (size_t)W * 3, H, hipMemcpyHostToDevice, s));
        rc = objects_run_chunk(ob, m, ob->dRgb, rp, rf, C, min_area, zero_border, nullptr, 0, 0, ob->dObj, cap, dCounts, dRois, s,
                               CcLabelsOut{labels ? ob->dLab : nullptr, lp, lplane, stats ? ob->dStats : nullptr});
        if (rc) return rc;
        int* hCounts = ob->hRec;
        int* hRois = ob->hRec + m * K;
        HIPC(hipMemcpyAsync(hCounts, dCounts, (size_t)m * K * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(hRois, dRois, (size_t)m * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        for (int j = 0; j < m; ++j) {
            long total = 0;
            for (int c = 0; c < K; ++c) { counts[(size_t)(i0 + j) * K + c] = hCounts[j * K + c]; total += hCounts[j * K + c]; }
            rois[i0 + j] = rtdm_region{hRois[4 * j], hRois[4 * j + 1], hRois[4 * j + 2], hRois[4 * j + 3]};
            const size_t stored = (size_t)std::min<long>(total, cap);                  // O4: the rest of the caller's array stays as it is
            if (stored) HIPC(hipMemcpyAsync(objects + (size_t)(i0 + j) * capacity, ob->dObj + (size_t)j * cap, stored * sizeof(rtdm_object),
                                            hipMemcpyDeviceToHost, s));
            if (stored && stats) HIPC(hipMemcpyAsync(stats + (size_t)(i0 + j) * capacity, ob->dStats + (size_t)j * cap,
                                                     stored * sizeof(rtdm_object_stats), hipMemcpyDeviceToHost, s));
            for (int c = 0; labels && c < K; ++c)
                HIPC(hipMemcpy2DAsync((uint8_t*)labels + ((size_t)(i0 + j) * K + c) * label_plane_stride, label_pitch,
                                      (uint8_t*)ob->dLab + ((size_t)j * K + c) * lplane, lp, lp, H, hipMemcpyDeviceToHost, s));
            for (int c = 0; masks && c < K; ++c)
                HIPC(hipMemcpy2DAsync(masks + ((size_t)(i0 + j) * K + c) * mask_plane_stride, mask_pitch,
                                      ob->dMaskOut + ((size_t)j * K + c) * iplane, ip, (size_t)W, H, hipMemcpyDeviceToHost, s));
        }
        HIPC(hipStreamSynchronize(s));
    }
    drain.armed = false;
    return RTDM_OK;
}

int rtdm_objects_detect_batch(rtdm_objects* ob, int n, const uint8_t* rgb, size_t pitch, size_t frame_stride,
                              const rtdm_hsv_range* ranges, const int* range_class, int nranges, int nclasses, int min_area,
                              int zero_border, uint8_t* masks, size_t mask_pitch, size_t mask_plane_stride,
                              rtdm_object* objects, int capacity, int* counts, rtdm_region* rois)
{
    return rtdm_objects_detect_labels_batch(ob, n, rgb, pitch, frame_stride, ranges, range_class, nranges, nclasses, min_area, zero_border,
                                            masks, mask_pitch, mask_plane_stride, objects, capacity, counts, rois, nullptr, 0, 0, nullptr);
}
