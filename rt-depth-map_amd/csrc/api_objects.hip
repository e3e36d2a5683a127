// api_objects.hip -- rtdm_objects: object detection -> boxes and ROI (estimator.cpp:40-53).
#include "rtdm_handles.h"

using namespace rtdm;

static const int OBJ_HEAD = 512;  // records fetched together with the count

void rtdm_objects_destroy(rtdm_objects* ob)
{
    if (!ob) return;
    (void)hipSetDevice(ob->device);
    if (ob->stream) (void)hipStreamSynchronize(ob->stream);
    ob->mem.release();
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
    morph_setting_default(&ob->morph);
    ob->maxRec = ((width + 1) / 2 + 1) * ((height + 1) / 2 + 1);          // more 8-connected components cannot exist
    const size_t px = (size_t)width * height;
    AllocList& m = ob->mem;
    m.err = hipStreamCreateWithFlags(&ob->stream, hipStreamNonBlocking);
    m.dev(&ob->dRgb, px * 3 + 16);
    m.dev(&ob->dMaskIn, px); m.dev(&ob->dMaskOut, px); m.dev(&ob->dT0, px); m.dev(&ob->dT1, px);
    m.dev(&ob->dScratch, cc_scratch_bytes(width, height, ob->maxRec));
    m.host(&ob->hRec, (size_t)(1 + 6 * OBJ_HEAD) * sizeof(int) + px * 3);
    if (m.err != hipSuccess) { const hipError_t e = m.err; rtdm_objects_destroy(ob); return create_failed("rtdm_objects_create", e); }
    *out = ob;
    return RTDM_OK;
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
