// api_morph.hip -- rtdm_morph, the VideoFilterDevice counterpart (open + close of a mask).
#include "rtdm_handles.h"

using namespace rtdm;

struct rtdm_morph {
    int W, H, maxB, device;
    hipStream_t stream;
    uint8_t *hIn, *hOut;           // page-locked host buffers handed to the application
    uint8_t *dIn, *dOut, *dT0, *dT1;
    MorphSetting set;              // rtdm_morph_set_op
    AllocList mem;
};

static std::atomic<int> g_morph_general{0};   // rtdm_debug_morph_general

int rtdm_morph_make_element(int shape, int width, int height, rtdm_morph_element* out)
{
    if (!out) return RTDM_ERR_NULL;
    if (shape != RTDM_MORPH_RECT && shape != RTDM_MORPH_CROSS && shape != RTDM_MORPH_ELLIPSE) return RTDM_ERR_BAD_PARAM;
    if (width < 1 || height < 1) return RTDM_ERR_BAD_PARAM;
    if (width > RTDM_MORPH_MAX_SIZE || height > RTDM_MORPH_MAX_SIZE) return RTDM_ERR_UNSUPPORTED;
    if (width == 1 && height == 1) shape = RTDM_MORPH_RECT;
    memset(out, 0, sizeof *out);
    out->width = width; out->height = height; out->anchor_x = width / 2; out->anchor_y = height / 2;
    const int r = height / 2, c = width / 2;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    for (int i = 0; i < height; ++i) {
        int j1 = 0, j2 = 0;                                        // members [j1, j2)
        if (shape == RTDM_MORPH_RECT || (shape == RTDM_MORPH_CROSS && i == out->anchor_y)) j2 = width;
        else if (shape == RTDM_MORPH_CROSS) { j1 = out->anchor_x; j2 = j1 + 1; }
        else {
            const int dy = i - r;
            if (std::abs(dy) <= r) {
                const int dx = (int)lrint(c * sqrt((r * r - dy * dy) * inv_r2));      // cvRound: ties to even
                j1 = std::max(c - dx, 0); j2 = std::min(c + dx + 1, width);
            }
        }
        for (int j = j1; j < j2; ++j) out->mask[i * width + j] = 1;
    }
    return RTDM_OK;
}

int rtdm::morph_setting_check(int op, int iterations, const rtdm_morph_element* el)
{
    if (!el) return RTDM_ERR_NULL;
    if (!((op >= RTDM_MORPH_ERODE && op <= RTDM_MORPH_BLACKHAT) || op == RTDM_MORPH_OPEN_CLOSE)) return RTDM_ERR_BAD_PARAM;
    if (iterations < 1 || iterations > RTDM_MORPH_MAX_ITERATIONS) return RTDM_ERR_BAD_PARAM;
    if (el->width < 1 || el->height < 1) return RTDM_ERR_BAD_PARAM;
    if (el->width > RTDM_MORPH_MAX_SIZE || el->height > RTDM_MORPH_MAX_SIZE) return RTDM_ERR_UNSUPPORTED;
    if (el->anchor_x < 0 || el->anchor_x >= el->width || el->anchor_y < 0 || el->anchor_y >= el->height) return RTDM_ERR_BAD_PARAM;
    for (int i = 0; i < el->width * el->height; ++i) if (el->mask[i]) return RTDM_OK;
    return RTDM_ERR_BAD_PARAM;
}

static bool same_bits(const MorphBits& a, const MorphBits& b)
{
    return a.w == b.w && a.h == b.h && a.ax == b.ax && a.ay == b.ay && !memcmp(a.rows, b.rows, sizeof a.rows);
}

void rtdm::morph_setting_store(MorphSetting* s, int op, int iterations, const rtdm_morph_element* el)
{
    static_assert(MORPH_MAX_SIZE == RTDM_MORPH_MAX_SIZE, "one limit");
    s->op = op; s->iterations = iterations;
    memset(&s->el, 0, sizeof s->el);
    s->el.width = el->width; s->el.height = el->height; s->el.anchor_x = el->anchor_x; s->el.anchor_y = el->anchor_y;
    for (int i = 0; i < el->width * el->height; ++i) s->el.mask[i] = el->mask[i] ? 1 : 0;
    (void)morph_element_bits(s->el.mask, el->width, el->height, el->anchor_x, el->anchor_y, &s->bits);
    rtdm_morph_element d;
    MorphBits db;
    (void)rtdm_morph_make_element(RTDM_MORPH_ELLIPSE, 10, 10, &d);
    (void)morph_element_bits(d.mask, d.width, d.height, d.anchor_x, d.anchor_y, &db);
    s->is_default = op == RTDM_MORPH_OPEN_CLOSE && iterations == 1 && same_bits(s->bits, db);
}

void rtdm::morph_setting_default(MorphSetting* s)
{
    rtdm_morph_element d;
    (void)rtdm_morph_make_element(RTDM_MORPH_ELLIPSE, 10, 10, &d);
    morph_setting_store(s, RTDM_MORPH_OPEN_CLOSE, 1, &d);
}

void rtdm::morph_setting_get(const MorphSetting& s, int* op, int* iterations, rtdm_morph_element* el)
{
    if (op) *op = s.op;
    if (iterations) *iterations = s.iterations;
    if (el) *el = s.el;
}

int rtdm::morph_run(const MorphSetting& s, Plane8 in, Plane8W out, uint8_t* t0, uint8_t* t1, int W, int H, int n, hipStream_t stream)
{
    if (s.is_default && !g_morph_general.load(std::memory_order_relaxed)) {
        launch_morph_open_close(in, out, t0, t1, W, H, n, stream);
        return RTDM_OK;
    }
    HIPC(launch_morph_general(s.op, s.iterations, s.bits, in, out, t0, t1, W, H, n, stream));
    return RTDM_OK;
}

void rtdm_debug_morph_general(int on) { g_morph_general.store(on ? 1 : 0, std::memory_order_relaxed); }

int rtdm_morph_set_op(rtdm_morph* mf, int op, int iterations, const rtdm_morph_element* el)
{
    const int rc = morph_setting_check(op, iterations, el);
    if (rc) return rc;
    if (!mf) return RTDM_ERR_NULL;
    morph_setting_store(&mf->set, op, iterations, el);
    return RTDM_OK;
}

int rtdm_morph_get_op(const rtdm_morph* mf, int* op, int* iterations, rtdm_morph_element* el)
{
    if (!mf) return RTDM_ERR_NULL;
    morph_setting_get(mf->set, op, iterations, el);
    return RTDM_OK;
}

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
    morph_setting_default(&mf->set);
    const size_t px = (size_t)width * height, all = px * max_batch;
    AllocList& m = mf->mem;
    m.err = hipStreamCreateWithFlags(&mf->stream, hipStreamNonBlocking);
    m.host(&mf->hIn, px); m.host(&mf->hOut, px);
    m.dev(&mf->dIn, all); m.dev(&mf->dOut, all); m.dev(&mf->dT0, all); m.dev(&mf->dT1, all);
    if (m.err != hipSuccess) { const hipError_t e = m.err; rtdm_morph_destroy(mf); return create_failed("rtdm_morph_create", e); }
    *out = mf;
    return RTDM_OK;
}

void rtdm_morph_destroy(rtdm_morph* mf)
{
    if (!mf) return;
    (void)hipSetDevice(mf->device);
    if (mf->stream) (void)hipStreamSynchronize(mf->stream);
    mf->mem.release();
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
        const int rc = morph_run(mf->set, in, out, mf->dT0, mf->dT1, width, height, m, s);
        if (rc) return rc;
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
    DrainOnError drain{s};
    HIPC(hipMemcpy2DAsync(mf->dIn, width, in, in_pitch, width, height, hipMemcpyHostToDevice, s));
    int rc = rtdm_morph_run_device(mf, 1, mf->dIn, width, (size_t)width * height, mf->dOut, width,
                                   (size_t)width * height, width, height, s);
    if (rc) return rc;
    HIPC(hipMemcpy2DAsync(out, out_pitch, mf->dOut, width, width, height, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    return RTDM_OK;
}
