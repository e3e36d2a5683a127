// api_morph.hip -- rtdm_morph, the VideoFilterDevice counterpart (open + close of a mask).
#include "rtdm_handles.h"

using namespace rtdm;

struct rtdm_morph {
    int W, H, maxB, device;
    hipStream_t stream;
    uint8_t *hIn, *hOut;           // page-locked host buffers handed to the application
    uint8_t *dIn, *dOut, *dT0, *dT1;
    AllocList mem;
};

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
