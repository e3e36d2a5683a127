// api_mjpeg.hip -- rtdm_mjpeg, the DecoderDevice counterpart: baseline MJPEG frames (estimator.cpp:24-27; rules J1-J5,
// DESIGN.md section 4.12).
#include "rtdm_handles.h"

using namespace rtdm;

static_assert(sizeof(rtdm_mjpeg_info) == sizeof(MjpegInfo), "rtdm_mjpeg_info and MjpegInfo are one layout");
static_assert(MJ_BAD_STREAM == RTDM_ERR_BAD_STREAM && MJ_UNSUPPORTED == RTDM_ERR_UNSUPPORTED && MJ_BAD_SIZE == RTDM_ERR_BAD_SIZE &&
              MJ_NULL == RTDM_ERR_NULL, "rtdm_mjpeg.h restates the status values");

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
    h->mem.release();
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
    AllocList& m = h->mem;
    m.err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (m.err == hipSuccess) m.err = hipEventCreateWithFlags(&h->evStaged, hipEventDisableTiming);
    m.host(&h->hStreams, slot * B); m.host(&h->hDesc, sizeof(MjpegDesc) * B); m.host(&h->hSegs, sizeof(MjpegSeg) * h->maxSegs * B);
    m.host(&h->hStatus, sizeof(int) * 2);
    m.dev(&h->dStreams, slot * B); m.dev(&h->dDesc, sizeof(MjpegDesc) * B); m.dev(&h->dSegs, sizeof(MjpegSeg) * h->maxSegs * B);
    m.dev(&h->dCoef, h->maxBlocks * 128 * B); m.dev(&h->dPlanes, h->maxBlocks * 64 * B);
    m.dev(&h->dRgb, (size_t)max_width * max_height * 3);
    m.dev(&h->dStatus, sizeof(int) * (B + 1));
    m.dev(&h->dSplitTotals, sizeof(unsigned long long) * 2); m.dev(&h->dSplitRounds, sizeof(int));
    if (m.err == hipSuccess) m.err = hipMemsetAsync(h->dSplitTotals, 0, sizeof(unsigned long long) * 2, h->stream);
    if (m.err == hipSuccess) m.err = hipMemsetAsync(h->dSplitRounds, 0, sizeof(int), h->stream);
    if (m.err == hipSuccess) m.err = hipStreamSynchronize(h->stream);
    h->splitBytes = MJ_SPLIT_DEFAULT;
    if (m.err != hipSuccess) { const hipError_t e = m.err; rtdm_mjpeg_destroy(h); return create_failed("rtdm_mjpeg_create", e); }
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

int rtdm::mjpeg_check(const rtdm_mjpeg* h, const uint8_t* stream, size_t len, int W, int H)
{
    MjpegDesc d;
    MjpegInfo info;
    const int st = mjpeg_parse(stream, len, &d, &info, nullptr, 0);
    return st ? st : mjpeg_fits(h, d, W, H, nullptr);
}

// m <= maxB frames: parse and stage on the host, then copies, the zeroing of coefficients and status words, and the three
// kernels on s.  *shape: the first frame of the CALL (ncomp 0 before it); d_status: m ints on the device.
int rtdm::mjpeg_chunk(rtdm_mjpeg* h, int m, const uint8_t* const* streams, const size_t* lens, int W, int H, uint8_t* d_rgb, size_t pitch,
                      size_t frame_stride, int* d_status, hipStream_t s, MjpegDesc* shape)
{
    if (h->staged) { HIPC(hipEventSynchronize(h->evStaged)); h->staged = false; }
    size_t nsegs = 0, bytes = 0;
    unsigned max_nseg = 1;
    MjpegSplitCall split = {(uint32_t)h->splitBytes, 0, 0, h->dSplitTotals, h->dSplitRounds};
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
        if (d.nseg == 1) {                                   // what k_mjpeg_huff_split works out for itself from the same figures
            const MjpegSeg sg = h->hSegs[d.seg_first];
            const uint32_t end = std::min(sg.end, d.stream_len), begin = std::min(sg.begin, end);
            uint32_t sp;
            const uint32_t nsub = mjpeg_split_plan(end - begin, split.bytes, &sp);
            if (nsub >= 2) { ++split.frames; split.max_nsub = std::max(split.max_nsub, nsub); }
        }
    }
    const size_t nb = mjpeg_frame_blocks(*shape);
    HIPC(hipMemcpyAsync(h->dStreams, h->hStreams, bytes, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(h->dDesc, h->hDesc, sizeof(MjpegDesc) * m, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(h->dSegs, h->hSegs, sizeof(MjpegSeg) * nsegs, hipMemcpyHostToDevice, s));
    HIPC(hipEventRecord(h->evStaged, s));
    h->staged = true;
    HIPC(hipMemsetAsync(h->dCoef, 0, nb * 128 * m, s));
    HIPC(hipMemsetAsync(d_status, 0, sizeof(int) * m, s));
    h->lastStream = s;
    h->used = true;
    launch_mjpeg(h->dStreams, h->dDesc, h->dSegs, m, *shape, max_nseg, split, h->dCoef, h->dPlanes, d_rgb, pitch, frame_stride, d_status, s);
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
    int st = mjpeg_check(h, stream, len, width, height);      // refusals come first: no device use for a frame that is not served
    if (st) return st;
    HIPC(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DrainOnError drain{s};
    const size_t row = (size_t)width * 3;
    st = mjpeg_chunk(h, 1, &stream, &len, width, height, h->dRgb, row, row * height, h->dStatus, s, &shape);
    if (st) return st;
    HIPC(hipMemcpy2DAsync(rgb, pitch, h->dRgb, row, row, height, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h->hStatus, h->dStatus, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    drain.armed = false;
    return h->hStatus[0] ? RTDM_ERR_BAD_STREAM : RTDM_OK;
}

int rtdm_mjpeg_set_split(rtdm_mjpeg* h, int subsequence_bytes)
{
    // the value first: what it may be does not depend on the handle
    if (subsequence_bytes != 0 && subsequence_bytes != -1 && (subsequence_bytes < MJ_SPLIT_MIN || subsequence_bytes > MJ_SPLIT_MAX))
        return RTDM_ERR_BAD_PARAM;
    if (!h) return RTDM_ERR_NULL;
    h->splitBytes = subsequence_bytes == -1 ? MJ_SPLIT_DEFAULT : subsequence_bytes;
    return RTDM_OK;
}

int rtdm_mjpeg_get_split(const rtdm_mjpeg* h, int* subsequence_bytes)
{
    if (!h || !subsequence_bytes) return RTDM_ERR_NULL;
    *subsequence_bytes = h->splitBytes;
    return RTDM_OK;
}

int rtdm_mjpeg_get_split_stats(rtdm_mjpeg* h, long* frames_split, long* subsequences, int* max_rounds)
{
    if (!h) return RTDM_ERR_NULL;
    HIPC(hipSetDevice(h->device));
    if (h->used) HIPC(hipStreamSynchronize(h->lastStream));
    unsigned long long tot[2];
    int rounds;
    HIPC(hipMemcpy(tot, h->dSplitTotals, sizeof tot, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(&rounds, h->dSplitRounds, sizeof rounds, hipMemcpyDeviceToHost));
    if (frames_split) *frames_split = (long)tot[0];
    if (subsequences) *subsequences = (long)tot[1];
    if (max_rounds) *max_rounds = rounds;
    return RTDM_OK;
}
