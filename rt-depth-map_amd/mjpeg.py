"""The baseline MJPEG decoder over rtdm_mjpeg_* (csrc/api_mjpeg.hip)."""
import ctypes as C

import numpy as np

from . import binding as B
from ._marshal import Handle


def mjpeg_probe(stream):
    """Headers of one baseline JPEG frame -> dict (width, height, components, h_samp, v_samp, restart_interval, segments,
    has_dht).  Pure host code; raises RtdmError with the status rtdm_mjpeg_probe refuses the frame with."""
    buf = bytes(stream)
    info = B.MJPEGInfo()
    B.check(B.lib().rtdm_mjpeg_probe(buf, len(buf), C.byref(info)), "rtdm_mjpeg_probe")
    return {n: getattr(info, n) for n, _ in B.MJPEGInfo._fields_}


class HIPMJPEGDecoder(Handle):
    """The reference's DecoderDevice (include/decoder/decoder.h, estimator.cpp:24-27) on the device: baseline MJPEG frames ->
    interleaved RGB, byte for byte what libjpeg gives with its defaults (JDCT_ISLOW, fancy upsampling).

    width x height: the largest frame; max_stream_bytes: the longest stream (SOI .. EOI).  split: the bytes per subsequence a
    frame without restart intervals is cut into, one lane each (rtdm_mjpeg_set_split): None or -1 = the built-in default,
    0 = off, 8 .. 65536."""
    _destroy = "rtdm_mjpeg_destroy"

    def __init__(self, width, height, max_batch=1, max_stream_bytes=None, device=0, split=None):
        self.width, self.height, self.max_batch, self.device = int(width), int(height), int(max_batch), device
        self.max_stream_bytes = int(max_stream_bytes) if max_stream_bytes else max(4096, self.width * self.height * 3)
        self._h = C.c_void_p()
        B.check(B.lib().rtdm_mjpeg_create(self.width, self.height, self.max_batch, self.max_stream_bytes, device,
                                          C.byref(self._h)), "rtdm_mjpeg_create")
        if split is not None:
            self.split = split

    @property
    def split(self):
        v = C.c_int()
        B.check(B.lib().rtdm_mjpeg_get_split(self._h, C.byref(v)), "rtdm_mjpeg_get_split")
        return v.value

    @split.setter
    def split(self, subsequence_bytes):
        B.check(B.lib().rtdm_mjpeg_set_split(self._h, -1 if subsequence_bytes is None else int(subsequence_bytes)),
                "rtdm_mjpeg_set_split")

    def split_stats(self):
        """(frames decoded the split way, their subsequences, the most rounds one took) since creation.  Synchronises the stream
        of the last call."""
        f, n, r = C.c_long(), C.c_long(), C.c_int()
        B.check(B.lib().rtdm_mjpeg_get_split_stats(self._h, C.byref(f), C.byref(n), C.byref(r)), "rtdm_mjpeg_get_split_stats")
        return f.value, n.value, r.value

    def decode(self, stream, out=None):
        """bytes -> H x W x 3 uint8 (host to host, synchronous); the size comes from the frame's own header."""
        buf = bytes(stream)
        info = mjpeg_probe(buf)
        W, H = info["width"], info["height"]
        if out is None:
            out = np.empty((H, W, 3), np.uint8)
        assert out.dtype == np.uint8 and out.shape == (H, W, 3) and out.strides[1] == 3 and out.strides[2] == 1
        B.check(B.lib().rtdm_mjpeg_decode(self._h, buf, len(buf), W, H, out.ctypes.data, out.strides[0]), "rtdm_mjpeg_decode")
        return out

    def decode_batch(self, streams, out=None, status=None, stream=None):
        """list of bytes (frames of one size and sampling) -> torch uint8 [n, H, W, 3] on the device, enqueued on `stream`
        (None = the null stream) and not synchronised.  out: a tensor to fill; its strides give pitch and frame stride.
        status (optional): torch int32 [n], 0 or -8 (damaged entropy data) per frame."""
        import torch
        bufs = [bytes(s) for s in streams]
        n = len(bufs)
        info = mjpeg_probe(bufs[0])
        W, H = info["width"], info["height"]
        if out is None:
            out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda:%d" % self.device)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (n, H, W, 3) and out.stride(3) == 1 and out.stride(2) == 3
        if status is not None:
            assert status.dtype == torch.int32 and status.numel() == n and status.is_contiguous()
        ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in bufs])
        lens = (C.c_size_t * n)(*[len(b) for b in bufs])
        B.check(B.lib().rtdm_mjpeg_decode_batch_device(self._h, n, ptrs, lens, W, H, out.data_ptr(), out.stride(1), out.stride(0),
                                                       status.data_ptr() if status is not None else None, stream),
                "rtdm_mjpeg_decode_batch_device")
        return out

    def compute(self, matcher, rectifier, left, right):
        """estimator.cpp:24-36 + 56: the two cameras' MJPEG frames -> x16 disparity of the rectified, cropped pair."""
        l, r = bytes(left), bytes(right)
        rw, rh = rectifier.roi[2], rectifier.roi[3]
        disp = np.empty((rh, rw), np.int16)
        B.check(B.lib().rtdm_bm_compute_mjpeg(matcher._h, rectifier._h, self._h, l, len(l), r, len(r), rectifier.width,
                                              rectifier.height, disp.ctypes.data, rw * 2), "rtdm_bm_compute_mjpeg")
        return disp
