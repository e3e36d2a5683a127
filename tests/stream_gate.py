"""A stream held by a host function, for the tests that show that a call enqueues and returns: the function waits on a
threading.Event for at most 3 s and records whether it was released or ran into the bound.  A call that synchronised the stream
would sit out the 3 s (released is False) -- it can never hang."""
import ctypes as C
import threading

HOSTFN = C.CFUNCTYPE(None, C.c_void_p)


class StreamGate:
    """Holds a stream by a host function that waits on an Event for at most 3 s and records how it ended."""

    def __init__(self):
        import torch
        self.hip = C.CDLL([p for p in open("/proc/self/maps").read().split() if "libamdhip64" in p][0])
        self.hip.hipLaunchHostFunc.argtypes = [C.c_void_p, HOSTFN, C.c_void_p]
        self.hip.hipLaunchHostFunc.restype = C.c_int
        self.event, self.released = threading.Event(), None
        self.fn = HOSTFN(self._wait)                                     # kept alive as long as the gate
        self.stream = torch.cuda.Stream()

    def _wait(self, _):
        self.released = self.event.wait(3.0)

    def hold(self):
        assert self.hip.hipLaunchHostFunc(C.c_void_p(self.stream.cuda_stream), self.fn, None) == 0
