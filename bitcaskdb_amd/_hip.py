"""Device buffers through the HIP runtime libbcw.so itself links: hipMalloc / hipMemcpy / hipFree via ctypes, for
the host mirror's device-resident objects (write.ActiveWal and the staged arrays of Index.write)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L  # noqa: F401  (loads libbcw.so and with it its HIP runtime)

_rt = None
H2D, D2H = 1, 2


def _hip():
    global _rt
    if _rt is None:
        for name in ("libamdhip64.so.7", "libamdhip64.so"):  # the runtime already in the process
            try:
                _rt = C.CDLL(name)
                break
            except OSError:
                continue
        if _rt is None:
            raise ImportError("the HIP runtime (libamdhip64) is not loadable")
        _rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _rt.hipFree.argtypes = [C.c_void_p]
        _rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _rt


def _chk(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: hipError {rc}")


class DevMem:
    """nbytes of device memory on the current device (hipMalloc), freed with the object"""

    def __init__(self, nbytes: int):
        self.n = max(int(nbytes), 1)
        self.p = C.c_void_p()
        _chk(_hip().hipMalloc(C.byref(self.p), self.n), "hipMalloc")

    @property
    def ptr(self) -> int:
        return int(self.p.value)

    def upload(self, data, off: int = 0):
        a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray))
                                 else data)
        if a.nbytes:
            _chk(_hip().hipMemcpy(C.c_void_p(self.ptr + off), a.ctypes.data_as(C.c_void_p), a.nbytes, H2D),
                 "hipMemcpy H2D")
        return self

    def download(self, nbytes: int, off: int = 0, dtype=np.uint8) -> np.ndarray:
        """blocking copy; the caller has synchronised the stream that produced the bytes"""
        out = np.empty(int(nbytes), dtype=np.uint8)
        if nbytes:
            _chk(_hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr + off), int(nbytes), D2H),
                 "hipMemcpy D2H")
        return out.view(dtype)

    def free(self):
        if self.p and self.p.value:
            _hip().hipFree(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
