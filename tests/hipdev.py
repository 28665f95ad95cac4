"""What the GPU tests of the line-batch drivers share: a numpy array's copy in device memory, and the launch counter.
A plain module like oraclelib.py; each test file keeps its own `dwt` fixture, because each resets its own options."""
import numpy as np


class Dev:
    """A host array copied to device memory (dwt_hip_malloc), freed by free() or with the object."""

    def __init__(self, dwt, arr):
        a = np.ascontiguousarray(arr)
        self.dwt, self.shape, self.dtype = dwt, a.shape, a.dtype
        self.ptr = dwt.lib.dwt_hip_malloc(max(a.nbytes, 16))
        assert self.ptr
        if a.nbytes:
            assert dwt.lib.dwt_hip_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes) == 0

    def data_ptr(self):
        """the address as a tensor would give it: the package's wrappers take the object itself"""
        return self.ptr

    def get(self, shape=None, dtype=None):
        """the buffer's content: as the array it was made from, or its first bytes as `shape` of `dtype`"""
        out = np.empty(self.shape if shape is None else shape, dtype or self.dtype)
        self.dwt.sync()
        if out.nbytes:
            assert self.dwt.lib.dwt_hip_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes) == 0
        return out

    def free(self):
        if self.ptr:
            self.dwt.lib.dwt_hip_free(self.ptr)
        self.ptr = None

    __del__ = free


def launches(dwt, f):
    """kernel launches the context counted while f ran"""
    n0 = dwt.get_option("stat_launches")
    f()
    return dwt.get_option("stat_launches") - n0
