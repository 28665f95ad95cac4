"""What the GPU tests of the line-batch drivers share: a numpy array's copy in device memory, the launch counter, and a
caller-owned LL workspace between guards (tests/test_hip_scratch.py).
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


# ---- a caller-owned LL workspace between guards ----------------------------------------------------------
GUARD = 64 << 10       # bytes in front of and behind each band.  A choice, not a measurement: a stray LL row at the shapes of the tests is about 2 KiB
CANARY = 0x5CA1AB1E    # what the guards hold
POISON = 0xFFFFFFFF    # what the bands hold before a call: NaN as binary32, as both binary16 halves and as binary64; -1 as ints
ELEM_SIZE = {"cdf97_d": 8, "cdf53_d": 8, "cdf53_i16": 2, "cdf97_h": 2}  # the others: 4


def ll_band_bytes(k, batch, w, h, es):
    """include/libdwt_hip.h, dwt_hip_set_workspace: the bytes of band k (0: the level-1 band, 1: the level-2 band)"""
    wk, hk = (w + (2 << k) - 1) >> (k + 1), (h + (2 << k) - 1) >> (k + 1)
    return (wk + 3) // 4 * 4 * hk * es * batch + 64


class GuardedWorkspace:
    """The two LL bands of dwt_hip_set_workspace for a batch of `batch` images of w x h of `wavelet`, each allocated as
    [GUARD | band of exactly the documented size | GUARD] and installed.  `short`: bytes by which the size TOLD to the library
    falls short of the documented one, per band (the size rule's test).  arm(): the bands to `poison`, the guards to CANARY;
    check(): asserts every guard word intact and returns the two bands as uint32 words; close(): hands the workspace back
    and frees it."""

    def __init__(self, dwt, wavelet, batch, w, h, short=(0, 0), poison=POISON):
        self.dwt, self.poison = dwt, poison
        self.es = ELEM_SIZE.get(wavelet, 4)
        self.bytes = [ll_band_bytes(k, batch, w, h, self.es) for k in range(2)]
        assert all(b % 4 == 0 for b in self.bytes)
        self.bufs = [Dev(dwt, np.zeros((2 * GUARD + b) // 4, np.uint32)) for b in self.bytes]
        self.arm()
        rc = dwt.lib.dwt_hip_set_workspace(self.bufs[0].ptr + GUARD, self.bytes[0] - short[0], self.bufs[1].ptr + GUARD, self.bytes[1] - short[1])
        assert rc == 0, dwt.last_error()

    def arm(self):
        self.dwt.sync()
        for buf, b in zip(self.bufs, self.bytes):
            host = np.full((2 * GUARD + b) // 4, CANARY, np.uint32)
            host[GUARD // 4:(GUARD + b) // 4] = self.poison
            assert self.dwt.lib.dwt_hip_memcpy_h2d(buf.ptr, host.ctypes.data, host.nbytes) == 0

    def check(self):
        bands = []
        for k, (buf, b) in enumerate(zip(self.bufs, self.bytes)):
            host = buf.get()
            front, back = host[:GUARD // 4], host[(GUARD + b) // 4:]
            assert (front == CANARY).all(), "band %d: %d words written in front of it, the last %d bytes before its start" % (
                k, int((front != CANARY).sum()), 4 * (len(front) - int(np.flatnonzero(front != CANARY)[0])))
            assert (back == CANARY).all(), "band %d: %d words written behind it, up to %d bytes past its end" % (
                k, int((back != CANARY).sum()), 4 * (int(np.flatnonzero(back != CANARY)[-1]) + 1))
            bands.append(host[GUARD // 4:(GUARD + b) // 4].copy())
        return bands

    def close(self):
        if self.bufs:
            assert self.dwt.lib.dwt_hip_set_workspace(None, 0, None, 0) == 0, self.dwt.last_error()
            for buf in self.bufs:
                buf.free()
        self.bufs = []
