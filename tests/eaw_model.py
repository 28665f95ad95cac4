"""A numpy restatement of libdwt's edge-avoiding CDF 5/3 wavelets (EAW, Fattal 2009), written from the reference's
semantics (src/libdwt.c:11070-11240 line steps, 11868-12000 inverse, 16602-16800 / 17932 / 18373 drivers), and a
ctypes binding of the reference's own dwt_eaw53_* where it was built.

float32 numpy arithmetic rounds every operation once, like the reference's C without contraction.  |d|^alpha is exact
for alpha 1 and 0; any other alpha is computed in double and rounded once to float (what the GPU kernels do; glibc's
powf differs from it by at most 1 ulp)."""
import ctypes as C
import os

import numpy as np

S1 = np.float32(1.41421356237309504880)  # dwt_cdf53_s1_s
S2 = np.float32(0.70710678118654752440)  # dwt_cdf53_s2_s
EPS = np.float32(1.0e-5)
TWO = np.float32(2)


def ceil_div_pow2(i, j):
    return (i + (1 << j) - 1) >> j


def ceil_log2(x):
    """src/inline.h:443 (32 for x == 0)."""
    if x == 0:
        return 32
    n = 0
    while n < 31 and (1 << n) < x:
        n += 1
    return n


def levels(inverse, sox, soy, j_max, decompose_one):
    lim = ceil_log2(max(sox, soy) if decompose_one else min(sox, soy))
    if not inverse:
        return lim if (j_max < 0 or j_max > lim) else j_max
    return j_max if 0 <= j_max < lim else lim


def weights(a, b, alpha):
    d = np.abs(a - b)
    if alpha == 0:
        p = np.ones_like(d)
    elif alpha == 1:
        p = d
    else:
        with np.errstate(all="ignore"):
            p = np.power(d.astype(np.float64), float(alpha)).astype(np.float32)
    with np.errstate(all="ignore"):
        return np.float32(1) / (p + EPS)


def fwd_lines(X, alpha):
    """Forward pass over the rows of X (lines x N): (result in sample order, weights lines x N; NaN where the
    reference writes nothing)."""
    X = np.asarray(X, dtype=np.float32)
    L, N = X.shape
    w = np.full((L, N), np.nan, dtype=np.float32)
    if N < 2:
        return X * S1, w
    W = weights(X[:, :-1], X[:, 1:], alpha)
    x = X.copy()
    with np.errstate(all="ignore"):
        i = np.arange(1, N - 1, 2)
        wl, wr = W[:, i - 1], W[:, i]
        x[:, i] = X[:, i] - (wl * X[:, i - 1] + wr * X[:, i + 1]) / (wl + wr)
        e = W[:, N - 2]
        if N % 2 == 0:
            x[:, N - 1] = X[:, N - 1] - (e * X[:, N - 2] + e * X[:, N - 2]) / (e + e)
        else:
            x[:, N - 1] = X[:, N - 1] + (e * x[:, N - 2] + e * x[:, N - 2]) / (TWO * (e + e))
        w0 = W[:, 0]
        x[:, 0] = X[:, 0] + (w0 * x[:, 1] + w0 * x[:, 1]) / (TWO * (w0 + w0))
        i = np.arange(2, N - 1, 2)
        wl, wr = W[:, i - 1], W[:, i]
        x[:, i] = X[:, i] + (wl * x[:, i - 1] + wr * x[:, i + 1]) / (TWO * (wl + wr))
        x[:, 0::2] *= S1
        x[:, 1::2] *= S2
    w[:, :-1] = W
    w[:, -1] = 0
    return x, w


def inv_lines(T, W):
    """Inverse pass: T (lines x N) in sample order, W the forward's weights of these lines."""
    t = np.array(T, dtype=np.float32)
    L, N = t.shape
    if N < 2:
        return t * S2
    W = np.asarray(W, dtype=np.float32)
    with np.errstate(all="ignore"):
        t[:, 0::2] *= S2
        t[:, 1::2] *= S1
        x = t.copy()
        i = np.arange(2, N - 1, 2)
        wl, wr = W[:, i - 1], W[:, i]
        x[:, i] = t[:, i] - (wl * t[:, i - 1] + wr * t[:, i + 1]) / (TWO * (wl + wr))
        w0 = W[:, 0]
        x[:, 0] = t[:, 0] - (w0 * t[:, 1] + w0 * t[:, 1]) / (TWO * (w0 + w0))
        e = W[:, N - 2]
        if N % 2:
            x[:, N - 1] = t[:, N - 1] - (e * t[:, N - 2] + e * t[:, N - 2]) / (TWO * (e + e))
        else:
            x[:, N - 1] = t[:, N - 1] + (e * x[:, N - 2] + e * x[:, N - 2]) / (e + e)
        i = np.arange(1, N - 1, 2)
        wl, wr = W[:, i - 1], W[:, i]
        x[:, i] = t[:, i] + (wl * x[:, i - 1] + wr * x[:, i + 1]) / (wl + wr)
    return x


def mallat_fwd(img, size_i=None, j_max=-1, decompose_one=0, zero_padding=0, alpha=1.0):
    """dwt_eaw53_2f_s on img (soy x sox, the outer frame), in place.  Returns (j, wH, wV); wV[k] is (columns, rows)."""
    soy, sox = img.shape
    siy, six = size_i or (soy, sox)
    J = levels(False, sox, soy, j_max, decompose_one)
    wH, wV = [], []
    for j in range(J):
        Wo, Ho, Wd, Hd = ceil_div_pow2(sox, j), ceil_div_pow2(soy, j), ceil_div_pow2(sox, j + 1), ceil_div_pow2(soy, j + 1)
        Wi, Hi = ceil_div_pow2(six, j), ceil_div_pow2(siy, j)
        out, w = fwd_lines(img[:Ho, :Wi], alpha)
        img[:Ho, :(Wi + 1) // 2] = out[:, 0::2]
        img[:Ho, Wd:Wd + Wi // 2] = out[:, 1::2]
        wH.append(w)
        out, w = fwd_lines(img[:Hi, :Wo].T, alpha)
        img[:(Hi + 1) // 2, :Wo] = out[:, 0::2].T
        img[Hd:Hd + Hi // 2, :Wo] = out[:, 1::2].T
        wV.append(w)
        if zero_padding:
            img[:Ho, (Wi + 1) // 2:Wd] = 0
            img[:Ho, Wd + Wi // 2:Wo] = 0
            img[(Hi + 1) // 2:Hd, :Wo] = 0
            img[Hd + Hi // 2:Ho, :Wo] = 0
    return J, wH, wV


def mallat_inv(img, wH, wV, size_i=None, j_max=-1, decompose_one=0, zero_padding=0):
    """dwt_eaw53_2i_s on img, in place."""
    soy, sox = img.shape
    siy, six = size_i or (soy, sox)
    for j in range(levels(True, sox, soy, j_max, decompose_one), 0, -1):
        Ws, Hs, Wo, Ho = ceil_div_pow2(sox, j), ceil_div_pow2(soy, j), ceil_div_pow2(sox, j - 1), ceil_div_pow2(soy, j - 1)
        Wi, Hi = ceil_div_pow2(six, j - 1), ceil_div_pow2(siy, j - 1)
        T = np.empty((Wo, Hi), dtype=np.float32)
        T[:, 0::2] = img[:(Hi + 1) // 2, :Wo].T
        T[:, 1::2] = img[Hs:Hs + Hi // 2, :Wo].T
        img[:Hi, :Wo] = inv_lines(T, wV[j - 1]).T
        T = np.empty((Ho, Wi), dtype=np.float32)
        T[:, 0::2] = img[:Ho, :(Wi + 1) // 2]
        T[:, 1::2] = img[:Ho, Ws:Ws + Wi // 2]
        img[:Ho, :Wi] = inv_lines(T, wH[j - 1])
        if zero_padding:
            img[:Ho, Wi:Wo] = 0
            img[Hi:Ho, :Wo] = 0
    return j_max


def interleaved_fwd(img, size_i=None, j_max=-1, decompose_one=0, alpha=1.0):
    """dwt_eaw53_2f_inplace_s on img, in place."""
    soy, sox = img.shape
    siy, six = size_i or (soy, sox)
    J = levels(False, sox, soy, j_max, decompose_one)
    wH, wV = [], []
    for j in range(J):
        Wi, Hi = ceil_div_pow2(six, j), ceil_div_pow2(siy, j)
        v = img[::1 << j, ::1 << j][:Hi, :Wi]
        out, w = fwd_lines(v, alpha)
        v[:] = out
        wH.append(w)
        out, w = fwd_lines(v.T, alpha)
        v[:] = out.T
        wV.append(w)
    return J, wH, wV


def interleaved_inv(img, wH, wV, size_i=None, j_max=-1, decompose_one=0):
    soy, sox = img.shape
    siy, six = size_i or (soy, sox)
    for j in range(levels(True, sox, soy, j_max, decompose_one), 0, -1):
        Wi, Hi = ceil_div_pow2(six, j - 1), ceil_div_pow2(siy, j - 1)
        v = img[::1 << (j - 1), ::1 << (j - 1)][:Hi, :Wi]
        v[:] = inv_lines(v.T, wV[j - 1]).T
        v[:] = inv_lines(v, wH[j - 1])
    return j_max


def written(w):
    """Mask of the weight entries the reference writes (lines of one sample get none)."""
    return ~np.isnan(w) if w.shape[1] != 1 else np.zeros(w.shape, dtype=bool)


# ---- the reference itself ---------------------------------------------------------------------------------------------
REF_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libdwt_ref.so")


class RefEaw:
    """dwt_eaw53_* of the compiled reference (oracle/_ref/libdwt_ref.so)."""

    def __init__(self):
        self.lib = C.CDLL(REF_SO)
        self.libc = C.CDLL(None)
        self.libc.free.argtypes = [C.c_void_p]
        P, I = C.c_void_p, C.c_int
        for n in ("dwt_eaw53_2f_s", "dwt_eaw53_2f_inplace_s"):
            getattr(self.lib, n).argtypes = [P, I, I, I, I, I, I, C.POINTER(I), I, I, P, P, C.c_float]
            getattr(self.lib, n).restype = None
        for n in ("dwt_eaw53_2i_s", "dwt_eaw53_2i_inplace_s"):
            getattr(self.lib, n).argtypes = [P, I, I, I, I, I, I, I, I, I, P, P]
            getattr(self.lib, n).restype = None
        self.lib.dwt_eaw53_2f_dummy_s.argtypes = [P, I, I, I, I, I, I, C.POINTER(I), I]
        self.lib.dwt_eaw53_2f_dummy_s.restype = None

    def fwd(self, img, size_i=None, j_max=-1, decompose_one=0, zero_padding=0, alpha=1.0, interleaved=False):
        """In place on the C-contiguous float32 img; returns (j, wH, wV) shaped as mallat_fwd's (NaN where the
        reference writes nothing)."""
        soy, sox = img.shape
        siy, six = size_i or (soy, sox)
        hp, vp = (C.c_void_p * 32)(), (C.c_void_p * 32)()
        j = C.c_int(j_max)
        f = self.lib.dwt_eaw53_2f_inplace_s if interleaved else self.lib.dwt_eaw53_2f_s
        f(img.ctypes.data, img.strides[0], 4, sox, soy, six, siy, C.byref(j), decompose_one, zero_padding, C.cast(hp, C.c_void_p),
          C.cast(vp, C.c_void_p), alpha)
        wH, wV = [], []
        for k in range(j.value):
            Hi, Wi = ceil_div_pow2(siy, k), ceil_div_pow2(six, k)
            if interleaved:
                sh, sv = (Hi, Wi), (Wi, Hi)
            else:
                sh, sv = (ceil_div_pow2(soy, k), Wi), (ceil_div_pow2(sox, k), Hi)
            for p, shape, out in ((hp[k], sh, wH), (vp[k], sv, wV)):
                n = shape[0] * shape[1]
                a = np.ctypeslib.as_array((C.c_float * n).from_address(p)).reshape(shape).copy() if n else np.zeros(shape, np.float32)
                if shape[1] == 1:
                    a[:] = np.nan  # uninitialised in the reference
                out.append(a)
                self.libc.free(p)
        return j.value, wH, wV

    def inv(self, img, wH, wV, size_i=None, j_max=-1, decompose_one=0, zero_padding=0, interleaved=False):
        soy, sox = img.shape
        siy, six = size_i or (soy, sox)
        keep = [np.ascontiguousarray(np.nan_to_num(a, nan=0.0), dtype=np.float32) for a in list(wH) + list(wV)]
        hp = (C.c_void_p * 32)(*[a.ctypes.data for a in keep[:len(wH)]])
        vp = (C.c_void_p * 32)(*[a.ctypes.data for a in keep[len(wH):]])
        f = self.lib.dwt_eaw53_2i_inplace_s if interleaved else self.lib.dwt_eaw53_2i_s
        f(img.ctypes.data, img.strides[0], 4, sox, soy, six, siy, j_max, decompose_one, zero_padding, C.cast(hp, C.c_void_p),
          C.cast(vp, C.c_void_p))

    def dummy(self, sox, soy, j_max, decompose_one):
        j = C.c_int(j_max)
        self.lib.dwt_eaw53_2f_dummy_s(None, 0, 0, sox, soy, sox, soy, C.byref(j), decompose_one)
        return j.value


def have_ref():
    return os.path.exists(REF_SO)


def same_weights(got, want):
    """Equal bits wherever the reference writes a weight (NaN in `want` marks entries it leaves alone)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    m = ~np.isnan(want)
    return np.array_equal(got[m].view(np.uint32), want[m].view(np.uint32))
