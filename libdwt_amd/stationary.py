"""The stationary wavelet transform with a choice of border, and its inverse (include/libdwt_hip.h): what
translation-invariant denoising and multiresolution editing need -- forward under the symmetric border, shrink or zero the
detail planes, and back, the shrinkage applied as the inverse reads the coefficients.  A submodule of its own: import it as
``from libdwt_amd import stationary``.

    st.swt1d_batch(dwt.CDF97_S, x, 4 * N, 4, lines, N, J, H, L, 1, 4 * N * lines, 4 * N, border=st.BORDER_SYMMETRIC)
    st.iswt1d_batch(dwt.CDF97_S, st.BORDER_SYMMETRIC, H, L, 4 * N * lines, 4 * N, lines, N, J, y, 4 * N,
                    ops=[st.BAND_SOFT] * J, params=[thr] * J)

Pointers are numpy arrays, torch tensors or integer addresses, all host memory or all device memory."""
import ctypes as C

import numpy as np

from . import CDF53_S, CDF97_S, WAVELET_ID, DwtError, _addr, _check, lib

_I, _P, _S = C.c_int, C.c_void_p, C.c_size_t

BORDER_REPLICATE, BORDER_SYMMETRIC = 0, 1  # DWT_HIP_SWT_BORDER_*
BAND_KEEP, BAND_ZERO, BAND_SCALE, BAND_HARD, BAND_SOFT, BAND_COMPRESS = range(6)  # DWT_HIP_BAND_* (COMPRESS: not on load)
MAX_LEVELS = 24  # DWT_HIP_SWT_MAX_LEVELS
ISWT2D_FUSED_LEVELS = 5  # DWT_HIP_ISWT2D_FUSED_LEVELS: dense device destinations take one launch per level on levels 0 .. 4

lib.dwt_hip_swt1d_batch_ex.argtypes = [_I, _P, _S, _S, _I, _I, _I, _P, _P, _I, _S, _S, _I]
lib.dwt_hip_swt2d_batch_ex.argtypes = [_I, _P, _S, _I, _I, _I, _I, _I, _I, _P, _P, _I, _S, _S, _I, _I]
lib.dwt_hip_iswt1d_batch.argtypes = [_I, _I, _P, _P, _S, _S, _I, _I, _I, _P, _P, _P, _S, _S]
lib.dwt_hip_iswt2d_batch.argtypes = [_I, _I, _P, _P, _S, _S, _I, _I, _I, _I, _I, _P, _P, _P, _S, _I, _I]
for _n in ("dwt_hip_swt1d_batch_ex", "dwt_hip_swt2d_batch_ex", "dwt_hip_iswt1d_batch", "dwt_hip_iswt2d_batch"):
    getattr(lib, _n).restype = _I


def _wavelet(wavelet):
    w = WAVELET_ID.get(wavelet, wavelet) if isinstance(wavelet, str) else wavelet
    if w not in (CDF97_S, CDF53_S):
        raise DwtError("the stationary transforms take cdf97_s or cdf53_s (got %r)" % (wavelet,))
    return w


def _nonneg(who, *values):
    if min(values) < 0:
        raise DwtError("%s: negative size or stride" % who)


def _tables(ops, params, n, who):
    """the host tables the C entry reads: (ops as int32 or None, params as float32 or None), each of n entries"""
    if ops is None:
        if params is not None:
            raise DwtError("%s: params without ops" % who)
        return None, None
    o = np.ascontiguousarray(ops, np.int32)
    p = None if params is None else np.ascontiguousarray(params, np.float32)
    if o.shape != (n,) or (p is not None and p.shape != (n,)):
        raise DwtError("%s: the operator tables take %d entries, one per detail plane" % (who, n))
    return o, p


def swt1d_batch(wavelet, src, line_stride, elem_stride, n_lines, size, levels, dst_h, dst_l=None, l_mode=0, plane_stride=0,
                dst_line_stride=0, border=BORDER_REPLICATE):
    """dwt_hip_swt1d_batch_ex: libdwt_amd.swt1d_batch with the border rule (BORDER_REPLICATE: that entry's bits)."""
    w = _wavelet(wavelet)
    _nonneg("swt1d_batch", line_stride, elem_stride, n_lines, size, levels, plane_stride, dst_line_stride)
    _check(lib.dwt_hip_swt1d_batch_ex(w, _addr(src), line_stride, elem_stride, n_lines, size, levels, _addr(dst_h),
                                      0 if dst_l is None else _addr(dst_l), l_mode, plane_stride, dst_line_stride, border),
           "dwt_hip_swt1d_batch_ex")


def swt2d_batch(wavelet, src, batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, dst_h, dst_l=None, l_mode=0,
                dst_batch_stride=0, plane_stride=0, dst_stride_x=0, border=BORDER_REPLICATE):
    """dwt_hip_swt2d_batch_ex: libdwt_amd.swt2d_batch with the border rule (BORDER_REPLICATE: that entry's bits)."""
    w = _wavelet(wavelet)
    _nonneg("swt2d_batch", batch_stride, stride_x, stride_y, dst_batch_stride, plane_stride, dst_stride_x)
    _check(lib.dwt_hip_swt2d_batch_ex(w, _addr(src), batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, _addr(dst_h),
                                      0 if dst_l is None else _addr(dst_l), l_mode, dst_batch_stride, plane_stride, dst_stride_x, border),
           "dwt_hip_swt2d_batch_ex")


def iswt1d_batch(wavelet, border, src_h, src_l, plane_stride, src_line_stride, n_lines, size, levels, dst, dst_line_stride,
                 dst_elem_stride=4, ops=None, params=None):
    """dwt_hip_iswt1d_batch: the rows back from the H planes (laid out as swt1d_batch writes dst_h) and the last level's L
    lines.  ops / params: one BAND_* operator and one parameter per level, applied to the H coefficients as they are read
    (None: KEEP everywhere).  Dense device lines of up to 8192 samples take one launch."""
    w = _wavelet(wavelet)
    _nonneg("iswt1d_batch", plane_stride, src_line_stride, dst_line_stride, dst_elem_stride)
    o, p = _tables(ops, params, levels, "iswt1d_batch")
    _check(lib.dwt_hip_iswt1d_batch(w, border, 0 if src_h is None else _addr(src_h), _addr(src_l), plane_stride, src_line_stride, n_lines, size,
                                    levels, None if o is None else o.ctypes.data, None if p is None else p.ctypes.data, _addr(dst),
                                    dst_line_stride, dst_elem_stride), "dwt_hip_iswt1d_batch")


def iswt2d_batch(wavelet, border, src_h, src_l, src_batch_stride, plane_stride, src_stride_x, batch, size_x, size_y, levels, dst,
                 dst_batch_stride, dst_stride_x, dst_stride_y=4, ops=None, params=None):
    """dwt_hip_iswt2d_batch: the images back from the detail planes (laid out as swt2d_batch writes dst_h) and the last
    level's LL of every image.  ops / params: 3 * levels entries, the plane's at index 3*l + k-1 (HL, LH, HH).  Dense device
    destinations take one launch per level on levels 0 .. ISWT2D_FUSED_LEVELS-1, two otherwise."""
    w = _wavelet(wavelet)
    _nonneg("iswt2d_batch", src_batch_stride, plane_stride, src_stride_x, dst_batch_stride, dst_stride_x, dst_stride_y)
    o, p = _tables(ops, params, 3 * levels if levels > 0 else 0, "iswt2d_batch")
    _check(lib.dwt_hip_iswt2d_batch(w, border, 0 if src_h is None else _addr(src_h), _addr(src_l), src_batch_stride, plane_stride, src_stride_x,
                                    batch, size_x, size_y, levels, None if o is None else o.ctypes.data, None if p is None else p.ctypes.data,
                                    _addr(dst), dst_batch_stride, dst_stride_x, dst_stride_y), "dwt_hip_iswt2d_batch")
