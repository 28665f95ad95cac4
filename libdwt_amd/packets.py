"""Wavelet packet transforms of row and image batches (include/libdwt_hip.h): every node is split again at
every level, not only the L node.  A submodule of its own: import it as ``from libdwt_amd import packets``.

    packets.wp1d_batch(dwt.CDF97_S, False, x, x, 4 * N, 4, n_lines, N, levels)   # in place, leaves in natural order
    packets.wp_features1d_batch("wps", x, 4 * N, 4, n_lines, N, levels, packets.FREQUENCY, fv, 1 << levels)

Pointers are numpy arrays, torch tensors or integer addresses, host or device memory, as everywhere in libdwt_amd.
"""
import ctypes as C

from . import CDF53_S, CDF97_S, INTERP53_S, DwtError, _addr, _check, feature_mask, lib

_I, _P, _S, _F = C.c_int, C.c_void_p, C.c_size_t, C.c_float
_IP = C.POINTER(_I)

WAVELETS = (CDF97_S, CDF53_S, INTERP53_S)
NATURAL, FREQUENCY = 0, 1  # node order of the feature entries
MAX_LEVELS_2D = 8
MAX_FEATURE_NODES = 96  # FEAT_MAX_BANDS: level <= 6 in 1-D, <= 3 in 2-D

lib.dwt_hip_wp_nodes.argtypes = [_I, _I, _IP, _IP]
lib.dwt_hip_wp_nodes.restype = _I
lib.dwt_hip_wp_freq_order.argtypes = [_I, _IP]
lib.dwt_hip_wp_freq_order.restype = _I
lib.dwt_hip_wp1d_batch.argtypes = [_I, _I, _P, _P, _S, _S, _I, _I, _I]
lib.dwt_hip_wp1d_batch.restype = _I
lib.dwt_hip_wp2d_batch.argtypes = [_I, _I, _P, _P, _S, _I, _I, _I, _I, _I, _I]
lib.dwt_hip_wp2d_batch.restype = _I
lib.dwt_hip_wp_features1d_batch.argtypes = [C.c_uint, _P, _S, _S, _I, _I, _I, _I, _F, _P, _S]
lib.dwt_hip_wp_features1d_batch.restype = _I
lib.dwt_hip_wp_features2d_batch.argtypes = [C.c_uint, _P, _S, _I, _I, _I, _I, _I, _I, _F, _P, _S]
lib.dwt_hip_wp_features2d_batch.restype = _I


def wp_nodes(size, level):
    """dwt_hip_wp_nodes: ([start], [len]) of the 2^level nodes of `level` of a line of `size` samples, natural order."""
    n = lib.dwt_hip_wp_nodes(size, level, None, None)
    if n < 0:
        raise DwtError("wp_nodes: level %d of a line of %d samples" % (level, size))
    start, length = (_I * n)(), (_I * n)()
    lib.dwt_hip_wp_nodes(size, level, start, length)
    return list(start), list(length)


def wp_freq_order(level):
    """dwt_hip_wp_freq_order: perm[f] = natural index of the node whose band is the f-th lowest (the Gray code)."""
    n = lib.dwt_hip_wp_freq_order(level, None)
    if n < 0:
        raise DwtError("wp_freq_order: level %d" % level)
    perm = (_I * n)()
    lib.dwt_hip_wp_freq_order(level, perm)
    return list(perm)


def wp1d_batch(wavelet, inverse, src, dst, line_stride, elem_stride, n_lines, size, levels):
    """dwt_hip_wp1d_batch: `levels` packet levels of n_lines rows (1 <= levels <= floor(log2 size)); src == dst is in
    place.  Device rows of up to 8192 samples take one launch."""
    _check(lib.dwt_hip_wp1d_batch(wavelet, 1 if inverse else 0, _addr(src), _addr(dst), line_stride, elem_stride, n_lines, size,
                                  levels), "dwt_hip_wp1d_batch")


def wp2d_batch(wavelet, inverse, src, dst, batch_stride, batch, stride_x, stride_y, size_x, size_y, levels):
    """dwt_hip_wp2d_batch: `levels` packet levels of a batch of images (1 <= levels <= min(floor(log2(min size)), 8));
    src == dst is in place.  Dense device images take one launch per level."""
    _check(lib.dwt_hip_wp2d_batch(wavelet, 1 if inverse else 0, _addr(src), _addr(dst), batch_stride, batch, stride_x, stride_y,
                                  size_x, size_y, levels), "dwt_hip_wp2d_batch")


def wp_features1d_batch(features, ptr, line_stride, elem_stride, n_lines, size, level, order, fv, fv_stride, p=2.0):
    """dwt_hip_wp_features1d_batch: the statistics of every node of `level` of transformed packet rows; per row one block
    of 2^level floats per feature of the mask, node order NATURAL or FREQUENCY."""
    _check(lib.dwt_hip_wp_features1d_batch(feature_mask(features), _addr(ptr), line_stride, elem_stride, n_lines, size, level,
                                           order, float(p), _addr(fv), fv_stride), "dwt_hip_wp_features1d_batch")


def wp_features2d_batch(features, ptr, batch_stride, batch, stride_x, size_x, size_y, level, order, fv, fv_stride, p=2.0):
    """dwt_hip_wp_features2d_batch: the same for images; node (ky, kx) at ky * 2^level + kx of a feature's block."""
    _check(lib.dwt_hip_wp_features2d_batch(feature_mask(features), _addr(ptr), batch_stride, batch, stride_x, size_x, size_y,
                                           level, order, float(p), _addr(fv), fv_stride), "dwt_hip_wp_features2d_batch")
