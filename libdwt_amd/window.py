"""Windowed and reduced-resolution inverse 2-D transforms (include/libdwt_hip.h): a viewport, a thumbnail
or a crop of a Mallat frame that stays resident on the device, without the full inverse and without a destination as
large as the frame.  A submodule of its own: import it as ``from libdwt_amd import window``.

    regions = window.window_regions(dwt.CDF97_S, W, H, J, 0, x0, y0, 512, 512)     # (3 J + 1, 4): x, y, size_x, size_y
    window.inverse_window_batch(dwt.CDF97_S, frames, 4 * W * H, B, 4 * W, W, H, J, 0, x0, y0, 512, 512, out, 4 * 512 * 512, 4 * 512)
    window.inverse_window_batch(dwt.CDF97_S, frames, 4 * W * H, B, 4 * W, W, H, J, 2, 0, 0, W // 4, H // 4, thumb, W * H // 4, W)

Frames and windows are device memory: torch tensors or integer addresses.  ``window_regions`` is host arithmetic and needs
no device."""
import ctypes as C

import numpy as np

from . import CDF53_I, CDF53_I16, CDF53_S, CDF97_S, INTERP53_S, WAVELET_ID, DwtError, _addr, _cdll, _check, lib

_I, _P, _S = C.c_int, C.c_void_p, C.c_size_t

WAVELETS = (CDF97_S, CDF53_S, INTERP53_S, CDF53_I, CDF53_I16)  # the wavelets with a windowed inverse
HALO = {CDF97_S: 4, CDF53_S: 2, CDF53_I: 2, CDF53_I16: 2, INTERP53_S: 1}  # K: interleaved samples of halo per level
ELEM_BYTES = {CDF97_S: 4, CDF53_S: 4, INTERP53_S: 4, CDF53_I: 4, CDF53_I16: 2}
TILE = 64  # DWT_HIP_WINDOW_TILE: a workgroup of the window kernels owns TILE x TILE samples of a level's region
GRID_BATCH = 4096  # DWT_HIP_WINDOW_GRID_BATCH: frames that one trip of the kernels' batch loop covers
ROUTE_INVERSE, ROUTE_AUTO, ROUTE_KERNELS = 0, 1, 2  # option "window_fused"

_WINDOW = [_I, _I, _I, _I, _I, _I, _I, _I, _I]  # wavelet, size_x, size_y, j_max, discard, x0, y0, w, h
_cdll.dwt_hip_window_regions.argtypes = _WINDOW + [_P]
_cdll.dwt_hip_window_regions.restype = _I
_cdll.dwt_hip_window_route.argtypes = [_I] + _WINDOW
_cdll.dwt_hip_window_route.restype = _I
lib.dwt_hip_inverse_window_batch.argtypes = [_I, _P, _S, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _S, _I]
lib.dwt_hip_inverse_window_batch.restype = _I


def _wavelet(wavelet):
    return WAVELET_ID.get(wavelet, wavelet) if isinstance(wavelet, str) else wavelet


def window_regions(wavelet, size_x, size_y, j_max, discard, x0, y0, w, h):
    """dwt_hip_window_regions -> int32 array (3 J + 1, 4) of {x, y, size_x, size_y}: the rectangle of every subband that
    the window [x0, x0 + w) x [y0, y0 + h) of LL(discard) depends on, in the slot order of band_geometry.  Raises DwtError
    for arguments the entry refuses."""
    out = np.zeros((94, 4), np.int32)  # DWT_HIP_BAND_MAX_SLOTS
    n = _cdll.dwt_hip_window_regions(_wavelet(wavelet), size_x, size_y, j_max, discard, x0, y0, w, h, out.ctypes.data)
    if n < 0:
        raise DwtError("dwt_hip_window_regions refuses wavelet %r, %d x %d, j_max %d, discard %d, window %d x %d at (%d, %d)"
                       % (wavelet, size_x, size_y, j_max, discard, w, h, x0, y0))
    return out[:n].copy()


def region_bytes(wavelet, regions):
    """bytes of coefficients in the rectangles of window_regions"""
    r = np.asarray(regions, np.int64)
    return int((r[:, 2] * r[:, 3]).sum()) * ELEM_BYTES[_wavelet(wavelet)]


def window_route(wavelet, batch, size_x, size_y, j_max, discard, x0, y0, w, h):
    """dwt_hip_window_route: ROUTE_KERNELS or ROUTE_INVERSE, what a call with these arguments takes under the calling
    thread's option "window_fused"."""
    r = _cdll.dwt_hip_window_route(_wavelet(wavelet), batch, size_x, size_y, j_max, discard, x0, y0, w, h)
    if r < 0:
        raise DwtError("dwt_hip_window_route: arguments that dwt_hip_window_regions refuses")
    return r


def inverse_window_batch(wavelet, src, batch_stride, batch, stride_x, size_x, size_y, j_max, discard, x0, y0, w, h, dst,
                         dst_batch_stride, dst_stride_x):
    """dwt_hip_inverse_window_batch: element (y, x) of window b at dst + b * dst_batch_stride + y * dst_stride_x is bit for bit
    element (y0 + y, x0 + x) of the inverse of frame b at J - discard levels on its top-left LL(discard)-sized rectangle.
    Strides in bytes; ordered on the context's stream, not synchronised."""
    _check(lib.dwt_hip_inverse_window_batch(_wavelet(wavelet), _addr(src), batch_stride, batch, stride_x, size_x, size_y, j_max, discard,
                                            x0, y0, w, h, _addr(dst), dst_batch_stride, dst_stride_x), "dwt_hip_inverse_window_batch")
