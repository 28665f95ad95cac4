"""The pixel front end (include/libdwt_hip.h): pictures of 8- / 16-bit unsigned pixels <-> the planes the
2-D transforms take, with the DC level shift and the RCT / ICT of ITU-T T.800 Annex G.  A submodule of its own: import it
as ``from libdwt_amd import pixels``.

    # 3 interleaved RGB8 pictures -> int16 Y, U, V planes, transformed (reversible 5/3), and back
    j = pixels.picture_forward_batch(dwt.CDF53_I16, pixels.U8, pix, 3 * W * H, 3 * W, 3, 1, 3, 3, pixels.RGB, 8, 128, 1.0,
                                     pixels.RCT, planes, 2 * W * H, 2 * W, W, H, -1)
    pixels.picture_inverse_batch(dwt.CDF53_I16, pixels.U8, pix, ..., pixels.RCT, planes, 2 * W * H, 2 * W, W, H, j)

Pointers are numpy arrays, torch tensors or integer addresses; each side host or device memory on its own.
"""
import ctypes as C

from . import CDF53_I, CDF53_I16, CDF53_S, CDF97_H, CDF97_I, CDF97_S, INTERP53_S, DwtError, _addr, _check, lib

_I, _P, _S, _F = C.c_int, C.c_void_p, C.c_size_t, C.c_float

U8, U16 = 0, 1  # pixel formats (DWT_HIP_PIX_*)
RGB, BGR = 0, 1  # which of the first three channels is R
NONE, RCT, ICT = 0, 1, 2  # component transforms
I16, I32, H, S = 0, 1, 2, 3  # plane types (DWT_HIP_PLANE_*)
PIXEL_BYTES = {U8: 1, U16: 2}
PLANE_BYTES = {I16: 2, I32: 4, H: 2, S: 4}
PLANE_DTYPE = {I16: "int16", I32: "int32", H: "float16", S: "float32"}
PLANE_OF_WAVELET = {CDF53_I16: I16, CDF53_I: I32, CDF97_I: I32, CDF97_H: H, CDF97_S: S, CDF53_S: S, INTERP53_S: S}
COLOURS_OF_PLANE = {I16: (NONE, RCT), I32: (NONE, RCT), H: (NONE, ICT), S: (NONE, ICT)}
PIXELS_PER_LANE = 16  # consecutive pixels of a row per lane: a wave spans 64 * 16 pixels
GRID_ROWS, GRID_BATCH = 16384, 4096  # rows / pictures that one trip of the kernel's loops covers
WIDE_PIX, WIDE_PLANES = 1, 2  # pixels_route: that side moves by 16-byte accesses

_PIX = [_I, _P, _S, _S, _S, _S, _I, _I, _I, _I, _I, _F, _I]  # fmt, pix, four strides, batch, channels, order, depth, offset, scale, colour
_PLANES = [_P, _S, _S, _I, _I]  # planes, plane_stride, plane_row_pitch, size_x, size_y
lib.dwt_hip_pixels_to_planes_batch.argtypes = _PIX + [_I] + _PLANES
lib.dwt_hip_planes_to_pixels_batch.argtypes = _PIX + [_I] + _PLANES
lib.dwt_hip_picture_forward_batch.argtypes = [_I] + _PIX + _PLANES + [C.POINTER(_I)]
lib.dwt_hip_picture_inverse_batch.argtypes = [_I] + _PIX + _PLANES + [_I]
lib.dwt_hip_pixels_route.argtypes = [_I, _I, _P, _S, _S, _S, _S, _I, _I, _I, _P, _S, _S, _I, _I]
for _n in ("dwt_hip_pixels_to_planes_batch", "dwt_hip_planes_to_pixels_batch", "dwt_hip_picture_forward_batch",
           "dwt_hip_picture_inverse_batch", "dwt_hip_pixels_route"):
    getattr(lib, _n).restype = _I


def pixels_to_planes_batch(fmt, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, order, depth, offset,
                           scale, colour, plane_type, planes, plane_stride, plane_row_pitch, size_x, size_y):
    """dwt_hip_pixels_to_planes_batch: plane (b, c) = the channel (after RCT / ICT: the component) c of picture b."""
    _check(lib.dwt_hip_pixels_to_planes_batch(fmt, _addr(pix), pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels,
                                              order, depth, offset, scale, colour, plane_type, _addr(planes), plane_stride,
                                              plane_row_pitch, size_x, size_y), "dwt_hip_pixels_to_planes_batch")


def planes_to_pixels_batch(fmt, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, order, depth, offset,
                           scale, colour, plane_type, planes, plane_stride, plane_row_pitch, size_x, size_y):
    """dwt_hip_planes_to_pixels_batch: the same arguments, the pixels written (`scale` the reciprocal of the forward one)."""
    _check(lib.dwt_hip_planes_to_pixels_batch(fmt, _addr(pix), pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels,
                                              order, depth, offset, scale, colour, plane_type, _addr(planes), plane_stride,
                                              plane_row_pitch, size_x, size_y), "dwt_hip_planes_to_pixels_batch")


def picture_forward_batch(wavelet, fmt, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, order, depth,
                          offset, scale, colour, planes, plane_stride, plane_row_pitch, size_x, size_y, j_max=-1):
    """dwt_hip_picture_forward_batch: the conversion and the batched 2-D transform of the batch * channels planes; returns
    the levels done."""
    j = _I(j_max)
    _check(lib.dwt_hip_picture_forward_batch(wavelet, fmt, _addr(pix), pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch,
                                             channels, order, depth, offset, scale, colour, _addr(planes), plane_stride,
                                             plane_row_pitch, size_x, size_y, C.byref(j)), "dwt_hip_picture_forward_batch")
    return j.value


def picture_inverse_batch(wavelet, fmt, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, order, depth,
                          offset, scale, colour, planes, plane_stride, plane_row_pitch, size_x, size_y, j_max):
    """dwt_hip_picture_inverse_batch: the planes (only read) through the inverse transform to pixels."""
    _check(lib.dwt_hip_picture_inverse_batch(wavelet, fmt, _addr(pix), pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch,
                                             channels, order, depth, offset, scale, colour, _addr(planes), plane_stride,
                                             plane_row_pitch, size_x, size_y, j_max), "dwt_hip_picture_inverse_batch")


def pixels_route(fmt, inverse, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, plane_type, planes,
                 plane_stride, plane_row_pitch, size_x, size_y):
    """dwt_hip_pixels_route: WIDE_PIX | WIDE_PLANES -- the sides a call with these addresses moves by 16-byte accesses."""
    r = lib.dwt_hip_pixels_route(fmt, 1 if inverse else 0, _addr(pix), pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch,
                                 channels, plane_type, _addr(planes), plane_stride, plane_row_pitch, size_x, size_y)
    if r < 0:
        raise DwtError("dwt_hip_pixels_route: " + lib.dwt_hip_last_error().decode(errors="replace"))
    return r
