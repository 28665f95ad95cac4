"""Embedded bit-plane streams of code-blocks (include/libdwt_hip.h): every code-block of int16 / int32
index planes packed on the device into a sign plane and as many magnitude planes as its largest magnitude has bits, most
significant first, in 64-bit words of 64 samples, the blocks in resolution order -- and unpacked again, with the least
significant planes left out on request.  A submodule of its own: import it as ``from libdwt_amd import bitplanes``.

    off = bitplanes.count_batch(quant.I16, idx, 2 * W * H, 2 * W, B, W, H, J, 6, 6)        # (B, S + 1) uint32, the sizing call
    cap = int(off[:, -1].max())
    bitplanes.pack_batch(quant.I16, idx, 2 * W * H, 2 * W, B, W, H, J, 6, 6, words, cap, offsets)
    bitplanes.unpack_batch(quant.I16, words, cap, offsets, idx, 2 * W * H, 2 * W, B, W, H, J, 6, 6, drop=1, mode=bitplanes.SHIFT)

Pointers are numpy arrays, torch tensors or integer addresses; the planes, the words and the offsets each host or device
memory on their own.
"""
import ctypes as C

import numpy as np

from . import DwtError, _addr, _check, lib

_I, _P, _S = C.c_int, C.c_void_p, C.c_size_t

I16, I32 = 0, 1  # index types (DWT_HIP_INDEX_*)
KEEP, SHIFT = 0, 1  # what unpack stores when planes are dropped (DWT_HIP_BITPLANE_*)
GRID_BLOCKS = 16384  # code-blocks that one trip of the pack / unpack kernels' loops covers
GRID_BATCH = 4096  # frames that one trip of the scan's loop covers

_FRAMES = [_I, _P, _S, _S, _I, _I, _I, _I, _I, _I]  # type, address, batch stride, row pitch, batch, size_x, size_y, j_max, cb exponents
lib.dwt_hip_bitplane_bands.argtypes = [_I, _I, _I, _I, _I, _P]
lib.dwt_hip_bitplane_block.argtypes = [_P, _I, _I, _I, _I, _P, _P, _P, _P]
lib.dwt_hip_bitplane_words.argtypes = [_I, _I]
lib.dwt_hip_bitplane_pack_batch.argtypes = _FRAMES + [_P, _S, _P]
lib.dwt_hip_bitplane_unpack_batch.argtypes = [_I, _P, _S, _P, _P, _S, _S, _I, _I, _I, _I, _I, _I, _I, _I]
lib.dwt_hip_bitplane_route.argtypes = _FRAMES
for _n in ("dwt_hip_bitplane_bands", "dwt_hip_bitplane_block", "dwt_hip_bitplane_words", "dwt_hip_bitplane_pack_batch",
           "dwt_hip_bitplane_unpack_batch", "dwt_hip_bitplane_route"):
    getattr(lib, _n).restype = _I


def bands(size_x, size_y, j_max, cb_log2_x, cb_log2_y):
    """dwt_hip_bitplane_bands -> int32 array (3 J + 2, 5): x, y, size_x, size_y and first stream block of every band in
    stream order; the last row holds the blocks of a frame."""
    levels = lib.dwt_hip_band_levels(size_x, size_y, j_max)
    if levels < 0:
        raise DwtError("bit-planes: bad sizes %d x %d (dwt_hip_band_levels refuses them)" % (size_x, size_y))
    table = np.zeros((3 * levels + 2, 5), np.int32)
    if lib.dwt_hip_bitplane_bands(size_x, size_y, j_max, cb_log2_x, cb_log2_y, table.ctypes.data) != len(table) - 1:
        raise DwtError("dwt_hip_bitplane_bands: bad arguments (%d x %d, code-blocks 2^%d x 2^%d)" % (size_x, size_y, cb_log2_x, cb_log2_y))
    return table


def block(table, cb_log2_x, cb_log2_y, s):
    """dwt_hip_bitplane_block -> (x, y, w, h) of stream block s of a table of bands()."""
    table = np.ascontiguousarray(table, np.int32)
    out = (C.c_int * 4)()
    ptrs = [C.addressof(out) + 4 * k for k in range(4)]
    if lib.dwt_hip_bitplane_block(table.ctypes.data, len(table) - 1, cb_log2_x, cb_log2_y, s, *ptrs) != 0:
        raise DwtError("dwt_hip_bitplane_block: no block %d" % s)
    return tuple(out)


def words_of(n, p):
    """dwt_hip_bitplane_words: the words of a block of n samples whose largest magnitude has p bits."""
    r = lib.dwt_hip_bitplane_words(n, p)
    if r < 0:
        raise DwtError("dwt_hip_bitplane_words: n %d (1 .. 4096), p %d (0 .. 32)" % (n, p))
    return r


def pack_batch(index_type, index, batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y, words, stream_stride,
               offsets=None):
    """dwt_hip_bitplane_pack_batch.  offsets=None: the offsets come back as a uint32 array (batch, S + 1) -- the call then
    ends synchronised; otherwise they go to `offsets` (host or device) and None is returned.  words=None: count only."""
    out = None
    if offsets is None:
        out = np.zeros((max(batch, 0), int(bands(size_x, size_y, j_max, cb_log2_x, cb_log2_y)[-1, 4]) + 1), np.uint32)
        if not out.size:
            return out
        offsets = out.ctypes.data
    _check(lib.dwt_hip_bitplane_pack_batch(index_type, _addr(index), batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x,
                                           cb_log2_y, None if words is None else _addr(words), stream_stride, _addr(offsets)),
           "dwt_hip_bitplane_pack_batch")
    return out


def count_batch(index_type, index, batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y, offsets=None):
    """the sizing call: dwt_hip_bitplane_pack_batch without words.  Offsets as in pack_batch."""
    return pack_batch(index_type, index, batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y, None, 0, offsets)


def unpack_batch(index_type, words, stream_stride, offsets, index, batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x,
                 cb_log2_y, drop=0, mode=KEEP):
    """dwt_hip_bitplane_unpack_batch: every own element of every frame is written; the min(drop, p) least significant
    magnitude planes of every block are not read (KEEP: the element keeps its step; SHIFT: the magnitude is |q| >> drop)."""
    _check(lib.dwt_hip_bitplane_unpack_batch(index_type, _addr(words), stream_stride, _addr(offsets), _addr(index), batch_stride,
                                             row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y, drop, mode),
           "dwt_hip_bitplane_unpack_batch")


def route(index_type, index, batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y):
    """dwt_hip_bitplane_route: 1 where a call with these arguments runs the wave kernels, 0 for the cross-check route."""
    r = lib.dwt_hip_bitplane_route(index_type, _addr(index), batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y)
    if r < 0:
        raise DwtError("dwt_hip_bitplane_route: " + lib.dwt_hip_last_error().decode(errors="replace"))
    return r
