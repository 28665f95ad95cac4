"""Sparse coefficient streams (include/libdwt_hip.h): the nonzero elements of coefficient or index planes
packed on the device into (position, value) entries in resolution order -- bands coarse to fine, raster order inside a
band --, and scattered back.  What keep_largest_batch and quantize_batch leave is almost all zeros; only the entries need
to cross PCIe.  A submodule of its own: import it as ``from libdwt_amd import sparse``.

    off = sparse.count_batch(sparse.I16, idx, 2 * W * H, 2 * W, B, W, H, J)            # (B, 3 J + 2) uint32, the sizing call
    cap = int(off[:, -1].max())
    sparse.pack_batch(sparse.I16, idx, 2 * W * H, 2 * W, B, W, H, J, pos, val, cap, offsets)
    sparse.unpack_batch(sparse.I16, pos, val, cap, offsets_address + 4 * (3 * J + 1), 3 * J + 2, idx, 2 * W * H, 2 * W, B, W, H)

Pointers are numpy arrays, torch tensors or integer addresses; the planes, the stream (pos, val) and the offsets / counts
each host or device memory on their own.  -0.0 is dropped and comes back as +0.0; everything else keeps its bits.
"""
import ctypes as C

import numpy as np

from . import DwtError, _addr, _check, lib

_I, _P, _S = C.c_int, C.c_void_p, C.c_size_t

F32, F16, I16, I32 = 0, 1, 2, 3  # element types (DWT_HIP_SPARSE_*)
ELEM_BYTES = {F32: 4, F16: 2, I16: 2, I32: 4}
ELEM_DTYPE = {F32: "float32", F16: "float16", I16: "int16", I32: "int32"}
TILE_SAMPLES = 2048  # samples of a tile
GRID_TILES, GRID_BATCH = 4096, 4096  # tiles / frames that one trip of the kernels' loops covers

_PLANES = [_I, _P, _S, _S]  # type, address, batch stride, row pitch
lib.dwt_hip_sparse_order.argtypes = [_I, _P]
lib.dwt_hip_sparse_bands.argtypes = [_I, _I, _I, _P]
lib.dwt_hip_sparse_tile.argtypes = [_P, _I, _I, _P, _P, _P]
lib.dwt_hip_sparse_pack_batch.argtypes = _PLANES + [_I, _I, _I, _I, _P, _P, _S, _P]
lib.dwt_hip_sparse_unpack_batch.argtypes = [_I, _P, _P, _S, _P, _S, _P, _S, _S, _I, _I, _I]
lib.dwt_hip_sparse_route.argtypes = _PLANES + [_I, _I, _I]
for _n in ("dwt_hip_sparse_order", "dwt_hip_sparse_bands", "dwt_hip_sparse_tile", "dwt_hip_sparse_pack_batch", "dwt_hip_sparse_unpack_batch",
           "dwt_hip_sparse_route"):
    getattr(lib, _n).restype = _I


def _levels(size_x, size_y, j_max):
    levels = lib.dwt_hip_band_levels(size_x, size_y, j_max)
    if levels < 0:
        raise DwtError("sparse: bad sizes %d x %d (dwt_hip_band_levels refuses them)" % (size_x, size_y))
    return levels


def _null(obj):
    return None if obj is None else _addr(obj)


def stream_order(levels):
    """dwt_hip_sparse_order -> int32 array of the 3 * levels + 1 slot numbers in stream order: LL, then HL, LH, HH of level
    `levels`, ... down to level 1."""
    slots = np.zeros(3 * max(levels, 0) + 1, np.int32)
    if lib.dwt_hip_sparse_order(levels, slots.ctypes.data) != slots.size:
        raise DwtError("dwt_hip_sparse_order: %d levels (0 .. 31)" % levels)
    return slots


def stream_bands(size_x, size_y, j_max):
    """dwt_hip_sparse_bands -> int32 array (3 J + 2, 5): x, y, size_x, size_y and first tile of every band in stream order;
    the last row holds the tiles of a frame."""
    table = np.zeros((3 * _levels(size_x, size_y, j_max) + 2, 5), np.int32)
    if lib.dwt_hip_sparse_bands(size_x, size_y, j_max, table.ctypes.data) != len(table) - 1:
        raise DwtError("dwt_hip_sparse_bands: bad sizes %d x %d" % (size_x, size_y))
    return table


def pack_batch(elem_type, planes, batch_stride, row_pitch, batch, size_x, size_y, j_max, pos, val, stream_stride, offsets=None):
    """dwt_hip_sparse_pack_batch.  offsets=None: the offsets come back as a uint32 array (batch, 3 J + 2) -- the call then
    ends synchronised; otherwise they go to `offsets` (host or device) and None is returned."""
    out = None
    if offsets is None:
        out = np.zeros((max(batch, 0), 3 * _levels(size_x, size_y, j_max) + 2), np.uint32)
        if not out.size:
            return out
        offsets = out.ctypes.data
    _check(lib.dwt_hip_sparse_pack_batch(elem_type, _addr(planes), batch_stride, row_pitch, batch, size_x, size_y, j_max, _null(pos),
                                         _null(val), stream_stride, _addr(offsets)), "dwt_hip_sparse_pack_batch")
    return out


def count_batch(elem_type, planes, batch_stride, row_pitch, batch, size_x, size_y, j_max, offsets=None):
    """the sizing call: dwt_hip_sparse_pack_batch without a stream.  Offsets as in pack_batch."""
    return pack_batch(elem_type, planes, batch_stride, row_pitch, batch, size_x, size_y, j_max, None, None, 0, offsets)


def unpack_batch(elem_type, pos, val, stream_stride, counts, counts_stride, planes, batch_stride, row_pitch, batch, size_x, size_y):
    """dwt_hip_sparse_unpack_batch: every own element of every frame is written, the entries' values and zero bits elsewhere.
    `counts`: uint32, frame b's at element b * counts_stride (host or device)."""
    _check(lib.dwt_hip_sparse_unpack_batch(elem_type, _addr(pos), _addr(val), stream_stride, _addr(counts), counts_stride, _addr(planes),
                                           batch_stride, row_pitch, batch, size_x, size_y), "dwt_hip_sparse_unpack_batch")


def sparse_route(elem_type, planes, batch_stride, row_pitch, batch, size_x, size_y):
    """dwt_hip_sparse_route: 1 where a call with these addresses reads / writes the planes by 16-byte accesses, 0 where not."""
    r = lib.dwt_hip_sparse_route(elem_type, _addr(planes), batch_stride, row_pitch, batch, size_x, size_y)
    if r < 0:
        raise DwtError("dwt_hip_sparse_route: " + lib.dwt_hip_last_error().decode(errors="replace"))
    return r
