"""Deadzone quantization of coefficient planes (include/libdwt_hip.h): the float coefficients of the
irreversible path <-> sign-magnitude integer indices with one step per subband (ITU-T T.800 Annex E), the per-band
counters, the step tables from the synthesis norms, and the magnitude bit-planes of every code-block.  A submodule of its
own: import it as ``from libdwt_amd import quant``.

    steps = quant.quant_steps(dwt.CDF97_S, J, 1.0 / 64)                      # 3 J + 1 steps, HL, LH, HH of level 1 .. J, LL(J)
    stats = quant.quantize_batch(quant.S, coef, 4 * W * H, 4 * W, quant.I16, idx, 2 * W * H, 2 * W, B, W, H, J, steps, stats=True)
    planes = quant.codeblock_bitplanes_batch(quant.I16, idx, 2 * W * H, 2 * W, B, W, H, J, 6, 6)
    quant.dequantize_batch(quant.I16, idx, 2 * W * H, 2 * W, quant.S, coef, 4 * W * H, 4 * W, B, W, H, J, steps, r=0.5)

Pointers are numpy arrays, torch tensors or integer addresses; each side host or device memory on its own.
"""
import ctypes as C

import numpy as np

from . import DwtError, _addr, _check, lib

_I, _P, _S, _F = C.c_int, C.c_void_p, C.c_size_t, C.c_float

S, H = 0, 1  # coefficient types (DWT_HIP_COEF_*): binary32, binary16
I16, I32 = 0, 1  # index types (DWT_HIP_INDEX_*)
COEF_BYTES = {S: 4, H: 2}
INDEX_BYTES = {I16: 2, I32: 4}
COEF_DTYPE = {S: "float32", H: "float16"}
INDEX_DTYPE = {I16: "int16", I32: "int32"}
MAX_LEVELS = 16  # of quant_norms / quant_steps
GRID_ROWS, GRID_BATCH = 16384, 4096  # rows / frames that one trip of the quantizer's loops covers
CODEBLOCK_GRID_BLOCKS = 65536  # code-blocks that one trip of the bit-plane kernel's loop covers
WIDE_COEF, WIDE_INDEX = 1, 2  # quant_route: that side moves by 16-byte accesses
STAT_NONZERO, STAT_MAX, STAT_CLIPPED = 0, 1, 2  # the three counters of a slot


def run_length(coef_type, index_type):
    """samples of a lane's run: the narrower side is one 16-byte access"""
    return 16 // min(COEF_BYTES[coef_type], INDEX_BYTES[index_type])


_COEF = [_I, _P, _S, _S]  # type, address, batch stride, row pitch
_FRAMES = [_I, _I, _I, _I]  # batch, size_x, size_y, j_max
lib.dwt_hip_quant_norms.argtypes = [_I, _I, _P, _P]
lib.dwt_hip_quant_steps.argtypes = [_I, _I, _F, _P]
lib.dwt_hip_quantize_batch.argtypes = _COEF + _COEF + _FRAMES + [_P, _S, _P]
lib.dwt_hip_dequantize_batch.argtypes = _COEF + _COEF + _FRAMES + [_P, _S, _F]
lib.dwt_hip_quant_route.argtypes = _COEF + _COEF + [_I, _I, _I]
lib.dwt_hip_codeblock_layout.argtypes = [_I, _I, _I, _I, _I, _P, _P]
lib.dwt_hip_codeblock_bitplanes_batch.argtypes = _COEF + _FRAMES + [_I, _I, _P, _S]
for _n in ("dwt_hip_quant_norms", "dwt_hip_quant_steps", "dwt_hip_quantize_batch", "dwt_hip_dequantize_batch", "dwt_hip_quant_route",
           "dwt_hip_codeblock_layout", "dwt_hip_codeblock_bitplanes_batch"):
    getattr(lib, _n).restype = _I


def _slots(size_x, size_y, j_max):
    levels = lib.dwt_hip_band_levels(size_x, size_y, j_max)
    if levels < 0:
        raise DwtError("quant: bad sizes %d x %d (dwt_hip_band_levels refuses them)" % (size_x, size_y))
    return 3 * levels + 1


def _table(steps):
    """the float32 array the C entry reads (None stays None: the entry refuses it)"""
    return None if steps is None else np.ascontiguousarray(steps, np.float32)


def quant_norms(wavelet, levels):
    """dwt_hip_quant_norms -> (norm_l, norm_h), float64 arrays of `levels` entries: the L2 norms of the 1-D synthesis
    functions of level 1 .. levels."""
    nl, nh = np.zeros(max(levels, 0), np.float64), np.zeros(max(levels, 0), np.float64)
    _check(lib.dwt_hip_quant_norms(wavelet, levels, nl.ctypes.data, nh.ctypes.data), "dwt_hip_quant_norms")
    return nl, nh


def quant_steps(wavelet, levels, base_step):
    """dwt_hip_quant_steps -> float32 array of 3 * levels + 1 steps: base_step over the 2-D synthesis norm of every slot."""
    steps = np.zeros(3 * max(levels, 0) + 1, np.float32)
    _check(lib.dwt_hip_quant_steps(wavelet, levels, float(base_step), steps.ctypes.data), "dwt_hip_quant_steps")
    return steps


def quantize_batch(coef_type, coef, coef_batch_stride, coef_row_pitch, index_type, index, index_batch_stride, index_row_pitch, batch,
                   size_x, size_y, j_max, steps, table_stride=0, stats=False):
    """dwt_hip_quantize_batch.  stats=True: returns the counters as an int64 array (batch, slots, 3) of nonzero indices,
    largest magnitude and clipped samples (the call then ends synchronised); otherwise None."""
    t = _table(steps)
    out = np.zeros((max(batch, 0), _slots(size_x, size_y, j_max), 3), np.int64) if stats else None
    _check(lib.dwt_hip_quantize_batch(coef_type, _addr(coef), coef_batch_stride, coef_row_pitch, index_type, _addr(index),
                                      index_batch_stride, index_row_pitch, batch, size_x, size_y, j_max,
                                      None if t is None else t.ctypes.data, table_stride, None if out is None else out.ctypes.data),
           "dwt_hip_quantize_batch")
    return out


def dequantize_batch(index_type, index, index_batch_stride, index_row_pitch, coef_type, coef, coef_batch_stride, coef_row_pitch, batch,
                     size_x, size_y, j_max, steps, table_stride=0, r=0.5):
    """dwt_hip_dequantize_batch: (|q| + r) * step with the sign of q, +0 for q = 0."""
    t = _table(steps)
    _check(lib.dwt_hip_dequantize_batch(index_type, _addr(index), index_batch_stride, index_row_pitch, coef_type, _addr(coef),
                                        coef_batch_stride, coef_row_pitch, batch, size_x, size_y, j_max,
                                        None if t is None else t.ctypes.data, table_stride, float(r)), "dwt_hip_dequantize_batch")


def quant_route(coef_type, coef, coef_batch_stride, coef_row_pitch, index_type, index, index_batch_stride, index_row_pitch, batch,
                size_x, size_y):
    """dwt_hip_quant_route: WIDE_COEF | WIDE_INDEX -- the sides a call with these addresses moves by 16-byte accesses."""
    r = lib.dwt_hip_quant_route(coef_type, _addr(coef), coef_batch_stride, coef_row_pitch, index_type, _addr(index), index_batch_stride,
                                index_row_pitch, batch, size_x, size_y)
    if r < 0:
        raise DwtError("dwt_hip_quant_route: " + lib.dwt_hip_last_error().decode(errors="replace"))
    return r


def codeblock_layout(size_x, size_y, j_max, cb_log2_x, cb_log2_y):
    """dwt_hip_codeblock_layout -> (first, blocks_x): int32 arrays of slots + 1 (the last entry the total) and slots."""
    n = _slots(size_x, size_y, j_max)
    first, blocks_x = np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
    if lib.dwt_hip_codeblock_layout(size_x, size_y, j_max, cb_log2_x, cb_log2_y, first.ctypes.data, blocks_x.ctypes.data) < 0:
        raise DwtError("dwt_hip_codeblock_layout: " + lib.dwt_hip_last_error().decode(errors="replace"))
    return first, blocks_x


def codeblock_bitplanes_batch(index_type, index, index_batch_stride, index_row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y,
                              planes=None, planes_frame_stride=0):
    """dwt_hip_codeblock_bitplanes_batch.  planes=None: returns a uint8 array (batch, total); otherwise the map goes to
    `planes` (host or device), frame b's at planes + b * planes_frame_stride."""
    out = None
    if planes is None:
        total = int(codeblock_layout(size_x, size_y, j_max, cb_log2_x, cb_log2_y)[0][-1])
        out = np.zeros((max(batch, 0), total), np.uint8)
        planes, planes_frame_stride = out.ctypes.data if out.size else 0, total
        if not out.size:
            return out
    _check(lib.dwt_hip_codeblock_bitplanes_batch(index_type, _addr(index), index_batch_stride, index_row_pitch, batch, size_x, size_y,
                                                 j_max, cb_log2_x, cb_log2_y, _addr(planes), planes_frame_stride),
           "dwt_hip_codeblock_bitplanes_batch")
    return out
