"""Numpy model of the sparse coefficient streams (include/libdwt_hip.h), written from their definition:
np.flatnonzero on the masked bits of every band, over the slot geometry of tests/shape_model.py.

* `stream_order(J)` -- the 3J + 1 slot numbers coarse to fine: LL, then HL, LH, HH of level J ... level 1;
* `kept(frames, type)` -- which elements an entry is made of: integers that are not 0, floats whose bits without the sign
  bit are not 0 (NaN, Inf, subnormals: kept; -0.0: dropped);
* `pack(frames, type, J, capacity)` -> (pos, val, offsets): pos uint32 (B, capacity), val in the frames' dtype (B,
  capacity), offsets uint32 (B, 3J + 2) -- always the true counts; entries past a frame's total (or all of them, past the
  capacity) hold `fill` / are absent;
* `unpack(pos, val, counts, dtype, B, H, W)` -- the way back: zero bits, then the entries whose position lies in the frame;
* `coarser(frames, J, k)` -- the frames with stream bands k .. zeroed: what a stream cut at off[k] unpacks to.
"""
import numpy as np

import shape_model as sm

F32, F16, I16, I32 = 0, 1, 2, 3
DTYPE = {F32: np.dtype(np.float32), F16: np.dtype(np.float16), I16: np.dtype(np.int16), I32: np.dtype(np.int32)}
TYPES = (F32, F16, I16, I32)
UINT = {2: np.uint16, 4: np.uint32}


def stream_order(J):
    return [3 * J] + [3 * (j - 1) + k for j in range(J, 0, -1) for k in range(3)]


def bands(W, H, J):
    """[(x0, y0, w, h)] of the 3J + 1 bands in stream order"""
    geo = sm.slots(W, H, W, H, J)
    return [geo[s] for s in stream_order(J)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def kept(frames, elem_type):
    u = bits(frames)
    if elem_type in (F32, F16):
        u = u & (np.iinfo(u.dtype).max >> 1)
    return u != 0


def pack(frames, elem_type, J, capacity=None, fill=0):
    """frames: (B, H, W) of DTYPE[elem_type].  capacity None: the largest total."""
    frames = np.ascontiguousarray(frames, DTYPE[elem_type])
    B, H, W = frames.shape
    keep = kept(frames, elem_type)
    u = bits(frames)
    geo = bands(W, H, J)
    offsets = np.zeros((B, len(geo) + 1), np.uint32)
    streams = []
    for b in range(B):
        pos = []
        for k, (x0, y0, w, h) in enumerate(geo):
            offsets[b, k] = sum(len(p) for p in pos)
            if w and h:
                at = np.flatnonzero(keep[b, y0:y0 + h, x0:x0 + w])
                pos.append(((y0 + at // w) * W + x0 + at % w).astype(np.uint32))
        pos = np.concatenate(pos) if pos else np.zeros(0, np.uint32)
        offsets[b, -1] = len(pos)
        streams.append(pos)
    if capacity is None:
        capacity = int(offsets[:, -1].max()) if B else 0
    pos_out = np.full((B, capacity), fill, np.uint32)
    val_out = np.full((B, capacity), fill & int(np.iinfo(u.dtype).max), u.dtype)
    for b, pos in enumerate(streams):
        n = min(len(pos), capacity)
        pos_out[b, :n] = pos[:n]
        val_out[b, :n] = u[b].reshape(-1)[pos[:n]]
    return pos_out, val_out.view(DTYPE[elem_type]), offsets


def unpack(pos, val, counts, elem_type, H, W):
    """pos, val: (B, capacity); counts: (B,) -> frames (B, H, W); positions outside the frame are skipped"""
    pos, val = np.asarray(pos), np.ascontiguousarray(val, DTYPE[elem_type])
    B, capacity = pos.shape
    out = np.zeros((B, H * W), UINT[DTYPE[elem_type].itemsize])
    v = bits(val)
    for b in range(B):
        n = min(int(counts[b]), capacity)
        p = pos[b, :n].astype(np.int64)
        ok = p < H * W
        out[b, p[ok]] = v[b, :n][ok]
    return out.view(DTYPE[elem_type]).reshape(B, H, W)


def coarser(frames, elem_type, J, k):
    """the frames with the stream bands k, k + 1, ... zeroed and -0.0 turned to +0.0"""
    frames = np.ascontiguousarray(frames, DTYPE[elem_type])
    u = bits(frames).copy()
    u[~kept(frames, elem_type)] = 0
    _, H, W = frames.shape
    for x0, y0, w, h in bands(W, H, J)[k:]:
        u[:, y0:y0 + h, x0:x0 + w] = 0
    return u.view(DTYPE[elem_type])
