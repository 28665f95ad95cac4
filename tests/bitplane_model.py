"""Numpy model of the embedded bit-plane streams of code-blocks (include/libdwt_hip.h), written from their
definition over the slot geometry of tests/shape_model.py and the stream order of tests/sparse_model.py.

* `bands(W, H, j_max, cbx, cby)` -- int array (3J + 2, 5): x, y, w, h and first stream block of every band in stream order,
  and the closing row {0, 0, 0, 0, S};
* `block(table, cbx, cby, s)` -- (x, y, w, h) of stream block s in frame coordinates; `blocks(...)` all of them;
* `words_of(n, p)` -- the size rule;
* `pack(frames, index_type, j_max, cbx, cby, capacity=None, fill=0)` -> (words uint64 (B, capacity), offsets uint32 (B, S + 1)):
  the offsets always the true sizes; a block is written only if it ends inside the capacity, every other word holds `fill`;
* `unpack(words, offsets, index_type, W, H, j_max, cbx, cby, drop=0, mode=KEEP)` -- the way back, including the rule for
  malformed blocks (written as zeros).
"""
import numpy as np

import shape_model as sm
import sparse_model as spm

I16, I32 = 0, 1
DTYPE = {I16: np.dtype(np.int16), I32: np.dtype(np.int32)}
PMAX = {I16: 16, I32: 32}
KEEP, SHIFT = 0, 1


def exponents_ok(cbx, cby):
    return 2 <= cbx <= 10 and 2 <= cby <= 10 and cbx + cby <= 12


def bands(W, H, j_max, cbx, cby):
    assert exponents_ok(cbx, cby)
    J = sm.levels(W, H, j_max)
    rows, first = [], 0
    for x, y, w, h in spm.bands(W, H, J):
        if w <= 0 or h <= 0:
            w = h = 0
        rows.append([x, y, w, h, first])
        first += -(-w // (1 << cbx)) * -(-h // (1 << cby))
    rows.append([0, 0, 0, 0, first])
    return np.array(rows, np.int64)


def block(table, cbx, cby, s):
    assert 0 <= s < table[-1, 4]
    k = max(i for i in range(len(table) - 1) if table[i, 4] <= s)  # (bands without blocks share their successor's first)
    x, y, w, h, first = (int(v) for v in table[k])
    nx = -(-w // (1 << cbx))
    bx, by = (s - first) % nx, (s - first) // nx
    return x + (bx << cbx), y + (by << cby), min(1 << cbx, w - (bx << cbx)), min(1 << cby, h - (by << cby))


def blocks(W, H, j_max, cbx, cby):
    """[(x, y, w, h)] of the S blocks of a frame in stream order"""
    out = []
    for x, y, w, h, _ in bands(W, H, j_max, cbx, cby)[:-1]:
        for by in range(0, h, 1 << cby):
            for bx in range(0, w, 1 << cbx):
                out.append((int(x + bx), int(y + by), int(min(1 << cbx, w - bx)), int(min(1 << cby, h - by))))
    return out


def words_of(n, p):
    assert 1 <= n <= 4096 and 0 <= p <= 32
    return (p + 1) * -(-n // 64) if p else 0


def bit_length(m):
    return int(m).bit_length()


def block_words(q):
    """q: the (ch, cw) samples of one block -> its words (uint64), sign plane first, then bit p - 1 ... bit 0 of |q|"""
    flat = q.reshape(-1).astype(np.int64)
    n = flat.size
    G = -(-n // 64)
    mag = np.abs(flat)
    p = bit_length(mag.max())
    if p == 0:
        return np.zeros(0, np.uint64)
    bits = np.zeros((p + 1, G * 64), np.uint8)
    bits[0, :n] = flat < 0
    for k in range(1, p + 1):
        bits[k, :n] = (mag >> (p - k)) & 1
    return np.packbits(bits, axis=-1, bitorder="little").reshape(-1).view("<u8").astype(np.uint64)


def frame_words(frame, rects):
    """the words of every block of one frame: block_words, taken for all the blocks of one shape and one p at a time"""
    parts = [None] * len(rects)
    shapes = {}
    for s, (x, y, w, h) in enumerate(rects):
        shapes.setdefault((w, h), []).append(s)
    for (w, h), members in shapes.items():
        n, G = w * h, -(-w * h // 64)
        flat = np.stack([frame[rects[s][1]:rects[s][1] + h, rects[s][0]:rects[s][0] + w].reshape(-1) for s in members]).astype(np.int64)
        mag = np.abs(flat)
        top = mag.max(axis=1)
        plen = np.array([bit_length(t) for t in top])
        for p in np.unique(plen):
            pick = np.flatnonzero(plen == p)
            if p == 0:
                for i in pick:
                    parts[members[i]] = np.zeros(0, np.uint64)
                continue
            bits = np.zeros((len(pick), p + 1, G * 64), np.uint8)
            bits[:, 0, :n] = flat[pick] < 0
            for k in range(1, p + 1):
                bits[:, k, :n] = (mag[pick] >> (p - k)) & 1
            words = np.packbits(bits, axis=-1, bitorder="little").reshape(len(pick), -1).view("<u8").astype(np.uint64)
            for i, row in zip(pick, words):
                parts[members[i]] = row
    return parts


def pack(frames, index_type, j_max, cbx, cby, capacity=None, fill=0):
    frames = np.ascontiguousarray(frames, DTYPE[index_type])
    B, H, W = frames.shape
    rects = blocks(W, H, j_max, cbx, cby)
    S = len(rects)
    offsets = np.zeros((B, S + 1), np.uint32)
    streams = []
    for b in range(B):
        parts = frame_words(frames[b], rects)
        offsets[b, 1:] = np.cumsum([len(p) for p in parts]) if S else 0
        streams.append(np.concatenate(parts) if parts else np.zeros(0, np.uint64))
    if capacity is None:
        capacity = int(offsets[:, -1].max()) if B else 0
    words = np.full((B, capacity), fill, np.uint64)
    for b, stream in enumerate(streams):
        # the blocks that end inside the capacity: a prefix, the offsets being monotone; the first block that does not, and
        # every later one, is not written
        over = np.flatnonzero(offsets[b, 1:] > capacity)
        end = int(offsets[b, over[0]]) if len(over) else int(offsets[b, -1])
        words[b, :end] = stream[:end]
    return words, offsets


def stream_planes(o0, o1, stream_stride, G, index_type):
    """p of a block from its two offsets; 0 for an empty block and for a malformed one"""
    o0, o1 = int(o0), int(o1)
    if o1 <= o0 or o1 > stream_stride or (o1 - o0) % G:
        return 0
    p = (o1 - o0) // G - 1
    return p if p <= PMAX[index_type] else 0


def unpack(words, offsets, index_type, W, H, j_max, cbx, cby, drop=0, mode=KEEP):
    words, offsets = np.ascontiguousarray(words, np.uint64), np.asarray(offsets)
    B, stream_stride = words.shape
    assert 0 <= drop <= 32 and mode in (KEEP, SHIFT)
    rects = blocks(W, H, j_max, cbx, cby)
    assert offsets.shape == (B, len(rects) + 1)
    out = np.zeros((B, H, W), np.int64)
    for b in range(B):
        for s, (x, y, w, h) in enumerate(rects):
            n = w * h
            G = -(-n // 64)
            p = stream_planes(offsets[b, s], offsets[b, s + 1], stream_stride, G, index_type)
            dk = min(drop, p)
            keep = p - dk
            if keep == 0:
                continue
            o0 = int(offsets[b, s])
            raw = words[b, o0:o0 + (keep + 1) * G].astype("<u8").view(np.uint8).reshape(keep + 1, G * 8)
            bits = np.unpackbits(raw, axis=-1, bitorder="little")[:, :n].astype(np.int64)
            m = np.zeros(n, np.int64)
            for k in range(1, keep + 1):
                m = (m << 1) | bits[k]
            v = m << dk if mode == KEEP else m
            v = np.where(bits[0] != 0, -v, v)  # (a magnitude of 0 stays 0)
            out[b, y:y + h, x:x + w] = v.reshape(h, w)
    dt = DTYPE[index_type]
    u = np.uint16 if dt.itemsize == 2 else np.uint32
    return (out & np.iinfo(u).max).astype(u).view(dt)  # truncated to the element type
