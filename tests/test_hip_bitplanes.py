"""GPU checks of the embedded bit-plane streams of code-blocks (dwt_hip_bitplane_pack_batch, dwt_hip_bitplane_unpack_batch;
libdwt_amd/bitplanes.py) against tests/bitplane_model.py, bit for bit.  Every buffer is a run of poison bytes with the
frames' elements, the words or the offsets laid into it; after a call the output holds the model's bytes and every other
byte of every buffer still holds the poison (the input: its own bytes too)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bitplane_model as bpm
import gridlimits
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
POISON64 = 0xA5A5A5A5A5A5A5A5
# empty bands, bands one sample wide; two sizes with partial blocks at the right and at the bottom
SHAPES = [(5, 3, 2), (1, 37, -1), (37, 1, -1), (72, 40, 3), (264, 136, 3)]
# n = 16, below one word; 256 samples of 8-sample rows; one row per group; rows wider and narrower than a wave
EXPONENTS = [(2, 2), (3, 5), (6, 6), (10, 2), (2, 10)]
PITCHES = ["dense", "prime", "padded16"]
PRIMES = (3, 7, 11, 41, 43, 67, 71, 73, 79, 131, 137, 269, 271, 277)
TYPES = (bpm.I16, bpm.I32)
GUARD = 64 << 10


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d
    from libdwt_amd import bitplanes

    d.dwt_util_init()
    d.bitplanes = bitplanes
    assert (bitplanes.I16, bitplanes.I32, bitplanes.KEEP, bitplanes.SHIFT) == (bpm.I16, bpm.I32, bpm.KEEP, bpm.SHIFT)
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("bitplane_wave", 1)


class Lay:
    """`batch` frames of W x H elements of `dtype` in a byte buffer: row pitch "dense", "prime" (an odd number of elements: no
    multiple of 16 bytes) or "padded16"; the base `base` bytes into the buffer; `gap` bytes between the frames; `tail` bytes
    behind the last frame"""

    def __init__(self, dtype, batch, W, H, pitch="dense", base=0, gap=0, tail=16):
        self.dtype = np.dtype(dtype)
        es = self.dtype.itemsize
        self.es, self.batch, self.W, self.H, self.base = es, batch, W, H, base
        row = W * es
        self.pitch = {"dense": lambda: row, "prime": lambda: es * next(p for p in PRIMES if p > W), "padded16": lambda: (row + 15) // 16 * 16 + 16}[pitch]()
        self.bs = self.pitch * H + gap
        self.nbytes = base + self.bs * batch + tail
        b, y, x = np.ix_(np.arange(batch), np.arange(H), np.arange(W))
        self.at = base + b * self.bs + y * self.pitch + x * es  # (B, H, W) byte offsets
        self.own = np.zeros(self.nbytes, bool)
        for k in range(es):
            self.own[self.at + k] = True

    def fill(self, values=None):
        buf = np.full(self.nbytes, POISON, np.uint8)
        if values is not None:
            raw = np.ascontiguousarray(values, self.dtype).view(np.uint8).reshape(self.at.shape + (self.es,))
            for k in range(self.es):
                buf[self.at + k] = raw[..., k]
        return buf

    def read(self, buf):
        raw = np.stack([buf[self.at + k] for k in range(self.es)], -1)
        return np.ascontiguousarray(raw).view(self.dtype).reshape(self.at.shape)

    def args(self, ptr):
        return (ptr + self.base, self.bs, self.pitch)


def poisoned(shape, dtype):
    return np.full(shape, POISON, np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype).reshape(shape) if np.prod(shape) else np.zeros(shape, dtype)


def place(dwt, hold, arr, dev):
    """the array where the call finds it: its own memory, or a copy on the device (kept in `hold`)"""
    if not dev:
        return arr.ctypes.data if arr.size else 8  # (an empty numpy array has no address worth passing)
    hold.append(Dev(dwt, arr))
    return hold[-1].ptr


def fetch(hold, arr, dev):
    return hold.pop(0).get() if dev else arr


_CONTENTS = {}


def contents(index_type, W, H, j_max, cbx, cby, seed=0):
    """three frames (kept: a reference shared by the tests, never written).  Frame 0: zeros.  Frame 1: the blocks take the
    classes in turn -- all zero, a single +-1, random with p = 3 .. 8, one INT_MIN among small values, the whole range.
    Frame 2: the whole range everywhere."""
    key = (index_type, W, H, j_max, cbx, cby, seed)
    if key not in _CONTENTS:
        dt = bpm.DTYPE[index_type]
        info = np.iinfo(dt)
        rng = np.random.default_rng([seed, index_type, W, H, cbx, cby])
        v = np.zeros((3, H, W), np.int64)
        for s, (x, y, w, h) in enumerate(bpm.blocks(W, H, j_max, cbx, cby)):
            cls = s % 5
            blk = np.zeros((h, w), np.int64)
            if cls == 1:
                blk[rng.integers(h), rng.integers(w)] = (-1) ** (s // 5)
            elif cls == 2:
                p = 3 + (s // 5) % 6
                blk = rng.integers(-(1 << p) + 1, 1 << p, (h, w))
                blk[rng.integers(h), rng.integers(w)] = (1 << p) - 1
            elif cls == 3:
                blk = rng.integers(-3, 4, (h, w))
                blk[rng.integers(h), rng.integers(w)] = info.min
            elif cls == 4:
                blk = rng.integers(info.min, int(info.max) + 1, (h, w))
            v[1, y:y + h, x:x + w] = blk
        v[2] = rng.integers(info.min, int(info.max) + 1, (H, W))
        v = v.astype(dt)
        v.setflags(write=False)
        _CONTENTS[key] = v
    return _CONTENTS[key]


_MODEL = {}


def model_pack(values, index_type, j_max, cbx, cby):
    """the model's whole stream and offsets of a reference array, computed once"""
    key = (id(values), index_type, j_max, cbx, cby)
    if key not in _MODEL:
        words, off = bpm.pack(values, index_type, j_max, cbx, cby)
        words.setflags(write=False)
        off.setflags(write=False)
        _MODEL[key] = (values, words, off)  # (the array is kept alive: its id stays its own)
    return _MODEL[key][1:]


def run_pack(dwt, lay, index_type, values, j_max, cbx, cby, capacity, device=(True, True, True), count_only=False, batch_capacity=None):
    """one call -> (words, offsets); asserts that the planes kept every byte.  The words lie in a buffer of batch x
    `batch_capacity` words (the capacity by default) and the call is told `capacity`"""
    BP = dwt.bitplanes
    B, W, H = lay.batch, lay.W, lay.H
    S = int(bpm.bands(W, H, j_max, cbx, cby)[-1, 4])
    planes = lay.fill(values)
    words = poisoned((B, capacity if batch_capacity is None else batch_capacity), np.uint64)
    off = poisoned((B, S + 1), np.uint32)
    hold = []
    pp, op = place(dwt, hold, planes, device[0]), place(dwt, hold, off, device[2])
    if count_only:
        BP.count_batch(index_type, *lay.args(pp), B, W, H, j_max, cbx, cby, op)
    else:
        wp = place(dwt, hold, words, device[1])
        BP.pack_batch(index_type, *lay.args(pp), B, W, H, j_max, cbx, cby, wp, capacity, op)
    dwt.sync()
    got_planes, got_off = fetch(hold, planes, device[0]), fetch(hold, off, device[2])
    if not count_only:
        words = fetch(hold, words, device[1])
    assert np.array_equal(got_planes, lay.fill(values)), "the planes were written"
    return words, got_off


def check_pack(dwt, lay, index_type, values, j_max, cbx, cby, capacity=None, slack=3, **kw):
    """pack against the model: the words, the poison behind the total and between the frames, the true offsets.  capacity
    None: the largest total + slack"""
    all_words, want_off = model_pack(values, index_type, j_max, cbx, cby)
    if capacity is None:
        capacity = all_words.shape[1] + slack
    want = poisoned((lay.batch, capacity), np.uint64)
    for b in range(lay.batch):
        over = np.flatnonzero(want_off[b, 1:] > capacity)  # the first block that does not end inside the capacity, if any
        end = int(want_off[b, over[0]]) if len(over) else int(want_off[b, -1])
        want[b, :end] = all_words[b, :end]
    words, off = run_pack(dwt, lay, index_type, values, j_max, cbx, cby, capacity, **kw)
    assert np.array_equal(off, want_off), np.argwhere(off != want_off)[:5]
    assert np.array_equal(words, want), np.argwhere(words != want)[:5]
    return words, off


def run_unpack(dwt, lay, index_type, words, off, j_max, cbx, cby, drop=0, mode=bpm.KEEP, device=(True, True, True), before=None, stream_stride=None):
    """one call into poisoned frames -> the buffer after it"""
    BP = dwt.bitplanes
    planes = lay.fill(before)
    hold = []
    pp = place(dwt, hold, planes, device[0])
    wp = place(dwt, hold, np.ascontiguousarray(words, np.uint64), device[1])
    op = place(dwt, hold, np.ascontiguousarray(off, np.uint32), device[2])
    BP.unpack_batch(index_type, wp, words.shape[1] if stream_stride is None else stream_stride, op, *lay.args(pp), lay.batch, lay.W, lay.H, j_max,
                    cbx, cby, drop, mode)
    dwt.sync()
    return fetch(hold, planes, device[0])


def check_unpack(dwt, lay, index_type, words, off, j_max, cbx, cby, want, **kw):
    got = run_unpack(dwt, lay, index_type, words, off, j_max, cbx, cby, **kw)
    assert (got[~lay.own] == POISON).all(), "bytes outside the frames were written"
    assert np.array_equal(lay.read(got), want), np.argwhere(lay.read(got) != want)[:5]


def round_trip(dwt, lay, index_type, values, j_max, cbx, cby, device=(True, True, True), **kw):
    words, off = check_pack(dwt, lay, index_type, values, j_max, cbx, cby, device=device, **kw)
    check_unpack(dwt, lay, index_type, words, off, j_max, cbx, cby, values, device=device)
    return words, off


# ---- shapes, exponents, types, pitches, contents --------------------------------------------------------------------
def test_the_exponents_cut_partial_blocks():
    """37 x 5 samples: G = 3 with a partial last word; blocks of 16 samples; blocks whose rows are wider than a wave"""
    rects = bpm.blocks(264, 136, 3, 6, 6)
    assert any(w * h % 64 for _, _, w, h in rects) and any(w == 64 and h == 64 for _, _, w, h in rects)
    assert (37, 5) in [(w, h) for _, _, w, h in bpm.blocks(37, 5, 0, 6, 6)] and bpm.words_of(37 * 5, 2) == 9
    assert all(w * h <= 16 for _, _, w, h in bpm.blocks(72, 40, 3, 2, 2))
    assert any(w > 64 for _, _, w, h in bpm.blocks(264, 136, 3, 10, 2)) and any(w < 64 and h > 64 for _, _, w, h in bpm.blocks(264, 136, 3, 2, 10))


@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_shapes_exponents_types_pitches_and_contents(dwt, W, H, j_max):
    """the five pairs of exponents, both types, the three pitches, three frames of every block class: words, offsets, the
    untouched bytes behind the total and between the frames are the model's, and unpack returns the input"""
    for cbx, cby in EXPONENTS:
        for index_type in TYPES:
            v = contents(index_type, W, H, j_max, cbx, cby)
            for pitch in PITCHES:
                lay = Lay(bpm.DTYPE[index_type], 3, W, H, pitch)
                _, off = round_trip(dwt, lay, index_type, v, j_max, cbx, cby)
                assert off[0, -1] == 0 and off[2, -1] >= off[1, -1], (cbx, cby, index_type, pitch)


@pytest.mark.parametrize("base", [2, 4])
def test_bases(dwt, base):
    """planes 2 and 4 bytes off a 16-byte boundary (launch 1 then reads element by element); words on an odd word, where the
    block runs start with a single 8-byte store"""
    W, H, j_max = 264, 136, 3
    for index_type in TYPES:
        if base % bpm.DTYPE[index_type].itemsize:
            continue  # (a 4-byte element 2 bytes off its size is refused: test_refusals)
        for cbx, cby in ((6, 6), (3, 5)):
            lay = Lay(bpm.DTYPE[index_type], 3, W, H, "padded16", base=base)
            v = contents(index_type, W, H, j_max, cbx, cby)
            round_trip(dwt, lay, index_type, v, j_max, cbx, cby)
    # the words one word into their allocation: every frame's run starts on an odd word
    BP = dwt.bitplanes
    v = contents(bpm.I16, W, H, j_max, 6, 6)
    words, off = model_pack(v, bpm.I16, j_max, 6, 6)
    cap = words.shape[1] + (words.shape[1] & 1)  # (an even stride: every frame starts alike)
    lay = Lay(np.int16, 3, W, H)
    planes, out, doff = Dev(dwt, lay.fill(v)), Dev(dwt, poisoned(3 * cap + 2, np.uint64)), Dev(dwt, poisoned(off.shape, np.uint32))
    BP.pack_batch(BP.I16, *lay.args(planes.ptr), 3, W, H, j_max, 6, 6, out.ptr + 8, cap, doff.ptr)
    got = out.get()
    assert got[0] == POISON64 and got[-1] == POISON64
    got = got[1:-1].reshape(3, cap)
    for b in range(3):
        assert np.array_equal(got[b, :off[b, -1]], words[b, :off[b, -1]]) and (got[b, off[b, -1]:] == POISON64).all()
    back = Dev(dwt, lay.fill())
    BP.unpack_batch(BP.I16, out.ptr + 8, cap, doff.ptr, *lay.args(back.ptr), 3, W, H, j_max, 6, 6)
    assert np.array_equal(lay.read(back.get()), v)


# ---- unpack with dropped planes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_type", TYPES)
@pytest.mark.parametrize("W, H, j_max, cbx, cby", [(72, 40, 3, 3, 5), (264, 136, 3, 6, 6), (37, 1, -1, 2, 2)])
def test_unpack_of_a_model_stream_with_dropped_planes(dwt, index_type, W, H, j_max, cbx, cby):
    """drop 0, 1, p - 1, p and 32 (p: the planes of the largest block, 16 / 32), KEEP and SHIFT: the model's elements"""
    v = contents(index_type, W, H, j_max, cbx, cby)
    words, off = model_pack(v, index_type, j_max, cbx, cby)
    p = bpm.PMAX[index_type]
    lay = Lay(bpm.DTYPE[index_type], 3, W, H, "prime")
    for drop in sorted({0, 1, p - 1, p, 32}):
        for mode in (bpm.KEEP, bpm.SHIFT):
            want = bpm.unpack(words, off, index_type, W, H, j_max, cbx, cby, drop, mode)
            if drop == 0:
                assert np.array_equal(want, v)
            check_unpack(dwt, lay, index_type, words, off, j_max, cbx, cby, want, drop=drop, mode=mode)


# ---- routes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_type", TYPES)
def test_wave_route_and_plain_route_give_the_same_bytes(dwt, index_type):
    BP = dwt.bitplanes
    W, H, j_max = 264, 136, 3
    for cbx, cby in ((6, 6), (10, 2), (2, 10)):
        lay = Lay(bpm.DTYPE[index_type], 3, W, H, "padded16")
        v = contents(index_type, W, H, j_max, cbx, cby)
        results = []
        for wave in (1, 0):
            dwt.set_option("bitplane_wave", wave)
            try:
                assert BP.route(index_type, 4096, lay.bs, lay.pitch, 3, W, H, j_max, cbx, cby) == wave
                words, off = round_trip(dwt, lay, index_type, v, j_max, cbx, cby)
                outs = [run_unpack(dwt, lay, index_type, words, off, j_max, cbx, cby, drop=d, mode=m) for d, m in ((3, bpm.KEEP), (5, bpm.SHIFT))]
                results.append([words, off] + outs)
            finally:
                dwt.set_option("bitplane_wave", 1)
        for a, b in zip(*results):
            assert a.tobytes() == b.tobytes()


# ---- count only, capacity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_count_only_equals_packs_offsets(dwt, W, H, j_max):
    BP = dwt.bitplanes
    for index_type, (cbx, cby) in ((bpm.I16, (3, 5)), (bpm.I32, (2, 2))):
        lay = Lay(bpm.DTYPE[index_type], 3, W, H, "prime")
        v = contents(index_type, W, H, j_max, cbx, cby)
        _, counted = run_pack(dwt, lay, index_type, v, j_max, cbx, cby, 0, count_only=True)
        _, packed = check_pack(dwt, lay, index_type, v, j_max, cbx, cby)
        assert np.array_equal(counted, packed)
    # the wrapper's own array
    planes = Dev(dwt, lay.fill(v))
    ret = BP.count_batch(index_type, *lay.args(planes.ptr), 3, W, H, j_max, cbx, cby)
    assert ret.dtype == np.uint32 and np.array_equal(ret, packed)


def test_capacity(dwt):
    """stream_stride ends inside a block of the second band of (72, 40, 3): the true offsets, a prefix of whole blocks, the
    sentinel words behind it untouched; unpack of that stream gives the prefix and zeros.  Also the exact total and 0"""
    W, H, j_max, cbx, cby = 72, 40, 3, 3, 3
    for index_type in TYPES:
        v = contents(index_type, W, H, j_max, cbx, cby)
        all_words, off = model_pack(v, index_type, j_max, cbx, cby)
        table = bpm.bands(W, H, j_max, cbx, cby)
        s = int(table[1, 4]) + 1  # a block of the second band
        assert table[1, 4] < s < table[2, 4] and off[2, s + 1] - off[2, s] > 1
        lay = Lay(bpm.DTYPE[index_type], 3, W, H, "padded16")
        rects = bpm.blocks(W, H, j_max, cbx, cby)
        for cap in (int(off[2, s]) + 1, int(off[:, -1].max()), 0):
            words, got_off = check_pack(dwt, lay, index_type, v, j_max, cbx, cby, capacity=cap)
            want = bpm.unpack(words, off, index_type, W, H, j_max, cbx, cby)
            check_unpack(dwt, lay, index_type, words, off, j_max, cbx, cby, want)
            if cap == int(off[2, s]) + 1:
                assert (words[2, off[2, s]:] == POISON64).all() and np.array_equal(words[2, :off[2, s]], all_words[2, :off[2, s]])
                prefix = np.zeros_like(v[2])
                for x, y, w, h in rects[:s]:
                    prefix[y:y + h, x:x + w] = v[2, y:y + h, x:x + w]
                assert np.array_equal(want[2], prefix) and want[2].any() and not np.array_equal(prefix, v[2])


# ---- foreign streams ------------------------------------------------------------------------------------------------
def foreign_stream(W, H, j_max, cbx, cby):
    """an int16 frame's stream rebuilt with foreign offsets for four blocks -> (frame (1, H, W), words, offsets (S + 1),
    stream_stride, the model's unpacked frame).  The model's answer is checked against the rule here: those blocks zeros,
    every other block the frame's"""
    v = contents(bpm.I16, W, H, j_max, cbx, cby)[1:2]
    words, off = bpm.pack(v, bpm.I16, j_max, cbx, cby)
    rects = bpm.blocks(W, H, j_max, cbx, cby)
    S = len(rects)
    G = [-(-w * h // 64) for _, _, w, h in rects]
    sizes = np.diff(off[0].astype(np.int64))
    odd = next(s for s in range(S) if G[s] > 1 and sizes[s] > 0)                     # a length of G * k + 1 words
    deep = next(s for s in range(odd + 1, S) if sizes[s] > 0)                        # 18 planes: p = 17
    back = next(s for s in range(deep + 1, S) if sizes[s] > 0 and sizes[s + 1] > 0)  # off[back + 1] < off[back]
    last = max(s for s in range(S) if sizes[s] > 0)                                  # ends beyond stream_stride
    assert last > back + 1
    new = sizes.copy()
    new[odd] += 1
    new[deep] = 18 * G[deep]
    starts = np.concatenate([[0], np.cumsum(new)])
    stream = np.full(int(starts[-1]) + 64, 0x0123456789ABCDEF, np.uint64)
    for s in range(S):  # every block's own words at its new start
        stream[starts[s]:starts[s] + sizes[s]] = words[0, off[0, s]:off[0, s + 1]]
    foreign = starts.copy()
    foreign[back + 1] = foreign[back] - 1  # (block back + 1 then starts in front of its words: whatever the rule makes of it)
    stride = int(starts[last]) + 1
    want = bpm.unpack(stream[None, :stride], foreign[None].astype(np.uint32), bpm.I16, W, H, j_max, cbx, cby)
    for s, (x, y, w, h) in enumerate(rects):
        if s in (odd, deep, back, last):
            assert v[0, y:y + h, x:x + w].any() and not want[0, y:y + h, x:x + w].any(), s
        elif s != back + 1:
            assert np.array_equal(want[0, y:y + h, x:x + w], v[0, y:y + h, x:x + w]), s
    return v, stream, foreign, stride, want


def test_malformed_offsets_come_back_as_zeros(dwt):
    """one block whose length is no multiple of G, one with p = 17 on int16, one whose offsets are not monotone, one that
    ends beyond stream_stride: zeros there, every other block right.  The stream lies inside a larger allocation between
    guards that hold other words: a missing check shows as wrong elements, not as a fault"""
    BP = dwt.bitplanes
    W, H, j_max, cbx, cby = 72, 40, 3, 3, 5
    v, stream, foreign, stride, want = foreign_stream(W, H, j_max, cbx, cby)
    lay = Lay(np.int16, 1, W, H, "prime", tail=GUARD)
    guard = np.full(GUARD // 8, 0xFFFFFFFFFFFFFFFF, np.uint64)  # (all planes set: a word read here turns a zero into a value)
    buf = Dev(dwt, np.concatenate([guard, stream, guard]))
    offs = Dev(dwt, np.concatenate([np.full(GUARD // 4, 0x7FFFFFFF, np.uint32), foreign.astype(np.uint32), np.full(GUARD // 4, 0x7FFFFFFF, np.uint32)]))
    for wave in (1, 0):
        dwt.set_option("bitplane_wave", wave)
        try:
            planes = Dev(dwt, lay.fill())
            BP.unpack_batch(BP.I16, buf.ptr + GUARD, stride, offs.ptr + GUARD, *lay.args(planes.ptr), 1, W, H, j_max, cbx, cby)
            got = planes.get()
            assert (got[~lay.own] == POISON).all() and np.array_equal(lay.read(got), want), wave
        finally:
            dwt.set_option("bitplane_wave", 1)


# ---- memory spaces --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [(p, s, o) for p in (False, True) for s in (False, True) for o in (False, True) if not (p and s and o)])
def test_host_sides_give_the_device_calls_bytes(dwt, device):
    """each of the planes, the words and the offsets in host memory: the model's bytes (which the device call gives), every
    poison byte kept -- with pitch padding and a gap, where the regions hold bytes that are not the frames'"""
    for index_type, pitch, gap, (W, H, j_max), (cbx, cby) in ((bpm.I32, "dense", 0, (72, 40, 3), (3, 5)), (bpm.I16, "prime", 6, (37, 1, -1), (2, 2)),
                                                             (bpm.I16, "padded16", 32, (264, 136, 3), (6, 6))):
        lay = Lay(bpm.DTYPE[index_type], 3, W, H, pitch, gap=gap)
        v = contents(index_type, W, H, j_max, cbx, cby)
        words, off = round_trip(dwt, lay, index_type, v, j_max, cbx, cby, device=device)
        _, counted = run_pack(dwt, lay, index_type, v, j_max, cbx, cby, 0, device=device, count_only=True)
        assert np.array_equal(counted, off)
        want = bpm.unpack(words, off, index_type, W, H, j_max, cbx, cby, 2, bpm.SHIFT)
        check_unpack(dwt, lay, index_type, words, off, j_max, cbx, cby, want, drop=2, mode=bpm.SHIFT, device=device)


# ---- launches, allocation -------------------------------------------------------------------------------------------
def test_launches_and_no_allocation_on_device_memory(dwt):
    """pack 3 launches, count only 2, unpack 1 -- for one frame and five, for planes of zeros and planes of the whole range;
    the second round allocates nothing; no frames: no launch"""
    BP = dwt.bitplanes
    W, H, J, cbx, cby = 264, 136, 3, 6, 6
    S = int(bpm.bands(W, H, J, cbx, cby)[-1, 4])
    cap = W * H * 17 // 64 + 17 * S
    counts = {}
    bufs = []
    rng = np.random.default_rng(21)
    for B in (1, 5):
        for what in ("zeros", "full"):
            lay = Lay(np.int16, B, W, H)
            v = np.zeros((B, H, W), np.int16) if what == "zeros" else rng.integers(-32768, 32768, (B, H, W)).astype(np.int16)
            planes = Dev(dwt, lay.fill(v))
            words, off = Dev(dwt, np.zeros((B, cap), np.uint64)), Dev(dwt, np.zeros((B, S + 1), np.uint32))
            out = Dev(dwt, lay.fill())
            calls = (lambda: BP.pack_batch(BP.I16, *lay.args(planes.ptr), B, W, H, J, cbx, cby, words.ptr, cap, off.ptr),
                     lambda: BP.count_batch(BP.I16, *lay.args(planes.ptr), B, W, H, J, cbx, cby, off.ptr),
                     lambda: BP.unpack_batch(BP.I16, words.ptr, cap, off.ptr, *lay.args(out.ptr), B, W, H, J, cbx, cby))
            for f in calls:  # the first call of a size may grow the workspace
                f()
            allocs = dwt.get_option("stat_allocs")
            counts[B, what] = [launches(dwt, f) for f in calls]
            assert dwt.get_option("stat_allocs") == allocs
            assert np.array_equal(lay.read(out.get()), v)
            bufs.append((lay, planes, words, off))
    assert all(c == [3, 2, 1] for c in counts.values()), counts
    lay, planes, words, off = bufs[-1]
    assert launches(dwt, lambda: BP.pack_batch(BP.I16, *lay.args(planes.ptr), 0, W, H, J, cbx, cby, words.ptr, cap, off.ptr)) == 0
    assert launches(dwt, lambda: BP.count_batch(BP.I16, *lay.args(planes.ptr), 0, W, H, J, cbx, cby, off.ptr)) == 0
    assert launches(dwt, lambda: BP.unpack_batch(BP.I16, words.ptr, cap, off.ptr, *lay.args(planes.ptr), 0, W, H, J, cbx, cby)) == 0


def test_empty_frames_launch_nothing_and_write_zero_offsets(dwt):
    BP = dwt.bitplanes
    for device in (True, False):
        off = poisoned((2, 1), np.uint32)  # (no blocks: one word a frame)
        hold = []
        op = place(dwt, hold, off, device)
        assert launches(dwt, lambda: BP.count_batch(BP.I16, 4096, 0, 0, 2, 0, 9, 1, 2, 2, op)) == 0
        dwt.sync()
        assert not fetch(hold, off, device).any()


# ---- grid caps ------------------------------------------------------------------------------------------------------
def test_blocks_past_the_grid_cap(dwt):
    """a 1024 x 1024 frame of 4 x 4 blocks: more blocks than one trip of the kernels' loops covers; rows of blocks repeating
    with period 251 (tests/gridlimits.py), so that a block taken one cap away from where it belongs meets other data"""
    BP = dwt.bitplanes
    W = H = 1024
    S = int(bpm.bands(W, H, 0, 2, 2)[-1, 4])
    assert S == 65536 > BP.GRID_BLOCKS and gridlimits.trips(S, BP.GRID_BLOCKS) == 4 and BP.GRID_BLOCKS % gridlimits.P
    rng = np.random.default_rng(22)
    cells = rng.integers(-200, 201, (gridlimits.P, 4, 4)).astype(np.int16)
    cells[rng.random(cells.shape) < 0.5] = 0
    cells[::7] = 0
    picks = gridlimits.tile(cells, S).reshape(256, 256, 4, 4)  # block s = by * 256 + bx holds cell s % 251
    v = np.ascontiguousarray(picks.transpose(0, 2, 1, 3)).reshape(1, H, W)
    lay = Lay(np.int16, 1, W, H)
    round_trip(dwt, lay, bpm.I16, v, 0, 2, 2, slack=0)


def test_frames_past_the_batch_cap(dwt):
    """5 frames more than one trip of the scan's loop covers, 8 x 8 samples each, frames repeating with period 251"""
    BP = dwt.bitplanes
    B, W, H, J = BP.GRID_BATCH + 5, 8, 8, 1
    assert BP.GRID_BATCH % gridlimits.P and gridlimits.trips(B, BP.GRID_BATCH) == 2
    frames = np.random.default_rng(23).integers(-9, 10, (gridlimits.P, H, W)).astype(np.int32)
    frames[::5, :4] = 0
    words, off = bpm.pack(frames, bpm.I32, J, 2, 2)
    v = gridlimits.tile(frames, B, axis=0)
    want_words, want_off = gridlimits.tile(words, B, axis=0), gridlimits.tile(off, B, axis=0)
    lay = Lay(np.int32, B, W, H)
    got_words, got_off = run_pack(dwt, lay, bpm.I32, v, J, 2, 2, words.shape[1])
    assert np.array_equal(got_off, want_off)
    written = np.arange(words.shape[1])[None, :] < want_off[:, -1:]
    assert np.array_equal(got_words, np.where(written, want_words, np.uint64(POISON64))), np.argwhere(got_words != np.where(written, want_words, np.uint64(POISON64)))[:5]
    check_unpack(dwt, lay, bpm.I32, got_words, got_off, J, 2, 2, v)


# ---- the flow -------------------------------------------------------------------------------------------------------
def test_picture_quantize_pack_unpack_dequantize(dwt):
    """pixels -> 9/7 planes -> int16 indices -> words -> indices -> coefficients: the bytes of the flow without the detour"""
    from libdwt_amd import pixels as P
    from libdwt_amd import quant as Q

    BP = dwt.bitplanes
    B, W, H, J = 2, 256, 192, 4
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(24)
    pix = np.stack([np.stack([(128 + 100 * np.sin(xx / (9.0 + b + c)) * np.cos(yy / 13.0) + rng.normal(0, 3, (H, W))).clip(0, 255) for c in range(3)], -1)
                    for b in range(B)]).astype(np.uint8)
    n = 3 * B
    dpix, coef = Dev(dwt, pix), Dev(dwt, np.zeros((n, H, W), np.float32))
    assert P.picture_forward_batch(dwt.CDF97_S, P.U8, dpix.ptr, 3 * W * H, 3 * W, 3, 1, B, 3, P.RGB, 8, 128, 1.0, P.ICT, coef.ptr, 4 * W * H, 4 * W, W, H, J) == J
    steps = Q.quant_steps(dwt.CDF97_S, J, 4.0)
    idx = Dev(dwt, np.zeros((n, H, W), np.int16))
    Q.quantize_batch(Q.S, coef.ptr, 4 * W * H, 4 * W, Q.I16, idx.ptr, 2 * W * H, 2 * W, n, W, H, J, steps)
    q = idx.get()
    off = BP.count_batch(BP.I16, idx.ptr, 2 * W * H, 2 * W, n, W, H, J, 6, 6)
    model_words, model_off = bpm.pack(q, bpm.I16, J, 6, 6)
    assert np.array_equal(off, model_off) and 0 < off[:, -1].max() * 8 < 2 * W * H
    cap = int(off[:, -1].max())
    words, doff = Dev(dwt, np.zeros((n, cap), np.uint64)), Dev(dwt, np.zeros_like(off))
    BP.pack_batch(BP.I16, idx.ptr, 2 * W * H, 2 * W, n, W, H, J, 6, 6, words.ptr, cap, doff.ptr)
    assert np.array_equal(words.get(), model_words)
    back = Dev(dwt, np.full((n, H, W), -77, np.int16))
    BP.unpack_batch(BP.I16, words.ptr, cap, doff.ptr, back.ptr, 2 * W * H, 2 * W, n, W, H, J, 6, 6)
    assert np.array_equal(back.get(), q)
    a, b = Dev(dwt, np.zeros((n, H, W), np.float32)), Dev(dwt, np.zeros((n, H, W), np.float32))
    Q.dequantize_batch(Q.I16, back.ptr, 2 * W * H, 2 * W, Q.S, a.ptr, 4 * W * H, 4 * W, n, W, H, J, steps)
    Q.dequantize_batch(Q.I16, idx.ptr, 2 * W * H, 2 * W, Q.S, b.ptr, 4 * W * H, 4 * W, n, W, H, J, steps)
    assert np.array_equal(a.get().view(np.uint32), b.get().view(np.uint32))
    # one plane dropped: the indices of twice the step, up to the deadzone's rounding toward zero
    BP.unpack_batch(BP.I16, words.ptr, cap, doff.ptr, back.ptr, 2 * W * H, 2 * W, n, W, H, J, 6, 6, 1, BP.SHIFT)
    assert np.array_equal(back.get(), bpm.unpack(model_words, model_off, bpm.I16, W, H, J, 6, 6, 1, bpm.SHIFT))


# ---- stream, example ------------------------------------------------------------------------------------------------
def test_entries_run_on_the_callers_stream():
    """pack, count only and unpack (both routes) once on a non-blocking stream behind a bounded delay, in a process of its own
    (tests/bitplane_stream.py, on the harness of tests/stream_cases.py): the model's bits; the calls on device memory queued
    without waiting for the stream, pack with host offsets synchronous"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bitplane_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]


def test_example_picture_embedded(dwt, tmp_path):
    """examples/picture_embedded.c compiles with the gcc line of its header comment, runs and exits 0, on its synthetic
    picture and on a PPM"""
    exe, libdir = tmp_path / "picture_embedded", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "picture_embedded.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.count("PSNR") == 5 and "bytes" in out.stdout, out.stdout + out.stderr
    ppm = tmp_path / "t.ppm"
    rng = np.random.default_rng(25)
    ppm.write_bytes(b"P6\n# a comment\n67 45\n255\n" + rng.integers(0, 256, 67 * 45 * 3).astype(np.uint8).tobytes())
    out = subprocess.run([str(exe), str(ppm)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "67 x 45" in out.stdout and out.stdout.count("PSNR") == 5, out.stdout + out.stderr


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals(dwt):
    """every refusal of the header returns its code with a message, launches nothing and leaves poisoned buffers untouched"""
    BP = dwt.bitplanes
    W, H, J, B = 32, 16, 2, 2
    cap = 64
    S = int(bpm.bands(W, H, J, 2, 2)[-1, 4])
    lay = Lay(np.int32, B, W, H)
    planes = Dev(dwt, lay.fill())
    words, off = Dev(dwt, poisoned((B, cap), np.uint64)), Dev(dwt, poisoned((B, S + 1), np.uint32))
    big = Dev(dwt, np.full(1 << 16, POISON, np.uint8))
    n0 = dwt.get_option("stat_launches")

    def refused(itype=BP.I32, pargs=None, batch=B, w=W, h=H, cb=(2, 2), wp=words.ptr, o=off.ptr, stride=cap, drop=0, mode=BP.KEEP, only=None):
        pa = pargs or lay.args(planes.ptr)
        for unpack in (False, True):
            if only is not None and only != unpack:
                continue
            with pytest.raises(dwt.DwtError) as e:
                if unpack:
                    BP.unpack_batch(itype, wp, stride, o, *pa, batch, w, h, J, *cb, drop, mode)
                else:
                    BP.pack_batch(itype, *pa, batch, w, h, J, *cb, wp, stride, o)
            assert len(str(e.value)) > 20, str(e.value)

    refused(pargs=(0, lay.bs, lay.pitch))  # null pointers
    refused(o=0)
    refused(wp=0, only=True)  # (pack without words is the count-only call)
    refused(itype=2)
    refused(itype=-1)
    refused(mode=2, only=True)
    refused(mode=-1, only=True)
    refused(drop=-1, only=True)
    refused(drop=33, only=True)
    for cb in ((1, 2), (2, 1), (11, 2), (2, 11), (7, 6), (6, 7)):
        refused(cb=cb)
    refused(w=-1)
    refused(h=-3)
    refused(batch=-1)
    refused(w=65536, h=32768, pargs=(planes.ptr, 0, 4 * 65536), batch=1)  # size_x * size_y > INT_MAX
    refused(pargs=(planes.ptr, lay.bs, lay.pitch - 4))  # a pitch below its row
    refused(pargs=(planes.ptr, lay.bs - 4, lay.pitch))  # frames closer than they span
    refused(pargs=(planes.ptr + 2, lay.bs, lay.pitch))  # int32 on a 2-byte boundary
    refused(pargs=(planes.ptr, lay.bs, lay.pitch + 2))
    refused(pargs=(planes.ptr, lay.bs + 2, lay.pitch))
    refused(itype=BP.I16, pargs=(planes.ptr + 1, 2 * W * H, 2 * W))
    refused(wp=words.ptr + 4)  # the words on a 4-byte boundary
    refused(o=off.ptr + 2)
    # regions that share a byte: the planes with the words, the planes with the offsets, the words with the offsets
    refused(pargs=lay.args(big.ptr), wp=big.ptr + lay.bs * B - 8)
    refused(pargs=lay.args(big.ptr), o=big.ptr + lay.bs)
    refused(pargs=lay.args(planes.ptr), wp=big.ptr, o=big.ptr + 8 * cap * B - 4)
    with pytest.raises(dwt.DwtError):
        BP.count_batch(BP.I32, *lay.args(big.ptr), B, W, H, J, 2, 2, big.ptr + 4 * W)
    with pytest.raises(dwt.DwtError):
        BP.route(BP.I32, planes.ptr, lay.bs, lay.pitch - 4, B, W, H, J, 2, 2)
    with pytest.raises(dwt.DwtError):
        BP.route(7, planes.ptr, lay.bs, lay.pitch, B, W, H, J, 2, 2)
    with pytest.raises(dwt.DwtError):
        BP.route(BP.I32, planes.ptr, lay.bs, lay.pitch, B, W, H, J, 1, 2)
    assert dwt.get_option("stat_launches") == n0, "a refused call launched"
    dwt.sync()
    for d in (planes, words, off, big):
        assert (d.get().view(np.uint8) == POISON).all(), "a refused call wrote"
