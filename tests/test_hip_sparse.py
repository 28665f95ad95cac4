"""GPU checks of the sparse coefficient streams (dwt_hip_sparse_pack_batch, dwt_hip_sparse_unpack_batch;
libdwt_amd/sparse.py) against tests/sparse_model.py, bit for bit.  Every buffer is a run of poison bytes with the
frames' elements, the entries or the offsets laid into it; after a call the output holds the model's bytes and every
other byte of every buffer still holds the poison (the input: its own bytes too)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gridlimits
import shape_model as sm
import sparse_model as spm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
# bands one or two samples wide, narrower than a lane's run; empty HL / LH bands; two sizes with several rows per tile and
# tiles that end inside a row
SHAPES = [(5, 3, 2), (1, 37, -1), (37, 1, -1), (72, 40, 3), (264, 136, 3)]
PITCHES = ["dense", "prime", "padded16"]
PRIMES = (3, 7, 11, 41, 43, 67, 71, 73, 79, 131, 137, 269, 271, 277)
GUARD = 64 << 10


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d
    from libdwt_amd import sparse

    d.dwt_util_init()
    d.sparse = sparse
    assert (sparse.F32, sparse.F16, sparse.I16, sparse.I32) == (spm.F32, spm.F16, spm.I16, spm.I32)
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("sparse_wide", 1)


class Lay:
    """`batch` frames of W x H elements of `dtype` in a byte buffer: row pitch "dense", "prime" (an odd number of elements: no
    multiple of 16 bytes) or "padded16"; the base `base` bytes into the buffer; `gap` bytes between the frames; `tail` bytes
    behind the last frame"""

    def __init__(self, dtype, batch, W, H, pitch="dense", base=0, gap=0, tail=16):
        self.dtype = np.dtype(dtype)
        es = self.dtype.itemsize
        self.es, self.batch, self.W, self.H, self.base = es, batch, W, H, base
        row = W * es
        self.pitch = {"dense": row, "prime": es * next(p for p in PRIMES if p > W), "padded16": (row + 15) // 16 * 16 + 16}[pitch]
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


def levels(W, H, j_max):
    return sm.levels(W, H, j_max)


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


def contents(elem_type, what, B, H, W, J, seed=0):
    """the frames of one content class"""
    dt = spm.DTYPE[elem_type]
    rng = np.random.default_rng([seed, elem_type, B, H, W, len(what)])
    if what == "zeros":
        return np.zeros((B, H, W), dt)
    if dt.kind == "f":
        full = rng.normal(0, 30, (B, H, W)).astype(dt)
        full[full == 0] = 1
    else:
        info = np.iinfo(dt)
        full = rng.integers(1, int(info.max) + 1, (B, H, W)).astype(dt) * rng.choice([-1, 1], (B, H, W)).astype(dt)
    if what == "full":
        return full
    if what == "one":  # exactly one nonzero, at the last sample of HH(1) (the whole frame where there are no levels)
        v = np.zeros((B, H, W), dt)
        x0, y0, w, h = sm.slots(W, H, W, H, J)[2 if J else 0]
        if w and h:
            v[:, y0 + h - 1, x0 + w - 1] = full[:, 0, 0]
        else:
            v[:, H - 1, W - 1] = full[:, 0, 0]
        return v
    assert what == "random"  # frame b at density 0.001, 0.05, 0.5, ...; a row of the values whose bits matter
    v = full.copy()
    for b in range(B):
        v[b][rng.random((H, W)) >= (0.001, 0.05, 0.5)[b % 3]] = 0
    if dt.kind == "f":
        u = np.uint32 if dt.itemsize == 4 else np.uint16
        sign = 1 << (8 * dt.itemsize - 1)
        special = np.concatenate([np.array([-0.0, np.nan, np.inf, -np.inf, 0.0], dt).view(u),
                                  np.array([1, sign | 1, sign | 2, (sign >> 1) | 5, sign | (sign >> 1) | 7], u)])  # subnormals, 0x80000001, NaN payloads
        special = special.view(dt)
    else:
        special = np.array([np.iinfo(dt).min, -1, 1, np.iinfo(dt).max, 0], dt)
    flat = v[B - 1].reshape(-1)
    n = min(len(special), flat.size)
    flat[flat.size - n:] = special[:n]  # (the last row: the end of HH(1), behind everything else in its band)
    return v


def run_pack(dwt, lay, elem_type, values, j_max, capacity, device=(True, True, True), count_only=False):
    """one call -> (pos, val, offsets) as the model returns them; asserts that the planes kept every byte"""
    S = dwt.sparse
    B, W, H = lay.batch, lay.W, lay.H
    J = levels(W, H, j_max)
    planes = lay.fill(values)
    pos, val = poisoned((B, capacity), np.uint32), poisoned((B, capacity), lay.dtype)
    off = poisoned((B, 3 * J + 2), np.uint32)
    hold = []
    pp, op = place(dwt, hold, planes, device[0]), place(dwt, hold, off, device[2])
    if count_only:
        S.count_batch(elem_type, *lay.args(pp), B, W, H, j_max, op)
    else:
        sp, vp = place(dwt, hold, pos, device[1]), place(dwt, hold, val, device[1])
        S.pack_batch(elem_type, *lay.args(pp), B, W, H, j_max, sp, vp, capacity, op)
    dwt.sync()
    got_planes, got_off = fetch(hold, planes, device[0]), fetch(hold, off, device[2])
    if not count_only:
        pos, val = fetch(hold, pos, device[1]), fetch(hold, val, device[1])
    assert np.array_equal(got_planes, lay.fill(values)), "the planes were written"
    return pos, val, got_off


def check_pack(dwt, lay, elem_type, values, j_max, capacity=None, slack=3, **kw):
    """pack against the model: entries, the poison behind them, the true offsets.  capacity None: the largest total + slack"""
    J = levels(lay.W, lay.H, j_max)
    values = np.ascontiguousarray(values, lay.dtype)
    all_pos, all_val, want_off = spm.pack(values, elem_type, J)
    if capacity is None:
        capacity = all_pos.shape[1] + slack
    want_pos, want_val = poisoned((lay.batch, capacity), np.uint32), poisoned((lay.batch, capacity), spm.UINT[lay.es])
    for b in range(lay.batch):
        n = min(int(want_off[b, -1]), capacity)
        want_pos[b, :n], want_val[b, :n] = all_pos[b, :n], spm.bits(all_val)[b, :n]
    pos, val, off = run_pack(dwt, lay, elem_type, values, j_max, capacity, **kw)
    assert np.array_equal(off, want_off), (off, want_off)
    assert np.array_equal(pos, want_pos), np.argwhere(pos != want_pos)[:5]
    assert np.array_equal(spm.bits(val), want_val), np.argwhere(spm.bits(val) != want_val)[:5]
    return pos, val, off


def run_unpack(dwt, lay, elem_type, pos, val, counts, counts_stride=1, device=(True, True, True), before=None):
    """one call into poisoned frames -> the buffer after it"""
    S = dwt.sparse
    planes = lay.fill(before)
    hold = []
    pp = place(dwt, hold, planes, device[0])
    sp, vp = place(dwt, hold, np.ascontiguousarray(pos, np.uint32), device[1]), place(dwt, hold, np.ascontiguousarray(val, lay.dtype), device[1])
    cp = place(dwt, hold, np.ascontiguousarray(counts, np.uint32), device[2])
    S.unpack_batch(elem_type, sp, vp, pos.shape[1], cp, counts_stride, *lay.args(pp), lay.batch, lay.W, lay.H)
    dwt.sync()
    return fetch(hold, planes, device[0])


def check_unpack(dwt, lay, elem_type, pos, val, counts, want, **kw):
    got = run_unpack(dwt, lay, elem_type, pos, val, counts, **kw)
    assert (got[~lay.own] == POISON).all(), "bytes outside the frames were written"
    assert np.array_equal(spm.bits(lay.read(got)), spm.bits(np.ascontiguousarray(want, lay.dtype))), np.argwhere(spm.bits(lay.read(got)) != spm.bits(want))[:5]


def round_trip(dwt, lay, elem_type, values, j_max, device=(True, True, True), **kw):
    J = levels(lay.W, lay.H, j_max)
    pos, val, off = check_pack(dwt, lay, elem_type, values, j_max, device=device, **kw)
    check_unpack(dwt, lay, elem_type, pos, val, off[:, -1], spm.coarser(values, elem_type, J, 3 * J + 1), device=device)
    return pos, val, off


# ---- shapes, types, pitches, contents ---------------------------------------------------------------------------------
def test_the_tile_size_cuts_the_large_shape():
    """at 264 x 136 HL(1) spans at least three tiles and a tile boundary falls inside a row"""
    from libdwt_amd import sparse as S

    W, H, J = SHAPES[-1]
    x0, y0, w, h = sm.slots(W, H, W, H, J)[0]
    assert (w, h) == (132, 68) and w * h > 2 * S.TILE_SAMPLES and S.TILE_SAMPLES % w != 0


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_shapes_pitches_types_and_contents(dwt, W, H, j_max, pitch):
    """the four types, three frames: all zeros, all nonzero, one nonzero at the end of HH(1), three densities with the
    special values -- entries, offsets and the way back are the model's; padded16 takes the wide route, prime the element route"""
    J = levels(W, H, j_max)
    assert J == dwt.band_levels(W, H, j_max)
    for elem_type in spm.TYPES:
        lay = Lay(spm.DTYPE[elem_type], 3, W, H, pitch)
        if pitch == "padded16":
            assert dwt.sparse.sparse_route(elem_type, 4096, lay.bs, lay.pitch, 3, W, H) == 1
        if pitch == "prime" and H > 1:
            assert dwt.sparse.sparse_route(elem_type, 4096, lay.bs, lay.pitch, 3, W, H) == 0
        for what in ("zeros", "full", "one", "random"):
            v = contents(elem_type, what, 3, H, W, J)
            _, _, off = round_trip(dwt, lay, elem_type, v, j_max)
            if what == "one":
                assert off[:, -1].tolist() == [1, 1, 1]
            if what == "full":
                assert off[:, -1].tolist() == [W * H] * 3
            if what == "random" and W * H > 2000:
                assert off[0, -1] < off[1, -1] < off[2, -1], "the frames' densities differ"


@pytest.mark.parametrize("elem_type", spm.TYPES)
def test_special_values_keep_their_bits(dwt, elem_type):
    """-0.0 is dropped and comes back as +0.0; NaN, the infinities, subnormals, 0x80000001 / INT_MIN, -1 and 1 are kept"""
    W, H, J = 72, 40, 3
    lay = Lay(spm.DTYPE[elem_type], 3, W, H)
    v = contents(elem_type, "random", 3, H, W, J, seed=5)
    pos, val, off = round_trip(dwt, lay, elem_type, v, J)
    last = spm.bits(v[2]).reshape(-1)[-10:] if lay.dtype.kind == "f" else spm.bits(v[2]).reshape(-1)[-5:]
    n = int(off[2, -1])
    tail = spm.bits(val)[2, :n][pos[2, :n] >= W * H - len(last)]
    sign = 1 << (8 * lay.es - 1)
    kept = [int(x) for x in last if (int(x) & (sign - 1 if lay.dtype.kind == "f" else -1)) != 0]
    assert tail.tolist() == kept and len(kept) == (8 if lay.dtype.kind == "f" else 4)


# ---- routes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [2, 4])
def test_unaligned_bases_take_the_element_route(dwt, base):
    W, H, J = 264, 136, 3
    for elem_type in spm.TYPES:
        if base % spm.DTYPE[elem_type].itemsize:
            continue  # (a 4-byte element 2 bytes off its size is refused: test_refusals)
        lay = Lay(spm.DTYPE[elem_type], 2, W, H, "padded16", base=base)
        assert dwt.sparse.sparse_route(elem_type, 4096 + base, lay.bs, lay.pitch, 2, W, H) == 0
        round_trip(dwt, lay, elem_type, contents(elem_type, "random", 2, H, W, J, seed=6), J)


@pytest.mark.parametrize("elem_type", spm.TYPES)
def test_wide_route_and_element_route_give_the_same_bytes(dwt, elem_type):
    W, H, J = 264, 136, 3
    lay = Lay(spm.DTYPE[elem_type], 2, W, H, "padded16")
    v = contents(elem_type, "random", 2, H, W, J, seed=7)
    results = []
    for wide in (1, 0):
        dwt.set_option("sparse_wide", wide)
        try:
            assert dwt.sparse.sparse_route(elem_type, 4096, lay.bs, lay.pitch, 2, W, H) == wide
            results.append(round_trip(dwt, lay, elem_type, v, J))
        finally:
            dwt.set_option("sparse_wide", 1)
    for a, b in zip(*results):
        assert a.tobytes() == b.tobytes()


# ---- capacity, count only -------------------------------------------------------------------------------------------
def test_capacity(dwt):
    """stream_stride the largest total, one less than a frame's total, off[k] of a middle band, 0: the first entries in
    stream order, poison behind them, the true totals in the offsets; a truncated stream unpacks to the coarser frame"""
    W, H, J = 72, 40, 3
    for elem_type in (spm.F32, spm.I16):
        lay = Lay(spm.DTYPE[elem_type], 3, W, H, "padded16")
        v = contents(elem_type, "random", 3, H, W, J, seed=8)
        _, _, off = spm.pack(v, elem_type, J)
        k = 5
        assert 0 < off[2, k] < off[2, -1] and off[1, -1] > 1
        for cap in (int(off[:, -1].max()), int(off[1, -1]) - 1, int(off[2, k]), 0):
            pos, val, got_off = check_pack(dwt, lay, elem_type, v, J, capacity=cap)
            assert np.array_equal(got_off, off)
            want = spm.unpack(pos, val, off[:, -1], elem_type, H, W)
            check_unpack(dwt, lay, elem_type, pos, val, off[:, -1], want)
        pos, val, _ = check_pack(dwt, lay, elem_type, v, J, capacity=int(off[2, k]))
        got = lay.read(run_unpack(dwt, lay, elem_type, pos, val, off[:, -1]))
        assert np.array_equal(spm.bits(got[2]), spm.bits(spm.coarser(v, elem_type, J, k)[2]))


@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_count_only_equals_packs_offsets(dwt, W, H, j_max):
    J = levels(W, H, j_max)
    for elem_type in (spm.F16, spm.I32):
        lay = Lay(spm.DTYPE[elem_type], 3, W, H, "prime")
        v = contents(elem_type, "random", 3, H, W, J, seed=9)
        _, _, counted = run_pack(dwt, lay, elem_type, v, j_max, 0, count_only=True)
        _, _, packed = check_pack(dwt, lay, elem_type, v, j_max)
        assert np.array_equal(counted, packed)
    # the wrapper's own array
    planes = Dev(dwt, lay.fill(v))
    ret = dwt.sparse.count_batch(elem_type, *lay.args(planes.ptr), 3, W, H, j_max)
    assert ret.dtype == np.uint32 and np.array_equal(ret, packed)


# ---- unpack ---------------------------------------------------------------------------------------------------------
def test_unpack_skips_positions_outside_the_frame(dwt):
    """a foreign stream with positions size_x * size_y and size_x * size_y + 3: skipped.  The frames lie in front of a 64 KiB
    guard of the same allocation: a missing check would land there (or in the poison between the frames), not outside"""
    W, H = 72, 40
    for elem_type in (spm.F32, spm.I16):
        lay = Lay(spm.DTYPE[elem_type], 2, W, H, "padded16", gap=64, tail=GUARD)
        pos = np.array([[5, W * H, W * H + 3, W * H - 1], [W * H + 3, 0, W * H, 7]], np.uint32)
        val = np.array([[11, 12, 13, 14], [21, 22, 23, 24]], lay.dtype)
        want = np.zeros((2, H * W), lay.dtype)
        want[0, 5], want[0, W * H - 1], want[1, 0], want[1, 7] = 11, 14, 22, 24
        check_unpack(dwt, lay, elem_type, pos, val, [4, 4], want.reshape(2, H, W))


def test_unpack_reads_counts_with_a_stride(dwt):
    """pack's totals where they lie: offsets + 3J + 1 with counts_stride 3J + 2; and counts smaller than the totals"""
    W, H, J = 72, 40, 3
    S = dwt.sparse
    lay = Lay(np.int16, 3, W, H, "prime", gap=6)
    v = contents(spm.I16, "random", 3, H, W, J, seed=10)
    pos, val, off = spm.pack(v, spm.I16, J)
    cap = pos.shape[1]
    for device in (True, False):
        planes = lay.fill()
        hold = []
        pp, sp, vp = place(dwt, hold, planes, True), place(dwt, hold, pos, True), place(dwt, hold, val, True)
        op = place(dwt, hold, off, device)
        S.unpack_batch(S.I16, sp, vp, cap, op + 4 * (3 * J + 1), 3 * J + 2, *lay.args(pp), 3, W, H)
        dwt.sync()
        got = hold[0].get()
        assert (got[~lay.own] == POISON).all() and np.array_equal(lay.read(got), spm.coarser(v, spm.I16, J, 3 * J + 1))
    cut = np.array([off[0, 4], 0, off[2, -1]], np.uint32)
    check_unpack(dwt, lay, spm.I16, pos, val, cut, spm.unpack(pos, val, cut, spm.I16, H, W))
    # a count beyond the capacity stops at the capacity
    assert off[2, -1] >= 7
    pos7, val7 = np.tile(pos[2:3, :7], (3, 1)), np.tile(val[2:3, :7], (3, 1))
    check_unpack(dwt, lay, spm.I16, pos7, val7, [1 << 30] * 3, spm.unpack(pos7, val7, [7] * 3, spm.I16, H, W))


# ---- memory spaces --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [(p, s, o) for p in (False, True) for s in (False, True) for o in (False, True) if not (p and s and o)])
def test_host_sides_give_the_device_calls_bytes(dwt, device):
    """each of the planes, the stream and the offsets / counts in host memory: the model's bytes (which the device call
    gives), every poison byte kept -- with pitch padding and a gap, where the regions hold bytes that are not the frames'"""
    for elem_type, pitch, gap, (W, H, j_max) in ((spm.F32, "dense", 0, (72, 40, 3)), (spm.I16, "prime", 6, (37, 1, -1)), (spm.F16, "padded16", 32, (264, 136, 3))):
        lay = Lay(spm.DTYPE[elem_type], 3, W, H, pitch, gap=gap)
        v = contents(elem_type, "random", 3, H, W, levels(W, H, j_max), seed=11)
        round_trip(dwt, lay, elem_type, v, j_max, device=device)
        _, _, counted = run_pack(dwt, lay, elem_type, v, j_max, 0, device=device, count_only=True)
        assert np.array_equal(counted, spm.pack(v, elem_type, levels(W, H, j_max))[2])


# ---- launches, allocation -------------------------------------------------------------------------------------------
def test_launches_and_no_allocation_on_device_memory(dwt):
    """pack 3 launches, count only 2, unpack 2 -- for one frame and three, for planes of zeros and planes without a zero;
    the second round allocates nothing; no frames: no launch"""
    S = dwt.sparse
    W, H, J = 264, 136, 3
    cap = W * H
    counts = {}
    bufs = []
    for B in (1, 3):
        for what in ("zeros", "full"):
            lay = Lay(np.float32, B, W, H)
            planes = Dev(dwt, lay.fill(contents(spm.F32, what, B, H, W, J)))
            pos, val, off = Dev(dwt, np.zeros((B, cap), np.uint32)), Dev(dwt, np.zeros((B, cap), np.float32)), Dev(dwt, np.zeros((B, 3 * J + 2), np.uint32))
            out = Dev(dwt, lay.fill())
            calls = (lambda: S.pack_batch(S.F32, *lay.args(planes.ptr), B, W, H, J, pos.ptr, val.ptr, cap, off.ptr),
                     lambda: S.count_batch(S.F32, *lay.args(planes.ptr), B, W, H, J, off.ptr),
                     lambda: S.unpack_batch(S.F32, pos.ptr, val.ptr, cap, off.ptr + 4 * (3 * J + 1), 3 * J + 2, *lay.args(out.ptr), B, W, H))
            for f in calls:  # the first call of a size may grow the workspace
                f()
            allocs = dwt.get_option("stat_allocs")
            counts[B, what] = [launches(dwt, f) for f in calls]
            assert dwt.get_option("stat_allocs") == allocs
            assert np.array_equal(lay.read(out.get()), spm.coarser(lay.read(planes.get()), spm.F32, J, 3 * J + 1))
            bufs.append((lay, planes, pos, val, off))
    assert all(c == [3, 2, 2] for c in counts.values()), counts
    lay, planes, pos, val, off = bufs[-1]
    assert launches(dwt, lambda: S.pack_batch(S.F32, *lay.args(planes.ptr), 0, W, H, J, pos.ptr, val.ptr, cap, off.ptr)) == 0
    assert launches(dwt, lambda: S.count_batch(S.F32, *lay.args(planes.ptr), 0, W, H, J, off.ptr)) == 0
    assert launches(dwt, lambda: S.unpack_batch(S.F32, pos.ptr, val.ptr, cap, off.ptr, 1, *lay.args(planes.ptr), 0, W, H)) == 0


def test_empty_frames_launch_nothing_and_write_zero_offsets(dwt):
    S = dwt.sparse
    for device in (True, False):
        off = poisoned((2, 5), np.uint32)  # (one level: 3 + 2 words a frame)
        hold = []
        op = place(dwt, hold, off, device)
        assert launches(dwt, lambda: S.count_batch(S.I16, 4096, 0, 0, 2, 0, 9, 1, op)) == 0
        dwt.sync()
        assert not fetch(hold, off, device).any()


# ---- grid caps ------------------------------------------------------------------------------------------------------
def test_tiles_past_the_grid_cap(dwt):
    """a narrow, tall frame with more tiles than one trip of the tile loop covers (and more rows than one trip of the zero
    fill's row loop), rows repeating with period 251 (tests/gridlimits.py): a tile taken one cap away from where it belongs
    meets other data"""
    S = dwt.sparse
    W, J = 8, 2
    H = (S.GRID_TILES + 40) * S.TILE_SAMPLES // W
    tiles = int(S.stream_bands(W, H, J)[-1, 4])
    assert tiles > S.GRID_TILES and gridlimits.trips(tiles, S.GRID_TILES) == 2 and S.GRID_TILES % gridlimits.P and H > 4 * S.GRID_TILES
    rng = np.random.default_rng(12)
    rows = rng.integers(1, 30000, (1, gridlimits.P, W)).astype(np.int16)
    rows[rng.random(rows.shape) < 0.9] = 0
    v = gridlimits.tile(rows, H, axis=1)
    lay = Lay(np.int16, 1, W, H)
    round_trip(dwt, lay, spm.I16, v, J, slack=0)


def test_frames_past_the_grid_cap(dwt):
    """5 frames more than one trip of the batch loops covers, 3 x 2 samples each, frames repeating with period 251"""
    S = dwt.sparse
    B, W, H, J = S.GRID_BATCH + 5, 3, 2, 1
    assert S.GRID_BATCH % gridlimits.P and gridlimits.trips(B, S.GRID_BATCH) == 2
    frames = np.random.default_rng(13).integers(-3, 4, (gridlimits.P, H, W)).astype(np.int32)
    v = gridlimits.tile(frames, B, axis=0)
    lay = Lay(np.int32, B, W, H)
    round_trip(dwt, lay, spm.I32, v, J)


# ---- flows ----------------------------------------------------------------------------------------------------------
def picture_planes(dwt, B, W, H, J, seed):
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(seed)
    img = np.stack([100 * np.sin(xx / (9.0 + b)) * np.cos(yy / 13.0) + ((xx * 3 + yy * 2) % 64) + rng.normal(0, 3, (H, W)) for b in range(B)]).astype(np.float32)
    src, dst = Dev(dwt, img), Dev(dwt, np.zeros_like(img))
    assert dwt.transform2d_batch("cdf97_s", 0, src.ptr, dst.ptr, 4 * W * H, B, 4 * W, W, H, J) == J
    return dst


def test_keep_largest_then_pack_unpack_inverse(dwt):
    """keep = 1 % of a 9/7 frame, packed, unpacked and inverted: the inverse of the kept planes"""
    S = dwt.sparse
    B, W, H, J = 2, 256, 192, 4
    planes = picture_planes(dwt, B, W, H, J, 14)
    keep = W * H // 100
    dwt.keep_largest_batch(planes.ptr, 4 * W * H, B, 1, 0, 4 * W, W, H, keep, J)
    kept = planes.get()
    off = S.count_batch(S.F32, planes.ptr, 4 * W * H, 4 * W, B, W, H, J)
    assert np.array_equal(off, spm.pack(kept, spm.F32, J)[2]) and (off[:, -1] <= keep).all() and (off[:, -1] > keep // 2).all()
    cap = int(off[:, -1].max())
    pos, val, doff = Dev(dwt, np.zeros((B, cap), np.uint32)), Dev(dwt, np.zeros((B, cap), np.float32)), Dev(dwt, np.zeros_like(off))
    S.pack_batch(S.F32, planes.ptr, 4 * W * H, 4 * W, B, W, H, J, pos.ptr, val.ptr, cap, doff.ptr)
    back = Dev(dwt, np.full((B, H, W), np.nan, np.float32))
    S.unpack_batch(S.F32, pos.ptr, val.ptr, cap, doff.ptr + 4 * (3 * J + 1), 3 * J + 2, back.ptr, 4 * W * H, 4 * W, B, W, H)
    assert np.array_equal(spm.bits(back.get()), spm.bits(spm.coarser(kept, spm.F32, J, 3 * J + 1)))
    a, b = Dev(dwt, np.zeros((B, H, W), np.float32)), Dev(dwt, np.zeros((B, H, W), np.float32))
    dwt.transform2d_batch("cdf97_s", 1, back.ptr, a.ptr, 4 * W * H, B, 4 * W, W, H, J)
    dwt.transform2d_batch("cdf97_s", 1, planes.ptr, b.ptr, 4 * W * H, B, 4 * W, W, H, J)
    assert np.array_equal(spm.bits(a.get()), spm.bits(b.get()))


def test_quantize_then_pack_unpack_dequantize(dwt):
    """int16 indices of a 9/7 frame packed, unpacked and dequantized: the dequantized indices"""
    from libdwt_amd import quant as Q

    S = dwt.sparse
    B, W, H, J = 2, 256, 192, 4
    planes = picture_planes(dwt, B, W, H, J, 15)
    steps = Q.quant_steps(dwt.CDF97_S, J, 4.0)
    idx = Dev(dwt, np.zeros((B, H, W), np.int16))
    Q.quantize_batch(Q.S, planes.ptr, 4 * W * H, 4 * W, Q.I16, idx.ptr, 2 * W * H, 2 * W, B, W, H, J, steps)
    q = idx.get()
    off = S.count_batch(S.I16, idx.ptr, 2 * W * H, 2 * W, B, W, H, J)
    assert np.array_equal(off[:, -1], (q != 0).reshape(B, -1).sum(1)) and 0 < off[:, -1].max() < W * H // 2
    cap = int(off[:, -1].max())
    pos, val, doff = Dev(dwt, np.zeros((B, cap), np.uint32)), Dev(dwt, np.zeros((B, cap), np.int16)), Dev(dwt, np.zeros_like(off))
    S.pack_batch(S.I16, idx.ptr, 2 * W * H, 2 * W, B, W, H, J, pos.ptr, val.ptr, cap, doff.ptr)
    back = Dev(dwt, np.full((B, H, W), -77, np.int16))
    S.unpack_batch(S.I16, pos.ptr, val.ptr, cap, doff.ptr + 4 * (3 * J + 1), 3 * J + 2, back.ptr, 2 * W * H, 2 * W, B, W, H)
    assert np.array_equal(back.get(), q)
    a, b = Dev(dwt, np.zeros((B, H, W), np.float32)), Dev(dwt, np.zeros((B, H, W), np.float32))
    Q.dequantize_batch(Q.I16, back.ptr, 2 * W * H, 2 * W, Q.S, a.ptr, 4 * W * H, 4 * W, B, W, H, J, steps)
    Q.dequantize_batch(Q.I16, idx.ptr, 2 * W * H, 2 * W, Q.S, b.ptr, 4 * W * H, 4 * W, B, W, H, J, steps)
    assert np.array_equal(spm.bits(a.get()), spm.bits(b.get()))


# ---- stream, example ------------------------------------------------------------------------------------------------
def test_entries_run_on_the_callers_stream():
    """pack, count only and unpack (both routes) once on a non-blocking stream behind a bounded delay, in a process of its own
    (tests/sparse_stream.py, on the harness of tests/stream_cases.py): the model's bits; the calls on device memory queued
    without waiting for the stream"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sparse_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]


def test_example_picture_sparse(dwt, tmp_path):
    """examples/picture_sparse.c compiles with the gcc line of its header comment, runs and exits 0, on its synthetic picture
    and on a PPM"""
    exe, libdir = tmp_path / "picture_sparse", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "picture_sparse.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.count("PSNR") == 2 and "bytes" in out.stdout, out.stdout + out.stderr
    ppm = tmp_path / "t.ppm"
    rng = np.random.default_rng(16)
    ppm.write_bytes(b"P6\n# a comment\n67 45\n255\n" + rng.integers(0, 256, 67 * 45 * 3).astype(np.uint8).tobytes())
    out = subprocess.run([str(exe), str(ppm)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "67 x 45" in out.stdout and out.stdout.count("PSNR") == 2, out.stdout + out.stderr


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals(dwt):
    """every refusal of the header returns its code with a message and leaves poisoned buffers untouched"""
    S = dwt.sparse
    W, H, J, B = 32, 16, 2, 2
    cap = 64
    lay = Lay(np.float32, B, W, H)
    planes = Dev(dwt, lay.fill())
    pos, val, off = Dev(dwt, poisoned((B, cap), np.uint32)), Dev(dwt, poisoned((B, cap), np.float32)), Dev(dwt, poisoned((B, 3 * J + 2), np.uint32))
    big = Dev(dwt, np.full(1 << 16, POISON, np.uint8))

    def refused(etype=S.F32, pargs=None, batch=B, w=W, h=H, p=pos.ptr, v=val.ptr, o=off.ptr, stride=cap, only=None):
        pa = pargs or lay.args(planes.ptr)
        for unpack in (False, True):
            if only is not None and only != unpack:
                continue
            with pytest.raises(dwt.DwtError) as e:
                if unpack:
                    S.unpack_batch(etype, p, v, stride, o, 1, *pa, batch, w, h)
                else:
                    S.pack_batch(etype, *pa, batch, w, h, J, p, v, stride, o)
            assert len(str(e.value)) > 20, str(e.value)

    refused(pargs=(0, lay.bs, lay.pitch))  # null pointers
    refused(o=0)
    refused(p=0, only=True)
    refused(v=0, only=True)
    refused(p=0, only=False)  # values without positions
    refused(v=0, only=False)  # positions without values
    refused(etype=4)
    refused(etype=-1)
    refused(w=-1)
    refused(h=-3)
    refused(batch=-1)
    refused(w=65536, h=32768, pargs=(planes.ptr, 0, 4 * 65536), batch=1)  # size_x * size_y > INT_MAX
    refused(pargs=(planes.ptr, lay.bs, lay.pitch - 4))  # a pitch below its row
    refused(pargs=(planes.ptr, lay.bs - 4, lay.pitch))  # frames closer than they span
    refused(pargs=(planes.ptr + 2, lay.bs, lay.pitch))  # binary32 on a 2-byte boundary
    refused(pargs=(planes.ptr, lay.bs, lay.pitch + 2))
    refused(pargs=(planes.ptr, lay.bs + 2, lay.pitch))
    refused(p=pos.ptr + 2)
    refused(v=val.ptr + 2)
    refused(o=off.ptr + 2)
    refused(etype=S.I16, v=val.ptr + 1, pargs=(planes.ptr, 2 * W * H, 2 * W))
    # the planes share a byte with the positions, the values, the offsets / counts
    refused(pargs=lay.args(big.ptr), p=big.ptr + lay.bs * B - 4)
    refused(pargs=lay.args(big.ptr), v=big.ptr + 8)
    refused(pargs=lay.args(big.ptr), o=big.ptr + lay.bs)
    with pytest.raises(dwt.DwtError):
        S.count_batch(S.F32, *lay.args(big.ptr), B, W, H, J, big.ptr + 4 * W)
    with pytest.raises(dwt.DwtError):
        S.sparse_route(S.F32, planes.ptr, lay.bs, lay.pitch - 4, B, W, H)
    with pytest.raises(dwt.DwtError):
        S.sparse_route(7, planes.ptr, lay.bs, lay.pitch, B, W, H)
    dwt.sync()
    for d in (planes, pos, val, off, big):
        assert (d.get().view(np.uint8) == POISON).all(), "a refused call wrote"
