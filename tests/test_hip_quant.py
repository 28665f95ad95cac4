"""GPU checks of the deadzone quantizer (dwt_hip_quantize_batch, dwt_hip_dequantize_batch, dwt_hip_codeblock_bitplanes_batch;
libdwt_amd/quant.py) against tests/quant_model.py, bit for bit.  Every buffer is a run of canary bytes with the frames'
elements laid into it; after a call the output's elements hold the model's bytes and every other byte of every buffer still
holds the canary (the input: its own bytes too)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gridlimits
import quant_model as qm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
F = np.float32
# the smallest frames at which the band lookup can go wrong: odd sizes at three levels; empty and one-sample bands at full
# depth; one row, one column; a long odd row; band edges inside a lane's run on the wide route; one slot
SHAPES = [(37, 53, 3), (5, 7, -1), (64, 1, -1), (1, 64, -1), (1001, 9, -1), (1024, 8, 5), (130, 66, 0)]
PAIRS = [(qm.S, qm.I16), (qm.S, qm.I32), (qm.H, qm.I16), (qm.H, qm.I32)]
PRIMES = (3, 7, 11, 67, 71, 131, 137, 1009, 1013, 1031)


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d
    from libdwt_amd import quant

    d.dwt_util_init()
    d.quant = quant
    assert (quant.GRID_ROWS, quant.GRID_BATCH) == (16384, 4096) and (quant.S, quant.H, quant.I16, quant.I32) == (qm.S, qm.H, qm.I16, qm.I32)
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("quant_wide", 1)


# ---- layouts: where the elements of the frames lie in a byte buffer ------------------------------------------------
class Lay:
    """`batch` frames of W x H elements of `dtype` in a byte buffer: row pitch "dense", "prime" (a prime number of elements: no
    multiple of 16 bytes) or "padded16"; the base `base` bytes into the buffer; `gap` bytes between the frames"""

    def __init__(self, dtype, batch, W, H, pitch="dense", base=0, gap=0):
        self.dtype = np.dtype(dtype)
        es = self.dtype.itemsize
        self.es, self.batch, self.W, self.H, self.base = es, batch, W, H, base
        row = W * es
        self.pitch = {"dense": row, "prime": es * next(p for p in PRIMES if p > W), "padded16": (row + 15) // 16 * 16 + 16}[pitch]
        self.bs = self.pitch * H + gap
        self.nbytes = base + self.bs * batch + 16
        b, y, x = np.ix_(np.arange(batch), np.arange(H), np.arange(W))
        self.at = base + b * self.bs + y * self.pitch + x * es  # (B, H, W) byte offsets
        self.own = np.zeros(self.nbytes, bool)
        for k in range(es):
            self.own[self.at + k] = True

    def fill(self, values=None):
        buf = np.full(self.nbytes, CANARY, np.uint8)
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


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


SPECIALS = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 1e9, -1e9, 3e38, 40000.0, -70000.0, 0.999, 1.0]


def rand_coef(shape, dtype, seed):
    """coefficients of three magnitudes, the special values scattered over them"""
    rng = np.random.default_rng([seed] + list(shape))
    v = rng.normal(0, 40, shape) * rng.choice([0.01, 1.0, 30.0], shape)
    flat = v.reshape(-1)
    at = rng.choice(flat.size, min(len(SPECIALS), flat.size), replace=False)
    flat[at] = SPECIALS[:len(at)]
    with np.errstate(over="ignore"):
        return v.astype(dtype)


def rand_index(shape, dtype, seed):
    rng = np.random.default_rng([seed, 7] + list(shape))
    info = np.iinfo(dtype)
    v = np.where(rng.random(shape) < 0.5, rng.integers(-40, 41, shape), rng.integers(info.min, int(info.max) + 1, shape))
    flat = v.reshape(-1)
    at = rng.choice(flat.size, min(4, flat.size), replace=False)
    flat[at] = [info.min, info.max, 0, -1][:len(at)]
    return v.astype(dtype)


def rand_steps(n, seed, tables=None):
    rng = np.random.default_rng([seed, 11, n])
    return rng.uniform(0.05, 2.0, n if tables is None else (tables, n)).astype(F)


def place(dwt, hold, buf, dev):
    if not dev:
        return buf.ctypes.data
    hold.append(Dev(dwt, buf))
    return hold[-1].ptr


def run(dwt, inverse, cl, il, ctype, itype, coef_buf, idx_buf, j_max, steps, table_stride=0, r=0.5, stats=False, device=(True, True)):
    """one call on the two buffers -> (coefficient buffer, index buffer, counters) after it"""
    Q = dwt.quant
    hold = []
    cp, ip = place(dwt, hold, coef_buf, device[0]), place(dwt, hold, idx_buf, device[1])
    frames = (cl.batch, cl.W, cl.H, j_max)
    if inverse:
        st = Q.dequantize_batch(itype, *il.args(ip), ctype, *cl.args(cp), *frames, steps, table_stride, r)
    else:
        st = Q.quantize_batch(ctype, *cl.args(cp), itype, *il.args(ip), *frames, steps, table_stride, stats)
    dwt.sync()
    out = [hold.pop(0).get() if dev else buf for buf, dev in ((coef_buf, device[0]), (idx_buf, device[1]))]
    return out[0], out[1], st


def tables_of(steps, batch, ns, table_stride):
    return steps[:ns] if not table_stride else np.asarray(steps).reshape(-1)[:batch * table_stride].reshape(batch, table_stride)[:, :ns]


def check_quantize(dwt, cl, il, ctype, itype, values, j_max, steps, table_stride=0, **kw):
    coef_buf, idx_buf = cl.fill(values), il.fill()
    coef0 = coef_buf.copy()
    got_coef, got_idx, stats = run(dwt, False, cl, il, ctype, itype, coef_buf, idx_buf, j_max, steps, table_stride, stats=True, **kw)
    assert np.array_equal(got_coef, coef0), "the coefficients were written"
    assert (got_idx[~il.own] == CANARY).all(), "bytes outside the indices were written"
    ns = 3 * qm.levels(cl.W, cl.H, j_max) + 1
    want, want_stats = qm.quantize_frames(cl.read(coef0), tables_of(steps, cl.batch, ns, table_stride), j_max, itype)
    got = il.read(got_idx)
    assert same_bits(got, want), np.argwhere(got != want)[:5]
    assert stats.shape == want_stats.shape and np.array_equal(stats, want_stats), (stats - want_stats).nonzero()
    return got, stats


def check_dequantize(dwt, cl, il, ctype, itype, values, j_max, steps, table_stride=0, r=0.5, **kw):
    coef_buf, idx_buf = cl.fill(), il.fill(values)
    idx0 = idx_buf.copy()
    got_coef, got_idx, _ = run(dwt, True, cl, il, ctype, itype, coef_buf, idx_buf, j_max, steps, table_stride, r=r, **kw)
    assert np.array_equal(got_idx, idx0), "the indices were written"
    assert (got_coef[~cl.own] == CANARY).all(), "bytes outside the coefficients were written"
    ns = 3 * qm.levels(cl.W, cl.H, j_max) + 1
    want = qm.dequantize_frames(il.read(idx0), tables_of(steps, cl.batch, ns, table_stride), j_max, r, ctype)
    got = cl.read(got_coef)
    u = np.uint16 if cl.es == 2 else np.uint32
    assert same_bits(got, want), np.argwhere(got.view(u) != want.view(u))[:5]
    return got


def layouts(ctype, itype, batch, W, H, pitch, **kw):
    return Lay(qm.COEF_DTYPE[ctype], batch, W, H, pitch, **kw), Lay(qm.INDEX_DTYPE[itype], batch, W, H, pitch, **kw)


def route(dwt, cl, il, ctype, itype, cbase=4096, ibase=1 << 20):
    return dwt.quant.quant_route(ctype, cbase + cl.base, cl.bs, cl.pitch, itype, ibase + il.base, il.bs, il.pitch, cl.batch, cl.W, cl.H)


# ---- shapes, pitches, types -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", ["dense", "prime", "padded16"])
@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_shapes_pitches_and_types(dwt, W, H, j_max, pitch):
    """every pair of coefficient and index type, both directions, two frames: indices, coefficients and counters are the
    model's; the padded pitch takes the wide route on both sides, the prime one the element route"""
    Q = dwt.quant
    ns = 3 * qm.levels(W, H, j_max) + 1
    assert ns == 3 * dwt.band_levels(W, H, j_max) + 1
    steps = rand_steps(ns, 1)
    for ctype, itype in PAIRS:
        cl, il = layouts(ctype, itype, 2, W, H, pitch)
        if pitch == "padded16":
            assert route(dwt, cl, il, ctype, itype) == Q.WIDE_COEF | Q.WIDE_INDEX
        if pitch == "prime" and H > 1:
            assert route(dwt, cl, il, ctype, itype) == 0
        check_quantize(dwt, cl, il, ctype, itype, rand_coef(cl.at.shape, cl.dtype, 2), j_max, steps)
        check_dequantize(dwt, cl, il, ctype, itype, rand_index(il.at.shape, il.dtype, 3), j_max, steps, r=0.5 if itype == qm.I16 else 0.375)


@pytest.mark.parametrize("base", [2, 4])
def test_unaligned_bases_take_the_element_route(dwt, base):
    """bases 2 bytes (the sides of 2-byte elements, in every pair that has one) and 4 bytes off a 16-byte boundary: that
    side goes element by element, the other one stays wide -- also where the wide side's run is 32 bytes"""
    Q = dwt.quant
    W, H, J = 1024, 8, 5
    steps = rand_steps(3 * J + 1, 4)
    for ctype, itype in PAIRS:
        for off_c, off_i in ((base, 0), (0, base), (base, base)):
            if (off_c % qm.COEF_DTYPE[ctype].itemsize) or (off_i % qm.INDEX_DTYPE[itype].itemsize):
                continue  # (a 4-byte element 2 bytes off its size is refused: test_refusals)
            cl = Lay(qm.COEF_DTYPE[ctype], 2, W, H, "padded16", base=off_c)
            il = Lay(qm.INDEX_DTYPE[itype], 2, W, H, "padded16", base=off_i)
            assert route(dwt, cl, il, ctype, itype) == (0 if off_c else Q.WIDE_COEF) | (0 if off_i else Q.WIDE_INDEX)
            check_quantize(dwt, cl, il, ctype, itype, rand_coef(cl.at.shape, cl.dtype, 5), J, steps)
            check_dequantize(dwt, cl, il, ctype, itype, rand_index(il.at.shape, il.dtype, 6), J, steps)


@pytest.mark.parametrize("ctype, itype", PAIRS)
def test_wide_route_and_element_route_give_the_same_bits(dwt, ctype, itype):
    """the same aligned data under option "quant_wide" = 1 (asserted: both sides by 16-byte accesses) and = 0 (asserted:
    neither): 1024 x 8 at five levels has the band edges 32, 64, 128, ... and 1, 2, 4 inside and between the lanes' runs"""
    Q = dwt.quant
    W, H, J = 1024, 8, 5
    steps = rand_steps(3 * J + 1, 7)
    cl, il = layouts(ctype, itype, 2, W, H, "dense")
    results = []
    for wide in (1, 0):
        dwt.set_option("quant_wide", wide)
        try:
            assert route(dwt, cl, il, ctype, itype) == ((Q.WIDE_COEF | Q.WIDE_INDEX) if wide else 0)
            results.append((check_quantize(dwt, cl, il, ctype, itype, rand_coef(cl.at.shape, cl.dtype, 8), J, steps),
                            check_dequantize(dwt, cl, il, ctype, itype, rand_index(il.at.shape, il.dtype, 9), J, steps)))
        finally:
            dwt.set_option("quant_wide", 1)
    assert same_bits(results[0][0][0], results[1][0][0]) and np.array_equal(results[0][0][1], results[1][0][1])
    assert same_bits(results[0][1], results[1][1])


def test_per_frame_tables_and_the_gap_between_frames(dwt):
    """table_stride != 0 on a batch of 3: frame b is quantized with its own table (the tables differ: the shared-table result is
    another one); 48 bytes between the frames keep their canaries"""
    W, H, J = 37, 53, 3
    ns = 3 * J + 1
    ts = ns + 2
    steps = rand_steps(ts, 10, tables=3)
    for ctype, itype in ((qm.S, qm.I16), (qm.H, qm.I32)):
        cl, il = layouts(ctype, itype, 3, W, H, "padded16", gap=48)
        vals = rand_coef(cl.at.shape, cl.dtype, 11)
        per_frame, _ = check_quantize(dwt, cl, il, ctype, itype, vals, J, steps, ts)
        shared, _ = check_quantize(dwt, cl, il, ctype, itype, vals, J, steps[0])
        assert same_bits(per_frame[0], shared[0]) and not same_bits(per_frame[1], shared[1])
        check_dequantize(dwt, cl, il, ctype, itype, rand_index(il.at.shape, il.dtype, 12), J, steps, ts)


@pytest.mark.parametrize("device", [(False, False), (False, True), (True, False)])
def test_host_memory_gives_the_device_calls_bits(dwt, device):
    """numpy coefficients and / or numpy indices: the model's bits (which the device call gives), canaries kept -- dense, and
    with pitch padding and a gap, where the written region holds bytes that are not the frames'"""
    for ctype, itype, pitch, gap in ((qm.S, qm.I16, "dense", 0), (qm.H, qm.I32, "prime", 12), (qm.S, qm.I32, "padded16", 32)):
        W, H, J = 37, 53, 3
        steps = rand_steps(3 * J + 1, 13)
        cl, il = layouts(ctype, itype, 2, W, H, pitch, gap=gap)
        check_quantize(dwt, cl, il, ctype, itype, rand_coef(cl.at.shape, cl.dtype, 14), J, steps, device=device)
        check_dequantize(dwt, cl, il, ctype, itype, rand_index(il.at.shape, il.dtype, 15), J, steps, device=device)


@pytest.mark.parametrize("device", [True, False])
def test_in_place_binary32_and_int32(dwt, device):
    """coef == index with equal strides: the indices replace the coefficients and the reconstruction the indices, padding
    and gap untouched"""
    Q = dwt.quant
    W, H, J = 130, 66, 4
    steps = rand_steps(3 * J + 1, 16)
    lay = Lay(np.float32, 2, W, H, "padded16", gap=16)
    vals = rand_coef(lay.at.shape, np.float32, 17)
    buf = lay.fill(vals)
    hold = []
    p = place(dwt, hold, buf, device)
    st = Q.quantize_batch(Q.S, *lay.args(p), Q.I32, *lay.args(p), 2, W, H, J, steps, stats=True)
    got = hold[0].get() if device else buf.copy()
    want, want_stats = qm.quantize_frames(vals, steps, J, qm.I32)
    assert (got[~lay.own] == CANARY).all() and same_bits(lay.read(got).view(np.int32), want) and np.array_equal(st, want_stats)
    Q.dequantize_batch(Q.I32, *lay.args(p), Q.S, *lay.args(p), 2, W, H, J, steps, r=0.5)
    dwt.sync()
    got = hold[0].get() if device else buf
    assert (got[~lay.own] == CANARY).all() and same_bits(lay.read(got), qm.dequantize_frames(want, steps, J, 0.5, qm.S))


# ---- the band counters ----------------------------------------------------------------------------------------------
def test_band_counters(dwt):
    """clipped samples whose count the construction states, NaNs, an all-zero band; two runs give identical counters"""
    W, H, J = 96, 40, 2
    geo = qm.geometry(W, H, J)
    steps = np.full(3 * J + 1, 0.5, F)
    vals = np.random.default_rng(18).normal(0, 20, (2, H, W)).astype(F)
    x, y, w, h = geo[2]  # HH(1) of frame 0: all zero
    vals[0, y:y + h, x:x + w] = 0.0
    x, y, w, h = geo[0]  # HL(1) of frame 1: 5 samples past the int16 range, 3 NaNs
    vals[1, y:y + 5, x + 1] = [20000.0, -20000.0, np.inf, 16384.0, -3e38]
    vals[1, y + h - 1, x + w - 3:x + w] = np.nan
    x, y, w, h = geo[6]  # LL(2) of frame 1: one sample on the bound, one just below it
    vals[1, y, x:x + 2] = [16384.0, 16383.75]
    cl, il = layouts(qm.S, qm.I16, 2, W, H, "dense")
    _, stats = check_quantize(dwt, cl, il, qm.S, qm.I16, vals, J, steps)
    assert stats[0, 2].tolist() == [0, 0, 0]
    assert stats[1, 0, 2] == 8 and stats[1, 0, 1] == 32767
    assert stats[1, 6, 2] == 1 and stats[1, 6, 1] == 32767 and stats[0, :, 2].sum() == 0
    assert qm.bit_length(stats[:, :, 1]).max() == 15 and qm.bit_length(stats[0, 2, 1]) == 0
    _, again = check_quantize(dwt, cl, il, qm.S, qm.I16, vals, J, steps)
    assert np.array_equal(stats, again)
    # without the counters the call returns None and the indices are the same
    coef_buf, idx_buf = cl.fill(vals), il.fill()
    _, got_idx, none = run(dwt, False, cl, il, qm.S, qm.I16, coef_buf, idx_buf, J, steps)
    assert none is None and same_bits(il.read(got_idx), qm.quantize_frames(vals, steps, J, qm.I16)[0])


# ---- the bit-plane map ----------------------------------------------------------------------------------------------
def check_bitplanes(dwt, il, itype, values, j_max, cbx, cby, device=(True, True), gap=0):
    Q = dwt.quant
    idx_buf = il.fill(values)
    total = int(qm.codeblock_layout(il.W, il.H, j_max, cbx, cby)[0][-1])
    stride = total + gap
    planes = np.full(stride * il.batch + 16, CANARY, np.uint8)
    hold = []
    ip, pp = place(dwt, hold, idx_buf, device[0]), place(dwt, hold, planes, device[1])
    Q.codeblock_bitplanes_batch(itype, *il.args(ip), il.batch, il.W, il.H, j_max, cbx, cby, pp, stride)
    dwt.sync()
    got_idx, got = [hold.pop(0).get() if dev else buf for buf, dev in ((idx_buf, device[0]), (planes, device[1]))]
    assert np.array_equal(got_idx, il.fill(values)), "the indices were written"
    want = np.full_like(planes, CANARY)
    model = qm.codeblock_bitplanes(il.read(got_idx), j_max, cbx, cby)
    for b in range(il.batch):
        want[b * stride:b * stride + total] = model[b]
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    return model


@pytest.mark.parametrize("cbx, cby", [(2, 2), (6, 6), (10, 2)])
@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_bitplane_map(dwt, W, H, j_max, cbx, cby):
    """4 x 4, 64 x 64 and 1024 x 4 blocks over the shapes above: bands smaller than a block, partial blocks at the right and
    at the bottom, empty bands; two frames with a gap between their maps"""
    for itype, pitch in ((qm.I16, "prime"), (qm.I32, "padded16")):
        il = Lay(qm.INDEX_DTYPE[itype], 2, W, H, pitch, gap=8)
        check_bitplanes(dwt, il, itype, rand_index(il.at.shape, il.dtype, 19), j_max, cbx, cby, gap=5)


def test_bitplane_map_of_the_extremes(dwt):
    """INT32_MIN (32 planes), INT32_MAX (31), INT16_MIN (16), a plane of zeros (0 everywhere), and small magnitudes"""
    W, H, J = 37, 53, 3
    v = np.zeros((1, H, W), np.int32)
    il = Lay(np.int32, 1, W, H)
    assert not check_bitplanes(dwt, il, qm.I32, v, J, 2, 2).any()
    v[0, 0, 0], v[0, 52, 36], v[0, 30, 3], v[0, 3, 30], v[0, 10, 10] = -2147483648, 2147483647, -1, 5, -4
    model = check_bitplanes(dwt, il, qm.I32, v, J, 2, 2)
    assert sorted(set(model[0].tolist())) == [0, 1, 3, 31, 32]
    il16 = Lay(np.int16, 1, W, H)
    v16 = np.zeros((1, H, W), np.int16)
    v16[0, 20, 20], v16[0, 0, 36] = -32768, 32767
    assert sorted(set(check_bitplanes(dwt, il16, qm.I16, v16, J, 3, 2)[0].tolist())) == [0, 15, 16]


@pytest.mark.parametrize("itype", [qm.I16, qm.I32])
def test_bitplane_map_routes_give_the_same_bytes(dwt, itype):
    """16-byte aligned index planes under option "quant_wide" = 1 (rows read by aligned 16-byte chunks, the elements around a
    block left out) and = 0 (element by element): the model's bytes both times; odd band offsets (37 x 53), bands that start
    inside a chunk, blocks narrower than a chunk, partial blocks"""
    for W, H, j_max in ((37, 53, 3), (1001, 9, -1), (130, 66, 2)):
        il = Lay(qm.INDEX_DTYPE[itype], 2, W, H, "padded16")
        vals = rand_index(il.at.shape, il.dtype, 30)
        for cbx, cby in ((2, 2), (3, 5), (6, 6)):
            maps = []
            for wide in (1, 0):
                dwt.set_option("quant_wide", wide)
                try:
                    maps.append(check_bitplanes(dwt, il, itype, vals, j_max, cbx, cby))
                finally:
                    dwt.set_option("quant_wide", 1)
            assert np.array_equal(maps[0], maps[1])


@pytest.mark.parametrize("device", [(False, False), (False, True), (True, False)])
def test_bitplane_map_on_host_memory(dwt, device):
    il = Lay(np.int16, 3, 130, 66, "prime", gap=6)
    check_bitplanes(dwt, il, qm.I16, rand_index(il.at.shape, il.dtype, 20), 4, 3, 4, device=device, gap=7)


# ---- launches, grid caps, stream --------------------------------------------------------------------------------------
def test_one_launch_and_no_allocation_on_device_memory(dwt):
    Q = dwt.quant
    W, H, J, B = 64, 48, 3, 3
    cl, il = layouts(qm.S, qm.I16, B, W, H, "dense")
    steps = rand_steps((3 * J + 1) * B, 21)
    a, b = Dev(dwt, cl.fill(rand_coef(cl.at.shape, cl.dtype, 22))), Dev(dwt, il.fill())
    total = int(qm.codeblock_layout(W, H, J, 3, 3)[0][-1])
    planes = Dev(dwt, np.zeros(B * total, np.uint8))
    calls = (lambda: Q.quantize_batch(Q.S, *cl.args(a.ptr), Q.I16, *il.args(b.ptr), B, W, H, J, steps),
             lambda: Q.quantize_batch(Q.S, *cl.args(a.ptr), Q.I16, *il.args(b.ptr), B, W, H, J, steps, 3 * J + 1),
             lambda: Q.quantize_batch(Q.S, *cl.args(a.ptr), Q.I16, *il.args(b.ptr), B, W, H, J, steps, 3 * J + 1, True),
             lambda: Q.dequantize_batch(Q.I16, *il.args(b.ptr), Q.S, *cl.args(a.ptr), B, W, H, J, steps, 3 * J + 1),
             lambda: Q.codeblock_bitplanes_batch(Q.I16, *il.args(b.ptr), B, W, H, J, 3, 3, planes.ptr, total))
    for f in calls:  # the first call of a size may grow the workspace
        f()
    allocs = dwt.get_option("stat_allocs")
    for f in calls:
        assert launches(dwt, f) == 1
    assert dwt.get_option("stat_allocs") == allocs
    # no frames: nothing to do, no launch
    assert launches(dwt, lambda: Q.quantize_batch(Q.S, *cl.args(a.ptr), Q.I16, *il.args(b.ptr), 0, W, H, J, steps)) == 0


def test_rows_past_the_grid_cap(dwt):
    """an 8-sample-wide frame with 300 rows more than one trip of the kernel's row loop covers, rows repeating with period
    251 (tests/gridlimits.py): a row taken one cap away from where it belongs meets other data and another band"""
    cap = dwt.quant.GRID_ROWS
    H, W, J = cap + 300, 8, 3
    assert cap % gridlimits.P and gridlimits.trips(H, cap) == 2
    vals = gridlimits.tile(np.random.default_rng(23).normal(0, 30, (1, gridlimits.P, W)).astype(F), H, axis=1)
    steps = rand_steps(3 * J + 1, 24)
    cl, il = layouts(qm.S, qm.I16, 1, W, H, "dense")
    got, _ = check_quantize(dwt, cl, il, qm.S, qm.I16, vals, J, steps)
    check_dequantize(dwt, cl, il, qm.S, qm.I16, got, J, steps)


def test_frames_past_the_grid_cap(dwt):
    """5 frames more than one trip of the kernel's batch loop covers, 3 x 2 samples each, frames repeating with period 251"""
    cap = dwt.quant.GRID_BATCH
    B, W, H, J = cap + 5, 3, 2, 1
    assert cap % gridlimits.P and gridlimits.trips(B, cap) == 2
    vals = gridlimits.tile(np.random.default_rng(25).normal(0, 30, (gridlimits.P, H, W)).astype(F), B, axis=0)
    steps = rand_steps(3 * J + 1, 26)
    cl, il = layouts(qm.S, qm.I32, B, W, H, "dense")
    got, _ = check_quantize(dwt, cl, il, qm.S, qm.I32, vals, J, steps)
    check_dequantize(dwt, cl, il, qm.S, qm.I32, got, J, steps)


def test_code_blocks_past_the_grid_cap(dwt):
    """256 x 257 blocks of 4 x 4 in one band, 256 more than one trip of the bit-plane kernel's loop covers; block rows repeat
    with period 251"""
    cap = dwt.quant.CODEBLOCK_GRID_BLOCKS
    W, H = 1024, 1028
    assert int(qm.codeblock_layout(W, H, 0, 2, 2)[0][-1]) == cap + 256 and gridlimits.trips(cap + 256, cap) == 2 and cap % gridlimits.P
    rows = np.random.default_rng(27).integers(-3000, 3001, (1, gridlimits.P, W)).astype(np.int16)
    vals = gridlimits.tile(rows, H, axis=1)
    il = Lay(np.int16, 1, W, H)
    check_bitplanes(dwt, il, qm.I16, vals, 0, 2, 2)


def test_entries_run_on_the_callers_stream():
    """quantize (both routes, with and without the counters), dequantize and the bit-plane map once on a non-blocking stream
    behind a bounded delay, in a process of its own (tests/quant_stream.py, on the harness of tests/stream_cases.py): the
    model's bits; the calls without counters queued without waiting for the stream"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "quant_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_picture_through_the_quantizer(dwt):
    """one RGB8 picture of 256 x 256: composite forward (ICT, CDF97_S, 5 levels), steps from dwt_hip_quant_steps, quantize to
    int16, dequantize (r = 0.5), composite inverse -- pixel for pixel the chain with the model's quantizer in the middle"""
    from libdwt_amd import pixels as P

    Q = dwt.quant
    W = H = 256
    J = 5
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(28)
    pic = np.stack([128 + 90 * np.sin(xx / 17.0) * np.cos(yy / 23.0), (xx * 3 + yy * 2) % 256, 40 + 0.7 * ((xx - 128) ** 2 + (yy - 128) ** 2) ** 0.5], -1)
    pic = np.clip(pic + rng.normal(0, 4, pic.shape), 0, 255).astype(np.uint8)
    pix_args = (3 * W * H, 3 * W, 3, 1, 1, 3, P.RGB, 8, 128, 1.0, P.ICT)
    plane_args = (4 * W * H, 4 * W, W, H)
    steps = Q.quant_steps(dwt.CDF97_S, J, 2.0)
    assert same_bits(steps, qm.steps(qm.CDF97, J, 2.0))
    src, planes, idx = Dev(dwt, pic), Dev(dwt, np.zeros((3, H, W), F)), Dev(dwt, np.zeros((3, H, W), np.int16))
    assert P.picture_forward_batch(dwt.CDF97_S, P.U8, src.ptr, *pix_args, planes.ptr, *plane_args, J) == J
    coef = planes.get()
    stats = Q.quantize_batch(Q.S, planes.ptr, 4 * W * H, 4 * W, Q.I16, idx.ptr, 2 * W * H, 2 * W, 3, W, H, J, steps, stats=True)
    Q.dequantize_batch(Q.I16, idx.ptr, 2 * W * H, 2 * W, Q.S, planes.ptr, 4 * W * H, 4 * W, 3, W, H, J, steps, r=0.5)
    out = Dev(dwt, np.zeros_like(pic))
    P.picture_inverse_batch(dwt.CDF97_S, P.U8, out.ptr, *pix_args, planes.ptr, *plane_args, J)
    got = out.get()
    # the model's quantizer between the same device transforms
    q, want_stats = qm.quantize_frames(coef, steps, J, qm.I16)
    assert same_bits(idx.get(), q) and np.array_equal(stats, want_stats) and stats[:, :, 2].sum() == 0
    model_planes, model_out = Dev(dwt, qm.dequantize_frames(q, steps, J, 0.5, qm.S)), Dev(dwt, np.zeros_like(pic))
    P.picture_inverse_batch(dwt.CDF97_S, P.U8, model_out.ptr, *pix_args, model_planes.ptr, *plane_args, J)
    assert np.array_equal(got, model_out.get())
    # it is a lossy path that still shows the picture: some indices are zero, the error is a few grey levels
    assert 0.05 < (q != 0).mean() < 0.9
    mse = np.mean((got.astype(np.float64) - pic) ** 2)
    assert 0 < mse < 8.0, mse


def test_example_picture_lossy(dwt, tmp_path):
    """examples/picture_lossy.c compiles with the gcc line of its header comment, runs and exits 0, on its synthetic picture
    and on a PPM"""
    exe, libdir = tmp_path / "picture_lossy", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "picture_lossy.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.count("PSNR") == 3, out.stdout + out.stderr
    ppm = tmp_path / "t.ppm"
    rng = np.random.default_rng(29)
    ppm.write_bytes(b"P6\n# a comment\n67 45\n255\n" + rng.integers(0, 256, 67 * 45 * 3).astype(np.uint8).tobytes())
    out = subprocess.run([str(exe), str(ppm)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "67 x 45" in out.stdout and out.stdout.count("PSNR") == 3, out.stdout + out.stderr


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals(dwt):
    """every refusal of the header returns its code with a message and leaves canaried buffers untouched, both directions"""
    Q = dwt.quant
    W, H, J = 32, 16, 2
    ns = 3 * J + 1
    cl, il = layouts(qm.S, qm.I16, 2, W, H, "dense")
    c, i = Dev(dwt, cl.fill()), Dev(dwt, il.fill())
    big = Dev(dwt, np.full(1 << 16, CANARY, np.uint8))
    good = np.full(ns, 0.5, F)

    def refused(steps=good, ts=0, r=0.5, ctype=qm.S, itype=qm.I16, cargs=None, iargs=None, batch=2, w=W, h=H, only=None):
        ca, ia = cargs or cl.args(c.ptr), iargs or il.args(i.ptr)
        for inverse in (False, True):
            if only is not None and only != inverse:
                continue
            with pytest.raises(dwt.DwtError) as e:
                if inverse:
                    Q.dequantize_batch(itype, *ia, ctype, *ca, batch, w, h, J, steps, ts, r)
                else:
                    Q.quantize_batch(ctype, *ca, itype, *ia, batch, w, h, J, steps, ts, True)
            assert len(str(e.value)) > 30, str(e.value)

    for bad in (0.0, -0.5, float("nan"), float("inf"), -float("inf")):
        t = good.copy()
        t[ns - 2] = bad
        refused(steps=t)
    t = np.full(2 * ns, 0.5, F)
    t[ns + 3] = 0.0  # in the second frame's table only
    refused(steps=t, ts=ns)
    refused(steps=np.full(2 * ns, 0.5, F), ts=ns - 1)  # a table shorter than the slots
    for r in (-0.25, 1.0, 1.5, float("nan")):
        refused(r=r, only=True)
    refused(steps=None)
    refused(cargs=(0, cl.bs, cl.pitch))
    refused(iargs=(0, il.bs, il.pitch))
    refused(w=-1)
    refused(h=-3)
    refused(batch=-1)
    refused(ctype=2)
    refused(itype=-1)
    refused(cargs=(c.ptr, cl.bs, cl.pitch - 4))  # a pitch below its row
    refused(iargs=(i.ptr, il.bs - 2, il.pitch))  # frames closer than they span
    refused(cargs=(c.ptr + 2, cl.bs, cl.pitch))  # binary32 on a 2-byte boundary
    refused(iargs=(i.ptr, il.bs, il.pitch + 1))
    # overlap: the indices inside the coefficients' region; binary32 / int16 at one address; binary32 / int32 at one address
    # with different pitches
    refused(cargs=cl.args(big.ptr), iargs=il.args(big.ptr + cl.bs))
    refused(cargs=cl.args(big.ptr), iargs=il.args(big.ptr))
    refused(cargs=cl.args(big.ptr), iargs=(big.ptr, cl.bs + 64, cl.pitch), itype=qm.I32)
    # binary16 / int16 at one address with equal strides: the same element size, but in place is binary32 <-> int32 alone
    refused(cargs=il.args(big.ptr), iargs=il.args(big.ptr), ctype=qm.H, itype=qm.I16)
    refused(cargs=cl.args(big.ptr), iargs=cl.args(big.ptr + 4), itype=qm.I32)  # binary32 / int32 one element apart
    # the counters in device memory
    assert dwt.lib.dwt_hip_quantize_batch(qm.S, *cl.args(c.ptr), qm.I16, *il.args(i.ptr), 2, W, H, J, good.ctypes.data, 0, big.ptr) != 0
    # the bit-plane map
    total = int(qm.codeblock_layout(W, H, J, 2, 2)[0][-1])
    for kw in ({"cb": (1, 6)}, {"cb": (11, 1)}, {"cb": (7, 6)}, {"itype": 5}, {"idx": 0}, {"planes": 0}, {"stride": total - 1}, {"w": -1},
               {"planes": i.ptr + 8}):
        with pytest.raises(dwt.DwtError):
            Q.codeblock_bitplanes_batch(kw.get("itype", qm.I16), kw.get("idx", i.ptr), il.bs, il.pitch, 2, kw.get("w", W), H, J, *kw.get("cb", (2, 2)),
                                        kw.get("planes", big.ptr), kw.get("stride", total))
    with pytest.raises(dwt.DwtError):
        Q.quant_route(qm.S, c.ptr, cl.bs, cl.pitch - 4, qm.I16, i.ptr, il.bs, il.pitch, 2, W, H)
    dwt.sync()
    for d in (c, i, big):
        assert (d.get() == CANARY).all(), "a refused call wrote"
