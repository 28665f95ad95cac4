"""GPU checks of the pixel front end (dwt_hip_pixels_to_planes_batch, dwt_hip_planes_to_pixels_batch,
dwt_hip_picture_forward_batch, dwt_hip_picture_inverse_batch; libdwt_amd/pixels.py) against tests/pixels_model.py, bit for
bit.  Every buffer is a run of canary bytes with the frame's elements laid into it; after a call the output's elements hold
the model's bytes and every other byte of every buffer still holds the canary (the input: its own bytes too)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gridlimits
import pixels_model as pm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
F = np.float32
PPL = 16  # asserted against the package's constant in the `dwt` fixture
WAVE = 64 * PPL
LAYOUTS = ("grey", "rgb", "planar", "bgra", "rgbx")  # 1; 3 interleaved; 3 planar; 4 interleaved BGRA; 3 used of a 4-element pixel
PRIMES = (2053, 4099, 8209, 16411, 32771)


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d
    from libdwt_amd import pixels

    d.dwt_util_init()
    d.pixels = pixels
    assert pixels.PIXELS_PER_LANE == PPL
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("pixels_wide", 1)


# ---- layouts: where the elements of a frame lie in a byte buffer ---------------------------------------------------
class Pix:
    """pictures of `kind` in a byte buffer: pitch "dense", "prime" or "padded16"; the base `base` bytes into the buffer"""

    def __init__(self, fmt, kind, batch, W, H, pitch="dense", base=0):
        pt = 1 if fmt == pm.U8 else 2
        self.fmt, self.pt, self.batch, self.W, self.H, self.base = fmt, pt, batch, W, H, base
        self.channels = {"grey": 1, "rgb": 3, "planar": 3, "bgra": 4, "rgbx": 3}[kind]
        self.order = pm.BGR if kind == "bgra" else pm.RGB
        per_pixel = {"grey": 1, "rgb": 3, "planar": 1, "bgra": 4, "rgbx": 4}[kind]
        self.pix_stride = per_pixel * pt
        row = W * self.pix_stride
        self.pitch = {"dense": row, "prime": next(p for p in PRIMES if p >= row), "padded16": (row + 15) // 16 * 16 + 16}[pitch]
        if kind == "planar":
            self.chan_stride = self.pitch * H
            self.bs = self.chan_stride * 3
        else:
            self.chan_stride = pt
            self.bs = self.pitch * H
        self.nbytes = base + self.bs * batch + 16
        b, y, x, c = np.ix_(np.arange(batch), np.arange(H), np.arange(W), np.arange(self.channels))
        self.at = base + b * self.bs + y * self.pitch + x * self.pix_stride + c * self.chan_stride  # (B, H, W, C) byte offsets
        self.own = np.zeros(self.nbytes, bool)
        for k in range(pt):
            self.own[self.at + k] = True

    def fill(self, values=None):
        buf = np.full(self.nbytes, CANARY, np.uint8)
        if values is not None:
            for k in range(self.pt):
                buf[self.at + k] = (np.asarray(values).astype(np.int64) >> (8 * k)) & 255
        return buf

    def read(self, buf):
        v = np.zeros(self.at.shape, np.int64)
        for k in range(self.pt):
            v |= buf[self.at + k].astype(np.int64) << (8 * k)
        return v.astype(pm.PIXEL_DTYPE[self.fmt])

    def args(self, ptr):
        return (self.fmt, ptr + self.base, self.bs, self.pitch, self.pix_stride, self.chan_stride, self.batch, self.channels, self.order)


class Planes:
    """batch * channels planes in a byte buffer: pitch "dense", "odd" (one element more) or "padded16"; base in elements"""

    def __init__(self, plane, n, W, H, pitch="dense", base=0, gap=0):
        es = 2 if plane in (pm.I16, pm.H) else 4
        self.plane, self.es, self.n, self.W, self.H = plane, es, n, W, H
        self.dtype = np.dtype(pm.PLANE_DTYPE[plane])
        row = W * es
        self.pitch = {"dense": row, "odd": row + es, "padded16": (row + 15) // 16 * 16 + 16}[pitch]
        self.stride = self.pitch * H + gap * es
        self.base = base * es
        self.nbytes = self.base + self.stride * n + 16
        p, y, x = np.ix_(np.arange(n), np.arange(H), np.arange(W))
        self.at = self.base + p * self.stride + y * self.pitch + x * es  # (n, H, W)
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
        return (ptr + self.base, self.stride, self.pitch, self.W, self.H)


def model_planes(pl, pix_values, order, offset, scale, colour):
    """(B, H, W, C) pixels -> (B * C, H, W) planes"""
    B, H, W, C = pix_values.shape
    out = pm.to_planes(pix_values, order, offset, scale, colour, pl.plane)  # (C, B, H, W)
    return np.ascontiguousarray(out.transpose(1, 0, 2, 3)).reshape(B * C, H, W)


def model_pixels(px, plane_values, depth, offset, scale, colour):
    """(B * C, H, W) planes -> (B, H, W, C) pixels"""
    C = px.channels
    p = plane_values.reshape(px.batch, C, px.H, px.W).transpose(1, 0, 2, 3)
    return pm.to_pixels(p, px.fmt, px.order, depth, offset, scale, colour)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rand_pixels(px, depth, seed, what="random"):
    if what == "zero":
        return np.zeros(px.at.shape, np.int64)
    if what == "max":
        return np.full(px.at.shape, (1 << depth) - 1, np.int64)
    return np.random.default_rng([seed, px.W, px.H, px.batch, px.channels]).integers(0, 1 << depth, px.at.shape)


def rand_planes(pl, depth, scale, seed):
    """samples in and around the pixel range of `depth` after the level shift; floats on a grid of eighths (ties included)"""
    rng = np.random.default_rng([seed, pl.W, pl.H, pl.n, pl.plane])
    half = 1 << (depth - 1)
    v = rng.integers(-3 * half // 2 * 8, 3 * half // 2 * 8 + 1, pl.at.shape)
    if pm.is_float(pl.plane):
        return ((v / 8.0) * scale).astype(pl.dtype)
    return (v // 8).astype(pl.dtype)


def convert(dwt, inverse, px, pl, depth, offset, scale, colour, pix_buf, plane_buf, device=(True, True), entry=None):
    """one conversion call on the two buffers -> (pixel buffer, plane buffer) after it; entry: called with the conversion
    entries' arguments in their place"""
    P = dwt.pixels
    hold = []

    def place(buf, dev):
        if not dev:
            return buf.ctypes.data
        hold.append(Dev(dwt, buf))
        return hold[-1].ptr

    pp, lp = place(pix_buf, device[0]), place(plane_buf, device[1])
    (entry or (P.planes_to_pixels_batch if inverse else P.pixels_to_planes_batch))(*px.args(pp), depth, offset, scale, colour, pl.plane, *pl.args(lp))
    dwt.sync()
    out = []
    for buf, dev in ((pix_buf, device[0]), (plane_buf, device[1])):
        out.append(hold.pop(0).get() if dev else buf)
    return out


def check_forward(dwt, px, pl, depth, offset, scale, colour, values, **kw):
    pix_buf, plane_buf = px.fill(values), pl.fill()
    pix0 = pix_buf.copy()
    got_pix, got_planes = convert(dwt, False, px, pl, depth, offset, scale, colour, pix_buf, plane_buf, **kw)
    assert np.array_equal(got_pix, pix0), "the pixels were written"
    assert (got_planes[~pl.own] == CANARY).all(), "bytes outside the planes were written"
    want = model_planes(pl, px.read(pix0), px.order, offset, scale, colour)
    got = pl.read(got_planes)
    assert same_bits(got, want), np.argwhere(got.view(np.uint16 if pl.es == 2 else np.uint32) != want.view(np.uint16 if pl.es == 2 else np.uint32))[:5]
    return got


def check_inverse(dwt, px, pl, depth, offset, scale, colour, values, **kw):
    pix_buf, plane_buf = px.fill(), pl.fill(values)
    planes0 = plane_buf.copy()
    got_pix, got_planes = convert(dwt, True, px, pl, depth, offset, scale, colour, pix_buf, plane_buf, **kw)
    assert np.array_equal(got_planes, planes0), "the planes were written"
    assert (got_pix[~px.own] == CANARY).all(), "bytes outside the pixels were written"
    want = model_pixels(px, pl.read(planes0), depth, offset, scale, colour)
    got = px.read(got_pix)
    assert same_bits(got, want), np.argwhere(got != want)[:5]
    return got


def combos(channels, fmt, depth):
    """every legal (plane type, colour) for this pixel type"""
    return [(plane, colour) for plane in (pm.I16, pm.I32, pm.H, pm.S) for colour in (pm.NONE, pm.RCT, pm.ICT)
            if pm.legal(fmt, channels, depth, colour, plane)]


# ---- the matrix ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("fmt, depth", [(pm.U8, 8), (pm.U16, 12), (pm.U16, 16)])
def test_matrix(dwt, fmt, depth, kind):
    """every pixel type, layout, legal colour and plane type, both directions: 2 pictures of 33 x 5 (two whole runs of a
    lane and a tail), everything aligned, so the whole runs move by 16-byte accesses and the tail element by element"""
    W, H, B = 33, 5, 2
    px = Pix(fmt, kind, B, W, H, "padded16")
    cs = combos(px.channels, fmt, depth)
    assert (pm.I32, pm.RCT) in cs or px.channels == 1
    assert ((pm.I16, pm.RCT) in cs) == (px.channels >= 3 and depth < 16)
    for plane, colour in cs:
        pl = Planes(plane, B * px.channels, W, H, "padded16")
        scale = 1.0 / 256 if pm.is_float(plane) and colour == pm.ICT else 1.0
        offset = 1 << (depth - 1)
        route = dwt.pixels.pixels_route(fmt, False, 4096, px.bs, px.pitch, px.pix_stride, px.chan_stride, B, px.channels, plane, 1 << 20,
                                        pl.stride, pl.pitch, W, H)
        assert route == dwt.pixels.WIDE_PIX | dwt.pixels.WIDE_PLANES
        check_forward(dwt, px, pl, depth, offset, scale, colour, rand_pixels(px, depth, 1))
        check_inverse(dwt, px, pl, depth, offset, 1.0 / scale, colour, rand_planes(pl, depth, scale, 2))


SHAPES = [(1, 1), (7, 1), (1, 7), (15, 3), (16, 16), (17, 5), (33, 2), (WAVE - 1, 2), (WAVE, 2), (WAVE + 1, 2)]


@pytest.mark.parametrize("pitch", ["dense", "prime", "padded16"])
@pytest.mark.parametrize("W, H", SHAPES)
def test_shapes_and_pitches(dwt, W, H, pitch):
    """the sizes where the kernel can go wrong (one pixel, less than / exactly / more than a lane's run and a wave's span)
    with dense, prime and padded aligned row pitches: RGB8 <-> int16 RCT, BGRA16 <-> binary32 ICT, grey16 <-> binary16"""
    ppitch = {"dense": "dense", "prime": "odd", "padded16": "padded16"}[pitch]
    for fmt, kind, depth, plane, colour in ((pm.U8, "rgb", 8, pm.I16, pm.RCT), (pm.U16, "bgra", 12, pm.S, pm.ICT), (pm.U16, "grey", 16, pm.H, pm.NONE)):
        px = Pix(fmt, kind, 2, W, H, pitch)
        pl = Planes(plane, 2 * px.channels, W, H, ppitch)
        offset = 1 << (depth - 1)
        check_forward(dwt, px, pl, depth, offset, 1.0, colour, rand_pixels(px, depth, 3))
        check_inverse(dwt, px, pl, depth, offset, 1.0, colour, rand_planes(pl, depth, 1.0, 4))


@pytest.mark.parametrize("base", [1, 2, 3])
def test_unaligned_bases_take_the_element_route(dwt, base):
    """a pixel base 1, 2 and 3 bytes off (u8; u16 on an odd address too) and a plane base one element off"""
    P = dwt.pixels
    for fmt, kind, depth, plane, colour in ((pm.U8, "rgb", 8, pm.I16, pm.RCT), (pm.U8, "bgra", 8, pm.S, pm.ICT), (pm.U16, "rgb", 12, pm.I32, pm.RCT)):
        W, H = 40, 3
        px = Pix(fmt, kind, 2, W, H, "padded16", base=base)
        pl = Planes(plane, 2 * px.channels, W, H, "padded16", base=1)
        for inverse in (False, True):
            assert P.pixels_route(fmt, inverse, 4096 + base, px.bs, px.pitch, px.pix_stride, px.chan_stride, 2, px.channels, plane,
                                  (1 << 20) + pl.base, pl.stride, pl.pitch, W, H) == 0
        check_forward(dwt, px, pl, depth, 1 << (depth - 1), 1.0, colour, rand_pixels(px, depth, 5))
        check_inverse(dwt, px, pl, depth, 1 << (depth - 1), 1.0, colour, rand_planes(pl, depth, 1.0, 6))
        # one side aligned, the other not
        px0, pl0 = Pix(fmt, kind, 2, W, H, "padded16"), Planes(plane, 2 * px.channels, W, H, "padded16")
        check_forward(dwt, px0, pl, depth, 1 << (depth - 1), 1.0, colour, rand_pixels(px0, depth, 5))
        check_inverse(dwt, px, pl0, depth, 1 << (depth - 1), 1.0, colour, rand_planes(pl0, depth, 1.0, 6))


@pytest.mark.parametrize("kind", LAYOUTS)
def test_wide_route_and_element_route_give_the_same_bits(dwt, kind):
    """the same aligned data under option "pixels_wide" = 1 (asserted: both sides by 16-byte accesses, except the pixels of an
    inverse call whose interleaved pixel has an unused element) and = 0 (asserted: neither)"""
    P = dwt.pixels
    W, H, B = 2 * WAVE + 5, 3, 2
    for fmt, depth in ((pm.U8, 8), (pm.U16, 16)):
        px = Pix(fmt, kind, B, W, H, "padded16")
        plane, colour = (pm.S, pm.ICT) if px.channels >= 3 else (pm.I32, pm.NONE)
        pl = Planes(plane, B * px.channels, W, H, "padded16")
        results = []
        for wide in (1, 0):
            dwt.set_option("pixels_wide", wide)
            try:
                for inverse in (False, True):
                    route = P.pixels_route(fmt, inverse, 4096, px.bs, px.pitch, px.pix_stride, px.chan_stride, B, px.channels, plane, 1 << 20,
                                           pl.stride, pl.pitch, W, H)
                    pix_wide = P.WIDE_PIX if not (inverse and kind == "rgbx") else 0
                    assert route == ((pix_wide | P.WIDE_PLANES) if wide else 0), (wide, inverse, route)
                results.append((check_forward(dwt, px, pl, depth, 1 << (depth - 1), 1.0, colour, rand_pixels(px, depth, 7)),
                                check_inverse(dwt, px, pl, depth, 1 << (depth - 1), 1.0, colour, rand_planes(pl, depth, 1.0, 8))))
            finally:
                dwt.set_option("pixels_wide", 1)
        assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1])


def test_one_launch_and_no_allocation_on_device_memory(dwt):
    px, pl = Pix(pm.U8, "rgb", 2, 64, 48), Planes(pm.I16, 6, 64, 48)
    a, b = Dev(dwt, px.fill(rand_pixels(px, 8, 9))), Dev(dwt, pl.fill())
    P = dwt.pixels
    allocs = dwt.get_option("stat_allocs")
    assert launches(dwt, lambda: P.pixels_to_planes_batch(*px.args(a.ptr), 8, 128, 1.0, pm.RCT, pm.I16, *pl.args(b.ptr))) == 1
    assert launches(dwt, lambda: P.planes_to_pixels_batch(*px.args(a.ptr), 8, 128, 1.0, pm.RCT, pm.I16, *pl.args(b.ptr))) == 1
    assert dwt.get_option("stat_allocs") == allocs
    # no pictures: nothing to do, no launch
    assert launches(dwt, lambda: P.pixels_to_planes_batch(pm.U8, a.ptr, px.bs, px.pitch, 3, 1, 0, 3, pm.RGB, 8, 128, 1.0, pm.RCT, pm.I16,
                                                          *pl.args(b.ptr))) == 0


# ---- inverse edge values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt, depth", [(pm.U8, 8), (pm.U16, 12), (pm.U16, 16)])
def test_inverse_edge_values(dwt, fmt, depth):
    """ties, NaN, +-Inf, -0.0, values just outside the range (float planes); INT_MAX, INT_MIN and neighbours (int planes)"""
    top = float(1 << depth)
    fl = [0.5, 1.5, 2.5, top - 1.5, top - 0.5, np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, top, -0.5, top - 1.0, 3.4e38, -3.4e38, 1e-40, 0.49999997]
    big = np.iinfo(np.int32)
    ints = [big.max, big.max - 5, big.max - 200, big.min, big.min + 1, -1, 0, 1, (1 << depth) - 1, 1 << depth, 70000, -70000]
    W = 40
    for plane, vals in ((pm.S, fl), (pm.H, [v for v in fl if abs(v) < 6e4 or not np.isfinite(v)] + [65504.0, -65504.0, 6e-8]), (pm.I32, ints),
                        (pm.I16, [-32768, 32767, -1, 0, 1, 255, 256])):
        px = Pix(fmt, "grey", 1, W, 1)
        pl = Planes(plane, 1, W, 1)
        with np.errstate(over="ignore", invalid="ignore"):
            row = np.resize(np.array(vals, np.float64 if pm.is_float(plane) else np.int64), W).astype(pl.dtype).reshape(1, 1, W)
        for offset in (0, 3, 1 << (depth - 1)):
            check_inverse(dwt, px, pl, depth, offset, 1.0, pm.NONE, row)
    # through the ICT: NaN and Inf spread to the channels the component feeds
    px, pl = Pix(fmt, "rgb", 1, W, 1), Planes(pm.S, 3, W, 1)
    rng = np.random.default_rng(11)
    v = rng.normal(0, top / 4, (3, 1, W)).astype(F)
    v[0, 0, 3], v[1, 0, 5], v[2, 0, 7], v[1, 0, 9] = np.nan, np.inf, -np.inf, np.nan
    check_inverse(dwt, px, pl, depth, 1 << (depth - 1), 1.0, pm.ICT, v)


# ---- composite entries ---------------------------------------------------------------------------------------------
def wavelet_cases(dwt):
    return {"cdf53_i16": (dwt.CDF53_I16, pm.U8, 8, pm.RCT, 1.0), "cdf53_i": (dwt.CDF53_I, pm.U16, 16, pm.RCT, 1.0),
            "cdf97_s": (dwt.CDF97_S, pm.U8, 8, pm.ICT, 1.0), "cdf97_h": (dwt.CDF97_H, pm.U8, 8, pm.ICT, 1.0 / 256)}


@pytest.mark.parametrize("name", ["cdf53_i16", "cdf53_i", "cdf97_s", "cdf97_h"])
def test_composite_entries_are_the_two_calls(dwt, name):
    """picture_forward_batch == pixels_to_planes_batch then transform2d_batch, picture_inverse_batch == transform2d_batch
    then planes_to_pixels_batch, bit for bit: 3 pictures of 64 x 48, 5 levels"""
    P = dwt.pixels
    wavelet, fmt, depth, colour, scale = wavelet_cases(dwt)[name]
    plane = P.PLANE_OF_WAVELET[wavelet]
    B, W, H, J = 3, 64, 48, 5
    px = Pix(fmt, "rgb", B, W, H)
    pl = Planes(plane, 3 * B, W, H)
    offset = 1 << (depth - 1)
    pix = Dev(dwt, px.fill(rand_pixels(px, depth, 12)))
    # the two calls
    conv, two = Dev(dwt, pl.fill()), Dev(dwt, pl.fill())
    P.pixels_to_planes_batch(*px.args(pix.ptr), depth, offset, scale, colour, plane, *pl.args(conv.ptr))
    assert dwt.transform2d_batch(wavelet, False, conv.ptr, two.ptr, pl.stride, 3 * B, pl.pitch, W, H, J) == J
    # the one call
    one = Dev(dwt, pl.fill())
    assert P.picture_forward_batch(wavelet, *px.args(pix.ptr), depth, offset, scale, colour, *pl.args(one.ptr), J) == J
    got, want = one.get(), two.get()
    assert np.array_equal(got, want) and (got[~pl.own] == CANARY).all()
    assert not np.array_equal(pl.read(got), pl.read(conv.get()))
    # the inverse: the two calls ...
    back = Dev(dwt, pl.fill())
    dwt.transform2d_batch(wavelet, True, two.ptr, back.ptr, pl.stride, 3 * B, pl.pitch, W, H, J)
    pix_two, pix_one = Dev(dwt, px.fill()), Dev(dwt, px.fill())
    P.planes_to_pixels_batch(*px.args(pix_two.ptr), depth, offset, 1.0 / scale, colour, plane, *pl.args(back.ptr))
    # ... and the one, which only reads the planes
    P.picture_inverse_batch(wavelet, *px.args(pix_one.ptr), depth, offset, 1.0 / scale, colour, *pl.args(one.ptr), J)
    a, b = pix_one.get(), pix_two.get()
    assert np.array_equal(a, b) and (a[~px.own] == CANARY).all()
    assert np.array_equal(one.get(), got), "the inverse wrote the planes"
    if name != "cdf97_h":  # (binary16 storage is lossy; tests/test_hip_f16.py bounds it)
        assert np.array_equal(a, pix.get()), "the round trip changed pixels"


@pytest.mark.parametrize("W, H, j_max", [(9, 1, -1), (1, 7, -1), (1, 1, 3), (20, 6, 0)])
@pytest.mark.parametrize("device", [True, False])
def test_composite_entries_without_a_level(dwt, device, W, H, j_max):
    """a picture one pixel wide or high, or j = 0: the transform is the identity, so the composite entries give the
    conversion's bits in the caller's planes (forward, *j = 0 stored) and pixels (inverse); batch 3, padded planes with a gap,
    canaries, device and host memory -- after a call that left other data in the scratch stack"""
    P = dwt.pixels
    B = 3
    for wavelet, fmt, kind, depth, colour, scale in ((dwt.CDF53_I16, pm.U8, "rgb", 8, pm.RCT, 1.0), (dwt.CDF97_S, pm.U16, "bgra", 12, pm.ICT, 0.25)):
        plane = P.PLANE_OF_WAVELET[wavelet]
        # other data in the scratch stack: a transform of larger planes
        spx, spl = Pix(fmt, kind, B, 32, 32), Planes(plane, B * (4 if kind == "bgra" else 3), 32, 32)
        a, b = Dev(dwt, spx.fill(rand_pixels(spx, depth, 30))), Dev(dwt, spl.fill())
        assert P.picture_forward_batch(wavelet, *spx.args(a.ptr), depth, 1 << (depth - 1), scale, colour, *spl.args(b.ptr), 2) == 2
        px = Pix(fmt, kind, B, W, H, "padded16")
        pl = Planes(plane, B * px.channels, W, H, "padded16", gap=3)
        offset = 1 << (depth - 1)
        ran = []

        def forward(*args):
            ran.append(P.picture_forward_batch(wavelet, *args[:-6], *args[-5:], j_max))

        def inverse(*args):
            P.picture_inverse_batch(wavelet, *args[:-6], *args[-5:], j_max)

        check_forward(dwt, px, pl, depth, offset, scale, colour, rand_pixels(px, depth, 31), device=(device, device), entry=forward)
        assert ran == [0]
        check_inverse(dwt, px, pl, depth, offset, 1.0 / scale, colour, rand_planes(pl, depth, scale, 32), device=(device, device), entry=inverse)


def test_composite_entries_on_padded_planes_with_a_gap(dwt):
    """the scratch stack takes the caller's strides: a padded row pitch and a gap between the planes, canaries around
    every row; forward equals the two calls, the inverse returns the pixels"""
    P = dwt.pixels
    B, W, H, J = 2, 50, 36, 3
    for wavelet, fmt, depth, colour in ((dwt.CDF53_I16, pm.U8, 8, pm.RCT), (dwt.CDF97_S, pm.U8, 8, pm.ICT)):
        plane = P.PLANE_OF_WAVELET[wavelet]
        px = Pix(fmt, "rgb", B, W, H, "prime", base=1)
        pl = Planes(plane, 3 * B, W, H, "padded16", gap=5)
        src = px.fill(rand_pixels(px, depth, 33))
        pix, conv, two, one, back = Dev(dwt, src), Dev(dwt, pl.fill()), Dev(dwt, pl.fill()), Dev(dwt, pl.fill()), Dev(dwt, px.fill())
        P.pixels_to_planes_batch(*px.args(pix.ptr), depth, 128, 1.0, colour, plane, *pl.args(conv.ptr))
        assert dwt.transform2d_batch(wavelet, False, conv.ptr + pl.base, two.ptr + pl.base, pl.stride, 3 * B, pl.pitch, W, H, J) == J
        assert P.picture_forward_batch(wavelet, *px.args(pix.ptr), depth, 128, 1.0, colour, *pl.args(one.ptr), J) == J
        got = one.get()
        assert np.array_equal(got, two.get()) and (got[~pl.own] == CANARY).all()
        assert not np.array_equal(pl.read(got), pl.read(conv.get()))
        P.picture_inverse_batch(wavelet, *px.args(back.ptr), depth, 128, 1.0, colour, *pl.args(one.ptr), J)
        assert np.array_equal(back.get(), src) and np.array_equal(one.get(), got)


LOSSLESS = [("rgb8", pm.U8, "rgb", 8, "cdf53_i16", pm.RCT), ("rgb12", pm.U16, "rgb", 12, "cdf53_i16", pm.RCT),
            ("grey16", pm.U16, "grey", 16, "cdf53_i16", pm.NONE), ("rgb16", pm.U16, "rgb", 16, "cdf53_i", pm.RCT)]


@pytest.mark.parametrize("name, fmt, kind, depth, wname, colour", LOSSLESS)
@pytest.mark.parametrize("what", ["random", "zero", "max"])
def test_lossless_round_trips(dwt, what, name, fmt, kind, depth, wname, colour):
    """identical pixels after forward and inverse; 16-bit grey through int16 with offset 32768 (u16 maps onto int16)"""
    P = dwt.pixels
    wavelet = {"cdf53_i16": dwt.CDF53_I16, "cdf53_i": dwt.CDF53_I}[wname]
    B, W, H = 2, 61, 47
    px = Pix(fmt, kind, B, W, H)
    pl = Planes(P.PLANE_OF_WAVELET[wavelet], B * px.channels, W, H)
    offset = 1 << (depth - 1)
    src = px.fill(rand_pixels(px, depth, 13, what))
    a, planes, b = Dev(dwt, src), Dev(dwt, pl.fill()), Dev(dwt, px.fill())
    j = P.picture_forward_batch(wavelet, *px.args(a.ptr), depth, offset, 1.0, colour, *pl.args(planes.ptr), -1)
    assert j >= 5
    P.picture_inverse_batch(wavelet, *px.args(b.ptr), depth, offset, 1.0, colour, *pl.args(planes.ptr), j)
    assert np.array_equal(b.get(), src)


def test_ict_float97_round_trip_is_the_models(dwt):
    """ICT + CDF97_S, 5 levels of a 64 x 48 picture: the planes are the model's (pixels_model and the float oracle) bit for
    bit, and the pixels come back as they were"""
    import f16_model

    orc = f16_model.oracle()
    P = dwt.pixels
    W, H, J = 64, 48, 5
    px, pl = Pix(pm.U8, "rgb", 1, W, H), Planes(pm.S, 3, W, H)
    vals = rand_pixels(px, 8, 97)
    want = model_planes(pl, vals.astype(np.uint8), pm.RGB, 128, 1.0, pm.ICT).copy()
    for c in range(3):
        a = want[c].copy()
        assert orc.fwd("cdf97_2f_s", a, J) == J
        want[c] = a
    a, planes, b = Dev(dwt, px.fill(vals)), Dev(dwt, pl.fill()), Dev(dwt, px.fill())
    assert P.picture_forward_batch(dwt.CDF97_S, *px.args(a.ptr), 8, 128, 1.0, pm.ICT, *pl.args(planes.ptr), J) == J
    assert same_bits(pl.read(planes.get()), want)
    back = want.copy()
    for c in range(3):
        t = back[c].copy()
        orc.inv("cdf97_2i_s", t, J)
        back[c] = t
    model_pix = model_pixels(px, back, 8, 128, 1.0, pm.ICT)
    P.picture_inverse_batch(dwt.CDF97_S, *px.args(b.ptr), 8, 128, 1.0, pm.ICT, *pl.args(planes.ptr), J)
    got = px.read(b.get())
    assert np.array_equal(got, model_pix) and np.array_equal(got, vals.astype(np.uint8))


# ---- host memory ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [(False, False), (False, True), (True, False)])
def test_host_memory_gives_the_device_calls_bits(dwt, device):
    """numpy pixels and / or numpy planes: the model's bits (which the device call gives), canaries kept -- also with pitch
    padding and an unused pixel element, where the written region holds bytes that are not the frame's"""
    for fmt, kind, depth, plane, colour, pitch in ((pm.U8, "rgb", 8, pm.I16, pm.RCT, "dense"), (pm.U8, "rgbx", 8, pm.S, pm.ICT, "prime"),
                                                   (pm.U16, "planar", 12, pm.H, pm.ICT, "padded16")):
        px = Pix(fmt, kind, 2, 50, 7, pitch, base=1 if pitch == "prime" else 0)
        pl = Planes(plane, 2 * px.channels, 50, 7, "dense" if pitch == "dense" else "odd", gap=0 if pitch == "dense" else 3)
        check_forward(dwt, px, pl, depth, 1 << (depth - 1), 1.0, colour, rand_pixels(px, depth, 14), device=device)
        check_inverse(dwt, px, pl, depth, 1 << (depth - 1), 1.0, colour, rand_planes(pl, depth, 1.0, 15), device=device)
    # the composite entries on host memory: the device call's bytes
    P = dwt.pixels
    px, pl = Pix(pm.U8, "rgb", 2, 64, 48), Planes(pm.I16, 6, 64, 48)
    src = px.fill(rand_pixels(px, 8, 16))
    a, planes_d = Dev(dwt, src), Dev(dwt, pl.fill())
    j = P.picture_forward_batch(dwt.CDF53_I16, *px.args(a.ptr), 8, 128, 1.0, pm.RCT, *pl.args(planes_d.ptr), 5)
    pix_h, planes_h = src.copy(), pl.fill()
    pp = pix_h.ctypes.data if not device[0] else a.ptr
    holder = Dev(dwt, planes_h) if device[1] else None
    lp = holder.ptr if device[1] else planes_h.ctypes.data
    assert P.picture_forward_batch(dwt.CDF53_I16, *px.args(pp), 8, 128, 1.0, pm.RCT, *pl.args(lp), 5) == j == 5
    got_planes = holder.get() if device[1] else planes_h
    assert np.array_equal(got_planes, planes_d.get())
    out = px.fill()
    out_d = Dev(dwt, out) if device[0] else None
    P.picture_inverse_batch(dwt.CDF53_I16, *px.args(out_d.ptr if device[0] else out.ctypes.data), 8, 128, 1.0, pm.RCT, *pl.args(lp), j)
    assert np.array_equal(out_d.get() if device[0] else out, src)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals(dwt):
    """every refusal of the header returns its code with a message and leaves canaried outputs untouched, both directions"""
    P = dwt.pixels
    W, H = 16, 8
    px8, px16 = Pix(pm.U8, "bgra", 2, W, H), Pix(pm.U16, "rgb", 2, W, H)
    bufs = {}

    def dev(layout):
        if id(layout) not in bufs:
            bufs[id(layout)] = (Dev(dwt, layout.fill()), layout)
        return bufs[id(layout)][0]

    planes = {p: Planes(p, 8, W, H) for p in (pm.I16, pm.I32, pm.H, pm.S)}

    def refused(px, plane, depth=8, scale=1.0, colour=pm.NONE, channels=None, lp=None, composite=None, batch=None):
        pl = planes[plane]
        a = list(px.args(dev(px).ptr))
        if channels is not None:
            a[7] = channels
        if batch is not None:
            a[6] = batch
        la = list(pl.args(dev(pl).ptr))
        if lp is not None:
            la[0] = lp
        for inverse in (False, True):
            with pytest.raises(dwt.DwtError) as e:
                if composite is None:
                    (P.planes_to_pixels_batch if inverse else P.pixels_to_planes_batch)(*a, depth, 128, scale, colour, plane, *la)
                elif inverse:
                    P.picture_inverse_batch(composite, *a, depth, 128, scale, colour, *la, 3)
                else:
                    P.picture_forward_batch(composite, *a, depth, 128, scale, colour, *la, 3)
            assert len(str(e.value)) > 40, str(e.value)

    refused(px8, pm.S, colour=pm.RCT)
    refused(px8, pm.H, colour=pm.RCT)
    refused(px8, pm.I16, colour=pm.ICT)
    refused(px8, pm.I32, colour=pm.ICT)
    refused(px8, pm.I32, scale=2.0)
    refused(px8, pm.I16, scale=float("nan"))
    refused(px8, pm.I32, colour=pm.RCT, channels=1)
    refused(px8, pm.S, colour=pm.ICT, channels=1)
    refused(px16, pm.I16, depth=16, colour=pm.RCT)
    refused(px8, pm.I32, depth=9)
    refused(px8, pm.I32, depth=0)
    refused(px16, pm.I32, depth=17)
    refused(px8, pm.I32, channels=2)
    refused(px8, pm.I32, channels=5)
    refused(px8, pm.I32, lp=dev(px8).ptr + 64)  # the planes inside the pixels
    refused(px8, pm.S, composite=dwt.CDF97_D)
    refused(px8, pm.S, composite=dwt.CDF53_D)
    refused(px8, pm.I32, composite=dwt.CDF53_I, colour=pm.ICT)
    # more than 65535 planes in a composite call: 16384 pictures of 4 channels, 1 x 1 (buffers large enough for them)
    many_pix, many_planes = Dev(dwt, np.full(1 << 16, CANARY, np.uint8)), Dev(dwt, np.full(1 << 18, CANARY, np.uint8))
    with pytest.raises(dwt.DwtError) as e:
        P.picture_forward_batch(dwt.CDF53_I, pm.U8, many_pix.ptr, 4, 4, 4, 1, 16384, 4, pm.BGR, 8, 128, 1.0, pm.NONE, many_planes.ptr, 4, 4, 1, 1, 1)
    assert "65535" in str(e.value)
    assert (many_pix.get() == CANARY).all() and (many_planes.get() == CANARY).all()
    for d, layout in bufs.values():
        assert (d.get() == CANARY).all(), "a refused call wrote"


# ---- past the launch grid's caps -----------------------------------------------------------------------------------
def test_rows_past_the_grid_cap(dwt):
    """an 8-pixel-wide RGB8 picture with 300 rows more than one trip of the kernel's row loop covers: row i is a copy of
    row i % 251 (tests/gridlimits.py), so a row taken one cap away from where it belongs meets other data"""
    P = dwt.pixels
    cap = P.GRID_ROWS
    H, W = cap + 300, 8
    assert cap % gridlimits.P and gridlimits.trips(H, cap) == 2
    rows = np.random.default_rng(17).integers(0, 256, (1, gridlimits.P, W, 3))
    px, pl = Pix(pm.U8, "rgb", 1, W, H), Planes(pm.I16, 3, W, H)
    vals = gridlimits.tile(rows, H, axis=1)
    want_rows = model_planes(Planes(pm.I16, 3, W, gridlimits.P), rows.astype(np.uint8), pm.RGB, 128, 1.0, pm.RCT)
    a, b = Dev(dwt, px.fill(vals)), Dev(dwt, pl.fill())
    P.pixels_to_planes_batch(*px.args(a.ptr), 8, 128, 1.0, pm.RCT, pm.I16, *pl.args(b.ptr))
    got = b.get()
    assert same_bits(pl.read(got), gridlimits.tile(want_rows, H, axis=1)) and (got[~pl.own] == CANARY).all()
    c = Dev(dwt, px.fill())
    P.planes_to_pixels_batch(*px.args(c.ptr), 8, 128, 1.0, pm.RCT, pm.I16, *pl.args(b.ptr))
    back = c.get()
    assert np.array_equal(px.read(back), vals.astype(np.uint8)) and (back[~px.own] == CANARY).all()


def test_pictures_past_the_grid_cap(dwt):
    """5 pictures more than one trip of the kernel's batch loop covers, 3 x 2 grey pixels each"""
    P = dwt.pixels
    cap = P.GRID_BATCH
    B, W, H = cap + 5, 3, 2
    assert cap % gridlimits.P and gridlimits.trips(B, cap) == 2
    pics = np.random.default_rng(18).integers(0, 256, (gridlimits.P, H, W, 1))
    px, pl = Pix(pm.U8, "grey", B, W, H), Planes(pm.S, B, W, H)
    vals = gridlimits.tile(pics, B, axis=0)
    want = gridlimits.tile(model_planes(Planes(pm.S, gridlimits.P, W, H), pics.astype(np.uint8), pm.RGB, 128, 0.5, pm.NONE), B, axis=0)
    a, b, c = Dev(dwt, px.fill(vals)), Dev(dwt, pl.fill()), Dev(dwt, px.fill())
    P.pixels_to_planes_batch(*px.args(a.ptr), 8, 128, 0.5, pm.NONE, pm.S, *pl.args(b.ptr))
    got = b.get()
    assert same_bits(pl.read(got), want) and (got[~pl.own] == CANARY).all()
    P.planes_to_pixels_batch(*px.args(c.ptr), 8, 128, 2.0, pm.NONE, pm.S, *pl.args(b.ptr))
    assert np.array_equal(px.read(c.get()), vals.astype(np.uint8))


# ---- the example and the stream --------------------------------------------------------------------------------------
def test_example_picture_lossless(dwt, tmp_path):
    """examples/picture_lossless.c: identical pixels through RCT + CDF53_I16, a small error through ICT + CDF97_H"""
    exe, libdir = tmp_path / "picture_lossless", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "picture_lossless.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "identical" in out.stdout, out.stdout + out.stderr
    # a binary PPM of its own
    ppm = tmp_path / "t.ppm"
    rng = np.random.default_rng(19)
    ppm.write_bytes(b"P6\n# a comment\n37 23\n255\n" + rng.integers(0, 256, 37 * 23 * 3).astype(np.uint8).tobytes())
    out = subprocess.run([str(exe), str(ppm)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "37 x 23" in out.stdout and "identical" in out.stdout, out.stdout + out.stderr


def test_entries_run_on_the_callers_stream():
    """all four entries once on a non-blocking stream behind a bounded delay, in a process of its own (tests/pixels_stream.py,
    on the harness of tests/stream_cases.py): the model's bits, queued without waiting for the stream"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pixels_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]
