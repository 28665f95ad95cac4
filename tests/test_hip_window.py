"""GPU checks of the windowed inverse (dwt_hip_inverse_window_batch; libdwt_amd/window.py) against tests/window_model.py: the
crop of the full inverse, bit for bit with a NaN equal to a NaN, under both routes.  The source has a padded pitch and batch
stride and is byte-identical after every call; the destination has a padded pitch and a base one element into a buffer of
canary words, every one of which outside the windows keeps the canary.  Every call starts on poisoned scratch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import floatends
import window_model as wm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (h, w): one tile exactly; one element past a tile; two tiles with odd sizes at every level, both ways; a few samples; no level at all
FRAMES = [(64, 64), (65, 129), (67, 131), (130, 70), (5, 5), (2, 9), (9, 1), (1, 9)]
ROUTES = (0, 2)
CANARY = {4: 0xC0FFEE11, 2: 0xC0DE}


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d
    from libdwt_amd import window

    d.dwt_util_init()
    d.window = window
    assert (window.TILE, window.GRID_BATCH) == (64, 4096)
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("window_fused", 1)


@pytest.fixture(scope="module")
def orc():
    from oraclelib import Oracle

    return Oracle()


def words(dtype):
    return {4: np.uint32, 2: np.uint16}[np.dtype(dtype).itemsize]


class Source:
    """`frames` (B, h, w) in device memory with a padded pitch and batch stride (both multiples of 4 bytes), canary between"""

    def __init__(self, dwt, frames):
        B, h, w = frames.shape
        u = words(frames.dtype)
        self.es = frames.dtype.itemsize
        self.pitch_e = (w + 7) // 2 * 2
        self.bs_e = self.pitch_e * h + 8
        self.host = np.full(B * self.bs_e + 8, CANARY[self.es], u)
        for b in range(B):
            rows = self.host[b * self.bs_e:b * self.bs_e + self.pitch_e * h].reshape(h, self.pitch_e)
            rows[:, :w] = np.ascontiguousarray(frames[b]).view(u)
        self.dev = Dev(dwt, self.host)
        self.B, self.h, self.w = B, h, w

    def args(self):
        return self.dev.ptr, self.bs_e * self.es, self.B, self.pitch_e * self.es, self.w, self.h

    def unchanged(self):
        return self.dev.get().tobytes() == self.host.tobytes()


def run_window(dwt, wavelet, src, j_max, r, win, route):
    """one call -> the windows (B, wh, ww); asserts the canary around them"""
    x0, y0, ww, wh = win
    dt = np.dtype(wm.DTYPE[wavelet])
    u, es = words(dt), dt.itemsize
    pitch_e, base_e = ww + 3, 1
    bs_e = pitch_e * wh + 5
    host = np.full(base_e + src.B * bs_e + 8, CANARY[es], u)
    dev = Dev(dwt, host)
    dwt.set_option("window_fused", route)
    try:
        dwt.window.inverse_window_batch(wavelet, *src.args(), j_max, r, x0, y0, ww, wh, dev.ptr + base_e * es, bs_e * es, pitch_e * es)
    finally:
        dwt.set_option("window_fused", 1)
    got = dev.get()
    dev.free()
    own = np.zeros(host.shape, bool)
    out = np.empty((src.B, wh, ww), dt)
    for b in range(src.B):
        at = base_e + b * bs_e + (np.arange(wh)[:, None] * pitch_e + np.arange(ww)[None, :])
        own[at] = True
        out[b] = got[at].view(dt)
    assert (got[~own] == CANARY[es]).all(), "%d words written outside the windows" % int((got[~own] != CANARY[es]).sum())
    return out


def parity_windows(bw, bh):
    """(x0, y0, w, h) in a band of bw x bh: the whole band, the 1 x 1 corners, the tile seams, every border, an odd interior"""
    out = [(0, 0, bw, bh), (0, 0, 1, 1), (bw - 1, 0, 1, 1), (0, bh - 1, 1, 1), (bw - 1, bh - 1, 1, 1)]
    if bw > 66:
        out.append((62, min(3, bh - 1), 5, min(7, bh - min(3, bh - 1))))  # columns 62 .. 66
    if bh > 66:
        out.append((min(5, bw - 1), 62, min(9, bw - min(5, bw - 1)), 5))  # rows 62 .. 66
    mx, my = min(3, bw), min(3, bh)
    cx, cy = bw // 3, bh // 3
    out += [(0, cy, mx, min(5, bh - cy)), (bw - mx, cy, mx, min(5, bh - cy)), (cx, 0, min(6, bw - cx), my), (cx, bh - my, min(6, bw - cx), my)]
    ox, oy = min(bw - 1, 7 if bw > 9 else 1), min(bh - 1, 5 if bh > 9 else 1)
    out.append((ox, oy, max(1, min(21, bw - ox - 1)), max(1, min(13, bh - oy - 1))))
    return list(dict.fromkeys(out))


def level_counts(h, w):
    Jf = wm.ceil_log2(min(h, w))
    return sorted({min(1, Jf), min(2, Jf), Jf})


def cases(h, w):
    """(j_max, discard, window, batch): J in {1, 2, full}, r in {0, 1, J}; three frames and one frame"""
    for j_max in level_counts(h, w):
        for r in sorted({0, min(1, j_max), j_max}):
            for win in parity_windows(wm.band(w, r), wm.band(h, r)):
                yield j_max, r, win, 3
                yield j_max, r, win, 1


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("wavelet", wm.WAVELETS)
def test_windows_are_crops_of_the_full_inverse(dwt, orc, wavelet, route):
    n = 0
    for h, w in FRAMES:
        frames = np.stack([wm.make_frame(wavelet, 5000 + 31 * h + w + b, h, w) for b in range(3)])
        srcs = {3: Source(dwt, frames), 1: Source(dwt, frames[1:2])}
        full = {}
        for j_max, r, win, batch in cases(h, w):
            if (j_max, r) not in full:
                full[j_max, r] = np.stack([wm.full_inverse(orc, wavelet, f, j_max, r) for f in frames])
            x0, y0, ww, wh = win
            want = full[j_max, r][:, y0:y0 + wh, x0:x0 + ww]
            got = run_window(dwt, wavelet, srcs[batch], j_max, r, win, route)
            assert wm.same(got, want if batch == 3 else want[1:2]), (wavelet, route, h, w, j_max, r, win, batch)
            n += 1
        for s in srcs.values():
            assert s.unchanged(), (wavelet, route, h, w)
            s.dev.free()
    print("%s route %d: %d calls" % (wavelet, route, n))
    assert n > 300


@pytest.mark.parametrize("wavelet", wm.WAVELETS)
def test_the_kernels_read_nothing_outside_the_regions(dwt, orc, wavelet):
    """route 2 on a source that holds NaN (floats) or other random integers everywhere outside window_regions' rectangles:
    the windows of the clean source, bit for bit"""
    n = 0
    for h, w in FRAMES[:6]:
        frame = wm.make_frame(wavelet, 5100 + 31 * h + w, h, w)
        full = {}
        for j_max, r, win, batch in cases(h, w):
            if batch != 3 or r == j_max:
                continue
            if (j_max, r) not in full:
                full[j_max, r] = wm.full_inverse(orc, wavelet, frame, j_max, r)
            x0, y0, ww, wh = win
            reg = dwt.window.window_regions(wavelet, w, h, j_max, r, x0, y0, ww, wh)
            assert np.array_equal(reg, wm.regions(wavelet, h, w, j_max, r, x0, y0, ww, wh))
            src = Source(dwt, wm.masked(wavelet, frame, reg, n)[None])
            got = run_window(dwt, wavelet, src, j_max, r, win, 2)
            src.dev.free()
            assert wm.same(got[0], full[j_max, r][y0:y0 + wh, x0:x0 + ww]), (wavelet, h, w, j_max, r, win)
            n += 1
    assert n > 60


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("klass", ["finite", "ends"])
@pytest.mark.parametrize("wavelet", wm.FLOAT_WAVELETS)
def test_float_classes_on_the_border_windows(dwt, orc, wavelet, klass, route):
    """the inputs of tests/floatends.py on the four 16-wide border windows (tests/test_window.py counts what they tell):
    the line-end forms on the device"""
    from test_window import ENDS_ENTRY, ENDS_SHAPES

    for k, shp in enumerate(ENDS_SHAPES):
        a = floatends.class_input(klass, 4400 + k, shp)
        depth = floatends.ends_level(orc, ENDS_ENTRY[wavelet], a) if klass == "ends" else 2
        full = wm.full_inverse(orc, wavelet, a, depth, 0)
        src = Source(dwt, a[None])
        for x0, y0, ww, wh in wm.border_windows(*shp):
            got = run_window(dwt, wavelet, src, depth, 0, (x0, y0, ww, wh), route)
            assert wm.same(got[0], full[y0:y0 + wh, x0:x0 + ww]), (wavelet, klass, route, shp, (x0, y0, ww, wh))
        src.dev.free()


def test_routes_and_launch_counts(dwt):
    """route 2 is one launch per level above the discarded ones, route 0 the driver's launches and the copy; the default
    takes the kernels for a small window and the driver for the whole band"""
    W = dwt.window
    h, w, J = 130, 70, 3
    src = Source(dwt, np.stack([wm.make_frame("cdf97_s", 5200 + b, h, w) for b in range(3)]))
    dst = Dev(dwt, np.zeros(3 * h * w, np.float32))

    def call(r, win):
        return launches(dwt, lambda: W.inverse_window_batch("cdf97_s", *src.args(), J, r, *win, dst.ptr, 4 * h * w, 4 * w))

    dwt.set_option("window_fused", 2)
    assert [call(r, (1, 1, 5, 7)) for r in (0, 1, 2, 3)] == [3, 2, 1, 1]
    dwt.set_option("window_fused", 0)
    assert call(0, (1, 1, 9, 7)) == 4 and call(3, (1, 1, 5, 7)) == 1
    # the default: the kernels for a window of up to 1 / 16 of a band of 8192^2 samples or more over the batch
    dwt.set_option("window_fused", 1)
    assert W.window_route("cdf97_s", 3, w, h, J, 0, 1, 1, 9, 7) == W.ROUTE_INVERSE and call(0, (1, 1, 9, 7)) == 4
    for batch, size, r, side, route in ((1, 8192, 0, 512, 2), (1, 8192, 0, 2048, 2), (1, 8192, 0, 2049, 0), (1, 8192, 0, 8192, 0), (1, 8192, 2, 128, 0),
                                        (16, 4096, 0, 512, 2), (4, 4096, 0, 512, 2), (3, 4096, 0, 512, 0), (1, 8191, 0, 512, 0)):
        assert W.window_route("cdf53_i16", batch, size, size, 5, r, 1, 1, side if side < size else size - 1, side if side < size else size - 1) == route, (batch, size, r, side)
    assert W.window_route("cdf97_s", 1, 8192, 8192, 5, 5, 0, 0, 16, 16) == W.ROUTE_INVERSE  # (nothing to undo)
    for route in (0, 2):
        dwt.set_option("window_fused", route)
        assert W.window_route("cdf97_s", 1, 8192, 8192, 5, 0, 1, 1, 8000, 8000) == route
    dwt.set_option("window_fused", 1)
    # nothing is allocated after the first call of a shape
    for route in (0, 2):
        dwt.set_option("window_fused", route)
        call(0, (1, 1, 40, 50))
        a0 = dwt.get_option("stat_allocs")
        call(0, (1, 1, 40, 50))
        assert dwt.get_option("stat_allocs") == a0
    dwt.set_option("window_fused", 1)
    src.dev.free()
    dst.free()


def test_refusals_write_nothing(dwt):
    W = dwt.window
    h, w, J = 20, 24, 2
    frames = np.stack([wm.make_frame("cdf53_s", 5300 + b, h, w) for b in range(2)])
    src = Dev(dwt, frames)
    canary = np.full(2 * h * w + 16, CANARY[4], np.uint32)
    dst = Dev(dwt, canary)
    host = np.zeros(2 * h * w, np.float32)
    good = dict(wavelet=dwt.CDF53_S, src=src.ptr, bs=4 * h * w, batch=2, sx=4 * w, w=w, h=h, j=J, r=1, x0=1, y0=2, ww=5, wh=4, dst=dst.ptr, dbs=4 * 40, dsx=4 * 8)

    def call(**kw):
        a = dict(good, **kw)
        return dwt.lib.dwt_hip_inverse_window_batch(a["wavelet"], a["src"], a["bs"], a["batch"], a["sx"], a["w"], a["h"], a["j"], a["r"], a["x0"], a["y0"],
                                                    a["ww"], a["wh"], a["dst"], a["dbs"], a["dsx"])

    assert call() == 0
    dwt.sync()
    assert dwt.lib.dwt_hip_memcpy_h2d(dst.ptr, canary.ctypes.data, canary.nbytes) == 0
    bad = [dict(wavelet=dwt.CDF97_H), dict(wavelet=dwt.CDF97_I), dict(wavelet=dwt.CDF97_D), dict(wavelet=7),  # unsupported wavelets
           dict(ww=0), dict(x0=-1), dict(x0=8, ww=5), dict(y0=7, wh=4), dict(r=3), dict(r=-1),  # windows that are empty or leave LL(r)
           dict(dst=src.ptr + 4 * h * w - 64), dict(dst=src.ptr + 4 * h * w + 16),  # the destination shares bytes with a source frame
           dict(dst=host.ctypes.data), dict(src=host.ctypes.data), dict(src=None), dict(dst=None),  # host and null pointers
           dict(batch=0), dict(sx=4 * w - 4), dict(sx=4 * w + 2), dict(bs=4 * h * w - 4), dict(dsx=4 * 4), dict(dsx=4 * 8 + 2), dict(dbs=4 * 20),
           dict(dst=dst.ptr + 2), dict(src=src.ptr + 2)]
    for route in ROUTES:
        dwt.set_option("window_fused", route)
        for kw in bad:
            n0 = dwt.get_option("stat_launches")
            assert call(**kw) != 0, (route, kw)
            assert dwt.last_error() and dwt.get_option("stat_launches") == n0, (route, kw)
    dwt.set_option("window_fused", 1)
    assert dst.get().tobytes() == canary.tobytes() and src.get().tobytes() == frames.tobytes()
    src.free()
    dst.free()


@pytest.mark.parametrize("route", ROUTES)
def test_batch_past_the_grid_cap(dwt, orc, route):
    """GRID_BATCH + 1 frames of 6 x 5: the kernels' batch loop takes a second trip"""
    B, h, w = dwt.window.GRID_BATCH + 1, 5, 6
    base = np.stack([wm.make_frame("cdf53_s", 5400 + b, h, w) for b in range(7)])
    frames = base[np.arange(B) % 7]
    src = Source(dwt, frames)
    full = np.stack([wm.full_inverse(orc, "cdf53_s", f, -1, 0) for f in base])[np.arange(B) % 7]
    for j_max, r, win in ((-1, 0, (1, 1, 4, 3)), (-1, 3, (0, 0, 1, 1))):
        got = run_window(dwt, "cdf53_s", src, j_max, r, win, route)
        x0, y0, ww, wh = win
        want = full[:, y0:y0 + wh, x0:x0 + ww] if r == 0 else frames[:, :1, :1]
        assert wm.same(got, want), (route, j_max, r)
    src.dev.free()


def test_example_picture_window(dwt, tmp_path):
    """examples/picture_window.c: both viewports pixel for pixel the crops of the full picture inverses"""
    exe, libdir = tmp_path / "picture_window", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "picture_window.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "viewports identical" in out.stdout and out.stdout.count(": 0 pixels differ") == 2, out.stdout + out.stderr


def test_entry_runs_on_the_callers_stream():
    """both routes once on a non-blocking stream behind a bounded delay, in a process of its own (tests/window_stream.py, on
    the harness of tests/stream_cases.py): the model's bits, the calls queued without waiting for the stream, the launch
    count that of the warm-up"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "window_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]
