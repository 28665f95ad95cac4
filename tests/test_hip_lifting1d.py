"""GPU checks of the user-defined lifting wavelets of line batches (dwt_hip_lifting1d_batch; libdwt_amd/lifting.py; DESIGN.md
s34) against tests/lifting1d_model.py: every bit of every sample, on both routes (option "lifting_fused" 1 and 0), forward and
inverse, in place and out of place.  There is no tolerance anywhere: the inputs are chosen so that the model's result holds
no NaN and no Inf, and the tests assert that.  Every line lies in a buffer of canary words (0xDEADBEEF) with a padded line
stride, or as one channel of three; after a call the canaries are intact and an out-of-place source is unchanged."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import lifting1d_model as l1
import lifting_model as lm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xDEADBEEF
# one sample, lines shorter than the reach (multi-bounce reflection), odd and even lengths, both sides of the launcher's
# rules for the threads of a line (a wave up to 512 samples, half a workgroup up to 2048), the longest line of one launch
SIZES = [1, 2, 3, 5, 17, 64, 65, 511, 513, 2047, 2049, 8191, 8192]
SCHEMES = sorted(lm.BUILTINS) + ["random R=8", "random R>8", "random int"]
N_LINES, J_MAX, LAYOUTS = (1, 3, 5), (-1, 1, 3), ("padded", "channel")
PER_CASE = 3  # of the 18 (n_lines, j, layout) combinations, a seeded sample for every (route, scheme, size)


@functools.lru_cache(maxsize=None)
def model_scheme(name):
    if name == "random R=8":
        return lm.random_scheme(lm.F32, 11, reach=8)
    if name == "random R>8":
        s = lm.random_scheme(lm.F32, 12, reach=11)
        assert s.reach > lm.FUSED_REACH
        return s
    if name == "random int":
        return lm.random_scheme(lm.I32, 2)
    return lm.builtin(name)


def to_lib(L, s):
    return L.scheme(s.type, [L.step(st.parity, st.terms, st.sign, st.add, st.shift) for st in s.steps], s.fwd_scale, s.inv_scale,
                    s.inverse_cols_first)


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d
    from libdwt_amd import lifting

    d.dwt_util_init()
    d.lifting = lifting
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("lifting_fused", 1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


@functools.lru_cache(maxsize=None)
def case(name, size, n_lines, j_max):
    """(input, its forward transform, the inverse of that, J) by the model, computed once and read-only: floats in [-1, 1),
    ints over the whole int32 range, wrapping included"""
    s = model_scheme(name)
    rng = np.random.default_rng([15, size, n_lines])
    if s.type == lm.I32:
        x = rng.integers(-(1 << 31), 1 << 31, (n_lines, size)).astype(np.int32)
    else:
        x = rng.uniform(-1, 1, (n_lines, size)).astype(np.float32)
    y, J = l1.fwd1d(s, x, j_max)
    back, _ = l1.inv1d(s, y, J)
    if s.type == lm.F32:
        assert np.isfinite(y).all() and np.isfinite(back).all()
    for a in (x, y, back):
        a.setflags(write=False)
    return x, y, back, J


class Lay:
    """n_lines lines of `size` 4-byte elements in a buffer of canary words, `pad` words behind every line, elements `ex` words
    apart: "padded" -- dense lines with a padded line stride; "channel" -- elem_stride 12, one channel of three"""

    def __init__(self, n_lines, size, kind="padded", lead=4):
        self.n_lines, self.size = n_lines, size
        ex, pad = (1, 3) if kind == "padded" else (3, 2)
        self.pitch = size * ex + pad
        self.lead = lead
        self.words = lead + self.pitch * n_lines + 4
        y, i = np.ix_(np.arange(n_lines), np.arange(size))
        self.at = lead + y * self.pitch + i * ex
        self.strides = (4 * self.pitch, 4 * ex)  # line_stride, elem_stride in bytes

    def fill(self, values=None):
        buf = np.full(self.words, CANARY, np.uint32)
        if values is not None:
            buf[self.at] = bits(values)
        return buf

    def read(self, buf, dtype):
        return buf[self.at].view(dtype)

    def canaries_intact(self, buf):
        mask = np.ones(self.words, bool)
        mask[self.at] = False
        return bool((buf[mask] == CANARY).all())


def run(dwt, sl, inverse, x, j_max, lay, in_place, device=True, shift=0):
    """one call -> (the destination's lines, the level count returned); the canaries of both buffers and an out-of-place
    source are checked.  shift: bytes by which a device buffer is moved off its alignment (the layout moves with it)"""
    L = dwt.lifting
    src_h, dst_h = lay.fill(x), lay.fill(None if not in_place else x)
    off = 4 * lay.lead
    if device:
        def up(h):
            raw = np.full(h.nbytes + 8, 0xEF, np.uint8)
            raw[shift:shift + h.nbytes] = h.view(np.uint8)
            return Dev(dwt, raw)

        def down(d):
            return d.get()[shift:shift + src_h.nbytes].copy().view(np.uint32)

        src = up(src_h)
        dst = src if in_place else up(dst_h)
        sp, dp = src.ptr + shift + off, dst.ptr + shift + off
    else:
        dst_h = src_h if in_place else dst_h
        sp, dp = src_h.ctypes.data + off, dst_h.ctypes.data + off
    ls, es = lay.strides
    J = L.lifting1d_batch(sl, inverse, sp, dp, ls, es, lay.n_lines, lay.size, j_max)
    if device:
        src_h, dst_h = down(src), down(dst)
    else:
        dwt.sync()
    assert lay.canaries_intact(dst_h) and lay.canaries_intact(src_h), "a word outside the lines was written"
    if not in_place:
        assert np.array_equal(src_h, lay.fill(x)), "the source of an out-of-place call changed"
    return lay.read(dst_h, x.dtype), J


def both_ways(dwt, name, sl, size, n_lines, j_max, layout, placements, **kw):
    """forward and inverse of one case under the placements (False: out of place, True: in place)"""
    x, y, back, J = case(name, size, n_lines, j_max)
    lay = Lay(n_lines, size, layout)
    for in_place in placements:
        got, Jg = run(dwt, sl, False, x, j_max, lay, in_place, **kw)
        assert Jg == J and same(got, y), (size, n_lines, j_max, layout, in_place, "forward", int((bits(got) != bits(y)).sum()))
        got, Jg = run(dwt, sl, True, y, J, lay, in_place, **kw)
        assert Jg == J and same(got, back), (size, n_lines, j_max, layout, in_place, "inverse", int((bits(got) != bits(back)).sum()))


# ---- against the model ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", SCHEMES)
def test_every_bit_is_the_models(dwt, name, fused):
    """The product of routes, schemes, sizes, n_lines, j, directions, placements and layouts is about twenty thousand calls, so
    it is thinned: every (route, scheme, size) runs a seeded sample of PER_CASE of the (n_lines, j, layout) combinations, each
    forward and inverse, out of place and in place.  Over a scheme's sizes every n_lines, every j and both layouts occur.  One
    test per route and scheme runs every size (a failure names the size): some 150 small calls, a fraction of a second."""
    L = dwt.lifting
    s = model_scheme(name)
    sl = to_lib(L, s)
    dwt.set_option("lifting_fused", fused)
    combos = list(itertools.product(N_LINES, J_MAX, LAYOUTS))
    for size in SIZES:
        assert L.route1d(sl, size) == (L.FUSED if fused else L.STEPS)
        rng = np.random.default_rng([19, SCHEMES.index(name), size])  # (the same sample on both routes: the model's cases are shared)
        for c in rng.choice(len(combos), PER_CASE, replace=False):
            n_lines, j_max, layout = combos[c]
            both_ways(dwt, name, sl, size, n_lines, j_max, layout, (False, True))
    dwt.set_option("lifting_fused", 1)


def test_the_sample_covers_every_value():
    """the thinning above leaves no n_lines, j or layout out for any scheme (no GPU work; it stands here with what it guards)"""
    combos = list(itertools.product(N_LINES, J_MAX, LAYOUTS))
    for name in SCHEMES:
        seen = set()
        for size in SIZES:
            rng = np.random.default_rng([19, SCHEMES.index(name), size])
            seen.update(combos[c] for c in rng.choice(len(combos), PER_CASE, replace=False))
        assert {c[0] for c in seen} == set(N_LINES) and {c[1] for c in seen} == set(J_MAX) and {c[2] for c in seen} == set(LAYOUTS), name


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("size", [8193, 20001])
@pytest.mark.parametrize("name", ["D4", "CDF53_INT"])
def test_lines_longer_than_the_cap(dwt, name, size, fused):
    """2 lines, full depth: the over-long levels step by step, the rest in one launch over the L prefix (option 0: every level
    step by step); the model's bits forward and inverse, out of place and in place"""
    L = dwt.lifting
    sl = L.builtin(name)
    dwt.set_option("lifting_fused", fused)
    assert L.route1d(sl, size) == L.STEPS
    both_ways(dwt, name, sl, size, 2, -1, "padded", (False, True))
    if fused:  # the levels above the cap, each 2 + the scheme's steps launches, and one launch for the rest
        x, y, _, J = case(name, size, 2, -1)
        n_steps, over = len(model_scheme(name).steps), sum(l1.length(size, k) > l1.N1D_MAX for k in range(J))
        src, dst = Dev(dwt, x), Dev(dwt, np.zeros_like(x))
        assert 0 < over < J and launches(dwt, lambda: L.lifting1d_batch(sl, False, src.ptr, dst.ptr, 4 * size, 4, 2, size, -1)) == over * (2 + n_steps) + 1
        assert same(dst.get(), y)
    dwt.set_option("lifting_fused", 1)


@pytest.mark.parametrize("size", [2, 17, 513, 8192])
@pytest.mark.parametrize("name, wavelet", [("CDF97", "cdf97_s"), ("CDF53", "cdf53_s"), ("INTERP53", "interp53_s")])
def test_cdf_tables_give_the_specialised_kernels_bits(dwt, name, wavelet, size):
    """lifting1d_batch with a CDF table against dwt_hip_transform1d_batch of the wavelet: 3 dense lines with |x| <= 1, forward
    and inverse"""
    L = dwt.lifting
    x, y, _, J = case(name, size, 3, -1)
    sl = L.builtin(name)
    for inverse, data in ((False, x), (True, y)):
        src = Dev(dwt, data)
        a, b = Dev(dwt, np.zeros_like(data)), Dev(dwt, np.zeros_like(data))
        assert L.lifting1d_batch(sl, inverse, src.ptr, a.ptr, 4 * size, 4, 3, size, -1 if not inverse else J) == J
        assert dwt.transform1d_batch(wavelet, inverse, src.ptr, b.ptr, 4 * size, 3, size, -1 if not inverse else J) == J
        assert same(a.get(), b.get()), (name, inverse)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", ["D4", "CDF97_INT"])
def test_host_and_misaligned_lines(dwt, name, fused):
    """host lines (dense and one channel of three), and device lines 6 bytes off their alignment: the staging path, the same
    bits"""
    L = dwt.lifting
    sl = L.builtin(name)
    dwt.set_option("lifting_fused", fused)
    for kw, layout in (({"device": False}, "padded"), ({"device": False}, "channel"), ({"shift": 6}, "channel"), ({"shift": 6}, "padded")):
        both_ways(dwt, name, sl, 333, 3, -1, layout, (False, True), **kw)
    dwt.set_option("lifting_fused", 1)


# ---- launches, routes, grid, errors -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["D4", "HAAR_INT", "random R>8"])
def test_fused_route_is_one_launch(dwt, name):
    """whatever the depth and the number of lines, in place and out of place; a second identical call allocates nothing; no
    level: no launch in place, one copy out of place"""
    L = dwt.lifting
    sl = to_lib(L, model_scheme(name))
    dwt.set_option("lifting_fused", 1)
    for size, n_lines, j_max in ((8192, 3, -1), (700, 5, 3), (64, 1, 1)):
        assert L.route1d(sl, size) == L.FUSED
        x, y, back, J = case(name, size, n_lines, j_max)
        src, dst = Dev(dwt, x), Dev(dwt, np.zeros_like(x))
        geom = (4 * size, 4, n_lines, size)
        for inverse, data, want in ((False, x, y), (True, y, back)):
            def upload():
                assert dwt.lib.dwt_hip_memcpy_h2d(src.ptr, np.ascontiguousarray(data).ctypes.data, data.nbytes) == 0

            calls = (lambda: L.lifting1d_batch(sl, inverse, src.ptr, dst.ptr, *geom, J if inverse else j_max),
                     lambda: L.lifting1d_batch(sl, inverse, src.ptr, src.ptr, *geom, J if inverse else j_max))
            upload()
            calls[0]()
            dwt.sync()
            allocs = dwt.get_option("stat_allocs")
            assert launches(dwt, calls[0]) == 1
            assert same(dst.get(), want)
            assert launches(dwt, calls[1]) == 1
            assert same(src.get(), want)
            assert dwt.get_option("stat_allocs") == allocs
        assert launches(dwt, lambda: L.lifting1d_batch(sl, False, src.ptr, src.ptr, *geom, 0)) == 0
        assert launches(dwt, lambda: L.lifting1d_batch(sl, False, src.ptr, dst.ptr, *geom, 0)) == 1
        assert same(dst.get(), src.get())


def test_routes(dwt):
    L = dwt.lifting
    far = to_lib(L, model_scheme("random R>8"))
    dwt.set_option("lifting_fused", 1)
    assert L.route(far) == L.STEPS  # (the tile kernels of the 2-D entry stop at reach 8)
    assert L.route1d(far, 8192) == L.FUSED and L.route1d(far, 1) == L.FUSED
    assert L.route1d(far, 8193) == L.STEPS
    dwt.set_option("lifting_fused", 0)
    assert L.route1d(far, 8192) == L.STEPS and L.route1d(L.builtin("HAAR"), 16) == L.STEPS
    dwt.set_option("lifting_fused", 1)
    bad = L.builtin("D4")
    bad.steps[1].terms[0].off_a = 2
    assert dwt.lib.dwt_hip_lifting1d_route(bad, 64) == -1 and "off_a" in dwt.last_error()
    assert dwt.lib.dwt_hip_lifting1d_route(L.builtin("D4"), 0) == -1 and "sizes" in dwt.last_error()
    with pytest.raises(dwt.DwtError):
        L.route1d(bad, 64)


@pytest.mark.parametrize("fused", [1, 0])
def test_more_lines_than_any_block_index_limit(dwt, fused):
    """The launch geometry has no cap on n_lines: 65536 * 4 + 1 lines of 2 samples -- more workgroups than
    the 65535 that cap other kernels' grid.y / grid.z, the last workgroup with one line of its four"""
    L = dwt.lifting
    dwt.set_option("lifting_fused", fused)
    s, sl = model_scheme("D4"), L.builtin("D4")
    n = 65536 * 4 + 1
    x = np.random.default_rng(8).uniform(-1, 1, (n, 2)).astype(np.float32)
    want, J = l1.fwd1d(s, x, -1)
    src, dst = Dev(dwt, x), Dev(dwt, np.full(x.shape, CANARY, np.uint32))
    assert L.lifting1d_batch(sl, False, src.ptr, dst.ptr, 8, 4, n, 2, -1) == J == 1
    assert same(dst.get(shape=x.shape, dtype=np.float32), want)
    dwt.set_option("lifting_fused", 1)


def test_refusals_leave_dst_untouched(dwt):
    L = dwt.lifting
    size, n_lines = 40, 3
    lay = Lay(n_lines, size)
    x = case("D4", size, n_lines, -1)[0]
    src, dst = Dev(dwt, lay.fill(x)), Dev(dwt, lay.fill())
    host = lay.fill(x)
    ls, es = lay.strides
    good = L.builtin("D4")

    def refused(word, scheme=good, s=src.ptr + 16, d=dst.ptr + 16, line_stride=ls, elem_stride=es, n=n_lines, size=size):
        n0 = dwt.get_option("stat_launches")
        with pytest.raises(dwt.DwtError) as e:
            L.lifting1d_batch(scheme, False, s, d, line_stride, elem_stride, n, size, -1)
        assert word in str(e.value), str(e.value)
        assert dwt.get_option("stat_launches") == n0, "a refused call launched"
        assert np.array_equal(dst.get(), lay.fill()) and np.array_equal(src.get(), lay.fill(x)), "a refused call wrote"

    bad = L.builtin("D4")
    bad.steps[1].terms[0].off_a = 2
    refused("off_a", scheme=bad)
    bad = L.builtin("HAAR_INT")
    bad.inverse_cols_first = 0
    refused("inverse_cols_first", scheme=bad)
    refused("sizes", size=0)
    refused("sizes", size=-5)
    refused("lines", n=0)
    refused("lines", n=-3)
    refused("strides", elem_stride=2)
    refused("strides", line_stride=4 * size - 4)
    refused("overlap", d=src.ptr + 16 + 8)
    refused("null", d=0)
    refused("null", s=0)
    refused("both", s=host.ctypes.data + 16)
    refused("both", d=host.ctypes.data + 16)
    # ... and the same call with nothing wrong runs
    assert L.lifting1d_batch(good, False, src.ptr + 16, dst.ptr + 16, ls, es, n_lines, size, -1) == lm.ceil_log2(size)
    assert same(lay.read(dst.get(), np.float32), case("D4", size, n_lines, -1)[1])


# ---- stream, example ------------------------------------------------------------------------------------------------------

def test_entry_runs_on_the_callers_stream():
    """forward and inverse on both routes, in place and out of place, once on a non-blocking stream behind a bounded delay, in
    a process of its own (tests/lifting1d_stream.py, on the harness of tests/stream_cases.py): the model's bits; the calls on
    device memory queued without waiting for the stream"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lifting1d_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]


def test_example_spectra_custom_wavelet(dwt, tmp_path):
    """examples/spectra_custom_wavelet.c compiles with the gcc line of its header comment, runs and exits 0"""
    exe, libdir = tmp_path / "spectra_custom_wavelet", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "spectra_custom_wavelet.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "round trip" in out.stdout and "lossless" in out.stdout, out.stdout + out.stderr
