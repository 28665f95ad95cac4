"""GPU checks of the user-defined lifting wavelets (dwt_hip_lifting2d_batch; libdwt_amd/lifting.py) against
tests/lifting_model.py: every bit of every sample, on both routes (option "lifting_fused" 1 and 0), forward and inverse,
in place and out of place.  There is no tolerance anywhere: the inputs are chosen so that the model's result holds no NaN
and no Inf, and the tests assert that.  Every frame lies in a buffer of canary words (0xDEADBEEF) with a padded row pitch
and a gap between the frames; after a call the canaries are intact and an out-of-place source is unchanged."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import lifting_model as lm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xDEADBEEF
# (W, H, batch): lines shorter than the reach (multi-bounce reflection); one tile; tile seams both ways with odd LL sizes
# deeper down; several tiles and a batch
SHAPES = [(2, 2, 1), (3, 5, 2), (5, 3, 1), (17, 9, 1), (64, 64, 1), (65, 63, 1), (66, 130, 1), (130, 66, 2), (200, 136, 3)]
SCHEMES = sorted(lm.BUILTINS) + ["random R=8", "random R>8"]


@functools.lru_cache(maxsize=None)
def model_scheme(name):
    if name == "random R=8":
        return lm.random_scheme(lm.F32, 11, reach=8)
    if name == "random R>8":
        s = lm.random_scheme(lm.F32, 12, reach=11)
        assert s.reach > lm.FUSED_REACH
        return s
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


@functools.lru_cache(maxsize=None)
def case(name, W, H, B, j_max, content="unit"):
    """(input, its forward transform, the inverse of that, J) by the model, computed once and read-only.  Contents: "unit" --
    floats in [-1, 1), ints in +-2^20; "wide" (float) -- magnitudes from subnormal to 1e30, both zeros, subnormals; "full"
    (int) -- the whole int32 range, wrapping included"""
    s = model_scheme(name)
    rng = np.random.default_rng([5, W, H, B, len(content)])
    if s.type == lm.I32:
        x = rng.integers(-(1 << 31), 1 << 31, (B, H, W)) if content == "full" else rng.integers(-(1 << 20), 1 << 20, (B, H, W))
        x = x.astype(np.int32)
    elif content == "wide":
        x = (rng.choice([-1.0, 1.0], (B, H, W)) * 10.0 ** rng.uniform(-44, 30, (B, H, W))).astype(np.float32)
        flat = x.reshape(-1)
        special = np.array([0.0, -0.0, 1e-45, -1e-40, 1e30, -1e30], np.float32)
        flat[rng.choice(flat.size, min(flat.size, len(special)), replace=False)] = special[:min(flat.size, len(special))]
    else:
        x = rng.uniform(-1, 1, (B, H, W)).astype(np.float32)
    while True:
        y, J = lm.fwd2d(s, x, j_max)
        back, _ = lm.inv2d(s, y, J)
        if s.type == lm.I32 or (np.isfinite(y).all() and np.isfinite(back).all()):
            break
        x = x * np.float32(1e-5)  # (a scheme that grows 1e30 beyond the float range: the same class, smaller)
    for a in (x, y, back):
        a.setflags(write=False)
    return x, y, back, J


class Lay:
    """`batch` frames of W x H 4-byte elements in a buffer of canary words: `pad` words behind every row, `gap` words between
    the frames, elements `ex` words apart"""

    def __init__(self, batch, W, H, pad=3, gap=5, ex=1):
        self.batch, self.W, self.H = batch, W, H
        self.pitch = W * ex + pad
        self.bs = self.pitch * H + gap
        self.words = 4 + self.bs * batch + 4
        b, y, x = np.ix_(np.arange(batch), np.arange(H), np.arange(W))
        self.at = 4 + b * self.bs + y * self.pitch + x * ex
        self.strides = (4 * self.bs, 4 * self.pitch, 4 * ex)  # batch stride, stride_x, stride_y in bytes

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


def run(dwt, sl, inverse, x, j_max, lay, in_place, device=True):
    """one call -> (the destination's frames, J); the canaries of both buffers and an out-of-place source are checked"""
    L = dwt.lifting
    src_h, dst_h = lay.fill(x), lay.fill(None if not in_place else x)
    if device:
        src = Dev(dwt, src_h)
        dst = src if in_place else Dev(dwt, dst_h)
        sp, dp = src.ptr + 16, dst.ptr + 16
    else:
        dst_h = src_h if in_place else dst_h
        sp, dp = src_h.ctypes.data + 16, dst_h.ctypes.data + 16
    bs, sx, sy = lay.strides
    J = L.lifting2d_batch(sl, inverse, sp, dp, bs, lay.batch, sx, sy, lay.W, lay.H, j_max)
    if device:
        src_h, dst_h = src.get(), dst.get()
    else:
        dwt.sync()
    assert lay.canaries_intact(dst_h) and lay.canaries_intact(src_h), "a word outside the frames was written"
    if not in_place:
        assert np.array_equal(src_h, lay.fill(x)), "the source of an out-of-place call changed"
    return lay.read(dst_h, x.dtype), J


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


# ---- against the model ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("W, H, B", SHAPES)
@pytest.mark.parametrize("name", SCHEMES)
def test_every_bit_is_the_models(dwt, name, W, H, B, fused):
    L = dwt.lifting
    s = model_scheme(name)
    sl = to_lib(L, s)
    dwt.set_option("lifting_fused", fused)
    assert L.route(sl) == (L.FUSED if fused and s.reach <= L.FUSED_REACH else L.STEPS)
    lay = Lay(B, W, H)
    for content in (("unit", "full") if s.type == lm.I32 else ("unit", "wide")):
        for j_max in (-1, 1):
            x, y, back, J = case(name, W, H, B, j_max, content)
            if s.type == lm.F32:
                assert np.isfinite(y).all() and np.isfinite(back).all()
            for in_place in (False, True):
                got, Jg = run(dwt, sl, False, x, j_max, lay, in_place)
                assert Jg == J and same(got, y), (content, j_max, in_place, "forward", int((bits(got) != bits(y)).sum()))
                got, Jg = run(dwt, sl, True, y, J, lay, in_place)
                assert Jg == J and same(got, back), (content, j_max, in_place, "inverse", int((bits(got) != bits(back)).sum()))
    dwt.set_option("lifting_fused", 1)


@pytest.mark.parametrize("W, H, B", [(66, 130, 1), (200, 136, 3)])
@pytest.mark.parametrize("name, wavelet", [("CDF97", "cdf97_s"), ("CDF53", "cdf53_s"), ("INTERP53", "interp53_s"), ("CDF53_INT", "cdf53_i"),
                                           ("CDF97_INT", "cdf97_i")])
def test_cdf_tables_give_the_specialised_kernels_bits(dwt, name, wavelet, W, H, B):
    """lifting2d_batch with a CDF table against dwt_hip_transform2d_batch of the wavelet, dense frames, forward and inverse"""
    L = dwt.lifting
    x, y, _, J = case(name, W, H, B, -1)
    sl = L.builtin(name)
    geom = (4 * W * H, B, 4 * W)
    for inverse, data in ((False, x), (True, y)):
        src = Dev(dwt, data)
        a, b = Dev(dwt, np.zeros_like(data)), Dev(dwt, np.zeros_like(data))
        assert L.lifting2d_batch(sl, inverse, src.ptr, a.ptr, *geom, 4, W, H, -1 if not inverse else J) == J
        assert dwt.transform2d_batch(wavelet, inverse, src.ptr, b.ptr, *geom, W, H, -1 if not inverse else J) == J
        assert same(a.get(), b.get()), (name, inverse)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", ["D4", "CDF97_INT"])
def test_host_and_strided_frames(dwt, name, fused):
    """host frames, and frames whose elements lie 8 bytes apart (host and device), on 33 x 47: the same bits"""
    L = dwt.lifting
    W, H, B = 33, 47, 2
    s = model_scheme(name)
    sl = to_lib(L, s)
    dwt.set_option("lifting_fused", fused)
    x, y, back, J = case(name, W, H, B, -1)
    for device, ex in ((False, 1), (False, 2), (True, 2)):
        lay = Lay(B, W, H, ex=ex)
        for in_place in (False, True):
            got, Jg = run(dwt, sl, False, x, -1, lay, in_place, device)
            assert Jg == J and same(got, y), (device, ex, in_place, "forward")
            got, Jg = run(dwt, sl, True, y, J, lay, in_place, device)
            assert Jg == J and same(got, back), (device, ex, in_place, "inverse")
    dwt.set_option("lifting_fused", 1)


# ---- launches, grid, errors -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["D4", "HAAR_INT"])
def test_fused_route_is_one_launch_per_level(dwt, name):
    """whatever the batch: J launches out of place, J + 1 in place (the copy the tiles read); a second identical call allocates
    nothing; no level: no launch in place, one copy out of place"""
    L = dwt.lifting
    sl = L.builtin(name)
    W, H = 200, 136
    dwt.set_option("lifting_fused", 1)
    assert L.route(sl) == L.FUSED
    for B in (1, 3):
        x, y, back, J = case(name, W, H, B, 4)
        assert J == 4
        src, dst = Dev(dwt, x), Dev(dwt, np.zeros_like(x))
        geom = (4 * W * H, B, 4 * W, 4, W, H)
        for inverse, data, want in ((False, x, y), (True, y, back)):
            def upload():
                assert dwt.lib.dwt_hip_memcpy_h2d(src.ptr, np.ascontiguousarray(data).ctypes.data, data.nbytes) == 0

            calls = (lambda: L.lifting2d_batch(sl, inverse, src.ptr, dst.ptr, *geom, 4), lambda: L.lifting2d_batch(sl, inverse, src.ptr, src.ptr, *geom, 4))
            upload()
            for f in calls:  # the first call of a size may grow the workspace
                f()
            dwt.sync()
            upload()
            allocs = dwt.get_option("stat_allocs")
            assert launches(dwt, calls[0]) == J
            assert same(dst.get(), want)
            assert launches(dwt, calls[1]) == J + 1
            assert same(src.get(), want)
            assert dwt.get_option("stat_allocs") == allocs
        assert launches(dwt, lambda: L.lifting2d_batch(sl, False, src.ptr, src.ptr, *geom, 0)) == 0
        assert launches(dwt, lambda: L.lifting2d_batch(sl, False, src.ptr, dst.ptr, *geom, 0)) == 1
        assert same(dst.get(), src.get())


@pytest.mark.parametrize("fused", [1, 0])
def test_a_batch_beyond_the_grid_is_refused_or_right(dwt, fused):
    """65536 frames of 2 x 2 (one more than grid.z takes): the model's bits, or an error that leaves dst untouched"""
    L = dwt.lifting
    dwt.set_option("lifting_fused", fused)
    s = model_scheme("D4")
    sl = L.builtin("D4")
    B = 65536
    x = np.random.default_rng(6).uniform(-1, 1, (B, 2, 2)).astype(np.float32)
    src, dst = Dev(dwt, x), Dev(dwt, np.full(x.shape, CANARY, np.uint32))
    try:
        J = L.lifting2d_batch(sl, False, src.ptr, dst.ptr, 16, B, 8, 4, 2, 2, -1)
    except dwt.DwtError as e:
        assert "frames" in str(e) and (dst.get() == CANARY).all()
    else:
        want, Jm = lm.fwd2d(s, x, -1)
        assert J == Jm and same(dst.get(shape=x.shape, dtype=np.float32), want)
    # the largest batch the entry takes
    B = L.MAX_BATCH
    want, Jm = lm.fwd2d(s, x[:B], -1)
    assert L.lifting2d_batch(sl, False, src.ptr, dst.ptr, 16, B, 8, 4, 2, 2, -1) == Jm
    assert same(dst.get(shape=x.shape, dtype=np.float32)[:B], want)
    dwt.set_option("lifting_fused", 1)


def test_refusals_leave_dst_untouched(dwt):
    L = dwt.lifting
    W, H, B = 24, 16, 2
    lay = Lay(B, W, H)
    x = case("D4", W, H, B, -1)[0]
    src, dst = Dev(dwt, lay.fill(x)), Dev(dwt, lay.fill())
    host = lay.fill(x)
    bs, sx, sy = lay.strides
    good = L.builtin("D4")

    def refused(word, scheme=good, s=src.ptr + 16, d=dst.ptr + 16, bstride=bs, batch=B, stride_x=sx, stride_y=sy, w=W, h=H):
        n0 = dwt.get_option("stat_launches")
        with pytest.raises(dwt.DwtError) as e:
            L.lifting2d_batch(scheme, False, s, d, bstride, batch, stride_x, stride_y, w, h, -1)
        assert word in str(e.value), str(e.value)
        assert dwt.get_option("stat_launches") == n0, "a refused call launched"
        assert np.array_equal(dst.get(), lay.fill()) and np.array_equal(src.get(), lay.fill(x)), "a refused call wrote"

    bad = L.builtin("D4")
    bad.steps[1].terms[0].off_a = 2
    refused("off_a", scheme=bad)
    bad = L.builtin("HAAR_INT")
    bad.inverse_cols_first = 0
    refused("inverse_cols_first", scheme=bad)
    refused("sizes", w=0)
    refused("sizes", h=-1)
    refused("frames", batch=0)
    refused("frames", batch=-3)
    refused("frames", batch=L.MAX_BATCH + 1)
    refused("strides", stride_y=2)
    refused("strides", stride_x=4 * W - 4)
    refused("apart", bstride=sx * (H - 1))
    refused("overlap", d=src.ptr + 16 + 8)
    refused("null", d=0)
    refused("both", s=host.ctypes.data + 16)
    refused("4 bytes", s=src.ptr + 18, d=dst.ptr + 18)
    # ... and the same call with nothing wrong runs
    assert L.lifting2d_batch(good, False, src.ptr + 16, dst.ptr + 16, bs, B, sx, sy, W, H, -1) == lm.levels(W, H, -1)
    assert same(lay.read(dst.get(), np.float32), case("D4", W, H, B, -1)[1])


# ---- stream, example ------------------------------------------------------------------------------------------------------

def test_entry_runs_on_the_callers_stream():
    """forward and inverse on both routes, in place and out of place, once on a non-blocking stream behind a bounded delay, in
    a process of its own (tests/lifting_stream.py, on the harness of tests/stream_cases.py): the model's bits; the calls on
    device memory queued without waiting for the stream"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lifting_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]


def test_example_custom_wavelet(dwt, tmp_path):
    """examples/custom_wavelet.c compiles with the gcc line of its header comment, runs and exits 0"""
    exe, libdir = tmp_path / "custom_wavelet", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "custom_wavelet.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PSNR" in out.stdout and "lossless" in out.stdout, out.stdout + out.stderr
