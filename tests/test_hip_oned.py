"""GPU parity of the 1-D transforms (dwt_cdf{97,53}_1f_s / _1i_s / _2f1_s, dwt_hip_transform1d*): bit for bit against
the compiled reference where it was built, otherwise against the restatement of tests/test_oned.py (which the CPU suite
pins to the reference).  Host and device pointers, element strides, sparse frames, the whole float range, the one-launch
fusion of dense lines and the torch entry."""
import ctypes as C
import warnings
import zlib

import numpy as np
import pytest

from conftest import full_range_floats, same_floats
from hipdev import Dev
from oraclelib import Oracle, Reference, have_reference
from test_oned import J_CASES, ceil_log2, ref_call, ref_lib, restated

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

N1D_MAX = 8192  # dwt_kernels.h
WAVELETS = ["cdf97", "cdf53"]
WID = {"cdf97": 0, "cdf53": 2}  # DWT_HIP_CDF97_S, DWT_HIP_CDF53_S


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("generic", 0)
    d.dwt_util_set_accel(0)
    d.dwt_util_finish()


@pytest.fixture(scope="module")
def expect():
    """expect(wv, inverse, line, so, si, j_max, zp) -> (expected line, j): the reference's call on a copy of the
    dense float32 line, or the restatement where the reference is not built."""
    if have_reference():
        L = ref_lib(Reference())

        def f(wv, inverse, a, so, si=None, j_max=-1, zp=0):
            b = np.ascontiguousarray(a, np.float32).copy()
            return b, ref_call(L, wv, inverse, b, so, si, j_max, zp)
    else:
        orc = Oracle()

        def f(wv, inverse, a, so, si=None, j_max=-1, zp=0):
            b = np.ascontiguousarray(a, np.float32).copy()
            return b, restated(orc, wv, inverse, b, so, si, j_max, zp)
    return f


def t1d(dwt, wv, inverse, ptr, stride, so, si, j, zp=0):
    jj = C.c_int(j)
    rc = dwt.lib.dwt_hip_transform1d(WID[wv], inverse, ptr, ptr, stride, so, si, C.byref(jj), zp)
    assert rc == 0, dwt.last_error()
    return jj.value


def entry(dwt, wv, inverse):
    return getattr(dwt, "dwt_%s_%s_s" % (wv, "1i" if inverse else "1f"))


def bits_equal(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000, 4095, 4096, 4097,
           N1D_MAX - 1, N1D_MAX, N1D_MAX + 1, 3 * N1D_MAX + 5, (1 << 20) + 3]


@pytest.mark.parametrize("wv", WAVELETS)
@pytest.mark.parametrize("inverse", [0, 1], ids=["fwd", "inv"])
def test_lengths_and_level_clamps(dwt, expect, wv, inverse):
    """Every length class (short, end cases, the cap and beyond it) and every j_max clamp case, host and device."""
    rng = np.random.default_rng(100 + inverse)
    for n in LENGTHS:
        for j in (J_CASES if n <= 4 * N1D_MAX else [-1, 2, 99]):
            a = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
            want, jw = expect(wv, inverse, a, n, n, j)
            got = a.copy()
            jg = entry(dwt, wv, inverse)(got, 4, n, n, j)
            assert jg == jw and bits_equal(got, want), ("host", wv, inverse, n, j)
            d = Dev(dwt, a)
            jg = t1d(dwt, wv, inverse, d.ptr, 4, n, n, j)
            got = d.get()
            d.free()
            assert jg == jw and bits_equal(got, want), ("device", wv, inverse, n, j)


@pytest.mark.parametrize("wv", WAVELETS)
@pytest.mark.parametrize("es", [4, 8, 12])
def test_element_strides(dwt, expect, wv, es):
    """One channel of interleaved data (elements es bytes apart), host and device: the other channels stay as they were."""
    rng = np.random.default_rng(es)
    ch = es // 4
    for n in (5, 64, 1001, N1D_MAX + 3):
        for inverse in (0, 1):
            buf = rng.random((n, ch), dtype=np.float32)
            c = ch - 1
            want_line, jw = expect(wv, inverse, buf[:, c], n, n, -1)
            want = buf.copy()
            want[:, c] = want_line
            got = buf.copy()
            base = got.ctypes.data + 4 * c
            jg = entry(dwt, wv, inverse)(base, es, n, n, -1)
            assert jg == jw and bits_equal(got, want), ("host", es, n, inverse)
            d = Dev(dwt, buf)
            jg = t1d(dwt, wv, inverse, d.ptr + 4 * c, es, n, n, -1)
            got = d.get()
            d.free()
            assert jg == jw and bits_equal(got, want), ("device", es, n, inverse)


@pytest.mark.parametrize("wv", WAVELETS)
@pytest.mark.parametrize("zp", [0, 1])
def test_sparse_frames(dwt, expect, wv, zp):
    """size_o > size_i: the reference's level loop with its zero fills, host and device."""
    rng = np.random.default_rng(7 + zp)
    for so, si in ((9, 5), (33, 1), (64, 0), (100, 61), (4097, 3000), (N1D_MAX + 9, N1D_MAX - 2)):
        for inverse in (0, 1):
            for j in (-1, 0, 2):
                a = (rng.random(so, dtype=np.float32) - 0.5).astype(np.float32)
                want, jw = expect(wv, inverse, a, so, si, j, zp)
                got = a.copy()
                jg = entry(dwt, wv, inverse)(got, 4, so, si, j, zp)
                assert jg == jw and bits_equal(got, want), ("host", so, si, inverse, j)
                d = Dev(dwt, a)
                jg = t1d(dwt, wv, inverse, d.ptr, 4, so, si, j, zp)
                got = d.get()
                d.free()
                assert jg == jw and bits_equal(got, want), ("device", so, si, inverse, j)


@pytest.mark.parametrize("wv", WAVELETS)
def test_series_padded_matrix(dwt, expect, wv):
    """_2f1_s on a matrix with padded rows (sentinel in the padding), odd row length, fewer inner rows than outer:
    rows below the inner height and the padding untouched, *j_max_ptr as the reference leaves it."""
    rng = np.random.default_rng(21)
    fn = getattr(dwt, "dwt_%s_2f1_s" % wv)
    for h, w, pitch, hi in ((9, 37, 45, 6), (5, 1023, 1030, 5), (3, 10001, 10004, 2)):
        m = np.full((h, pitch), -3.5, np.float32)
        m[:, :w] = rng.random((h, w), dtype=np.float32)
        want = m.copy()
        jw = -1
        for y in range(hi):
            want[y, :w], jw = expect(wv, 0, m[y, :w], w, w, -1)
        for j in (-1, 99):
            got = m.copy()
            assert fn(got, pitch * 4, 4, w, h, w, hi, j) == jw == ceil_log2(w)
            assert bits_equal(got, want), (h, w, pitch, hi, "host")
            d = Dev(dwt, m)
            assert fn(d.ptr, pitch * 4, 4, w, h, w, hi, j) == jw
            got = d.get()
            d.free()
            assert bits_equal(got, want), (h, w, pitch, hi, "device")
    got = m.copy()
    assert fn(got, 45 * 4, 4, 37, 9, 37, 0, -7) == -7  # no rows: untouched, j too
    assert bits_equal(got, m)


def test_series_large_device_matrix(dwt, expect):
    """A 4096 x 4096 device-resident matrix against per-row reference calls (one launch for all rows)."""
    rng = np.random.default_rng(9)
    m = rng.random((4096, 4096), dtype=np.float32)
    want = np.empty_like(m)
    for y in range(4096):
        want[y], jw = expect("cdf97", 0, m[y], 4096, 4096, -1)
    d = Dev(dwt, m)
    n0 = dwt.get_option("stat_launches")
    assert dwt.dwt_cdf97_2f1_s(d.ptr, 4096 * 4, 4, 4096, 4096, 4096, 4096, -1) == jw == 12
    assert dwt.get_option("stat_launches") - n0 == 1
    got = d.get()
    d.free()
    assert bits_equal(got, want)


@pytest.mark.parametrize("wv", WAVELETS)
@pytest.mark.parametrize("klass", ["subnormal", "tiny", "huge", "mixed"])
@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "nonfinite"])
def test_float_range(dwt, expect, wv, klass, nonfinite):
    """+-0, subnormals, +-Inf, NaN and near-overflow samples (the line ends included, where the reference writes
    (2c)*x): forward and inverse as batches of device rows and as host lines, compared as test_hip_float_range does."""
    rng = np.random.default_rng(zlib.crc32(("%s %s %d" % (wv, klass, nonfinite)).encode()))
    for n in (2, 3, 4, 5, 17, 64, 257, N1D_MAX + 5):
        rows = full_range_floats(rng, (6, n), np.float32, klass, nonfinite)
        for inverse in (0, 1):
            want = np.empty_like(rows)
            for y in range(rows.shape[0]):
                want[y], _ = expect(wv, inverse, rows[y], n, n, -1)
            d = Dev(dwt, rows)
            jj = C.c_int(-1)
            assert dwt.lib.dwt_hip_transform1d_batch(WID[wv], inverse, d.ptr, d.ptr, n * 4, 4, rows.shape[0], n, n,
                                                     C.byref(jj), 0) == 0, dwt.last_error()
            got = d.get()
            d.free()
            assert same_floats(got, want), (klass, n, inverse, "device batch")
            got = rows[2].copy()
            entry(dwt, wv, inverse)(got, 4, n, n, -1)
            assert same_floats(got, want[2]), (klass, n, inverse, "host")


@pytest.mark.parametrize("wv", WAVELETS)
@pytest.mark.parametrize("inverse", [0, 1], ids=["fwd", "inv"])
def test_dense_batch_is_one_launch(dwt, expect, wv, inverse):
    """A device batch of dense lines up to N1D_MAX is one kernel launch at any depth; "generic" (the per-level line
    passes) gives the same bits."""
    rng = np.random.default_rng(31)
    for n_lines, n in ((300, 256), (7, 4095), (3, N1D_MAX)):
        a = rng.random((n_lines, n), dtype=np.float32)
        for j in (1, -1):
            want = np.empty_like(a)
            for y in range(n_lines):
                want[y], jw = expect(wv, inverse, a[y], n, n, j)
            outs = []
            for generic in (0, 1):
                dwt.set_option("generic", generic)
                d = Dev(dwt, a)
                n0 = dwt.get_option("stat_launches")
                jj = C.c_int(j)
                rc = dwt.lib.dwt_hip_transform1d_batch(WID[wv], inverse, d.ptr, d.ptr, n * 4, 4, n_lines, n, n, C.byref(jj), 0)
                launches = dwt.get_option("stat_launches") - n0
                dwt.set_option("generic", 0)
                assert rc == 0, dwt.last_error()
                if not generic:
                    assert launches == 1, (n_lines, n, j)
                outs.append(d.get())
                d.free()
            assert bits_equal(outs[0], want) and bits_equal(outs[1], want), (n_lines, n, j)


TORCH_SCRIPT = r"""
import sys, numpy as np
import torch                      # first: this process then shares torch's HIP runtime
sys.path.insert(0, ROOT)
import libdwt_amd as dwt
dwt.dwt_util_init()
a = np.load(PATH + "/in.npy")
n_lines, n = a.shape
for wv in ("cdf97_s", "cdf53_s"):
    x = torch.from_numpy(a.copy()).cuda()
    torch.cuda.synchronize()
    j = dwt.transform1d_batch(wv, 0, x, x, n * 4, n_lines, n)
    dwt.sync()
    np.save(PATH + "/%s_fwd.npy" % wv, x.cpu().numpy())
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    assert dwt.transform1d_batch(wv, 1, x, y, n * 4, n_lines, n, j_max=j) == j
    dwt.sync()
    np.save(PATH + "/%s_inv.npy" % wv, y.cpu().numpy())
    print(wv, j)
print("torch OK")
"""


def test_torch_round_trip(expect, tmp_path):
    """transform1d_batch forward then inverse (out of place) on cuda tensors equals the reference composition.  Own
    process: torch before the library, so that both use one HIP runtime."""
    import os
    import subprocess
    import sys

    pytest.importorskip("torch")
    rng = np.random.default_rng(41)
    a = rng.random((64, 1000), dtype=np.float32)
    np.save(tmp_path / "in.npy", a)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\nPATH = %r\n" % (root, str(tmp_path)) + TORCH_SCRIPT],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "torch OK" in out.stdout, out.stderr[-2000:]
    for wv in WAVELETS:
        assert "%s_s %d" % (wv, ceil_log2(1000)) in out.stdout
        want = np.empty_like(a)
        for y in range(64):
            want[y], _ = expect(wv, 0, a[y], 1000, 1000, -1)
        assert bits_equal(np.load(tmp_path / ("%s_s_fwd.npy" % wv)), want)
        for y in range(64):
            want[y], _ = expect(wv, 1, want[y], 1000, 1000, -1)
        assert bits_equal(np.load(tmp_path / ("%s_s_inv.npy" % wv)), want)
