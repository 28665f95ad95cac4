"""CPU checks of the float CDF 9/7 on IEEE binary16 storage (DWT_HIP_CDF97_H): the model of
tests/f16_model.py against the golden file the compiled reference wrote (scripts/gen_h16_golden.py) and against the float
oracle, the host conversions dwt_util_float_to_half / dwt_util_half_to_float against numpy, the accuracy of the scheme,
its overflow rule, and the names the feature adds.

Accuracy bounds.  The issue that asked for the transform measured, with a prototype, forward max|model - float| / max|float
coefficient| <= 6.9e-4 and a round trip within 0.5 grey levels (PSNR >= 69.9 dB) on these inputs; the test asserts about
twice that -- 2^-9 and 1.0 grey level -- so that other seeds keep their margin.  Measured by this file's model: forward
<= 6.5e-4 of the largest coefficient, round trip <= 0.5 grey levels, PSNR >= 70.3 dB (printed by the test)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import f16_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same16(got, want):
    """binary16 arrays: identical bits wherever `want` is no NaN, NaNs at identical positions."""
    ng, nw = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(ng, nw) and np.array_equal(got.view(np.uint16)[~nw], want.view(np.uint16)[~nw])


def test_model_equals_the_golden_file():
    with open(os.path.join(ROOT, "tests", "golden", "cdf97_h_manifest.json")) as f:
        cases = json.load(f)["files"]["cdf97_h.npz"]["cases"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "cdf97_h.npz"))
    assert len(cases) >= 39
    for i, c in enumerate(cases):
        kw = dict(size_o=tuple(c["size_o"]), size_i=tuple(c["size_i"]), decompose_one=c["decompose_one"], zero_padding=c["zero_padding"])
        a = z["in_%d" % i].view(np.float16).copy()
        assert M.fwd2d(a, j_max=c["j_max"], **kw) == c["levels"]
        assert same16(a, z["fwd_%d" % i].view(np.float16)), ("forward", c)
        M.inv2d(a, j_max=c["levels"], **kw)
        assert same16(a, z["inv_%d" % i].view(np.float16)), ("inverse", c)


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (2, 2), (3, 5), (9, 14), (67, 131), (130, 67), (40, 1025)])
def test_unrounded_chain_is_the_multilevel_float_transform(shape):
    """The shapes and level counts the GPU tests use the model for, decompose_one and one-line directions included."""
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    x = rng.integers(0, 256, size=shape).astype(np.float32)
    for j_max in (-1, 0, 1, 2, 40):
        for d1 in (0, 1):
            M.assert_chain_is_multilevel(x, j_max=j_max, decompose_one=d1)


def test_unrounded_chain_on_sparse_frames():
    rng = np.random.default_rng(5)
    x = rng.random((40, 50), dtype=np.float32)
    for zp in (0, 1):
        assert M.assert_chain_is_multilevel(x, size_o=(50, 40), size_i=(37, 29), j_max=3, zero_padding=zp) == 3
    assert M.assert_chain_is_multilevel(x[:5], j_max=-1, decompose_one=1) == 6


# ---- the host conversions ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conv():
    import libdwt_amd as dwt

    I, P = C.c_int, C.c_void_p
    for n in ("dwt_util_float_to_half", "dwt_util_half_to_float"):
        getattr(dwt.lib, n).argtypes = [P, I, I, P, I, I, I, I]
        getattr(dwt.lib, n).restype = None

    def f2h(x):
        x = np.ascontiguousarray(x, np.float32).reshape(1, -1)
        out = np.zeros(x.shape, np.uint16)
        dwt.lib.dwt_util_float_to_half(out.ctypes.data, out.strides[0], 2, x.ctypes.data, x.strides[0], 4, x.shape[1], 1)
        return out.reshape(-1)

    def h2f(bits):
        bits = np.ascontiguousarray(bits, np.uint16).reshape(1, -1)
        out = np.zeros(bits.shape, np.float32)
        dwt.lib.dwt_util_half_to_float(out.ctypes.data, out.strides[0], 4, bits.ctypes.data, bits.strides[0], 2, bits.shape[1], 1)
        return out.reshape(-1)

    return dwt, f2h, h2f


def np_f2h(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)


def assert_f2h(f2h, x):
    x = np.asarray(x, np.float32)
    got, want = f2h(x).view(np.float16), np_f2h(x)
    assert same16(got, want), [(float(a), hex(b), hex(c)) for a, b, c in zip(x, got.view(np.uint16), want.view(np.uint16)) if b != c][:5]


def test_half_to_float_on_all_patterns(conv):
    _, _, h2f = conv
    bits = np.arange(65536, dtype=np.uint16)
    got, want = h2f(bits), bits.view(np.float16).astype(np.float32)
    assert M.same_bits(got, want)
    assert np.isnan(got).sum() == 2 * 1023


def test_float_to_half_random(conv):
    _, f2h, _ = conv
    rng = np.random.default_rng(16)
    assert_f2h(f2h, rng.standard_normal(100000).astype(np.float32) * 300)
    assert_f2h(f2h, rng.random(100000, dtype=np.float32))
    assert_f2h(f2h, (rng.random(100000, dtype=np.float32) - 0.5) * 1e-4)  # the subnormal halves and below
    assert_f2h(f2h, rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32).view(np.float32))  # any binary32 pattern


def test_float_to_half_ties_and_boundaries(conv):
    _, f2h, _ = conv
    # every tie between adjacent halves in a few binades (normal, around 1, the largest, subnormal), and its two float neighbours
    pts = []
    for lo in (0x0001, 0x03F0, 0x0400, 0x3BF0, 0x3C00, 0x5800, 0x7800, 0x7BF0):
        h = np.arange(lo, min(lo + 0x410, 0x7BFF), dtype=np.uint16).view(np.float16).astype(np.float64)
        up = np.arange(lo + 1, min(lo + 0x410, 0x7BFF) + 1, dtype=np.uint16).view(np.float16).astype(np.float64)
        tie = ((h + up) / 2).astype(np.float32)  # exact in binary32
        pts += [tie, np.nextafter(tie, np.float32(0)), np.nextafter(tie, np.float32(np.inf))]
    x = np.concatenate(pts)
    assert_f2h(f2h, x)
    assert_f2h(f2h, -x)
    # the subnormal boundary, the smallest subnormal and its tie with zero
    e = np.float32(2.0) ** np.arange(-30, -12, dtype=np.float32)
    x = np.concatenate([e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1)), e * np.float32(1.5), e * np.float32(0.75)])
    assert_f2h(f2h, x)
    assert_f2h(f2h, -x)
    # the overflow boundary: 65504 is the largest half, 65520 the tie that rounds to Inf
    x = np.array([65504, 65519.99, 65520, np.nextafter(np.float32(65520), np.float32(0)), 65536, 1e38, 3.4e38], np.float32)
    assert list(f2h(x)) == [0x7BFF, 0x7BFF, 0x7C00, 0x7BFF, 0x7C00, 0x7C00, 0x7C00]
    assert_f2h(f2h, x)
    assert_f2h(f2h, -x)
    # +-0, +-Inf, NaN, float subnormals
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 1e-40], np.float32)
    got = f2h(x)
    assert list(got[:4]) == [0x0000, 0x8000, 0x7C00, 0xFC00] and list(got[6:]) == [0x0000, 0x8000, 0x0000]
    assert np.isnan(got[4:6].view(np.float16)).all()
    snan = np.array([0x7F800001, 0xFF800001, 0x7FC00000, 0x7FFFFFFF], np.uint32).view(np.float32)  # payloads that vanish when shifted
    assert np.isnan(f2h(snan).view(np.float16)).all()


def test_conversions_on_strided_frames(conv):
    """A channel of an interleaved image on either side, padded pitches: only the frame's elements are written."""
    dwt, _, _ = conv
    rng = np.random.default_rng(7)
    h, w = 13, 29
    src = (rng.standard_normal((h, w + 3, 3)) * 100).astype(np.float32)
    dst = np.full((h, w + 5, 2), 0x5AA5, np.uint16)
    dwt.lib.dwt_util_float_to_half(dst.ctypes.data + 2, dst.strides[0], dst.strides[1], src.ctypes.data + 8, src.strides[0], src.strides[1], w, h)
    assert same16(np.ascontiguousarray(dst[:, :w, 1]).view(np.float16), np_f2h(src[:, :w, 2]))
    assert (dst[:, :, 0] == 0x5AA5).all() and (dst[:, w:, :] == 0x5AA5).all()
    back = np.full((h, w + 1, 3), -7.0, np.float32)
    dwt.lib.dwt_util_half_to_float(back.ctypes.data + 4, back.strides[0], back.strides[1], dst.ctypes.data + 2, dst.strides[0], dst.strides[1], w, h)
    assert np.array_equal(back[:, :w, 1], np.ascontiguousarray(dst[:, :w, 1]).view(np.float16).astype(np.float32))
    assert (back[:, :, 0] == -7.0).all() and (back[:, :, 2] == -7.0).all() and (back[:, w:, :] == -7.0).all()


# ---- accuracy of the scheme (the model alone, against the float oracle) ---------------------------------------------------
def accuracy_images():
    rng = np.random.default_rng(97)
    yy, xx = np.mgrid[0:256, 0:256]
    return {"random 256 x 256": rng.integers(0, 256, size=(256, 256)).astype(np.float32),
            "sin cos 256 x 256": np.round(127.5 + 127.5 * np.sin(xx / 17.0) * np.cos(yy / 29.0)).astype(np.float32),
            "random 131 x 67": rng.integers(0, 256, size=(131, 67)).astype(np.float32)}


def test_accuracy_against_the_float_transform():
    worst_f, worst_rt, worst_psnr = 0.0, 0.0, np.inf
    for name, img in accuracy_images().items():
        assert img.min() >= 0 and img.max() <= 255
        for J in (1, 3, 5):
            a = img.astype(np.float16)
            assert np.array_equal(a.astype(np.float32), img)  # 8-bit data is exact in binary16
            assert M.fwd2d(a, j_max=J) == J
            f = img.copy()
            M.oracle().fwd("cdf97_2f_s", f, J)
            fwd_err = float(np.abs(a.astype(np.float64) - f).max() / np.abs(f).max())
            M.inv2d(a, j_max=J)
            diff = a.astype(np.float64) - img
            rt = float(np.abs(diff).max())
            psnr = float(10 * np.log10(255.0 ** 2 / np.mean(diff ** 2))) if diff.any() else np.inf
            print("%s J=%d: forward %.3g of the largest coefficient, round trip %.3g grey levels, PSNR %.1f dB" % (name, J, fwd_err, rt, psnr))
            worst_f, worst_rt, worst_psnr = max(worst_f, fwd_err), max(worst_rt, rt), min(worst_psnr, psnr)
            assert fwd_err <= 2.0 ** -9, (name, J, fwd_err)
            assert rt <= 1.0, (name, J, rt)
    print("worst: forward %.3g, round trip %.3g grey levels, PSNR %.1f dB" % (worst_f, worst_rt, worst_psnr))


def test_overflow_rule():
    """A level doubles the gain of the LL band: 12-bit data is finite at 3 levels and holds Inf at 5."""
    rng = np.random.default_rng(12)
    img = rng.integers(0, 4096, size=(64, 64)).astype(np.float16)
    a = img.copy()
    M.fwd2d(a, j_max=3)
    assert np.isfinite(a).all()
    a = img.copy()
    M.fwd2d(a, j_max=5)
    assert np.isinf(a).any()


# ---- the names the feature adds -------------------------------------------------------------------------------------------
def test_public_names():
    import libdwt_amd as dwt

    assert "DWT_HIP_CDF97_H = 9" in open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "libdwt.h")).read()
    for name in ("dwt_cdf97_2f_h", "dwt_cdf97_2i_h", "dwt_util_float_to_half", "dwt_util_half_to_float"):
        assert name + "(" in hdr and hasattr(dwt.lib, name), name
    assert dwt.CDF97_H == 9 and dwt.WAVELET_ID["cdf97_h"] == 9
    assert dwt.FORWARD["cdf97_h"] is dwt.dwt_cdf97_2f_h and dwt.INVERSE["cdf97_h"] is dwt.dwt_cdf97_2i_h
