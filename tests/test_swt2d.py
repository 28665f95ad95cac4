"""CPU checks of the 2-D stationary wavelet transform: the numpy float32 restatement (tests/swt2d_model.py) against the
reference's two row functions run over the rows and then the columns (tests/golden/swt2d.npz, written by
scripts/gen_swt2d_golden.py), the conditions on the input kinds, the ABI of the built library and the argument checks."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import swt2d_model as m2
import swt_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(m2.GOLDEN)
F32 = np.float32


def test_manifest():
    with open(m2.MANIFEST) as f:
        info = json.load(f)["files"]["swt2d.npz"]
    with open(m2.GOLDEN, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == info["sha256"]
    assert [(c["seed"], c["wavelet"], c["kind"], c["size_y"], c["size_x"], c["levels"]) for c in info["cases"]] == m2.CASES
    assert os.path.getsize(m2.GOLDEN) < 1 << 20
    assert sorted(GOLD.files) == sorted(["%s_%d" % (n, i) for n in ("D", "LL") for i in range(len(m2.CASES))])


@pytest.mark.parametrize("i", range(len(m2.CASES)))
def test_restatement_equals_golden(i):
    seed, wavelet, kind, size_y, size_x, levels = m2.CASES[i]
    LL, D = m2.swt2d_levels(m2.make_input(seed, kind, size_y, size_x), wavelet, levels)
    assert GOLD["D_%d" % i].shape == (levels, 3, size_y, size_x) and GOLD["LL_%d" % i].shape == (size_y, size_x)
    assert sm.same(D, GOLD["D_%d" % i]) and sm.same(LL[-1], GOLD["LL_%d" % i])


@pytest.mark.parametrize("i", range(len(m2.CASES)))
def test_input_kind_conditions(i):
    """float_range: at most 10 % of the expected coefficients non-finite; tiny: at least half of them subnormal -- on the
    reference's own outputs"""
    seed, wavelet, kind, size_y, size_x, levels = m2.CASES[i]
    m2.check_kind(kind, GOLD["LL_%d" % i][None], GOLD["D_%d" % i])
    x = m2.make_input(seed, kind, size_y, size_x)
    if kind == "tiny":
        assert (np.abs(x) < m2.TINY).all() and (x == 0).mean() < 0.2
    if kind == "float_range":
        assert np.isfinite(x[4:]).all() and np.isfinite(x[:, 4:]).all() and not np.isfinite(x[:4, :4]).all()
        assert (np.abs(x[4:]) <= 1e38).all() and (np.abs(x[:, 4:]) <= 1e38).all()


def test_kinds_are_all_held():
    assert {c[2] for c in m2.CASES} == set(m2.KINDS) and {c[1] for c in m2.CASES} == set(sm.WAVELETS)


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_one_row_image(wavelet):
    """level 0 of a 1-row image: swt_model over the row, then the N = 1 column rule -- every tap of the column filter reads
    the one sample, summed from +0 in tap order"""
    row = sm.make_input(9, "float_range", 1, 40)[0]
    L, H = sm.swt_level(row, wavelet, 0)
    gl, gh = sm.FILTERS[wavelet]

    def column_of_one(v, g):
        y = np.zeros_like(v)
        with np.errstate(all="ignore"):
            for tap in g:
                y = (y + (v * tap).astype(F32)).astype(F32)
        return y

    LL, HL, LH, HH = m2.swt2d_level(row[None], wavelet, 0)
    assert sm.same(LL[0], column_of_one(L, gl)) and sm.same(LH[0], column_of_one(L, gh))
    assert sm.same(HL[0], column_of_one(H, gl)) and sm.same(HH[0], column_of_one(H, gh))


def test_model_is_separable_and_batched():
    """a stack of images gives each image's planes; a 1-column image is the row model down the column"""
    stack = np.stack([m2.make_input(3 + k, "normal", 12, 17) for k in range(3)])
    LL, D = m2.swt2d_levels(stack, "cdf97_s", 3)
    for k in range(3):
        LLk, Dk = m2.swt2d_levels(stack[k], "cdf97_s", 3)
        assert sm.same(LL[:, k], LLk) and sm.same(D[:, :, k], Dk)
    col = m2.make_input(8, "normal", 23, 1)
    assert m2.swt2d_level(col, "cdf53_s", 2)[0].shape == (23, 1)


def test_abi_exports():
    lib = C.CDLL(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so"))
    for s in ["dwt_hip_swt2d_batch", "dwt_hip_swt2d_level"]:
        assert hasattr(lib, s), s
    import libdwt_amd as dwt

    assert callable(dwt.swt2d_batch) and callable(dwt.swt2d_level)
    assert dwt.SWT2D_FUSED_LEVELS >= 5  # dilations 1 .. 16 at least
    hdr = open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()
    for name, v in (("FUSED_LEVELS", dwt.SWT2D_FUSED_LEVELS), ("TILE_W", dwt.SWT2D_TILE_W), ("TILE_H", dwt.SWT2D_TILE_H)):
        assert "#define DWT_HIP_SWT2D_%s %d" % (name, v) in hdr
    assert dwt.get_option("swt2d_fused") == 1


def test_argument_errors():
    """refused before any device is touched, and nothing is written"""
    import libdwt_amd as dwt

    w, h, levels, batch = 16, 6, 2, 2
    x = np.zeros((batch, h, w), F32)
    dh = np.full((batch, 3 * levels, h, w), 7, F32)
    dl = np.full((batch, levels, h, w), 7, F32)
    sx, plane = 4 * w, 4 * w * h
    bs, dbs = plane, plane * 3 * levels

    def call(wavelet="cdf97_s", src=x, bs=bs, batch=batch, sx=sx, sy=4, w=w, h=h, levels=levels, dst_h=dh, dst_l=dl, l_mode=2, dbs=dbs, ps=plane,
             dsx=sx):
        return lambda: dwt.swt2d_batch(wavelet, src, bs, batch, sx, sy, w, h, levels, dst_h, dst_l, l_mode, dbs, ps, dsx)

    bad = [
        call(wavelet="cdf53_i"), call(wavelet=7), call(levels=-1), call(levels=25), call(batch=0), call(w=0), call(h=0),
        call(dst_l=None), call(l_mode=3),
        call(dst_h=x), call(dst_l=x.ctypes.data + 8, l_mode=1), call(dst_l=dh.ctypes.data + plane, l_mode=1),  # overlaps
        call(ps=plane - 4), call(dbs=dbs - 4), call(bs=bs - 4), call(dsx=sx - 4), call(sx=sx - 4), call(sy=2),
        call(l_mode=2, dbs=plane * levels - 4, dst_h=dh[:1], batch=2),  # the LL stacks of two images collide
    ]
    for i, f in enumerate(bad):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    planes = [np.full((h, w), 7, F32) for _ in range(4)]
    bad_level = [
        lambda: dwt.swt2d_level("cdf53_d", x[0], sx, 4, w, h, 0, *planes, sx),
        lambda: dwt.swt2d_level("cdf97_s", x[0], sx, 4, w, h, 24, *planes, sx),
        lambda: dwt.swt2d_level("cdf97_s", x[0], sx, 4, w, h, -1, *planes, sx),
        lambda: dwt.swt2d_level("cdf97_s", x[0], sx, 4, 0, h, 0, *planes, sx),
        lambda: dwt.swt2d_level("cdf97_s", x[0], sx, 2, w, h, 0, *planes, sx),
        lambda: dwt.swt2d_level("cdf97_s", x[0], sx, 4, w, h, 0, *planes, sx - 4),
        lambda: dwt.swt2d_level("cdf97_s", x[0], sx, 4, w, h, 0, planes[0], planes[0], planes[2], planes[3], sx),
        lambda: dwt.swt2d_level("cdf97_s", x[0], sx, 4, w, h, 0, planes[0], planes[1], x[0], planes[3], sx),
    ]
    for i, f in enumerate(bad_level):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    # the same refusals at the C-ABI, which the Python checks above stand in front of
    lib = dwt.lib
    p = lambda a: a.ctypes.data  # noqa: E731
    assert lib.dwt_hip_swt2d_batch(1, p(x), bs, batch, sx, 4, w, h, levels, p(dh), p(dl), 2, dbs, plane, sx) != 0
    assert lib.dwt_hip_swt2d_batch(0, p(x), bs, batch, sx, 4, w, h, 25, p(dh), p(dl), 2, dbs, plane, sx) != 0
    assert lib.dwt_hip_swt2d_batch(0, p(x), bs, 0, sx, 4, w, h, levels, p(dh), p(dl), 2, dbs, plane, sx) != 0
    assert lib.dwt_hip_swt2d_batch(0, p(x), bs, batch, sx, 4, w, 0, levels, p(dh), p(dl), 2, dbs, plane, sx) != 0
    assert lib.dwt_hip_swt2d_batch(0, p(x), bs, batch, sx, 4, w, h, levels, p(dh), p(dl), 5, dbs, plane, sx) != 0
    assert lib.dwt_hip_swt2d_batch(0, p(x), bs, batch, sx, 4, w, h, levels, p(dh), None, 1, dbs, plane, sx) != 0
    assert lib.dwt_hip_swt2d_level(0, p(x), sx, 4, w, h, 24, *[p(a) for a in planes], sx, 4) != 0
    assert b"SWT" in lib.dwt_hip_last_error()
    assert lib.dwt_hip_swt2d_batch(0, p(x), bs, batch, sx, 4, w, h, 0, p(dh), None, 0, dbs, plane, sx) == 0  # 0 levels: nothing to do
    assert (dh == 7).all() and (dl == 7).all() and all((a == 7).all() for a in planes) and (x == 0).all()


def test_call_with_or_without_device():
    """without a device every call fails cleanly (DwtError, no abort); with one, a small host call gives the restatement"""
    import libdwt_amd as dwt

    w, h, levels = 20, 9, 2
    x = m2.make_input(5, "normal", h, w)
    dh = np.zeros((3 * levels, h, w), F32)
    dl = np.zeros((1, h, w), F32)
    planes = [np.zeros((h, w), F32) for _ in range(4)]
    calls = [
        lambda: dwt.swt2d_batch("cdf97_s", x, 4 * w * h, 1, 4 * w, 4, w, h, levels, dh, dl, 1, dh.nbytes, 4 * w * h, 4 * w),
        lambda: dwt.swt2d_level("cdf53_s", x, 4 * w, 4, w, h, 1, *planes, 4 * w),
    ]
    if dwt.lib.dwt_hip_init() != 0:
        for f in calls:
            with pytest.raises(dwt.DwtError) as e:
                f()
            assert "device" in str(e.value)
        return
    for f in calls:
        f()
    LL, D = m2.swt2d_levels(x, "cdf97_s", levels)
    assert sm.same(dh.reshape(levels, 3, h, w), D) and sm.same(dl[0], LL[-1])
    assert all(sm.same(a, b) for a, b in zip(planes, m2.swt2d_level(x, "cdf53_s", 1)))
