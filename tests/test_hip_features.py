"""GPU checks of the per-subband feature statistics (dwt_hip_features2d / _2d_batch / _1d_batch, the libdwt.h entries,
dwt_hip_abs) against the compiled reference where it is built, else the sequential-float32 restatement, and against
the float64 model of tests/features_model.py.  The bounds are derived, none is tuned to output."""
import math

import numpy as np
import pytest

import features_model as fm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
ALL = list(fm.NAMES)
COMPARED = {"pairs": 0, "ran": 0}


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("feat_groups", 0)


def reference(img, sox, soy, six, siy, j_max, p):
    if fm.RefFeatures.available():
        return fm.RefFeatures().features(img, sox, soy, six, siy, j_max, p)
    return fm.seq32(img, sox, soy, six, siy, j_max, p)


def run(dwt, names, imgs, six, siy, j_max, p, how, device):
    """features of a stack of equal images (batch, h, w) -> array (batch, len(names), count), names in enum order"""
    names = [n for n in fm.NAMES if n in names]
    batch, h, w = imgs.shape
    nb = fm.count_subbands(w, h, six, siy, j_max)
    block = len(names) * nb
    fv = np.full((batch, max(block, 1)), np.nan, F32)
    src = Dev(dwt, imgs) if device else None
    dfv = Dev(dwt, fv) if device else None
    ip, fp = (src.ptr, dfv.ptr) if device else (imgs.ctypes.data, fv.ctypes.data)
    if how == "single":
        assert (six, siy) != (None, None)
        for b in range(batch):
            dwt.features2d(names, ip + b * h * w * 4, w * 4, 4, w, h, six, siy, j_max, fp + b * fv.shape[1] * 4, p)
    elif how == "batch2d":
        assert (six, siy) == (w, h)
        dwt.features2d_batch(names, ip, h * w * 4, batch, w * 4, w, h, j_max, fp, fv.shape[1], p)
    else:
        assert h == 1 and six == w
        dwt.features1d_batch(names, ip, w * 4, 4, batch, w, j_max, fp, fv.shape[1], p)
    if device:
        fv = dfv.get(fv.shape)
        src.free()
        dfv.free()
    return fv[:, :block].reshape(batch, len(names), nb), names


def balanced(rng, w, h, six, siy, j_max):
    """values of {-3 .. 3} with every band summing to exactly 0 (pairs x, -x, shuffled); one band all zero"""
    img = rng.integers(-3, 4, (h, w)).astype(F32)
    for k, (x0, y0, bw, bh, _) in enumerate(fm.bands(w, h, six, siy, j_max)):
        n = bw * bh
        assert n <= 1 << 17
        half = rng.integers(-3, 4, n // 2).astype(F32)
        v = np.concatenate([half, -half, np.zeros(n % 2, F32)])
        if k == 1:
            v[:] = 0
        img[y0:y0 + bh, x0:x0 + bw] = rng.permutation(v).reshape(bh, bw)
    return img


HOWS = [("single", False), ("single", True), ("batch2d", False), ("batch2d", True)]
# (w, h, j_max): rows for the line kernel, a longer row and images for the slab kernels
EXACT_SHAPES = [(4096, 1, 13), (64, 64, 5), (512, 512, 4), (37, 53, 4), (20000, 1, 6), (8192, 1, 4)]


def equal_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


@pytest.mark.parametrize("shape", EXACT_SHAPES)
@pytest.mark.parametrize("p", [1.0, 2.0])
def test_exact_class_bit_identical(dwt, shape, p):
    w, h, j_max = shape
    rng = np.random.default_rng(w * 31 + h)
    imgs = np.stack([balanced(rng, w, h, w, h, j_max) for _ in range(2)])
    nb = fm.count_subbands(w, h, w, h, j_max)
    want = [reference(im, w, h, w, h, j_max, p) for im in imgs]
    assert any(np.isnan(q["skew"]).any() for q in want)  # the all-zero band: 0/0 in the reference too
    hows = HOWS + ([("lines", False), ("lines", True)] if h == 1 else [])
    for how, device in hows:
        got, names = run(dwt, ALL, imgs, w, h, j_max, p, how, device)
        for b in range(2):
            for i, n in enumerate(names):
                ok = np.array_equal(got[b, i], want[b][n]) if n == "med" else equal_bits(got[b, i], want[b][n])
                assert ok, (how, device, n, got[b, i], want[b][n])
        COMPARED["pairs"] += 2 * nb * len(ALL)
    COMPARED["ran"] += 1


def general(rng, w, h, kind):
    a = rng.standard_normal((h, w)).astype(F32) if kind == "normal" else rng.uniform(-1, 1, (h, w)).astype(F32)
    m = rng.random((h, w))
    a[m < 0.05] = F32(0.0)
    a[m > 0.95] = F32(-0.0)
    a[(m > 0.4) & (m < 0.45)] = F32(0.75)  # ties
    a[(m > 0.5) & (m < 0.55)] = F32(-0.75)
    return a


ORDER_SHAPES = [(5, 3, 5, "normal"), (6, 4, 4, "uniform"), (7, 1, 4, "normal"), (101, 77, 5, "uniform"), (8192, 1, 13, "normal"),
                (30000, 1, 8, "uniform"), (2048, 2048, 3, "normal")]


@pytest.mark.parametrize("shape", ORDER_SHAPES)
def test_order_statistics_exact(dwt, shape):
    w, h, j_max, kind = shape
    rng = np.random.default_rng(w + 7 * h)
    imgs = general(rng, w, h, kind)[None]
    names = ["maxidx", "med", "maxnorm"]
    bs = fm.bands(w, h, w, h, j_max)
    want = {n: np.array([fm.order_stats(fm.band_values(imgs[0], b))[n] for b in bs], F32) for n in names}
    if fm.RefFeatures.available():
        ref = fm.RefFeatures().features(imgs[0], w, h, w, h, j_max, 2.0)
        for n in names:
            assert np.array_equal(ref[n], want[n]), n
    for how, device in HOWS + ([("lines", True), ("lines", False)] if h == 1 else []):
        got, order = run(dwt, names, imgs, w, h, j_max, 2.0, how, device)
        for i, n in enumerate(order):
            ok = np.array_equal(got[0, i], want[n]) if n == "med" else equal_bits(got[0, i], want[n])
            assert ok, (how, device, n, got[0, i], want[n])
        COMPARED["pairs"] += len(bs) * 3
    COMPARED["ran"] += 1


SUM_OF = {"wps": ["S2"], "mean": ["S1"], "var": ["M2"], "stdev": ["M2"], "skew": ["M2", "M3"], "kurt": ["M2", "M4"], "lpnorm": ["Sp"], "norm": ["S2"]}
PLANES = ["S1", "S2", "Sp", "M2", "M3", "M4"]  # dwt_hip_features_raw_sums
SUM_SHAPES = [(4096, 1, 13, "normal", 1.5), (8192, 1, 5, "uniform", 3.0), (300, 200, 4, "normal", 1.0), (20000, 1, 5, "normal", 2.5),
              (1024, 1024, 3, "uniform", 2.5)]
U = 2.0 ** -24


def guard_model_with_reference(img, w, h, j_max, p, bs):
    """The float64 model against the reference's own error bound, per sum the reference lets us recover: S2 = wps * 2^j
    (exact), S1 = mean * n and M2 = var * n (about the REFERENCE's float mean, which `mean` is).  With u = 2^-24: each
    float term is within u |t| of the model's (x*x, d*d rounded; glibc's powf may add another u |t|: 2 u T in all), the
    sequential float sum of n terms adds (n-1) u T (Higham), and undoing the final float division costs one rounding of
    the quotient and one of the product, 2 u |S|.  Hence |S_ref - S_64| <= (n + 2) u T + 2 u |S|, to first order."""
    if fm.RefFeatures.available():
        ref, who = fm.RefFeatures().features(img, w, h, w, h, j_max, p), "reference"
    elif w * h <= 1 << 16:
        ref, who = fm.seq32(img, w, h, w, h, j_max, p), "restatement"
    else:
        print("guard of the model: no reference built here and %d x %d is too large for the restatement -- NOT run" % (w, h))
        return
    for k, b in enumerate(bs):
        n = b[2] * b[3]
        m = fm.model64_band(fm.band_values(img, b), p, mean=ref["mean"][k])
        for name, s_ref in (("S2", float(ref["wps"][k]) * (1 << b[4])), ("S1", float(ref["mean"][k]) * n), ("M2", float(ref["var"][k]) * n)):
            s, t, _ = m[name]
            assert abs(s_ref - s) <= (n + 2) * U * t + 2 * U * abs(s_ref), (who, "vs model", name, k, s_ref, s)


@pytest.mark.parametrize("shape", SUM_SHAPES)
def test_sums_against_float64_model(dwt, shape):
    """Every raw device sum S (dwt_hip_features_raw_sums) satisfies |S_gpu - S_64| <= 2^-24 |S_64| + n 2^-53 T against the
    float64 model; the central sums are modelled about the device's own float mean, which must be the float quotient of
    its S1.  Every finished feature equals the host finalisation (features_model.finish) of the device's own sums."""
    w, h, j_max, kind, p = shape
    rng = np.random.default_rng(3 * w + h)
    img = general(rng, w, h, kind)
    bs = fm.bands(w, h, w, h, j_max)
    names = [n for n in fm.NAMES if n in SUM_OF]
    vals = [fm.band_values(img, b) for b in bs]
    guard_model_with_reference(img, w, h, j_max, p, bs)
    for how, device in [("single", True), ("batch2d", True), ("single", False), ("batch2d", False)] + ([("lines", True), ("lines", False)] if h == 1 else []):
        got, order = run(dwt, names, img[None], w, h, j_max, p, how, device)
        raw = {q: dwt.features_raw_sums(i, len(bs)) for i, q in enumerate(PLANES)}
        for k, b in enumerate(bs):
            size, j = b[2] * b[3], b[4]
            mean_dev = F32(F32(raw["S1"][k]) / F32(size))
            m = fm.model64_band(vals[k], p, mean=mean_dev)
            for q in PLANES:
                s, t, n = m[q]
                err, bound = abs(raw[q][k] - s), U * abs(s) + n * 2.0 ** -53 * t
                print("%s %s band %d %s: |S_gpu - S_64| = %.3e, bound %.3e" % (how, "dev" if device else "host", k, q, err, bound))
                assert err <= bound, (how, device, q, k, raw[q][k], s)
            sums = {q: F32(raw[q][k]) for q in PLANES}
            for i, name in enumerate(order):
                want = np.asarray(fm.finish(name, sums, size, j, p), F32)
                assert equal_bits(got[0, i, k], want), (how, device, name, k, got[0, i, k], want)
        COMPARED["pairs"] += len(bs) * len(names)
    COMPARED["ran"] += 1


def test_reproducible_across_runs_and_geometries(dwt):
    rng = np.random.default_rng(5)
    imgs = np.stack([general(rng, 700, 500, "normal") for _ in range(3)])
    outs = []
    for groups in (0, 0, 7, 1000):
        dwt.set_option("feat_groups", groups)
        outs.append(run(dwt, ALL, imgs, 700, 500, 5, 1.7, "batch2d", True)[0])
    dwt.set_option("feat_groups", 0)
    for o in outs[1:]:
        assert equal_bits(o, outs[0])
    row = general(rng, 4096, 1, "uniform")[None]
    a = run(dwt, ALL, row, 4096, 1, 12, 1.7, "lines", True)[0]
    assert equal_bits(a, run(dwt, ALL, row, 4096, 1, 12, 1.7, "lines", True)[0])
    assert equal_bits(a, run(dwt, ALL, row, 4096, 1, 12, 1.7, "single", True)[0])  # dwt_util_*_s on a row == the batch call


def test_launch_counts(dwt):
    rows = np.zeros((16, 1, 8192), F32)
    src, fv = Dev(dwt, rows), Dev(dwt, np.zeros(16 * 11 * 16, F32))
    for names in (["wps"], ALL, ["med", "kurt"]):
        assert launches(dwt, lambda: dwt.features1d_batch(names, src.ptr, 8192 * 4, 4, 16, 8192, 13, fv.ptr, 11 * 16, 1.5)) == 1
    src.free()
    imgs = np.zeros((64, 128, 128), F32)
    src = Dev(dwt, imgs)
    big = Dev(dwt, np.zeros(64 * 11 * 16, F32))

    def count(names, batch):
        return launches(dwt, lambda: dwt.features2d_batch(names, src.ptr, 128 * 128 * 4, batch, 128 * 4, 128, 128, 5, big.ptr, 11 * 16, 1.5))

    for names in (["wps"], ["wps", "var"], ["med"], ALL):
        assert count(names, 1) == count(names, 64)
    assert count(["wps", "mean", "maxnorm", "lpnorm"], 8) == 2  # pass 1 and its fold: no pass 2, no select
    assert count(["var"], 8) == 4 and count(["med"], 8) == 2 + 8 and count(ALL, 8) == 4 + 8
    for d in (src, fv, big):
        d.free()


def test_refusals(dwt):
    a = np.zeros((16, 16), F32)
    fv = np.zeros(64, F32)
    d, dfv = Dev(dwt, a), Dev(dwt, fv)
    bad = [
        lambda: dwt.features2d("wps", a, 64, 4, 16, 16, 17, 16, 3, fv),
        lambda: dwt.features2d("wps", a, 64, 4, 16, -1, 16, -1, 3, fv),
        lambda: dwt.features2d("wps", d.ptr, 64, 6, 8, 16, 8, 16, 3, dfv.ptr),
        lambda: dwt.features2d("lpnorm", a, 64, 4, 16, 16, 16, 16, 3, fv, 0.0),
        lambda: dwt.features2d("lpnorm", a, 64, 4, 16, 16, 16, 16, 3, fv, -1.0),
        lambda: dwt.features2d("wps", a, 64, 4, 16, 16, 16, 16, 3, 0),
        lambda: dwt.features2d("wps", d.ptr, 64, 4, 16, 16, 16, 16, 3, fv),
        lambda: dwt.features2d("wps", a, 64, 4, 16, 16, 16, 16, 3, dfv.ptr),
        lambda: dwt.features2d_batch("wps", d.ptr, 1024, 1, 64, 16, 16, 3, fv, 64),
        lambda: dwt.features1d_batch("wps", a, 64, 4, 16, 16, 3, dfv.ptr, 4),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    d.free()
    dfv.free()


def test_abs(dwt):
    rng = np.random.default_rng(9)
    a = rng.standard_normal((37, 53)).astype(F32)
    a[0, :4] = [-0.0, 0.0, -np.inf, np.inf]
    want = np.abs(a)
    h = a.copy()
    dwt.dwt_util_abs_s(h, h.strides[0], 4, 53, 37)
    assert np.array_equal(h.view(np.uint32), want.view(np.uint32))
    h = a.copy()
    dwt.dwt_hip_abs(h, h.strides[0], 4, 53, 37)
    assert np.array_equal(h.view(np.uint32), want.view(np.uint32))
    d = Dev(dwt, a)
    dwt.dwt_hip_abs(d.ptr, 53 * 4, 4, 53, 37)
    assert np.array_equal(d.get(a.shape).view(np.uint32), want.view(np.uint32))
    d.free()


def test_libdwt_entries_and_band_primitives(dwt):
    rng = np.random.default_rng(11)
    img = balanced(rng, 64, 48, 64, 48, 4)
    want = reference(img, 64, 48, 64, 48, 4, 1.0)
    d = Dev(dwt, img)
    for ptr in (img, d.ptr):
        for n in fm.NAMES:
            got = getattr(dwt, "dwt_util_%s_s" % n)(ptr, 64 * 4, 4, 64, 48, 64, 48, 4, None, *([1.0] if n == "lpnorm" else []))
            assert np.array_equal(got, want[n]) if n == "med" else equal_bits(got, want[n]), n
        x0, y0, w, h, j = fm.bands(64, 48, 64, 48, 4)[2]
        base = (ptr if isinstance(ptr, int) else ptr.ctypes.data) + (y0 * 64 + x0) * 4
        assert dwt.dwt_util_band_wps_s(base, 256, 4, w, h, j) == want["wps"][2]
        assert dwt.dwt_util_band_var_s(base, 256, 4, w, h) == want["var"][2]
        assert dwt.dwt_util_band_cmoment_s(base, 256, 4, w, h, 2) == want["var"][2]
        assert dwt.dwt_util_band_smoment_s(base, 256, 4, w, h, 3) == want["skew"][2]
        assert dwt.dwt_util_band_med_s(base, 256, 4, w, h) == want["med"][2]
        v = fm.band_values(img, (x0, y0, w, h, j))
        assert dwt.dwt_util_band_moment_s(base, 256, 4, w, h, 2, 1.0) == F32(F32(((v - F32(1)) ** 2).sum()) / F32(w * h))
    d.free()


def test_c_example(dwt, tmp_path):
    """examples/spectra_features.c: the spectra flow from C -- per-row dwt_util_wps_s against the batch call, host and
    device rows, one launch and one download (the feature matrix) on the device."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = tmp_path / "spectra_features", os.path.join(root, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "spectra_features.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "host rows: success" in out.stderr and "device rows: success" in out.stderr and "1 launch(es)" in out.stderr


def n_hows(h, base):
    return base + (2 if h == 1 else 0)


# what the parametrisation above asks for, counted from the shape lists alone: (statistic, band) pairs x ways of calling
EXPECTED_PAIRS = sum(2 * fm.count_subbands(w, h, w, h, j) * len(ALL) * n_hows(h, 4) * 2 for (w, h, j) in EXACT_SHAPES) + \
    sum(fm.count_subbands(w, h, w, h, j) * 3 * n_hows(h, 4) for (w, h, j, _) in ORDER_SHAPES) + \
    sum(fm.count_subbands(w, h, w, h, j) * len(SUM_OF) * n_hows(h, 4) for (w, h, j, _, _) in SUM_SHAPES)
EXPECTED_RUNS = 2 * len(EXACT_SHAPES) + len(ORDER_SHAPES) + len(SUM_SHAPES)


def test_zz_every_parametrised_pair_was_compared():
    """No case fell out on the way: the comparisons made equal the number the shape lists ask for (counted above from the
    lists, not by the tests).  Meaningful for a run of the whole file only."""
    if COMPARED["ran"] != EXPECTED_RUNS:
        pytest.skip("only part of the file was run")
    assert COMPARED["pairs"] == EXPECTED_PAIRS, (COMPARED, EXPECTED_PAIRS)
