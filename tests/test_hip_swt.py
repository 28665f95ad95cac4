"""GPU checks of the stationary wavelet transform of row batches (dwt_hip_swt1d_batch, dwt_hip_swt_features1d_batch, the
two swt_*_f_ex_stride_s entries) against the float32 restatement of tests/swt_model.py, which tests/test_swt.py pins to the
reference's outputs.  Every coefficient comparison is bitwise with NaN == NaN; the feature comparisons are those of
tests/test_hip_features.py: order statistics exact, every raw sum within the derived bound of the float64 model, every
finished feature the host finalisation of the device's own sums."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import features_model as fm
import swt_model as sm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
CANARY = np.uint32(0xDEADBEEF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPARED = {"planes": 0, "matched": 0}


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("swt_fused", 1)


def run_swt(dwt, wavelet, x, levels, device, pad, es, l_mode):
    """-> (H planes, L planes or None, launches).  Lines `pad` elements longer than N on both sides, elements es bytes
    apart in src; the outputs lie in canary-filled buffers whose every word outside the addressed coefficients must come
    back untouched -- the line padding, the gap between planes, and the L planes the mode does not ask for."""
    n_lines, n = x.shape
    step = es // 4
    src = np.full((n_lines, (n + pad) * step), F32(-7.5), F32)
    src[:, :n * step:step] = x
    dls_e = n + pad  # elements per output line
    plane_e = n_lines * dls_e + 16
    out_h = np.full(max(levels, 1) * plane_e, CANARY, np.uint32)
    out_l = np.full(max(levels, 1) * plane_e, CANARY, np.uint32)
    bufs = [Dev(dwt, a) for a in (src, out_h, out_l)] if device else None
    sp, hp, lp = [b.ptr for b in bufs] if device else [a.ctypes.data for a in (src, out_h, out_l)]
    k = launches(dwt, lambda: dwt.swt1d_batch(wavelet, sp, src.shape[1] * 4, es, n_lines, n, levels, hp, lp, l_mode, plane_e * 4, dls_e * 4))
    if device:
        assert np.array_equal(bufs[0].get(src.shape).view(np.uint32), src.view(np.uint32))  # src is never written
        out_h, out_l = bufs[1].get(out_h.shape, np.uint32), bufs[2].get(out_l.shape, np.uint32)
        for b in bufs:
            b.free()

    def planes(buf, which):
        """the addressed coefficients of the planes `which`; everything else must still be the canary"""
        v = buf.reshape(max(levels, 1), plane_e)
        body = v[:, :n_lines * dls_e].reshape(max(levels, 1), n_lines, dls_e)
        assert (v[:, n_lines * dls_e:] == CANARY).all() and (body[:, :, n:] == CANARY).all()
        for l in range(max(levels, 1)):
            if l not in which:
                assert (body[l] == CANARY).all(), ("plane written though not asked for", l)
        return np.stack([body[l, :, :n] for l in which]).view(F32) if which else np.zeros((0, n_lines, n), F32)

    H = planes(out_h, list(range(levels)))
    L = planes(out_l, list(range(levels)) if l_mode == 2 else [0] if l_mode == 1 and levels else [])
    return H, L, k


# (wavelet, N, levels, lines, device, pad, elem_stride, l_mode, kind): every N of {1, 2, 3, 5, 64, 77, 1000, 4096, 8192,
# 8193, 20000}, every depth of {0, 1, 3, 10, 14}, batches of 1, 3 and 300, both memory spaces, padded lines, elements 8
# bytes apart, the three l_modes and the three kinds of input; long lines and deep levels with few lines
COEFF_CASES = [
    ("cdf97_s", 1, 3, 3, True, 0, 4, 2, "normal"),
    ("cdf53_s", 2, 10, 1, True, 3, 4, 1, "small_ints"),
    ("cdf97_s", 3, 14, 3, False, 0, 4, 2, "normal"),
    ("cdf53_s", 5, 1, 300, True, 1, 4, 0, "float_range"),
    ("cdf97_s", 64, 10, 300, True, 0, 4, 2, "float_range"),
    ("cdf53_s", 64, 0, 3, True, 0, 4, 2, "normal"),
    ("cdf97_s", 77, 3, 3, True, 5, 8, 2, "small_ints"),
    ("cdf53_s", 77, 14, 1, False, 2, 8, 1, "float_range"),
    ("cdf97_s", 1000, 10, 300, True, 0, 4, 0, "normal"),
    ("cdf53_s", 1000, 3, 3, False, 8, 4, 2, "float_range"),
    ("cdf53_s", 1000, 10, 3, True, 0, 4, 1, "small_ints"),
    ("cdf97_s", 4096, 10, 3, True, 0, 4, 2, "float_range"),
    ("cdf53_s", 4096, 14, 1, True, 4, 4, 1, "normal"),
    ("cdf97_s", 4096, 1, 300, False, 0, 4, 0, "normal"),
    ("cdf97_s", 8192, 14, 1, True, 0, 4, 2, "normal"),
    ("cdf53_s", 8192, 3, 3, False, 0, 4, 0, "small_ints"),
    ("cdf53_s", 8192, 10, 3, True, 1, 4, 2, "float_range"),
    ("cdf97_s", 8193, 3, 3, True, 0, 4, 2, "float_range"),
    ("cdf53_s", 8193, 10, 1, False, 3, 4, 1, "normal"),
    ("cdf97_s", 20000, 10, 1, True, 0, 4, 2, "normal"),
    ("cdf53_s", 20000, 1, 3, True, 16, 8, 0, "float_range"),
    ("cdf97_s", 20000, 3, 1, False, 0, 4, 1, "small_ints"),
]


def check_planes(got, want, what):
    for l in range(want.shape[0]):
        COMPARED["planes"] += 1
        ok = sm.same(got[l], want[l])
        COMPARED["matched"] += ok
        assert ok, (what, "level", l)


@pytest.mark.parametrize("case", COEFF_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_coefficients_bit_identical(dwt, case):
    wavelet, n, levels, lines, device, pad, es, l_mode, kind = case
    x = sm.make_input(n * 13 + levels + lines, kind, lines, n)
    wantL, wantH = sm.swt_levels(x, wavelet, levels)
    H, L, k = run_swt(dwt, wavelet, x, levels, device, pad, es, l_mode)
    check_planes(H, wantH, "H")
    check_planes(L, wantL if l_mode == 2 else wantL[-1:] if l_mode == 1 else wantL[:0], "L")
    if device and es == 4 and levels:
        assert k == (1 if n <= 8192 else levels), k


def test_all_planes_matched():
    """the share of compared planes that must match is 100 % (meaningful for a run of the whole file)"""
    assert COMPARED["planes"] == COMPARED["matched"]


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_level_passes_equal_fused(dwt, wavelet):
    """option swt_fused = 0: one launch per level through global memory, the same bits"""
    x = sm.make_input(77, "float_range", 5, 1500)
    fused = run_swt(dwt, wavelet, x, 6, True, 0, 4, 2)
    dwt.set_option("swt_fused", 0)
    try:
        plain = run_swt(dwt, wavelet, x, 6, True, 0, 4, 2)
    finally:
        dwt.set_option("swt_fused", 1)
    assert fused[2] == 1 and plain[2] == 6
    assert sm.same(fused[0], plain[0]) and sm.same(fused[1], plain[1])
    wantL, wantH = sm.swt_levels(x, wavelet, 6)
    assert sm.same(plain[0], wantH) and sm.same(plain[1], wantL)


def test_one_launch(dwt):
    for n, levels, lines in [(64, 1, 1), (64, 10, 300), (1000, 14, 3), (4096, 10, 300), (8192, 10, 1), (8192, 24, 7)]:
        x = np.zeros((lines, n), F32)
        src, h, l = Dev(dwt, x), Dev(dwt, np.zeros((levels, lines, n), F32)), Dev(dwt, np.zeros((levels, lines, n), F32))
        fv = Dev(dwt, np.zeros((lines, len(fm.NAMES) * levels), F32))
        for w in sm.WAVELETS:
            for l_mode in (0, 1, 2):
                assert launches(dwt, lambda: dwt.swt1d_batch(w, src.ptr, n * 4, 4, lines, n, levels, h.ptr, l.ptr, l_mode, lines * n * 4, n * 4)) == 1
            for names in (["wps"], ["wps", "mean", "maxnorm", "norm"], list(fm.NAMES), ["med"]):
                for band in (0, 1):
                    assert launches(dwt, lambda: dwt.swt_features1d_batch(w, names, src.ptr, n * 4, 4, lines, n, levels, fv.ptr,
                                                                          len(fm.NAMES) * levels, band, 1.5)) == 1
        for d in (src, h, l, fv):
            d.free()


# ---- features ----------------------------------------------------------------------------------------------------------
ALL = list(fm.NAMES)
SUM_OF = {"wps": ["S2"], "mean": ["S1"], "var": ["M2"], "stdev": ["M2"], "skew": ["M2", "M3"], "kurt": ["M2", "M4"], "lpnorm": ["Sp"], "norm": ["S2"]}
PLANES = ["S1", "S2", "Sp", "M2", "M3", "M4"]  # dwt_hip_features_raw_sums
U = 2.0 ** -24


def run_features(dwt, wavelet, names, x, levels, band, p, device, es=4):
    """-> (array (lines, len(names), levels), names in enum order)"""
    names = [n for n in fm.NAMES if n in names]
    lines, n = x.shape
    step = es // 4
    src = np.zeros((lines, n * step), F32)
    src[:, ::step] = x
    stride = len(names) * levels + 3
    fv = np.full((lines, stride), np.nan, F32)
    d, dfv = (Dev(dwt, src), Dev(dwt, fv)) if device else (None, None)
    sp, fp = (d.ptr, dfv.ptr) if device else (src.ctypes.data, fv.ctypes.data)
    dwt.swt_features1d_batch(wavelet, names, sp, src.shape[1] * 4, es, lines, n, levels, fp, stride, band, p)
    if device:
        fv = dfv.get(fv.shape)
        d.free()
        dfv.free()
    assert np.isnan(fv[:, len(names) * levels:]).all()  # the tail of every line's block is untouched
    return fv[:, :len(names) * levels].reshape(lines, len(names), levels), names


def ref_band(name, v, j, p):
    """the reference's dwt_util_band_<name>_s over a plane where the reference is built, else its sequential restatement"""
    if fm.RefFeatures.available():
        lib = C.CDLL(fm.REF_SO)
        f = getattr(lib, "dwt_util_band_%s_s" % name)
        f.restype = C.c_float
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + ([C.c_int] if name == "wps" else [C.c_float] if name == "lpnorm" else [])
        v = np.ascontiguousarray(v, F32)
        return F32(f(v.ctypes.data, 0, 4, len(v), 1, *([j] if name == "wps" else [float(p)] if name == "lpnorm" else [])))
    return F32(fm.seq32_band(np.ascontiguousarray(v, F32), j, p)[name])


# (wavelet, N, levels, lines, band, kind, p)
FEATURE_SHAPES = [("cdf97_s", 4096, 10, 3, 0, "normal", 1.5), ("cdf53_s", 1000, 6, 5, 1, "small_ints", 3.0), ("cdf97_s", 8192, 4, 2, 0, "normal", 1.0),
                  ("cdf53_s", 77, 5, 4, 0, "small_ints", 2.5), ("cdf97_s", 20000, 3, 2, 1, "normal", 2.5), ("cdf53_s", 64, 12, 3, 0, "normal", 2.0)]


@pytest.mark.parametrize("shape", FEATURE_SHAPES)
def test_order_statistics_exact(dwt, shape):
    wavelet, n, levels, lines, band, kind, p = shape
    x = sm.make_input(n + levels, kind, lines, n)
    planes = sm.swt_levels(x, wavelet, levels)[0 if band else 1]
    names = ["maxidx", "med", "maxnorm"]
    want = {q: np.array([[fm.order_stats(planes[l, y])[q] for l in range(levels)] for y in range(lines)], F32) for q in names}
    for q in names:  # the reference's own values over the same planes
        assert want[q][0, 0] == ref_band(q, planes[0, 0], 0, p) and want[q][-1, -1] == ref_band(q, planes[-1, -1], levels - 1, p)
    for device in (True, False):
        got, order = run_features(dwt, wavelet, names, x, levels, band, p, device)
        for i, q in enumerate(order):
            ok = np.array_equal(got[:, i], want[q]) if q == "med" else sm.same(got[:, i], want[q])
            assert ok, (device, q, got[:, i], want[q])


@pytest.mark.parametrize("shape", FEATURE_SHAPES)
def test_sums_against_float64_model(dwt, shape):
    """Every raw device sum S satisfies |S_gpu - S_64| <= 2^-24 |S_64| + n 2^-53 T against the float64 model over the
    restatement's plane (the central sums about the device's own float mean); every finished feature equals the host
    finalisation (features_model.finish) of the device's own sums.  The model itself is held against the reference's
    dwt_util_band_*_s with the reference's own error bound, as in tests/test_hip_features.py."""
    wavelet, n, levels, lines, band, kind, p = shape
    x = sm.make_input(3 * n + levels, kind, lines, n)
    planes = sm.swt_levels(x, wavelet, levels)[0 if band else 1]
    names = [q for q in fm.NAMES if q in SUM_OF]
    for y, l in ((0, 0), (lines - 1, levels - 1)):  # the guard of the model
        v = planes[l, y]
        mean_ref = ref_band("mean", v, l, p)
        m = fm.model64_band(v, p, mean=mean_ref)
        for name, s_ref in (("S2", float(ref_band("wps", v, l, p)) * (1 << l)), ("S1", float(mean_ref) * n), ("M2", float(ref_band("var", v, l, p)) * n)):
            s, t, _ = m[name]
            assert abs(s_ref - s) <= (n + 2) * U * t + 2 * U * abs(s_ref), ("reference vs model", name, y, l, s_ref, s)
    first = None
    for device, es in ((True, 4), (False, 4), (True, 8)):
        got, order = run_features(dwt, wavelet, names, x, levels, band, p, device, es)
        if first is None:
            first = got
        assert sm.same(got, first), (device, es)  # every way of calling gives the same bits
        if n > 8192 or es != 4:
            # (the raw sums kept from a call over long lines are those of its last level only; their finished features are
            # held to dwt_hip_band_feature in test_feature_mode_equals_coefficient_mode_then_band_feature)
            continue
        # (plane Sp is formed and downloaded only where lpnorm needs it: p other than 2, where it is plane S2)
        planes_here = [q for q in PLANES if q != "Sp" or p != 2.0]
        raw = {q: dwt.features_raw_sums(PLANES.index(q), lines * levels) for q in planes_here}
        for y in range(lines):
            for l in range(levels):
                r = y * levels + l
                mean_dev = F32(F32(raw["S1"][r]) / F32(n))
                m = fm.model64_band(planes[l, y], p, mean=mean_dev)
                for q in planes_here:
                    s, t, cnt = m[q]
                    err, bound = abs(raw[q][r] - s), U * abs(s) + cnt * 2.0 ** -53 * t
                    assert err <= bound, (device, q, y, l, raw[q][r], s, err, bound)
                sums = {q: F32(raw[q][r]) for q in planes_here}
                for i, name in enumerate(order):
                    want = np.asarray(fm.finish(name, sums, n, l, p), F32)
                    assert sm.same(got[y, i, l], want), (device, name, y, l, got[y, i, l], want)


@pytest.mark.parametrize("shape", FEATURE_SHAPES)
def test_feature_mode_equals_coefficient_mode_then_band_feature(dwt, shape):
    """no coefficient stored == coefficients stored, then dwt_hip_band_feature on each plane: bit for bit, every feature;
    and the level passes (swt_fused = 0) give the same features"""
    wavelet, n, levels, lines, band, kind, p = shape
    x = sm.make_input(7 * n + levels, kind, lines, n)
    src = Dev(dwt, x)
    h, l = Dev(dwt, np.zeros((levels, lines, n), F32)), Dev(dwt, np.zeros((levels, lines, n), F32))
    dwt.swt1d_batch(wavelet, src.ptr, n * 4, 4, lines, n, levels, h.ptr, l.ptr, 2, lines * n * 4, n * 4)
    base = l.ptr if band else h.ptr
    got, order = run_features(dwt, wavelet, ALL, x, levels, band, p, True)
    v = C.c_float()
    for y in range(lines):
        for lev in range(levels):
            for i, name in enumerate(order):
                rc = dwt.lib.dwt_hip_band_feature(fm.NAMES.index(name), base + ((lev * lines + y) * n) * 4, 0, 4, n, 1, lev, p, C.byref(v))
                assert rc == 0, dwt.last_error()
                assert sm.same(got[y, i, lev], F32(v.value)), (name, y, lev, got[y, i, lev], v.value)
    dwt.set_option("swt_fused", 0)
    try:
        plain, _ = run_features(dwt, wavelet, ALL, x, levels, band, p, True)
    finally:
        dwt.set_option("swt_fused", 1)
    assert sm.same(plain, got)
    host, _ = run_features(dwt, wavelet, ALL, x, levels, band, p, False)
    assert sm.same(host, got)
    for d in (src, h, l):
        d.free()


def test_reference_entries(dwt):
    """swt_cdf97_f_ex_stride_s / swt_cdf53_f_ex_stride_s: one level of one line, host and device memory, any byte stride"""
    for name, wavelet in (("swt_cdf97_f_ex_stride_s", "cdf97_s"), ("swt_cdf53_f_ex_stride_s", "cdf53_s")):
        fn = getattr(dwt, name)
        for n, level, step in ((1, 0, 1), (100, 0, 1), (100, 3, 3), (4096, 9, 1), (9000, 2, 2), (257, 23, 1)):
            x = sm.make_input(n + level, "float_range" if n == 100 else "normal", 1, n)[0]
            wantL, wantH = sm.swt_level(x, wavelet, level)
            src = np.full(n * step, F32(9), F32)
            src[::step] = x
            for device in (False, True):
                outs = [np.full(n * step, CANARY, np.uint32) for _ in range(2)]
                bufs = [Dev(dwt, a) for a in [src] + outs] if device else None
                ptrs = [b.ptr for b in bufs] if device else [a.ctypes.data for a in [src] + outs]
                fn(ptrs[0], ptrs[1], ptrs[2], n, 4 * step, level)
                if device:
                    outs = [b.get(outs[0].shape, np.uint32) for b in bufs[1:]]
                    for b in bufs:
                        b.free()
                for o, want in zip(outs, (wantL, wantH)):
                    assert sm.same(o[::step].view(F32), want), (name, n, level, step, device)
                    mask = np.ones(n * step, bool)
                    mask[::step] = False
                    assert (o[mask] == CANARY).all()


def test_refusals(dwt):
    x = np.zeros((3, 32), F32)
    d = Dev(dwt, x)
    h, dh = np.zeros((4, 3, 32), F32), Dev(dwt, np.zeros((4, 3, 32), F32))
    fv, dfv = np.zeros((3, 8), F32), Dev(dwt, np.zeros((3, 8), F32))
    bad = [
        lambda: dwt.swt1d_batch("cdf97_s", d.ptr, 128, 4, 3, 32, 4, h, None, 0, 384, 128),  # device src, host dst
        lambda: dwt.swt1d_batch("cdf97_s", x, 128, 4, 3, 32, 4, dh.ptr, None, 0, 384, 128),
        lambda: dwt.swt1d_batch("cdf97_s", d.ptr, 128, 4, 3, 32, 4, dh.ptr, h, 2, 384, 128),
        lambda: dwt.swt1d_batch("cdf97_s", d.ptr, 128, 6, 2, 16, 4, dh.ptr, None, 0, 384, 128),  # device stride not a multiple of 4
        lambda: dwt.swt1d_batch("cdf97_s", d.ptr, 128, 4, 3, 32, 4, d.ptr, None, 0, 384, 128),  # overlap
        lambda: dwt.swt_features1d_batch("cdf97_s", "wps", d.ptr, 128, 4, 3, 32, 4, fv, 8),
        lambda: dwt.swt_features1d_batch("cdf97_s", "wps", x, 128, 4, 3, 32, 4, dfv.ptr, 8),
        lambda: dwt.swt_features1d_batch("cdf97_s", ["wps", "med", "var"], d.ptr, 128, 4, 3, 32, 4, dfv.ptr, 8),  # fv stride
    ]
    for i, f in enumerate(bad):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    for b in (d, dh, dfv):
        b.free()


def test_c_example(dwt, tmp_path):
    """examples/spectra_swt.c: the reference's spectra-swt loop from C against one batch call per feature matrix"""
    exe, libdir = tmp_path / "spectra_swt", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "spectra_swt.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "host rows: success" in out.stderr and "device rows: success" in out.stderr and "2 launch(es)" in out.stderr
    assert (out.stderr + out.stdout).count("success") == 2
