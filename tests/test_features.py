"""CPU checks of the feature statistics: the sequential-float32 restatement (tests/features_model.py) against the compiled
reference where it is built and against tests/golden/features.npz, the band count, and the ABI of the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import features_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(fm.GOLDEN)


def same(a, b):
    """bit-equal float32 vectors, NaNs of any payload equal"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)]) and \
        np.array_equal(np.isnan(a), np.isnan(b))


def same_value(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32))


@pytest.mark.parametrize("i", range(len(fm.CASES)))
def test_restatement_equals_golden(i):
    seed, kind, sox, soy, six, siy, j_max, p = fm.CASES[i]
    c = GOLD["cases"][i]
    assert (int(c["seed"]), str(c["kind"]), int(c["sox"]), int(c["soy"]), int(c["j_max"])) == (seed, kind, sox, soy, j_max)
    img = fm.make_input(seed, kind, sox, soy)
    assert fm.count_subbands(sox, soy, six, siy, j_max) == int(GOLD["count_%d" % i])
    got = fm.seq32(img, sox, soy, six, siy, j_max, p)
    for n in fm.NAMES:
        want = GOLD["%s_%d" % (n, i)]
        assert (same_value if n == "med" else same)(got[n], want), (n, got[n], want)


SHAPES = [(256, 1, 256, 1, 9, 1.0), (77, 1, 77, 1, 5, 1.0), (31, 19, 31, 19, 4, 2.0), (48, 40, 30, 21, 4, 1.0), (16, 16, 16, 16, 9, 3.0),
          (16, 16, 16, 16, 1, 2.0), (16, 16, 16, 16, 0, 2.0), (3, 2, 3, 2, 3, 1.0)]


@pytest.mark.skipif(not fm.RefFeatures.available(), reason="the reference is not built here")
@pytest.mark.parametrize("shape", SHAPES + [c[2:] for c in fm.CASES[::5]])
def test_restatement_equals_reference(shape):
    sox, soy, six, siy, j_max, p = shape
    ref = fm.RefFeatures()
    for kind in ("normal", "small_ints"):
        img = fm.make_input(7 + sox, kind, sox, soy)
        assert ref.count(img, sox, soy, six, siy, j_max) == fm.count_subbands(sox, soy, six, siy, j_max)
        want = ref.features(img, sox, soy, six, siy, j_max, p)
        got = fm.seq32(img, sox, soy, six, siy, j_max, p)
        for n in fm.NAMES:
            assert (same_value if n == "med" else same)(got[n], want[n]), (n, kind, got[n], want[n])


def test_count_zero_features():
    assert fm.count_subbands(16, 16, 16, 16, 1) == 0 and fm.count_subbands(16, 16, 16, 16, 0) == 0
    assert fm.count_subbands(4096, 1, 4096, 1, 13) == 12 and fm.count_subbands(64, 64, 64, 64, 5) == 12


NEW_SYMBOLS = ["dwt_hip_count_subbands", "dwt_hip_features2d", "dwt_hip_features2d_batch", "dwt_hip_features1d_batch", "dwt_hip_abs",
               "dwt_hip_band_feature", "dwt_hip_band_moment", "dwt_hip_features2d_hostfv", "dwt_hip_features_raw_sums", "dwt_util_count_subbands_s", "dwt_util_subband_const_s", "dwt_util_abs_s"] + \
    ["dwt_util_%s_s" % n for n in fm.NAMES] + ["dwt_util_band_%s_s" % n for n in fm.NAMES + ("moment", "cmoment", "smoment")]


def test_abi_exports():
    lib = C.CDLL(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so"))
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s


def test_mirrors_and_count_without_device():
    import libdwt_amd as dwt

    for s in ["features2d", "features2d_batch", "features1d_batch", "count_subbands", "dwt_hip_abs"] + [s for s in NEW_SYMBOLS if s.startswith("dwt_util")]:
        assert callable(getattr(dwt, s)), s
    assert set(dwt.FEATURE) == set(fm.NAMES) and dwt.FEATURE["wps"] == 1 and dwt.FEATURE["norm"] == 1 << 10
    for sox, soy, six, siy, j in [(64, 64, 64, 64, 5), (37, 53, 30, 40, 4), (4096, 1, 4096, 1, 13), (8, 8, 8, 8, 1), (5, 3, 5, 3, 6)]:
        assert dwt.count_subbands(sox, soy, six, siy, j) == fm.count_subbands(sox, soy, six, siy, j)
    with pytest.raises(dwt.DwtError):
        dwt.count_subbands(8, 8, 9, 8, 3)


def test_call_without_device_fails_cleanly():
    import libdwt_amd as dwt

    if dwt.lib.dwt_hip_init() == 0:
        pytest.skip("a device is present: covered by the GPU suite")
    a = np.zeros((8, 8), np.float32)
    fv = np.zeros(16, np.float32)
    with pytest.raises(dwt.DwtError):
        dwt.features2d("wps", a, 32, 4, 8, 8, 8, 8, 3, fv)
    with pytest.raises(dwt.DwtError):
        dwt.dwt_util_wps_s(a, 32, 4, 8, 8, 8, 8, 3)
    with pytest.raises(dwt.DwtError):
        dwt.dwt_hip_abs(a, 32, 4, 8, 8)
