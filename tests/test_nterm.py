"""CPU checks of the N-term approximation: the numpy model (tests/nterm_model.py) against its literal restatement (full
descending sort, index n-1, strict <), against the bits a C restatement of examples/displ-vectors/vectors.c:254-297
recorded (tests/golden/nterm.npz, written by scripts/gen_nterm_golden.py), the manifest, and the ABI of the built
library."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import nterm_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(nm.GOLDEN)
F32 = np.float32

# (kind, channels, size_y, size_x) beside the fixture's cases: every channel count, every kind, rows and columns
SMALL = [(kind, ch, h, w) for kind in nm.KINDS for ch, h, w in ((1, 5, 7), (2, 1, 9), (3, 6, 5), (4, 7, 1))]


def same_result(a, b):
    return np.array_equal(nm.bits(a[0]), nm.bits(b[0])) and nm.bits(a[1]) == nm.bits(b[1]) and a[2] == b[2]


def test_manifest():
    with open(nm.MANIFEST) as f:
        info = json.load(f)["files"]["nterm.npz"]
    with open(nm.GOLDEN, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == info["sha256"]
    assert [(c["name"], (c["source"], c["seed"], c["wavelet"], c["size_y"], c["size_x"])) for c in info["cases"]] == list(nm.CASES.items())
    assert os.path.getsize(nm.GOLDEN) < 1 << 20
    want = [n + s for n, c in nm.CASES.items() for s in (".mag", ".thr", ".kept") + ((".coef",) if c[0] == "flow" else ())]
    assert sorted(GOLD.files) == sorted(want)
    assert sum(GOLD[k].size for k in GOLD.files) < 200000


@pytest.mark.parametrize("name", list(nm.CASES))
def test_model_equals_recorded_bits(name):
    """magnitudes, thresholds and kept counts of the two-channel cases, as libc's sqrtf and qsort gave them"""
    _, _, _, size_y, size_x = nm.CASES[name]
    planes = nm.case_planes(name, GOLD)
    assert planes.shape == (2, size_y, size_x) and not np.isnan(planes).any()
    mag = nm.magnitudes(planes)
    assert np.array_equal(nm.bits(mag), nm.bits(GOLD[name + ".mag"]))
    for i, n in enumerate(nm.keeps_of(mag.size)):
        out, thr, kept = nm.keep_largest(planes, n)
        assert nm.bits(thr) == nm.bits(GOLD[name + ".thr"][i]) and kept == GOLD[name + ".kept"][i], (name, n)
        gone = mag < thr
        assert not out[:, gone].any() and not np.signbit(out[:, gone]).any()
        assert np.array_equal(nm.bits(out[:, ~gone]), nm.bits(planes[:, ~gone]))


@pytest.mark.parametrize("name", [n for n in nm.CASES if n != "flow97"])
def test_model_equals_literal_on_cases(name):
    planes = nm.case_planes(name, GOLD)
    M = planes[0].size
    for n in (1, M // 10, M // 2, M, 0):
        assert same_result(nm.keep_largest(planes, n), nm.literal(planes, n)), (name, n)
    for j_max in (1, -1):
        assert same_result(nm.keep_largest(planes, M // 4, nm.DETAILS, j_max), nm.literal(planes, M // 4, nm.DETAILS, j_max)), (name, j_max)


@pytest.mark.parametrize("kind,channels,size_y,size_x", SMALL)
def test_model_equals_literal_on_small_groups(kind, channels, size_y, size_x):
    planes = nm.make_input(77 + channels, kind, channels, size_y, size_x)
    M = size_y * size_x
    for scope, j_max in ((nm.FRAME, -1), (nm.DETAILS, -1), (nm.DETAILS, 1), (nm.DETAILS, 0)):
        for n in (1, 2, M - 1, M, 0, -1, M + 1):
            assert same_result(nm.keep_largest(planes, n, scope, j_max), nm.literal(planes, n, scope, j_max)), (scope, j_max, n)


def test_magnitude_of_one_channel_is_exact():
    """fabsf, not sqrtf(c * c): magnitudes below 2^-75 survive"""
    x = np.array([[[1e-30, -1e-40, -0.0, 3.0]]], F32)
    assert np.array_equal(nm.bits(nm.magnitudes(x)), nm.bits(np.abs(x[0])))
    assert nm.magnitudes(np.concatenate([x, x]))[0, 0] == 0


def test_scope_and_levels():
    assert nm.band_levels(37, 53) == 6 and nm.band_levels(37, 53, 3) == 3 and nm.band_levels(1, 7) == 3 and nm.band_levels(1, 1) == 0
    m = nm.scope_mask(53, 37, nm.DETAILS, 3)
    assert not m[:7, :5].any() and m.sum() == 53 * 37 - 35
    assert not nm.scope_mask(4, 4, nm.DETAILS, 0).any() and nm.scope_mask(4, 4).all()
    p = nm.make_input(1, "normal", 2, 4, 4)
    out, thr, kept = nm.keep_largest(p, 3, nm.DETAILS, 0)
    assert thr == 0 and kept == 0 and np.array_equal(nm.bits(out), nm.bits(p))


def test_abi_exports():
    lib = C.CDLL(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so"))
    for s in ["dwt_hip_keep_largest_batch", "dwt_hip_keep_largest", "dwt_hip_magnitude_batch"]:
        assert hasattr(lib, s), s
    import libdwt_amd as dwt

    assert callable(dwt.keep_largest_batch) and callable(dwt.keep_largest) and callable(dwt.magnitude_batch)
    hdr = open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()
    assert "enum dwt_hip_nterm_scope { DWT_HIP_NTERM_FRAME = %d, DWT_HIP_NTERM_DETAILS = %d };" % (dwt.NTERM_FRAME, dwt.NTERM_DETAILS) in hdr
    assert (dwt.NTERM_FRAME, dwt.NTERM_DETAILS) == (nm.FRAME, nm.DETAILS)
    for s in ["dwt_hip_keep_largest_batch", "dwt_hip_keep_largest", "dwt_hip_magnitude_batch"]:
        assert "int %s(" % s in hdr
    assert dwt.band_levels(37, 53) == nm.band_levels(37, 53) and dwt.band_levels(1, 7, -1) == nm.band_levels(1, 7)
