"""CPU checks of the per-band coefficient operators' contract: the numpy model of tests/shape_model.py
against the reference-generated fixture tests/golden/shape.npz (scripts/gen_shape_golden.py asserts model == reference
for geometry, SCALE, ZERO and the median magnitude before it writes), and the library's host-side slot arithmetic against
the model.  Nothing here needs a GPU."""
import hashlib
import json

import numpy as np
import pytest

import shape_model as sm

F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(sm.GOLDEN)


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    return d


def test_manifest_matches_fixture():
    with open(sm.MANIFEST) as f:
        man = json.load(f)
    with open(sm.GOLDEN, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == man["files"]["shape.npz"]["sha256"]
    assert [c["name"] for c in man["files"]["shape.npz"]["cases"]] == list(sm.CASES)


@pytest.mark.parametrize("name", list(sm.CASES))
def test_model_equals_fixture(golden, name):
    sox, soy, six, siy, j_max, _ = sm.CASES[name]
    x, J, ops, params = sm.case_arrays(name)
    assert np.array_equal(golden[name + ".geometry"], np.array(sm.slots(sox, soy, six, siy, J), np.int32))
    assert np.array_equal(golden[name + ".ops"], ops) and np.array_equal(golden[name + ".params"].view(np.uint32), params.view(np.uint32))
    assert sm.same(sm.apply_table(x, sox, soy, six, siy, J, ops, params), golden[name + ".out"])
    if name + ".lambda" in golden:
        assert golden[name + ".lambda"].view(np.uint32) == sm.threshold(sm.threshold_input(x, sox, soy), sox, soy).view(np.uint32)


def test_every_operator_and_special_value_is_covered(golden):
    seen = set()
    for name in sm.CASES:
        x, J, ops, _ = sm.case_arrays(name)
        seen |= set(int(o) for o in ops)
        if x.size >= 400:
            assert np.isnan(x).any() and np.isinf(x).any() and (x == 0).any() and (np.abs(x) == 0.5).any()
            assert ((x != 0) & (np.abs(x) < np.finfo(F32).tiny)).any() and (np.abs(x) > 1e38).any()
    assert seen == set(range(6))


def test_operator_definitions():
    c = np.array([0.0, -0.0, 0.5, -0.5, 0.75, -0.75, np.inf, -np.inf, np.nan, 2.0, -2.0], F32)
    assert sm.same(sm.apply_op(c, sm.HARD, 0.5), np.array([0, 0, 0, 0, 0.75, -0.75, np.inf, -np.inf, np.nan, 2, -2], F32))
    assert sm.same(sm.apply_op(c, sm.SOFT, 0.5), np.array([0, 0, 0, 0, 0.25, -0.25, np.inf, -np.inf, np.nan, 1.5, -1.5], F32))
    assert sm.same(sm.apply_op(c, sm.ZERO, 0.0), np.zeros(len(c), F32))
    # hdr.c: the sign of a coefficient that is not > 0 is -1, so both zeros come out as -0
    got = sm.apply_op(c, sm.COMPRESS, 2.0)
    assert sm.same(got, np.array([-0.0, -0.0, 0.25, -0.25, 0.5625, -0.5625, np.inf, -np.inf, np.nan, 4, -4], F32))
    assert sm.same(sm.apply_op(np.array([1.0, 0.0, -1.0, np.nan], F32), sm.LOG, 0.0), np.array([0.0, -np.inf, np.nan, np.nan], F32))
    assert sm.same(sm.apply_op(np.array([0.0, -np.inf, np.nan], F32), sm.EXP, 0.5), np.array([0.5, -0.5, np.nan], F32))


def test_float64_model_is_within_one_ulp_of_libm(golden):
    """pow / log / exp in double rounded once against the host's powf / logf / expf: both sit within 1 ulp of the exact value"""
    for a, b in (("compress.out", "compress.libm"), ("hdr.compressed", "hdr.compressed.libm"), ("map.log", "map.log.libm"), ("map.exp", "map.exp.libm")):
        assert sm.ulps(golden[a], golden[b]).max() <= 1, a


def test_levels_rule():
    assert sm.levels(5, 3) == 2 and sm.levels(130, 1) == 8 and sm.levels(1, 130) == 8 and sm.levels(64, 64, 6) == 6
    assert sm.levels(64, 48, 99) == 6 and sm.levels(37, 29, 3) == 3 and sm.levels(0, 0) == 0


@pytest.mark.parametrize("sizes", [(37, 29, 37, 29, 3), (64, 64, 64, 64, 6), (5, 3, 5, 3, -1), (130, 1, 130, 1, -1), (1, 130, 1, 130, -1),
                                   (96, 80, 90, 77, 3), (1024, 1024, 1024, 1024, 5), (8, 8, 8, 8, 0), (64, 48, 64, 48, 99)])
def test_library_slot_arithmetic(dwt, sizes):
    """dwt_hip_band_levels / _slots / _geometry are host arithmetic: no device is touched"""
    sox, soy, six, siy, j_max = sizes
    J = sm.levels(sox, soy, j_max)
    assert dwt.band_levels(sox, soy, j_max) == J and dwt.band_slots(J) == 3 * J + 1
    assert np.array_equal(dwt.band_geometry(sox, soy, six, siy, j_max), np.array(sm.slots(sox, soy, six, siy, J), np.int32))


def test_library_slot_arithmetic_errors(dwt):
    with pytest.raises(dwt.DwtError):
        dwt.band_slots(-1)
    with pytest.raises(dwt.DwtError):
        dwt.band_slots(32)
    with pytest.raises(dwt.DwtError):
        dwt.band_levels(-4, 4)
    with pytest.raises(dwt.DwtError):
        dwt.band_geometry(8, 8, 9, 8)
    assert dwt.BAND_OP == {n: i for i, n in enumerate(sm.OP_NAMES)}
