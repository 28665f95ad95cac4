"""CPU checks of what tests/test_hip_grid_limits.py expects without running a model on every line: the periodic tiling of
tests/gridlimits.py equals the full model on 600 lines (more than two periods of 251, the last one cut short) for the
three kinds of independent lines the GPU file tiles, and the restatement of detect_ridges3_s equals the fixtures."""
import numpy as np

import condition_model as cm
import gridlimits as gl
import swt_model as sm
import timefreq_model as tm

F32 = np.float32
LINES = 600


def test_period_divides_no_cap():
    assert gl.P == 251 and all(gl.P % d for d in range(2, 16))  # prime
    assert [c % gl.P for c in (16384, 65535, 65536)] == [69, 24, 25]
    assert gl.trips(65835, 65535) == 2 and gl.trips(65535, 65535) == 1 and gl.trips(16684, 16384) == 2


def test_tile_is_periodic():
    a = np.arange(gl.P * 3).reshape(gl.P, 3)
    t = gl.tile(a, LINES)
    assert t.shape == (LINES, 3) and all(np.array_equal(t[i], a[i % gl.P]) for i in range(LINES))
    assert np.array_equal(gl.tile(a.T, LINES, axis=1), t.T)


def test_swt_lines_tile():
    base = sm.make_input(1, "normal", gl.P, 8)
    for wavelet in sm.WAVELETS:
        L, H = sm.swt_levels(base, wavelet, 3)
        fullL, fullH = sm.swt_levels(gl.tile(base, LINES), wavelet, 3)
        assert sm.same(gl.tile(L, LINES, axis=1), fullL) and sm.same(gl.tile(H, LINES, axis=1), fullH)


def test_condition_rows_tile():
    base = cm.make_input(2, "spectrum", gl.P, 5)
    rows, info = cm.condition(base, cm.MED_SHIFT | cm.SCALE, 20, -1.0, 2.5)
    full_rows, full_info = cm.condition(gl.tile(base, LINES), cm.MED_SHIFT | cm.SCALE, 20, -1.0, 2.5)
    assert np.array_equal(gl.tile(rows, LINES).view(np.uint32), full_rows.view(np.uint32))
    assert np.array_equal(gl.tile(info, LINES), full_info)
    # rows cycle with period 251, displacements with period 5: the expected rows come from a 5 x 251 table
    i = np.arange(LINES)
    displ = np.array([cm.displacement(dn, 5) for dn in cm.DISPLACEMENTS])[i % 5]
    for zero in (True, False):
        full = np.stack([cm.displace1(r, int(d), zero) for r, d in zip(gl.tile(base, LINES), displ)])
        per = np.stack([[cm.displace1(r, cm.displacement(dn, 5), zero) for r in base] for dn in cm.DISPLACEMENTS])
        assert np.array_equal(per[i % 5, i % gl.P].view(np.uint32), full.view(np.uint32))


def test_oracle_lines_tile(oracle):
    base = sm.make_input(3, "normal", gl.P, 16)
    for wv in ("cdf97", "cdf53"):
        fwd, j = gl.oned(oracle, wv, 0, base, 2)
        full, jf = gl.oned(oracle, wv, 0, gl.tile(base, LINES), 2)
        assert j == jf == 2 and np.array_equal(gl.tile(fwd, LINES).view(np.uint32), full.view(np.uint32))
        inv, _ = gl.oned(oracle, wv, 1, fwd, 2)
        full_inv, _ = gl.oned(oracle, wv, 1, full, 2)
        assert np.array_equal(gl.tile(inv, LINES).view(np.uint32), full_inv.view(np.uint32))
        assert np.abs(inv - base).max() < 1e-5


def test_ridges3_restatement_equals_the_fixtures():
    """the fixtures hold no point within 2^-20 of a direction threshold (tests/test_timefreq.py), so the float64 angle of
    the restatement and the reference's float libm pick the same neighbour everywhere"""
    gold = np.load(tm.GOLDEN)
    seen = 0
    for i in range(len(tm.CASES)):
        mag = gold["mag_%d" % i]
        assert tm.same(tm.ridges3(mag, 0.0), gold["r3_%d" % i]), tm.CASES[i]
        seen += int(np.count_nonzero(gold["r3_%d" % i]))
    assert seen > 100
