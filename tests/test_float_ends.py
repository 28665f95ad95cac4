"""CPU-only: the oracle pinned to the reference on the two input classes of tests/floatends.py -- `finite_floats` (no
result has a NaN or an Inf: every sample of every result is compared bit for bit) and `ends_floats` (finite values above
MAX/2 next to the line ends, a few isolated Inf / NaN) -- for every float entry: Mallat 9/7 and 5/3 in float and double,
the interleaved layout, the 1-D lines, interp53 in 2-D and 1-D, one 3-D level.  Inverses run on an input of the class
itself, read as coefficients.

What tests/test_float_range.py cannot show on its overflowing classes is asserted here with the oracle alone:
  (a) the NaN share of every expected result is at most floatends.NAN_CAP (0.25);
  (b) per (entry, direction) at least floatends.TELLING_MIN (8) samples, summed over the shapes, differ between the oracle
      and the oracle with reflected line ends: a kernel with the wrong end form fails on them.
The shapes of a few samples ((2, 9), (9, 1), (1, 9), the 9 x 7 x 6 volume) are compared with the reference like the others
and left out of (a) and (b): one overflow reaches every sample of them.  interp53 has a doubled tap only at the last odd
sample of an even line (one of the four end / parity combinations the 9/7 has), so its counts are the smallest; its "ends"
cases run one level (floatends.ends_level says why).

Measured with the oracle on the fixture cases (telling samples forward / inverse, worst NaN share forward / inverse):
see `test_conditions_a_and_b_hold_for_every_entry`, which prints the table (pytest -s)."""
import json
import os
import warnings

import numpy as np
import pytest

import floatends as F
from conftest import GOLDEN, bits, same_floats
from test_float_range import ENTRY, canonical_sha

warnings.filterwarnings("ignore", category=RuntimeWarning)


def float_ends_cases():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)["files"]["float_ends.npz"]["cases"]


def float_ends_input(m):
    a = F.case_input(m)
    assert canonical_sha(a) == m["sha"]["in"], "the input generator changed: regenerate tests/golden/float_ends.npz"
    return a


CASES = float_ends_cases()


@pytest.fixture(scope="module")
def stored():
    return np.load(os.path.join(GOLDEN, "float_ends.npz"))


def test_the_case_table_is_the_fixture():
    assert F.ENTRY2D == ENTRY
    assert [(m["entry"], m["klass"], tuple(m["shape"]), m["decompose_one"], m["full"]) for m in CASES] == F.case_list()


@pytest.mark.parametrize("m", CASES, ids=lambda m: m["name"])
def test_oracle_matches_the_float_ends_fixtures(oracle, stored, m):
    """Outputs of the reference itself (oracle/gen_golden.py float_ends): small cases stored in full, larger ones as a hash
    over NaN-canonical bits.  The "ends" depth is the one the rule picks; a "finite" result is finite."""
    a = float_ends_input(m)
    e, d1 = m["entry"], m["decompose_one"]
    if m["klass"] == "ends":
        assert F.ends_level(oracle, e, a, d1) == m["j_in"]
    fwd, j = F.transform(oracle, e, 0, a, m["j_in"], d1)
    assert j == m["j_out"]
    inv, _ = F.transform(oracle, e, 1, a, j, d1)
    if m["klass"] == "finite":
        assert np.isfinite(fwd).all() and np.isfinite(inv).all()
    if m["full"]:
        assert np.array_equal(bits(a), bits(stored[m["name"] + ".in"]))
        assert same_floats(fwd, stored[m["name"] + ".fwd"])
        assert same_floats(inv, stored[m["name"] + ".inv"])
    assert canonical_sha(fwd) == m["sha"]["fwd"]
    assert canonical_sha(inv) == m["sha"]["inv"]


def test_conditions_a_and_b_hold_for_every_entry(oracle):
    """(a) and (b) of the module docstring, for every (entry, direction) on the "ends" cases of the fixture."""
    rows = []
    for e in F.ENTRIES:
        tell, worst = [0, 0], [0.0, 0.0]
        for m in CASES:
            if m["entry"] != e or m["klass"] != "ends" or F.is_tiny(m["shape"]):
                continue
            a = F.case_input(m)
            for inv in (0, 1):
                j = m["j_out"] if inv else m["j_in"]
                want, _ = F.transform(oracle, e, inv, a, j, m["decompose_one"])
                with F.reflected_ends(oracle):
                    refl, _ = F.transform(oracle, e, inv, a, j, m["decompose_one"])
                share = F.nan_share(want)
                assert share <= F.NAN_CAP, (m["name"], "inverse" if inv else "forward", share)
                tell[inv] += F.telling(want, refl)
                worst[inv] = max(worst[inv], share)
        rows.append((e, tell, worst))
        print("%-12s telling fwd %4d inv %4d   worst NaN share fwd %.3f inv %.3f" % (e, tell[0], tell[1], worst[0], worst[1]))
    for e, tell, _ in rows:
        assert min(tell) >= F.TELLING_MIN, (e, tell)


@pytest.mark.parametrize("klass", ["finite", "ends"])
@pytest.mark.parametrize("e", F.ENTRIES)
def test_oracle_equals_reference_on_the_new_classes(oracle, reference, e, klass):
    """Seeded sweep against the compiled reference: every shape of the tables and the degenerate ones, one level, two and
    the full depth, forward and the inverse of the input itself."""
    dt = F.entry_dtype(e)
    shapes = list(F.entry_shapes(e)) + (F.TINY_SHAPES if e in F.ENTRY2D or e == "interp53_2d" else [])
    for k, shp in enumerate(shapes):
        d1 = 1 if shp in F.TINY_SHAPES else 0
        a = F.class_input(klass, 500 + k, shp, dt, e.endswith("_1d"))
        for j in ((1,) if e == "cdf97_3d" else (1, 2, -1)):
            for inv in (0, 1):
                want, jw = F.transform(reference, e, inv, a, j, d1)
                got, jg = F.transform(oracle, e, inv, a, j, d1)
                assert jg == jw and same_floats(got, want), (e, klass, shp, j, inv)
                if not np.isnan(want).any():
                    assert np.array_equal(bits(got), bits(want)), (e, klass, shp, j, inv)
                if klass == "finite":
                    assert np.isfinite(want).all(), (e, shp, j, inv)
