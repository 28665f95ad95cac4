"""Every 16-byte fast path at every base, pitch and length residue, on the GPU: one test per family over
the cells of tests/alignment_cases.py, whose CPU test (tests/test_alignment_matrix.py) shows that they stand on both sides
of every term of every predicate.  Each call runs on frames that lie 16 + off bytes into allocations full of canaries;
every byte of every allocation is compared -- the samples with the CPU model's bits, everything else with the canary, the
source of an out-of-place call with itself.  A variant reports every cell that differs, not the first alone."""
import time

import pytest

import alignment_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    for name, value in ac.DEFAULTS.items():
        d.set_option(name, value)
    d.dwt_util_finish()


def check(dwt, family, variant):
    f = ac.FAMILIES[family]
    t0 = time.perf_counter()
    bad = f.run(dwt, variant)
    print("%s %s: %d cells in %.2f s" % (family, variant, len(f.cells_of(variant)), time.perf_counter() - t0))
    assert not bad, "%d differences:\n  %s" % (len(bad), "\n  ".join(bad[:40]))


def variants(family):
    return pytest.mark.parametrize("variant", ac.FAMILIES[family].variants)


@variants("oned")
def test_oned(dwt, variant):
    check(dwt, "oned", variant)


@variants("lifting1d")
def test_lifting1d(dwt, variant):
    check(dwt, "lifting1d", variant)


@variants("swt")
def test_swt(dwt, variant):
    check(dwt, "swt", variant)


@variants("swt_features")
def test_swt_features(dwt, variant):
    check(dwt, "swt_features", variant)


@variants("iswt")
def test_iswt(dwt, variant):
    check(dwt, "iswt", variant)


@variants("wp")
def test_wp(dwt, variant):
    check(dwt, "wp", variant)


@variants("condition")
def test_condition(dwt, variant):
    check(dwt, "condition", variant)


@variants("nterm")
def test_nterm(dwt, variant):
    check(dwt, "nterm", variant)


@variants("bandops")
def test_bandops(dwt, variant):
    check(dwt, "bandops", variant)


@variants("window")
def test_window(dwt, variant):
    check(dwt, "window", variant)


@variants("mallat2d")
def test_mallat2d(dwt, variant):
    check(dwt, "mallat2d", variant)


# (the 3-D family last: its interior tiles fetch 16-byte halos from rows that are only 4-byte aligned, which no other test does)
@variants("vol3d")
def test_vol3d(dwt, variant):
    check(dwt, "vol3d", variant)
