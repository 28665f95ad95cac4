"""CPU checks of the user-defined lifting wavelets of line batches and of the quantizer norms of a scheme
(include/libdwt_hip.h).  The numpy model (tests/lifting1d_model.py) fed the CDF tables must give the bits of
the oracle's 1-D transforms (the restatement of the reference's 1-D driver in tests/test_oned.py, and
tests/interp53_model.py); int schemes are reversible bit for bit; dwt_hip_lifting_norms / _quant_steps (host code) agree
with dwt_hip_quant_norms / _quant_steps for the CDF tables, with the closed form for Haar and with the float64 model.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lifting1d_model as l1
import lifting_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 3, 5, 17, 64, 65, 513]
CDF = {"CDF97": "cdf97_s", "CDF53": "cdf53_s", "INTERP53": "interp53_s"}
LMAX = l1.QUANT_MAX_LEVELS


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def oracle():
    import oraclelib as ol

    return ol.Oracle()


@pytest.fixture(scope="module")
def dwt():
    import __graft_entry__ as g

    if not os.path.exists(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")):
        g.build()
    import libdwt_amd as d
    from libdwt_amd import lifting, quant

    d.lifting, d.quant = lifting, quant
    return d


def to_lib(L, s):
    return L.scheme(s.type, [L.step(st.parity, st.terms, st.sign, st.add, st.shift) for st in s.steps], s.fwd_scale, s.inv_scale,
                    s.inverse_cols_first)


def random_far():
    s = lm.random_scheme(lm.F32, 12, reach=11)
    assert s.reach > lm.FUSED_REACH
    return s


# ---- the model against the oracle ------------------------------------------------------------------------------------------

def oracle_1d(oracle, name, inverse, lines, j):
    """the oracle's 1-D transform of every line, in place; returns the level count"""
    if name == "INTERP53":
        import interp53_model as im

        if inverse:
            im.inv1d(lines, j_max=j)
            return j
        return im.fwd1d(lines, j_max=j)
    import test_oned

    J = j
    for row in lines:
        J = test_oned.restated(oracle, name.lower(), inverse, row, lines.shape[1], j_max=j)
    return J


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", sorted(CDF))
def test_cdf_tables_give_the_oracles_1d_bits(oracle, name, size, full):
    """forward and inverse, depth 1 and full; inputs uniform in [-1, 1), so that no doubled end tap overflows and the two
    line-end forms are the same float (libdwt_amd/csrc/dwt_lift.h)"""
    s = lm.builtin(name)
    j = -1 if full else 1
    x = np.random.default_rng([41, size]).uniform(-1, 1, (3, size)).astype(np.float32)
    want = x.copy()
    J = oracle_1d(oracle, name, False, want, j)
    got, Jm = l1.fwd1d(s, x, j)
    assert Jm == J == (lm.ceil_log2(size) if full else 1) and same(got, want)
    back = want.copy()
    oracle_1d(oracle, name, True, back, J)
    got_back, Jb = l1.inv1d(s, got, J)
    assert Jb == J and same(got_back, back)


def test_layout_and_level_clamp():
    s = lm.builtin("HAAR_INT")
    x = np.arange(1, 8, dtype=np.int32)[None] * 10
    y, J = l1.fwd1d(s, x, 1)
    # odd -= left even; even += right odd >> 1 (sample 6 reads sample 7, reflected to 5): L takes ceil(7/2) samples at
    # offset 0, H floor(7/2) behind them
    assert J == 1 and y.tolist() == [[15, 35, 55, 75, 10, 10, 10]]
    assert [l1.levels1d(7, j) for j in (-1, 0, 2, 3, 4, 99)] == [3, 0, 2, 3, 3, 3]
    assert [l1.levels1d(7, j, True) for j in (-1, 0, 2, 3, 4)] == [3, 0, 2, 3, 3]
    assert l1.levels1d(1, -1) == 0 and same(l1.fwd1d(s, x[:, :1])[0], x[:, :1])


@pytest.mark.parametrize("size", [1, 2, 3, 5, 17])
@pytest.mark.parametrize("which", ["CDF53_INT", "CDF97_INT", "HAAR_INT", "random 1", "random 2"])
def test_int_schemes_are_reversible_bit_for_bit(which, size):
    """the whole int32 range, INT32_MIN and INT32_MAX among the samples: the wrapped values come back too"""
    s = lm.random_scheme(lm.I32, int(which.split()[1])) if which.startswith("random") else lm.builtin(which)
    x = np.random.default_rng([43, size]).integers(-(1 << 31), 1 << 31, (4, size)).astype(np.int32)
    x.reshape(-1)[:2] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    for j in (-1, 1):
        y, J = l1.fwd1d(s, x, j)
        assert J == l1.levels1d(size, j)
        back, _ = l1.inv1d(s, y, J)
        assert same(back, x)
        if size >= 2:
            assert not same(y, x)


# ---- norms and step tables -----------------------------------------------------------------------------------------------

def close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool((np.abs(a - b) <= rel * np.abs(b)).all())


@pytest.mark.parametrize("name", sorted(CDF))
def test_norms_of_the_cdf_tables_are_the_quantizers(dwt, name):
    """both are double evaluations of the same sums of a few thousand terms: 1e-12 relative, at every level count"""
    L = dwt.lifting
    want_l, want_h = dwt.quant.quant_norms(dwt.WAVELET_ID[CDF[name]], LMAX)
    for levels in range(LMAX + 1):
        nl, nh = L.norms(L.builtin(name), levels)
        assert len(nl) == len(nh) == levels
        assert close(nl, want_l[:levels]) and close(nh, want_h[:levels]), levels


@pytest.mark.parametrize("name", sorted(CDF))
def test_quant_steps_of_the_cdf_tables_are_the_quantizers(dwt, name):
    """the same floats, or neighbours where a norm differs in its last bits"""
    L = dwt.lifting
    for levels, base in ((0, 1.0), (1, 0.37), (5, 2.5), (LMAX, 1e-3)):
        got = np.array(L.quant_steps(L.builtin(name), levels, base)[:], np.float32)
        want = dwt.quant.quant_steps(dwt.WAVELET_ID[CDF[name]], levels, base)
        assert got.shape == want.shape and (want > 0).all()
        ulps = np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64))
        assert ulps.max() <= 1, (levels, base, int(ulps.max()))


def test_norms_of_haar_are_powers_of_two(dwt):
    """the inverse maps a unit L to (1, 1) and a unit H to (-1/2, 1/2): 2^j ones, and 2^(j-1) halves of either sign"""
    L = dwt.lifting
    nl, nh = L.norms(L.builtin("HAAR"), LMAX)
    j = np.arange(1, LMAX + 1)
    assert close(nl, 2.0 ** (j / 2)) and close(nh, 2.0 ** ((j - 2) / 2))


@pytest.mark.parametrize("which", ["D4", "random R>8", "CDF97"])
def test_norms_are_the_models(dwt, which):
    """the C entry against the float64 restatement (tests/lifting1d_model.py): the same operations, the final sum in another
    order.  Ten levels: the model's line of 2 (R + 2) << 10 samples is what numpy does in a moment; the level loop has nothing
    that changes beyond it"""
    L = dwt.lifting
    s = random_far() if which.startswith("random") else lm.builtin(which)
    levels = 10
    want_l, want_h = l1.norms(s, levels)
    nl, nh = L.norms(to_lib(L, s), levels)
    assert close(nl, want_l) and close(nh, want_h)
    got = np.array(L.quant_steps(to_lib(L, s), levels, 0.75)[:], np.float32)
    want = l1.quant_steps(s, levels, 0.75)
    assert np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64)).max() <= 1


def test_norms_of_a_far_reaching_scheme_at_every_level(dwt):
    """R > 8 at the largest level count: finite and positive, and the norms of a shallower call are a prefix of them"""
    L = dwt.lifting
    nl, nh = L.norms(to_lib(L, random_far()), LMAX)
    assert len(nl) == LMAX and np.isfinite(nl).all() and np.isfinite(nh).all() and min(nl) > 0 and min(nh) > 0
    assert L.norms(to_lib(L, random_far()), 10) == (nl[:10], nh[:10])


def test_norm_entries_refuse(dwt):
    L = dwt.lifting
    d4 = L.builtin("D4")

    def refused(f, word):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert "lifting:" in str(e.value) and word in str(e.value), str(e.value)

    for name in ("CDF53_INT", "CDF97_INT", "HAAR_INT"):
        refused(lambda: L.norms(L.builtin(name), 3), "int scheme")
        refused(lambda: L.quant_steps(L.builtin(name), 3, 1.0), "int scheme")
    refused(lambda: L.norms(d4, -1), "levels")
    refused(lambda: L.norms(d4, LMAX + 1), "levels")
    refused(lambda: L.quant_steps(d4, LMAX + 1, 1.0), "levels")
    for base in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: L.quant_steps(d4, 3, base), "base step")
    bad = L.builtin("D4")
    bad.steps[1].terms[0].off_a = 2
    refused(lambda: L.norms(bad, 3), "off_a")
    nl = (C.c_double * 4)()
    assert dwt.lib.dwt_hip_lifting_norms(C.byref(d4), 3, None, nl) != 0 and "null" in dwt.last_error()
    assert dwt.lib.dwt_hip_lifting_norms(None, 3, nl, nl) != 0 and "null" in dwt.last_error()
    assert dwt.lib.dwt_hip_lifting_quant_steps(C.byref(d4), 3, 1.0, None) != 0 and "null" in dwt.last_error()
    assert L.norms(d4, 0) == ([], []) and L.quant_steps(d4, 0, 2.0)[:] == [2.0]  # (a refusal does not stick)


def test_python_names_and_constants(dwt):
    import re

    L = dwt.lifting
    header = open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()
    assert re.search(r"#define DWT_HIP_QUANT_MAX_LEVELS %d\s" % L.QUANT_MAX_LEVELS, header) and L.QUANT_MAX_LEVELS == LMAX
    assert L.MAX_LINE_FUSED == l1.N1D_MAX
    for n in ("dwt_hip_lifting_norms", "dwt_hip_lifting_quant_steps", "dwt_hip_lifting1d_route"):
        assert n in dwt.NEVER_PREFILLED
    assert "dwt_hip_lifting1d_batch" not in dwt.NEVER_PREFILLED


def test_norm_code_under_asan_ubsan(tmp_path):
    """tests/san/san_lifting_norms.c: a stand-alone program around libdwt_amd/csrc/dwt_lifting_scheme.c, built with
    -fsanitize=address,undefined and run on the CPU; any report aborts it"""
    exe = tmp_path / "san_lifting_norms"
    subprocess.check_call(["gcc", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g",
                           "-O1", os.path.join(ROOT, "tests", "san", "san_lifting_norms.c"),
                           os.path.join(ROOT, "libdwt_amd", "csrc", "dwt_lifting_scheme.c"), "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "san_lifting_norms: OK" in out.stdout, out.stdout + out.stderr
