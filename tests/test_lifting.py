"""CPU checks of the user-defined lifting wavelets (include/libdwt_hip.h).  The numpy model
(tests/lifting_model.py) fed the CDF tables must give the bits of the oracle's dwt_cdf97_2f_s, dwt_cdf53_2f_s,
dwt_cdf53_2f_i, dwt_cdf97_2f_i and of the restatement of dwt_interp53_2f_s (tests/interp53_model.py, itself pinned to the
reference); its D4 and Haar must give the bits the reference's cores gave (tests/golden/lifting.npz); int schemes are
reversible bit for bit; the library's check, built-in tables and reach (host code) agree with the model.  No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

import lifting_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lifting.npz")
ANCHOR_SHAPES = [(2, 2), (3, 5), (5, 3), (9, 17), (37, 53), (64, 64), (66, 130)]  # (W, H), both sides >= 2
ANCHORS = {"CDF97": "cdf97_2%s_s", "CDF53": "cdf53_2%s_s", "CDF53_INT": "cdf53_2%s_i", "CDF97_INT": "cdf97_2%s_i"}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def frames(s, B, H, W, seed):
    rng = np.random.default_rng([seed, B, H, W])
    if s.type == lm.I32:
        return rng.integers(-(1 << 15), (1 << 15) + 1, (B, H, W)).astype(np.int32)
    return rng.uniform(-1, 1, (B, H, W)).astype(np.float32)


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
    from libdwt_amd import lifting

    d.lifting = lifting
    return d


# ---- anchors -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("j_max", [-1, 1])
@pytest.mark.parametrize("W, H", ANCHOR_SHAPES)
@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_cdf_tables_give_the_oracles_bits(oracle, name, W, H, j_max):
    s = lm.builtin(name)
    x = frames(s, 1, H, W, 1)
    want = x[0].copy()
    J = oracle.fwd(ANCHORS[name] % "f", want, j_max)
    got, Jm = lm.fwd2d(s, x, j_max)
    assert Jm == J and same(got[0], want)
    back = want.copy()
    oracle.inv(ANCHORS[name] % "i", back, J)
    got_back, _ = lm.inv2d(s, got, J)
    assert same(got_back[0], back)


@pytest.mark.parametrize("j_max", [-1, 1])
@pytest.mark.parametrize("W, H", ANCHOR_SHAPES)
def test_interp53_table_gives_the_restatements_bits(W, H, j_max):
    import interp53_model as im

    s = lm.builtin("INTERP53")
    x = frames(s, 1, H, W, 2)
    want = x[0].copy()
    J = im.fwd2d(want, j_max=j_max)
    got, Jm = lm.fwd2d(s, x, j_max)
    assert Jm == J and same(got[0], want)
    back = want.copy()
    im.inv2d(back, j_max=J)
    assert same(lm.inv2d(s, got, J)[0][0], back)


# ---- the reference's cores (tests/golden/lifting.npz, scripts/gen_lifting_golden.py) -------------------------------------

def _golden():
    z = np.load(GOLDEN)
    return z, json.load(open(GOLDEN[:-4] + "_manifest.json"))


def test_golden_d4_matches_the_model_away_from_the_borders():
    """fdwt2_d4_sep_horiz / idwt2_d4_sep_horiz, one level, interleaved subbands: the reference truncates its steps at the
    borders where the model reflects, so the samples at least 4 away from every border are compared -- bit for bit"""
    z, man = _golden()
    s = lm.builtin("D4")
    cases = [c for c in man["cases"] if c["core"] == "d4"]
    assert {c["size"] for c in cases} == {32, 64}
    for c in cases:
        x, fwd, inv = z[c["key"] + "_in"], z[c["key"] + "_fwd"], z[c["key"] + "_inv"]
        r = x[None].copy()
        lm.level2d(s, r, False)
        m = man["margin"]
        assert m == 4 and same(r[0][m:-m, m:-m], fwd[m:-m, m:-m])
        r = fwd[None].copy()  # the inverse of the REFERENCE's coefficients
        lm.level2d(s, r, True)
        assert same(r[0][m:-m, m:-m], inv[m:-m, m:-m])


def test_golden_haar_matches_the_model_everywhere():
    """cores2f_haar_v2x2_f32 / cores2i_haar_v2x2_f32 on even sizes: Haar needs no border there, the whole frame is compared"""
    z, man = _golden()
    s = lm.builtin("HAAR")
    cases = [c for c in man["cases"] if c["core"] == "haar"]
    assert cases or man["haar_left_out"], "neither cases nor a reason"
    for c in cases:
        x, fwd, inv = z[c["key"] + "_in"], z[c["key"] + "_fwd"], z[c["key"] + "_inv"]
        r = x[None].copy()
        lm.level2d(s, r, False)
        assert same(r[0], fwd)
        r = fwd[None].copy()
        lm.level2d(s, r, True)
        assert same(r[0], inv)


# ---- properties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W, H, j_max", [(1, 1, -1), (1, 9, -1), (9, 1, -1), (2, 2, -1), (3, 5, -1), (17, 9, -1), (66, 130, -1), (65, 63, 1), (40, 24, 9)])
@pytest.mark.parametrize("which", ["CDF53_INT", "CDF97_INT", "HAAR_INT", "random 1", "random 2", "random 3"])
def test_int_schemes_are_reversible_bit_for_bit(which, W, H, j_max):
    """every int builtin and seeded random int schemes, on the whole int32 range (INT32_MIN and INT32_MAX among the samples):
    the wrapped values come back too"""
    s = lm.random_scheme(lm.I32, int(which.split()[1])) if which.startswith("random") else lm.builtin(which)
    rng = np.random.default_rng([3, W, H])
    x = rng.integers(-(1 << 31), 1 << 31, (2, H, W)).astype(np.int32)
    x.reshape(-1)[:2] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max][:x.size]
    y, J = lm.fwd2d(s, x, j_max)
    assert J == lm.levels(W, H, j_max)
    back, _ = lm.inv2d(s, y, J)
    assert same(back, x)
    if J and W * H > 4:
        assert not same(y, x)


@pytest.mark.parametrize("name", ["CDF97", "CDF53", "INTERP53", "HAAR", "D4"])
def test_float_builtins_round_trip(name):
    s = lm.builtin(name)
    x = frames(s, 2, 48, 80, 4)
    y, J = lm.fwd2d(s, x, 5)
    assert J == 5
    back, _ = lm.inv2d(s, y, J)
    assert np.abs(back.astype(np.float64) - x).max() <= 1e-5 * np.abs(x).max()


def test_d4_border_is_not_a_lifted_reflected_halo():
    """A halo filled by reflection once and then lifted like interior samples is right only for symmetric steps: with D4 the
    model's forward (every tap reflected at every step) differs from it near the borders, and only there -- so the border cases
    of the GPU tests are not vacuous."""
    s = lm.builtin("D4")
    x = frames(s, 1, 16, 16, 5)
    model = x.copy()
    lm.level2d(s, model, False)
    pad = 8  # even: parities stay; the padded array's own ends are more than the reach (3) away from the frame
    halo = np.pad(x, ((0, 0), (pad, pad), (pad, pad)), mode="reflect")
    lm.pass_lines(s, halo, False)
    t = np.ascontiguousarray(halo.transpose(0, 2, 1))
    lm.pass_lines(s, t, False)
    naive = np.ascontiguousarray(t.transpose(0, 2, 1)[:, pad:-pad, pad:-pad])
    differs = bits(naive) != bits(model)
    assert differs.any() and not differs[0, 4:-4, 4:-4].any()
    # the same construction is exact for a symmetric scheme
    c = lm.builtin("CDF97")
    model = x.copy()
    lm.level2d(c, model, False)
    halo = np.pad(x, ((0, 0), (pad, pad), (pad, pad)), mode="reflect")
    lm.pass_lines(c, halo, False)
    t = np.ascontiguousarray(halo.transpose(0, 2, 1))
    lm.pass_lines(c, t, False)
    assert same(np.ascontiguousarray(t.transpose(0, 2, 1)[:, pad:-pad, pad:-pad]), model)


def test_reflection_bounces_more_than_once():
    assert lm.reflect(np.arange(-7, 10), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert lm.reflect([-7, 8], 2).tolist() == [1, 0]
    # parity is kept
    for N in (2, 3, 4, 5, 8):
        i = np.arange(-20, 30)
        assert ((lm.reflect(i, N) - i) % 2 == 0).all()


# ---- the library's host code --------------------------------------------------------------------------------------------

def to_lib(L, s):
    """the model's scheme as the library's"""
    return L.scheme(s.type, [L.step(st.parity, st.terms, st.sign, st.add, st.shift) for st in s.steps], s.fwd_scale, s.inv_scale,
                    s.inverse_cols_first)


@pytest.mark.parametrize("name", sorted(lm.BUILTINS))
def test_builtin_tables_and_reach_of_the_library(dwt, name):
    L = dwt.lifting
    assert L.BUILTIN_IDS[name] == lm.IDS[name]
    s = L.builtin(name)
    assert s.table() == lm.builtin(name).table()
    assert L.check(s) == lm.builtin(name).reach
    assert to_lib(L, lm.builtin(name)).table() == s.table()
    assert L.builtin(lm.IDS[name]).table() == s.table()


@pytest.mark.parametrize("seed", range(6))
def test_reach_of_random_schemes(dwt, seed):
    L = dwt.lifting
    for t in (lm.F32, lm.I32):
        s = lm.random_scheme(t, seed)
        assert L.check(to_lib(L, s)) == s.reach
    assert L.check(to_lib(L, lm.random_scheme(lm.F32, seed, reach=8))) == 8


def test_check_refuses_malformed_schemes(dwt):
    L = dwt.lifting

    def refused(change, base="CDF97", word=None):
        s = L.builtin(base)
        change(s)
        with pytest.raises(dwt.DwtError) as e:
            L.check(s)
        msg = str(e.value)
        assert "lifting:" in msg and (word is None or word in msg), msg

    refused(lambda s: setattr(s.steps[1].terms[0], "off_a", 2), word="off_a")          # an even offset
    refused(lambda s: setattr(s.steps[1].terms[0], "off_a", 0), word="off_a")          # no first tap
    refused(lambda s: setattr(s.steps[2].terms[0], "off_b", 9), word="off_b")          # offset 9
    refused(lambda s: setattr(s.steps[2].terms[0], "off_b", -4), word="off_b")
    refused(lambda s: setattr(s.steps[0], "n_terms", 0), word="terms")                 # 0 terms
    refused(lambda s: setattr(s.steps[0], "n_terms", 5), word="terms")
    refused(lambda s: setattr(s, "n_steps", 9), word="steps")                          # 9 steps
    refused(lambda s: setattr(s, "n_steps", 0), word="steps")
    refused(lambda s: setattr(s, "inverse_cols_first", 0), "CDF53_INT", word="inverse_cols_first")  # an int scheme that is no mirror
    refused(lambda s: setattr(s.steps[3].terms[0], "coef", float("nan")), word="finite")  # a NaN coefficient
    refused(lambda s: setattr(s.steps[3].terms[0], "coef", float("inf")), word="finite")
    refused(lambda s: s.fwd_scale.__setitem__(1, float("nan")), word="scale")
    refused(lambda s: setattr(s, "type", 2), word="type")
    refused(lambda s: setattr(s.steps[0], "parity", 2), word="parity")
    refused(lambda s: setattr(s.steps[0], "sign", 0), "CDF97_INT", word="sign")
    refused(lambda s: setattr(s.steps[0], "shift", 32), "CDF97_INT", word="shift")
    with pytest.raises(dwt.DwtError):
        L.builtin(8)
    assert L.check(L.builtin("D4")) == 3  # (a refusal does not stick)


def test_constants_and_namespace(dwt):
    import re

    import libdwt_amd

    L = dwt.lifting
    assert (L.F32, L.I32, L.MAX_STEPS, L.MAX_TERMS, L.MAX_OFFSET, L.FUSED_REACH) == (lm.F32, lm.I32, lm.MAX_STEPS, lm.MAX_TERMS, lm.MAX_OFFSET, lm.FUSED_REACH)
    header = open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()
    for name, value in (("MAX_STEPS", L.MAX_STEPS), ("MAX_TERMS", L.MAX_TERMS), ("MAX_OFFSET", L.MAX_OFFSET), ("FUSED_REACH", L.FUSED_REACH),
                        ("MAX_BATCH", L.MAX_BATCH)):
        assert re.search(r"#define DWT_HIP_LIFT_%s %d\s" % (name, value), header), name
    assert not [n for n in ("builtin", "check", "lifting2d_batch", "route", "scheme", "step", "Scheme") if n in vars(libdwt_amd)]


def test_scheme_code_under_asan_ubsan(tmp_path):
    """tests/san/san_lifting.c: a stand-alone program around libdwt_amd/csrc/dwt_lifting_scheme.c, built with
    -fsanitize=address,undefined and run on the CPU; any report aborts it"""
    exe = tmp_path / "san_lifting"
    subprocess.check_call(["gcc", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g",
                           "-O1", os.path.join(ROOT, "tests", "san", "san_lifting.c"), os.path.join(ROOT, "libdwt_amd", "csrc", "dwt_lifting_scheme.c"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "san_lifting: OK" in out.stdout, out.stdout + out.stderr
