"""CPU checks of the deadzone quantizer's arithmetic as include/libdwt_hip.h specifies it (tests/quant_model.py), and of the
library's host entries (dwt_hip_quant_norms, dwt_hip_quant_steps, dwt_hip_codeblock_layout) against that model.  The device
entries are held to the same model in tests/test_hip_quant.py."""
import os

import numpy as np
import pytest

import quant_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
STEPS = [0.1, 1 / 3, 0.7, 2.5, 1e-3, 37.0]


@pytest.fixture(scope="module")
def dwt():
    import __graft_entry__ as g

    if not os.path.exists(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")):
        g.build()
    import libdwt_amd as d
    from libdwt_amd import quant

    d.quant = quant
    return d


@pytest.fixture(scope="module")
def indices():
    """2 * 10^6 indices with |q| < 2^20, the small magnitudes over-represented, the ends included"""
    rng = np.random.default_rng(2601)
    q = np.concatenate([rng.integers(-(1 << 20) + 1, 1 << 20, 1_500_000), rng.integers(-40, 41, 499_990),
                        [1, -1, 2, -2, (1 << 20) - 1, -(1 << 20) + 1, 0, 0, 3, -3]])
    return q.astype(np.int32)


@pytest.fixture(scope="module")
def gaussians():
    return np.random.default_rng(2602).normal(0, 1, 4_000_000).astype(F)


@pytest.mark.parametrize("r", [0.5, 0.375])
@pytest.mark.parametrize("step", STEPS)
def test_quantizing_a_reconstruction_returns_the_index(indices, step, r):
    """quantize(dequantize(q)) == q for every |q| < 2^20: (|q| + r) * step lies inside the cell of q, 2^-4 cells or more
    from its edges at these magnitudes, while the three roundings move it by less than 2^-22 of its value"""
    c = qm.dequantize(indices, F(step), r, qm.S)
    back, clipped = qm.quantize(c, F(step), qm.I32)
    assert np.array_equal(back, indices) and not clipped.any()


def test_offset_zero_is_legal_but_not_idempotent(indices):
    """r = 0 is inside [0, 1) and legal -- it is the reconstruction a decoder uses that has no estimate of the
    distribution inside the cell -- but it puts the value on the lower EDGE of the cell of q: |q| * step * (1 / step) is |q|
    only up to the roundings of the two products and of the reciprocal, and where it comes out below |q| truncation gives
    |q| - 1.  With step 0.7 that happens to a few per cent of the indices; with a step whose reciprocal is exact (a power of
    two) it cannot happen."""
    changed = (qm.quantize(qm.dequantize(indices, F(0.7), 0.0, qm.S), F(0.7), qm.I32)[0] != indices).mean()
    assert 0.02 < changed < 0.15, changed
    assert np.array_equal(qm.quantize(qm.dequantize(indices, F(0.25), 0.0, qm.S), F(0.25), qm.I32)[0], indices)


@pytest.mark.parametrize("step", STEPS)
def test_reconstruction_error_is_half_a_step(gaussians, step):
    """|c - dequantize(quantize(c))| <= step * (0.5 + 2^-10) where the index is not 0 (r = 0.5: the middle of a cell one step
    wide; the roundings of 1 / step, of the product and of the reconstruction move it by a few 2^-24 of |q| steps, and |q| stays
    below 2^13 here); inside the deadzone the index is 0, the reconstruction +0 and the error |c| < step"""
    c = gaussians
    q, clipped = qm.quantize(c, F(step), qm.I32)
    assert not clipped.any() and np.abs(q).max() < (1 << 13)
    back = qm.dequantize(q, F(step), 0.5, qm.S)
    err = np.abs(back.astype(np.float64) - c.astype(np.float64))
    nz = q != 0
    assert (err[nz] <= float(F(step)) * (0.5 + 2.0 ** -10)).all()
    assert (err[~nz] < float(F(step))).all() and (back[~nz].view(np.uint32) == 0).all()
    assert (np.signbit(back[nz]) == np.signbit(c[nz])).all()


def test_special_values():
    """+-0, subnormals, +-Inf, NaN; both sides of each saturation bound; INT32_MIN in the inverse"""
    one = F(1.0)
    c = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, np.nan, -np.nan, 0.99999994, -0.99999994, 1.0, -1.0], F)
    q, clipped = qm.quantize(c, one, qm.I32)
    assert q.tolist() == [0, 0, 0, 0, 0, 2147483647, -2147483647, 0, 0, 0, 0, 1, -1]
    assert clipped.tolist() == [False] * 5 + [True] * 4 + [False] * 4
    q16, clipped16 = qm.quantize(c, one, qm.I16)
    assert q16.tolist() == [0, 0, 0, 0, 0, 32767, -32767, 0, 0, 0, 0, 1, -1] and np.array_equal(clipped16, clipped)
    # a subnormal step: its reciprocal overflows, 0 * Inf is NaN -- index 0, counted as clipped
    assert [x.tolist() for x in qm.quantize(np.array([0.0, 1.0], F), F(1e-45), qm.I16)] == [[0, 32767], [True, True]]
    # the bounds: the largest float below 32768 and 32768 itself; below 2^31 and 2^31
    c = np.array([32767.998, 32768.0, -32767.998, -32768.0, 32767.0], F)
    q, clipped = qm.quantize(c, one, qm.I16)
    assert q.tolist() == [32767, 32767, -32767, -32767, 32767] and clipped.tolist() == [False, True, False, True, False]
    c = np.array([2147483520.0, 2147483648.0, -2147483520.0, -2147483648.0, 3e38], F)
    q, clipped = qm.quantize(c, one, qm.I32)
    assert q.tolist() == [2147483520, 2147483647, -2147483520, -2147483647, 2147483647]
    assert clipped.tolist() == [False, True, False, True, True]
    # the inverse: 0 gives +0 whatever r; INT32_MIN has the magnitude 2^31; INT16_MIN 2^15
    q = np.array([0, -2147483648, 2147483647, 1, -1], np.int32)
    v = qm.dequantize(q, F(0.5), 0.5, qm.S)
    assert v.view(np.uint32)[0] == 0 and v.tolist() == [0.0, -1073741824.0, 1073741824.0, 0.75, -0.75]
    v = qm.dequantize(np.array([-32768, 32767, 0], np.int16), F(2.0), 0.0, qm.S)
    assert v.tolist() == [-65536.0, 65534.0, 0.0]


def test_binary16_on_both_ends():
    """binary16 coefficients widen exactly (subnormals too) before the product; a binary16 destination rounds the binary32
    reconstruction once more, to nearest even, and overflows to Inf"""
    h = np.array([6e-8, -6e-8, 65504.0, -65504.0, 0.333251953125, np.inf, np.nan, -0.0], np.float16)
    q, clipped = qm.quantize(h, F(2.0 ** -24), qm.I32)
    assert q.tolist() == [1, -1, 2147483647, -2147483647, 5591040, 2147483647, 0, 0]
    assert clipped.tolist() == [False, False, True, True, False, True, True, False]
    same = qm.quantize(h.astype(F), F(2.0 ** -24), qm.I32)
    assert np.array_equal(q, same[0]) and np.array_equal(clipped, same[1])
    # (2049 + 0.5) * 1 = 2049.5 -> binary16 has a spacing of 2 there: 2050 is the nearer; (2048 + 0.5) -> 2048 (tie: even)
    v = qm.dequantize(np.array([2049, 2048, -2049, 70000, 0], np.int32), F(1.0), 0.5, qm.H)
    assert v.dtype == np.float16 and v.tolist() == [2050.0, 2048.0, -2050.0, np.inf, 0.0]
    # one rounding from binary32, not from the exact value: (4097 + 0.5) * 0.25 = 1024.375 is a binary32 value
    assert qm.dequantize(np.array([4097], np.int32), F(0.25), 0.5, qm.H).tolist() == [1024.0]


def test_band_counters_of_the_model():
    coef = np.zeros((1, 8, 8), F)
    coef[0, 0, 0], coef[0, 0, 4], coef[0, 7, 7], coef[0, 4, 0] = 100.0, -3.5, np.nan, 1e9
    q, stats = qm.quantize_frames(coef, np.ones(4, F), 1, qm.I16)
    assert q[0, 0, 0] == 100 and q[0, 0, 4] == -3 and q[0, 7, 7] == 0 and q[0, 4, 0] == 32767
    # HL (x >= 4, y < 4), LH, HH, LL
    assert stats[0].tolist() == [[1, 3, 0], [1, 32767, 1], [0, 0, 1], [1, 100, 0]]
    assert qm.bit_length(stats[0, :, 1]).tolist() == [2, 15, 0, 7]


def test_norms_reproduce_the_stated_figures():
    nl, nh = qm.norms(qm.CDF97, 6)
    for j, want_l, want_h in ((1, 0.991440, 1.020018), (2, 1.015186, 0.983471), (6, 1.029844, 1.043397)):
        assert abs(nl[j - 1] - want_l) < 1e-6 and abs(nh[j - 1] - want_h) < 1e-6, (j, nl[j - 1], nh[j - 1])
    # 5/3: the low-pass (1/2, 1, 1/2) / sqrt 2 and the high-pass (-1/8, -1/4, 3/4, -1/4, -1/8) sqrt 2, in the float constants
    nl, nh = qm.norms(qm.CDF53, 1)
    assert abs(nl[0] - np.sqrt(1.5) * float(F(0.70710678118654752440))) < 1e-12
    assert abs(nh[0] - np.sqrt(0.71875) * float(F(1.41421356237309504880))) < 1e-12
    # interpolating 5/3: the same low-pass; the high-pass is the sample itself, scaled
    nl, nh = qm.norms(qm.INTERP53, 1)
    assert abs(nl[0] - np.sqrt(1.5) * float(F(0.70710678118654752440))) < 1e-12 and abs(nh[0] - float(F(1.41421356237309504880))) < 1e-12


def wavelets(dwt):
    return ((dwt.CDF97_S, qm.CDF97), (dwt.CDF53_S, qm.CDF53), (dwt.INTERP53_S, qm.INTERP53))


def test_library_norms_equal_the_model(dwt):
    for wid, name in wavelets(dwt):
        nl, nh = dwt.quant.quant_norms(wid, 16)
        ml, mh = qm.norms(name, 16)
        assert np.allclose(nl, ml, rtol=1e-9, atol=0) and np.allclose(nh, mh, rtol=1e-9, atol=0), name
    assert dwt.quant.quant_norms(dwt.CDF97_S, 0)[0].shape == (0,)
    for bad in (dwt.CDF53_I, dwt.CDF97_D, dwt.CDF53_I16, dwt.CDF97_H, 77):
        with pytest.raises(dwt.DwtError):
            dwt.quant.quant_norms(bad, 3)
    for levels in (-1, 17):
        with pytest.raises(dwt.DwtError):
            dwt.quant.quant_norms(dwt.CDF97_S, levels)


def test_library_steps_equal_the_model(dwt):
    for wid, name in wavelets(dwt):
        for levels in (0, 1, 5, 16):
            for base in (1.0, 1 / 64, 0.3, 1e-6, 1e6):
                got, want = dwt.quant.quant_steps(wid, levels, base), qm.steps(name, levels, base)
                assert got.shape == want.shape == (3 * levels + 1,)
                ulp = np.spacing(np.abs(want))
                assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), (name, levels, base)
    # HL and LH of a level share their step; a coarser level of the 9/7 has its own
    s = dwt.quant.quant_steps(dwt.CDF97_S, 5, 1.0)
    assert all(s[3 * j] == s[3 * j + 1] != s[3 * j + 2] for j in range(5))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(dwt.DwtError):
            dwt.quant.quant_steps(dwt.CDF97_S, 3, bad)


SHAPES = [(37, 53, 3), (5, 7, -1), (64, 1, -1), (1, 64, -1), (1001, 9, -1), (1024, 8, 5), (130, 66, 0), (4096, 4096, 5)]


@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_model_geometry_is_the_librarys(dwt, W, H, j_max):
    assert dwt.band_levels(W, H, j_max) == qm.levels(W, H, j_max)
    assert np.array_equal(dwt.band_geometry(W, H, W, H, j_max), qm.geometry(W, H, j_max))
    if W * H < 1 << 20:
        qm.slot_map(W, H, j_max)  # asserts: every position in exactly one rectangle


@pytest.mark.parametrize("cbx, cby", [(2, 2), (6, 6), (10, 2), (5, 7)])
@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_codeblock_layout_counts_the_blocks(dwt, W, H, j_max, cbx, cby):
    """the totals equal a brute-force count from dwt_hip_band_geometry: every block holds a sample, every sample a block"""
    first, blocks_x = dwt.quant.codeblock_layout(W, H, j_max, cbx, cby)
    geo = dwt.band_geometry(W, H, W, H, j_max)
    assert len(first) == len(geo) + 1 and first[0] == 0
    for k, (x, y, w, h) in enumerate(geo):
        corners = {(i >> cbx, j >> cby) for i in range(0, w, 1 << cbx) for j in range(0, h, 1 << cby)}  # one sample per block
        assert first[k + 1] - first[k] == len(corners), k
        assert blocks_x[k] == (max(i for i, _ in corners) + 1 if corners else 0)
    mf, mb = qm.codeblock_layout(W, H, j_max, cbx, cby)
    assert np.array_equal(first, mf) and np.array_equal(blocks_x, mb)


def test_codeblock_layout_refusals(dwt):
    for cbx, cby in ((1, 6), (11, 1), (6, 7), (10, 3), (2, 11)):
        with pytest.raises(dwt.DwtError):
            dwt.quant.codeblock_layout(64, 64, 3, cbx, cby)
    with pytest.raises(dwt.DwtError):
        dwt.quant.codeblock_layout(-1, 64, 3, 6, 6)


def test_the_package_namespace_is_unchanged(dwt):
    import libdwt_amd

    assert not [n for n in ("quantize_batch", "dequantize_batch", "quant_steps", "quant_norms", "codeblock_layout") if n in vars(libdwt_amd)]
