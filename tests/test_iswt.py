"""CPU checks of tests/iswt_model.py, the model of the stationary transform under the symmetric border and of its inverse
(DESIGN.md s29): under the replicated border it is swt_model / swt2d_model bit for bit; under the symmetric one it is the
reference's coefficients wherever no border is reached; the planes of a symmetrically extended input are symmetric; the
float32 round trip stays within the bounds the GPU tests hold the device to; operators on load equal operators on the
stored plane."""
import ctypes as C
import os

import numpy as np
import pytest

import iswt_model as im
import swt2d_model as m2
import swt_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
GOLD1, GOLD2 = np.load(sm.GOLDEN), np.load(m2.GOLDEN)
# the round-trip bounds, relative to max|x|: 3.4 x and 3.8 x the largest float32 errors of the model when the bounds were set
# (2.9e-7 and 5.2e-7; the cases below give 2.9e-7 and 4.0e-7); the float64 restatement -- the share of the 8-digit filter
# literals -- stays below 3e-7 (1.7e-7 and 2.5e-7 here)
BOUND_1D, BOUND_2D, BOUND_F64 = 1e-6, 2e-6, 3e-7
# The sizes are paired with depths as swt_model.CASES and swt2d_model.CASES pair theirs.  The literals' share is a gain error
# per level (at DC: gl.sl + gh.sh = 2 (1 + 2.8e-8) for 5/3), and a line of one to three samples is all DC at every dilation,
# so its error grows by that much with every level and every direction: the tiny sizes take the few levels they take there
# (1 x 1 at two levels is 4 x 5.5e-8 = 2.2e-7 in float64 already).
ROUND_TRIP_1D = [(1, 3), (2, 3), (3, 4), (7, 5), (100, 10), (257, 10), (4096, 4)]  # (N, levels)
ROUND_TRIP_2D = [(1, 1, 2), (1, 9, 3), (5, 3, 3), (37, 300, 7), (70, 41, 5), (256, 256, 4)]  # (rows, columns, levels)


def test_reflect():
    assert im.reflect(np.arange(-7, 8), 1).tolist() == [0] * 15
    assert im.reflect(np.arange(-5, 6), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert im.reflect(np.arange(-6, 11), 4).tolist() == [0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]


def test_synthesis_filters():
    """alternating signs around the centre; with the analysis filters they satisfy the undecimated reconstruction identity
    gl * sl + gh * sh = 2 delta to the precision of the 8-digit literals"""
    for w in sm.WAVELETS:
        gl, gh = sm.FILTERS[w]
        sl, sh = im.synthesis(w)
        assert len(sl) == len(gh) and len(sh) == len(gl)
        assert np.array_equal(np.abs(sl), np.abs(gh)) and np.array_equal(np.abs(sh), np.abs(gl))
        assert sl[len(sl) // 2] == gh[len(gh) // 2] and sh[len(sh) // 2] == gl[len(gl) // 2] and sl[len(sl) // 2 - 1] == -gh[len(gh) // 2 - 1]
        total = np.convolve(gl.astype(F64), sl.astype(F64)) + np.convolve(gh.astype(F64), sh.astype(F64))
        delta = np.zeros_like(total)
        delta[len(total) // 2] = 2
        assert np.abs(total - delta).max() < 2e-7


@pytest.mark.parametrize("i", range(len(sm.CASES)))
def test_replicate_equals_swt_model(i):
    seed, wavelet, kind, n, levels = sm.CASES[i]
    x = sm.make_input(seed, kind, 1, n)[0]
    L, H = im.swt_levels(x, wavelet, levels, im.REPLICATE)
    L0, H0 = sm.swt_levels(x, wavelet, levels)
    assert sm.same(L, L0) and sm.same(H, H0)


@pytest.mark.parametrize("i", range(len(m2.CASES)))
def test_replicate_equals_swt2d_model(i):
    seed, wavelet, kind, size_y, size_x, levels = m2.CASES[i]
    x = m2.make_input(seed, kind, size_y, size_x)
    LL, D = im.swt2d_levels(x, wavelet, levels, im.REPLICATE)
    LL0, D0 = m2.swt2d_levels(x, wavelet, levels)
    assert sm.same(LL, LL0) and sm.same(D, D0)


def test_symmetric_equals_reference_in_the_interior():
    """only the border reach differs from the reference: plane l is compared wherever l + 1 levels of the longer filter
    reach no border (which holds every J > l of the issue's J-level interior too)"""
    nonempty = {w: 0 for w in sm.WAVELETS}
    for i, (seed, wavelet, kind, n, levels) in enumerate(sm.CASES):
        L, H = im.swt_levels(sm.make_input(seed, kind, 1, n)[0], wavelet, levels, im.SYMMETRIC)
        for l in range(levels):
            s = im.interior(n, l + 1, wavelet)
            assert sm.same(L[l, s], GOLD1["L_%d" % i][l, s]) and sm.same(H[l, s], GOLD1["H_%d" % i][l, s]), (i, l)
            nonempty[wavelet] += s.stop > s.start
    assert all(nonempty.values()), nonempty
    nonempty = {w: 0 for w in sm.WAVELETS}
    for i, (seed, wavelet, kind, size_y, size_x, levels) in enumerate(m2.CASES):
        LL, D = im.swt2d_levels(m2.make_input(seed, kind, size_y, size_x), wavelet, levels, im.SYMMETRIC)
        for l in range(levels):
            sy, sx = im.interior(size_y, l + 1, wavelet), im.interior(size_x, l + 1, wavelet)
            assert sm.same(D[l][:, sy, sx], GOLD2["D_%d" % i][l][:, sy, sx]), (i, l)
            if l == levels - 1:
                assert sm.same(LL[l][sy, sx], GOLD2["LL_%d" % i][sy, sx]), (i, l)
            nonempty[wavelet] += sy.stop > sy.start and sx.stop > sx.start
    assert all(nonempty.values()), nonempty


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_plane_symmetry(wavelet):
    """the input extended by hand by the whole reach of the transform, CL * (2^levels - 1) samples to either side, and
    transformed under the replicated border (which the middle never sees): over the input's own samples every plane equals
    the symmetric-border plane of the plain input.  Levels beyond the first hold only if the planes of an extended input
    are themselves symmetric -- what lets the inverse extend them the same way.  Level 0 reads the same values in the same
    order and is equal bit for bit.  A deeper level reads a mirrored sample of the plane before it, which the hand-extended
    transform summed with its taps in the mirrored order: equal as real numbers, not as float32 sums.  So the deeper levels
    are held in float64, within 1e-12 max|x|: 9 taps x 2^-53 x the low-pass gain of at most 1.96 per level x 5 levels is
    1.4e-13."""
    for n, levels in ((1, 3), (2, 3), (7, 4), (33, 5), (100, 3)):
        x = sm.make_input(70 + n, "normal", 1, n)[0]
        reach = (len(sm.FILTERS[wavelet][0]) // 2) * ((1 << levels) - 1)
        ext = x[im.reflect(np.arange(-reach, n + reach), n)]
        Le, He = sm.swt_levels(ext, wavelet, 1)
        L, H = im.swt_levels(x, wavelet, 1, im.SYMMETRIC)
        assert sm.same(Le[:, reach:reach + n], L) and sm.same(He[:, reach:reach + n], H), n
        Le, He = im.swt_levels(ext, wavelet, levels, im.REPLICATE, F64)
        L, H = im.swt_levels(x, wavelet, levels, im.SYMMETRIC, F64)
        tol = 1e-12 * np.abs(x).max()
        assert np.abs(Le[:, reach:reach + n] - L).max() <= tol and np.abs(He[:, reach:reach + n] - H).max() <= tol, n


def _rel(a, b, x):
    return float(np.abs(a.astype(F64) - b.astype(F64)).max() / np.abs(x).max())


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_round_trip_1d(wavelet):
    for n, levels in ROUND_TRIP_1D:
        x = sm.make_input(9000 + n + levels, "normal", 2, n)
        L, H = im.swt_levels(x, wavelet, levels)
        e32 = _rel(im.iswt_levels(L[-1], H, wavelet), x, x)
        L64, H64 = im.swt_levels(x, wavelet, levels, dtype=F64)
        e64 = _rel(im.iswt_levels(L64[-1], H64, wavelet, dtype=F64), x, x)
        print("1-D %s N %d levels %d: float32 %.2e float64 %.2e" % (wavelet, n, levels, e32, e64))
        assert e32 <= BOUND_1D and e64 < BOUND_F64, (n, levels, e32, e64)


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_round_trip_2d(wavelet):
    for h, w, levels in ROUND_TRIP_2D:
        x = m2.make_input(9100 + h + w, "normal", h, w)
        LL, D = im.swt2d_levels(x, wavelet, levels)
        e32 = _rel(im.iswt2d_levels(LL[-1], D, wavelet), x, x)
        LL64, D64 = im.swt2d_levels(x, wavelet, levels, dtype=F64)
        e64 = _rel(im.iswt2d_levels(LL64[-1], D64, wavelet, dtype=F64), x, x)
        print("2-D %s %d x %d levels %d: float32 %.2e float64 %.2e" % (wavelet, h, w, levels, e32, e64))
        assert e32 <= BOUND_2D and e64 < BOUND_F64, (h, w, levels, e32, e64)


def tables(n, shift=0):
    """one operator and one parameter per plane: every code on load, mixed"""
    codes = [im.SOFT, im.KEEP, im.ZERO, im.SCALE, im.HARD]
    ops = np.array([codes[(i + shift) % 5] for i in range(n)], np.int32)
    params = np.array([{im.SOFT: 0.4, im.HARD: 0.7, im.SCALE: -1.75}.get(int(o), 0.0) for o in ops], F32)
    return ops, params


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_operators_on_load(wavelet):
    """operators on load equal the operator on the stored plane followed by the plain inverse, NaN included"""
    levels = 5
    x = sm.make_input(77, "float_range", 2, 100)
    L, H = im.swt_levels(x, wavelet, levels)
    ops, params = tables(levels)
    shaped = np.stack([im.shp.apply_op(H[l], ops[l], params[l]) for l in range(levels)])
    assert sm.same(im.iswt_levels(L[-1], H, wavelet, ops, params), im.iswt_levels(L[-1], shaped, wavelet))
    poisoned = H.copy()
    poisoned[ops == im.ZERO] = np.nan  # a ZERO plane is never read
    assert sm.same(im.iswt_levels(L[-1], poisoned, wavelet, ops, params), im.iswt_levels(L[-1], shaped, wavelet))
    levels = 3
    x2 = m2.make_input(78, "normal", 20, 31)
    LL, D = im.swt2d_levels(x2, wavelet, levels)
    ops, params = tables(3 * levels, 1)
    shaped = np.stack([np.stack([im.shp.apply_op(D[l, k], ops[3 * l + k], params[3 * l + k]) for k in range(3)]) for l in range(levels)])
    assert sm.same(im.iswt2d_levels(LL[-1], D, wavelet, ops, params), im.iswt2d_levels(LL[-1], shaped, wavelet))
    with pytest.raises(ValueError):
        im.iswt_levels(L[-1], H[:1], wavelet, [im.COMPRESS], [0.5])


def test_abi_exports():
    lib = C.CDLL(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so"))
    for s in ("dwt_hip_swt1d_batch_ex", "dwt_hip_swt2d_batch_ex", "dwt_hip_iswt1d_batch", "dwt_hip_iswt2d_batch"):
        assert hasattr(lib, s), s
    import libdwt_amd as dwt
    from libdwt_amd import stationary as st

    for s in ("swt1d_batch", "swt2d_batch", "iswt1d_batch", "iswt2d_batch"):
        assert callable(getattr(st, s)), s
        assert s.startswith("swt") or not hasattr(dwt, s), s  # the package namespace keeps to its table (tests/test_hip_streams.py)
    assert (st.BORDER_REPLICATE, st.BORDER_SYMMETRIC, st.ISWT2D_FUSED_LEVELS) == (0, 1, 5)
    with open(os.path.join(ROOT, "include", "libdwt_hip.h")) as f:
        header = f.read()
    assert "#define DWT_HIP_ISWT2D_FUSED_LEVELS %d" % st.ISWT2D_FUSED_LEVELS in header


def test_argument_errors():
    """refused before any device is touched, the destination untouched"""
    from libdwt_amd import stationary as st
    import libdwt_amd as dwt

    n, lines, levels = 32, 3, 2
    h, l = np.zeros((levels, lines, n), F32), np.zeros((lines, n), F32)
    dst = np.full((lines, n), -7.5, F32)
    good = dict(wavelet="cdf97_s", border=st.BORDER_SYMMETRIC, src_h=h, src_l=l, plane_stride=4 * n * lines, src_line_stride=4 * n, n_lines=lines,
                size=n, levels=levels, dst=dst, dst_line_stride=4 * n)
    bad = [dict(border=st.BORDER_REPLICATE), dict(border=2), dict(wavelet="cdf53_i"), dict(levels=25), dict(levels=-1),
           dict(ops=[st.BAND_COMPRESS, st.BAND_KEEP], params=[0.5, 0]), dict(ops=[9, 0], params=[0, 0]), dict(ops=[st.BAND_SOFT, 0]),
           dict(dst=h[0]), dict(dst=l), dict(src_line_stride=4 * n - 4), dict(dst_elem_stride=2), dict(plane_stride=4 * n)]
    for i, kw in enumerate(bad):
        with pytest.raises(dwt.DwtError) as e:
            st.iswt1d_batch(**dict(good, **kw))
        assert len(str(e.value)) > 10, i
    assert "reconstruct" in str(pytest.raises(dwt.DwtError, st.iswt1d_batch, **dict(good, border=0)).value)
    W, H, B = 16, 6, 2
    d, ll = np.zeros((B, 3 * levels, H, W), F32), np.zeros((B, 3 * levels, H, W), F32)
    out = np.full((B, H, W), -7.5, F32)
    good2 = dict(wavelet="cdf53_s", border=1, src_h=d, src_l=ll, src_batch_stride=3 * levels * 4 * W * H, plane_stride=4 * W * H, src_stride_x=4 * W,
                 batch=B, size_x=W, size_y=H, levels=levels, dst=out, dst_batch_stride=4 * W * H, dst_stride_x=4 * W)
    bad2 = [dict(border=0), dict(wavelet="cdf97_d"), dict(levels=25), dict(ops=[st.BAND_COMPRESS] * 6, params=[0.5] * 6), dict(dst=d), dict(batch=0),
            dict(size_x=0), dict(src_stride_x=4 * W - 4), dict(plane_stride=4 * W * H - 4), dict(dst_batch_stride=4 * W * H - 4), dict(dst_stride_y=2)]
    for i, kw in enumerate(bad2):
        with pytest.raises(dwt.DwtError) as e:
            st.iswt2d_batch(**dict(good2, **kw))
        assert len(str(e.value)) > 10, i
    with pytest.raises(dwt.DwtError):
        st.swt1d_batch("cdf97_s", l, 4 * n, 4, lines, n, levels, h, border=2)
    assert (dst == F32(-7.5)).all() and (out == F32(-7.5)).all() and not h.any() and not d.any()
