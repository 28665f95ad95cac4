"""Every instantiation of the fused 4-byte tile sweeps at the shapes where a tile sweep can go wrong: fwd_launch<W, CPT in
{4, 8}, RING in {8, 16}, NT in {3, 7, 15}> and inv_launch<W, CPT, RING in {8, 16}, NT in {0, 1}> for the six wavelet policies
(Cdf97S, Cdf53S, Cdf53I, Cdf97I, Interp53S, Cdf97SFma), under every tile height, wave count and block order -- 72 forward and
36 inverse (policy, CPT, RING, NT) combinations, each at six shapes.

Shapes (h, w):
  (131, 1030)  5 tiles of 256 or 3 of 512 columns, the last 6 wide; one wave of a side-by-side workgroup has no tile;
               66 row pairs; the levels go down to 2 x 9
  (67, 259)    the last tile 3 columns wide; level 1 below 64 rows
  (40, 513)    one column past a 512-column tile; fewer than 64 rows at level 0
  (12, 256)    one full tile, the last column lane 63's last; the level shorter than a 16-row ring
  (9, 257)     the last column lane 0's first, in a tile of its own
  (5, 1541)    reflection with several bounces; 7 tiles at level 0 and 4 at level 1

Inputs: tests/floatends.py `finite_floats` at full depth (every bit compared) and `ends_floats` at the depth of
floatends.ends_level (values above MAX/2 next to the line ends: the int-free policies' end forms under every variant);
conftest.full_range_ints for the int policies (their end_mask forms under the wave-shift taps).  The forward matrix runs on
the input, the inverse matrix on the expected coefficients -- for `ends`, as everywhere with that class, on the input itself
read as coefficients.  Expectation: the oracle's bits (interp53: its model's, as tests/test_hip_interp53.py); `fma` = 1: the
bits of its own ring 8, nt 7, cpt 4 result, that one within 1e-5 of the oracle as tests/test_hip_float_range.py holds it.

Then: the launcher's own choice of the deep ring on a batch of 800 short wide images, the in-place device entry under
settings that forbid a riding copy, fuse01 = 2 under settings that have no fused kernel, and the 3-D knobs no test sets."""
import itertools
import os
import warnings

import numpy as np
import pytest

import floatends as F
import interp53_model as M53
from conftest import bits, full_range_ints, same_floats

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

PLAIN_BUILD = os.path.basename(os.environ.get("DWT_HIP_LIB", "")).startswith("libdwt_hip_plain")
KNOBS = ("cpt", "ring", "nt", "tile_pairs", "waves", "xcd_swizzle", "ring_inv", "inv_ll_temporal", "fma", "fuse01", "ride_copy",
         "vol_nt", "vol_swizzle", "vol_fused", "vol_tile_pairs")
# wavelet row -> (library wavelet, oracle entry of floatends.transform or the int entries, dtype, classes)
WAVELETS = {
    "cdf97_s": ("cdf97_s", "cdf97_s", np.float32, ("finite", "ends")),
    "cdf53_s": ("cdf53_s", "cdf53_s", np.float32, ("finite", "ends")),
    "cdf53_i": ("cdf53_i", ("cdf53_2f_i", "cdf53_2i_i"), np.int32, ("ints",)),
    "cdf97_i": ("cdf97_i", ("cdf97_2f_i", "cdf97_2i_i"), np.int32, ("ints",)),
    "interp53_s": ("interp53_s", "interp53_2d", np.float32, ("finite", "ends")),
    "cdf97_s_fma": ("cdf97_s", "cdf97_s", np.float32, ("finite", "ends")),
}
FWD_MATRIX = [dict(cpt=c, ring=r, nt=n, tile_pairs=t, waves=w, xcd_swizzle=s)
              for c, r, n, t, w in itertools.product((4, 8), (8, 16), (3, 7, 15), (0, 8, 64), (1, 4)) for s in ((0, 1) if w == 4 else (1,))]
INV_MATRIX = [dict(cpt=c, ring_inv=r, tile_pairs=t, waves=w, inv_ll_temporal=l)
              for c, r, t, w, l in itertools.product((4, 8), (8, 16), (0, 8, 64), (1, 4), (0, 1))]
DEFAULTS = {}  # knob -> the library's own value, read before the first test sets any
FMA_BASE = dict(cpt=4, ring=8, nt=7, tile_pairs=0, waves=4, xcd_swizzle=1, ring_inv=8, inv_ll_temporal=1)


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    DEFAULTS.update({k: d.get_option(k) for k in KNOBS})
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    restore(d)
    d.dwt_util_finish()


def restore(dwt):
    """Every knob this file touches back to what the library started with."""
    for k, v in DEFAULTS.items():
        dwt.set_option(k, v)


def checker(oracle, entry, inverse, a, j):
    """(expected result, level count) of one direction by the oracle / the interp53 model."""
    if isinstance(entry, tuple):
        b = a.copy()
        return b, (oracle.inv if inverse else oracle.fwd)(entry[inverse], b, j)
    with (F.reflected_ends(oracle) if PLAIN_BUILD else warnings.catch_warnings()):
        return F.transform(oracle, entry, inverse, a, j)


def make_case(oracle, wname, shape, klass):
    """(input, j, expected forward, the inverse's input, expected inverse)."""
    _, entry, dt, _ = WAVELETS[wname]
    rng = np.random.default_rng(shape[0] * 4099 + shape[1])
    if klass == "ints":
        a, j = full_range_ints(rng, shape), -1
    elif klass == "finite":
        a, j = F.finite_floats(rng, shape, dt), -1
    else:
        a = F.ends_floats(rng, shape, dt)
        j = F.ends_level(oracle, entry, a)
    want_f, jo = checker(oracle, entry, 0, a, j)
    coef = a if klass == "ends" else want_f
    want_i, _ = checker(oracle, entry, 1, coef, jo)
    if klass == "finite":
        assert np.isfinite(want_f).all() and np.isfinite(want_i).all()
    if klass == "ends" and not PLAIN_BUILD:
        assert max(F.nan_share(want_f), F.nan_share(want_i)) <= F.NAN_CAP
    return a, j, jo, want_f, coef, want_i


def same(got, want):
    return np.array_equal(bits(got), bits(want)) if got.dtype == np.int32 else same_floats(got, want)


def within_fma_bound(got, want):
    """tests/test_hip_float_range.py, test_fma_option_over_the_whole_float_range: 1e-5 of the largest coefficient on the
    samples finite on both sides; a contracted step may stay finite where mul-then-add overflowed, so at least half of the
    finite samples must be."""
    both = np.isfinite(got) & np.isfinite(want)
    if both.sum() < 0.5 * np.isfinite(want).sum():
        return False
    if not both.any():
        return True
    g, w_ = got[both].astype(np.float64), want[both].astype(np.float64)
    return np.abs(g - w_).max() <= 1e-5 * max(np.abs(w_).max(), float(np.finfo(np.float32).tiny))


CASES = [pytest.param(w, s, k, id="%s-%dx%d-%s" % (w, s[0], s[1], k)) for w in WAVELETS for s in F.SWEEP_SHAPES for k in WAVELETS[w][3]]


@pytest.mark.parametrize("wname,shape,klass", CASES)
def test_every_sweep_instantiation_at_the_edge_shapes(dwt, oracle, wname, shape, klass):
    lib_w, _, dt, _ = WAVELETS[wname]
    fma = wname.endswith("_fma")
    h, w = shape
    a, j, jo, want_f, coef, want_i = make_case(oracle, wname, shape, klass)
    wid = dwt.WAVELET_ID[lib_w]
    poison = np.full(shape, 7, dt)
    src_f, src_i, dst = dwt.DeviceImage(h, w).upload(a), dwt.DeviceImage(h, w).upload(coef), dwt.DeviceImage(h, w)

    def run(inverse, opts):
        for k, v in opts.items():
            dwt.set_option(k, v)
        dst.upload(poison)
        src = src_i if inverse else src_f
        if inverse:
            dwt._inv(wid, src.ptr, dst.ptr, dst.stride_x, 4, w, h, w, h, jo, 0, 0, "inv")
        else:
            assert dwt._fwd(wid, src.ptr, dst.ptr, dst.stride_x, 4, w, h, w, h, j, 0, 0, "fwd") == jo
        return dst.download(dt)

    try:
        dwt.set_option("fma", int(fma))
        if fma:
            base_f, base_i = run(0, FMA_BASE), run(1, FMA_BASE)
            if klass == "finite":
                assert np.isfinite(base_f).all() and np.isfinite(base_i).all()
            assert within_fma_bound(base_f, want_f) and within_fma_bound(base_i, want_i)
            want_f, want_i = base_f, base_i
        for opts in FWD_MATRIX:
            got = run(0, opts)
            assert same(got, want_f), ("forward", opts, F.telling(got, want_f) if dt != np.int32 else None)
        restore(dwt)
        dwt.set_option("fma", int(fma))
        for opts in INV_MATRIX:
            got = run(1, opts)
            assert same(got, want_i), ("inverse", opts, F.telling(got, want_i) if dt != np.int32 else None)
        assert np.array_equal(bits(src_f.download(dt)), bits(a)) and np.array_equal(bits(src_i.download(dt)), bits(coef)), "source modified"
    finally:
        restore(dwt)
        for d in (src_f, src_i, dst):
            d.free()


# ---- the launcher's own choice of the deep ring --------------------------------------------------------------------------
def deep_ring(ntx, nty, batch, waves=4):
    """fwd_level_t's rule, restated: the 16-row ring where a row of tiles has a tile for every wave of a workgroup and the
    launch has 3072 tiles or more."""
    return ntx >= waves and ntx * nty * batch >= 3072


@pytest.mark.parametrize("wname", list(WAVELETS))
def test_a_batch_of_short_wide_images_takes_the_deep_ring_by_itself(dwt, oracle, wname):
    """800 images of 7 x 1541, 3 levels, no option set: levels 0 and 1 (7 and 4 tiles of 256 columns in a row, one tile row:
    5600 and 3200 tiles) take the deep ring with side-by-side waves, level 2 (2 tiles in a row) the shallow one -- at levels of
    7, 4 and 2 rows, shorter than either ring.  Rows padded by 3 elements, images by 64, the padding a NaN pattern that must
    stay.  Forward and inverse through dwt_hip_transform2d_batch."""
    nb, h, w, J = 800, 7, 1541, 3
    for lvl, deep in ((0, True), (1, True), (2, False)):
        wl, hl = F_ceil(w, lvl), F_ceil(h, lvl)
        # W < 2048: 4 columns per lane, tiles of 256; the tile heights pick_tile_pairs gives these levels (64, 4 and 2 row
        # pairs for more than 4 Mi, more than 1 Mi and fewer samples a launch) cover their 4, 2 and 1 row pairs: one tile row
        tp = 64 if wl * hl * nb > (4 << 20) else 4 if wl * hl * nb > (1 << 20) else 2
        ntx, nty = (wl + 255) // 256, ((hl + 1) // 2 + tp - 1) // tp
        assert nty == 1 and deep_ring(ntx, nty, nb) == deep, lvl
    assert [(F_ceil(w, lvl) + 255) // 256 for lvl in (0, 1)] == [7, 4]
    lib_w, entry, dt, _ = WAVELETS[wname]
    fma = wname.endswith("_fma")
    rng = np.random.default_rng(800)
    imgs = (full_range_ints(rng, (nb * h, w)) if dt == np.int32 else F.finite_floats(rng, (nb * h, w), dt)).reshape(nb, h, w)
    want_f, want_i = np.empty_like(imgs), np.empty_like(imgs)
    if entry == "interp53_2d":  # (the model takes the batch as one stack of lines per direction: 800 calls of it are slow)
        want_f = interp53_batch(imgs, J, False)
        want_i = interp53_batch(want_f, J, True)
    else:
        for b in range(nb):
            want_f[b], jo = checker(oracle, entry, 0, imgs[b], J)
            assert jo == J
            want_i[b], _ = checker(oracle, entry, 1, want_f[b], J)
    pitch, bstride = w + 3, (w + 3) * h + 64
    pad = np.array([0x7fc01234], np.uint32).view(dt)[0]
    host = np.full((nb, bstride), pad, dt)
    view = host[:, :pitch * h].reshape(nb, h, pitch)
    L = dwt.lib
    src, dst = L.dwt_hip_malloc(host.nbytes), L.dwt_hip_malloc(host.nbytes)
    try:
        dwt.set_option("fma", int(fma))
        got = np.empty_like(host)
        for inverse, inp, want in ((0, imgs, want_f), (1, want_f, want_i)):
            view[:, :, :w] = inp
            assert L.dwt_hip_memcpy_h2d(src, host.ctypes.data, host.nbytes) == 0
            view[:, :, :w] = pad
            assert L.dwt_hip_memcpy_h2d(dst, host.ctypes.data, host.nbytes) == 0
            assert dwt.transform2d_batch(lib_w, inverse, src, dst, bstride * 4, nb, pitch * 4, w, h, J) == J
            assert L.dwt_hip_memcpy_d2h(got.ctypes.data, dst, got.nbytes) == 0
            out = got[:, :pitch * h].reshape(nb, h, pitch)
            assert np.all(bits(out[:, :, w:]) == 0x7fc01234) and np.all(bits(got[:, pitch * h:]) == 0x7fc01234), "padding written"
            res = np.ascontiguousarray(out[:, :, :w])
            if fma:
                assert np.isfinite(res).all() and within_fma_bound(res, want), inverse
            else:
                assert np.array_equal(bits(res), bits(want)), ("inverse" if inverse else "forward", int((bits(res) != bits(want)).sum()))
    finally:
        restore(dwt)
        L.dwt_hip_free(src)
        L.dwt_hip_free(dst)


def F_ceil(n, j):
    return (n + (1 << j) - 1) >> j


def interp53_batch(imgs, J, inverse):
    """tests/interp53_model.py level by level on a whole batch of dense images at once (its line functions take any
    number of lines): rows then columns forward, the inverse of that backwards."""
    nb, h, w = imgs.shape
    a = imgs.copy()

    def lines(x, N, hoff):
        # x: (lines, samples); samples [0, N) <-> L at [0, ceil(N/2)), H at hoff
        (M53._inv_rows if inverse else M53._fwd_rows)(x, x.shape[0], N, hoff)

    levels = range(J, 0, -1) if inverse else range(J)
    for lv in levels:
        j = lv - 1 if inverse else lv
        ws, hs = F_ceil(w, j), F_ceil(h, j)
        wd, hd = F_ceil(w, j + 1), F_ceil(h, j + 1)
        # (forward: every row of the level, then every column; the reference's inverse runs the same order)
        r = np.ascontiguousarray(a[:, :hs, :].reshape(nb * hs, w))
        lines(r, ws, wd)
        a[:, :hs, :] = r.reshape(nb, hs, w)
        c = np.ascontiguousarray(a[:, :, :ws].transpose(0, 2, 1).reshape(nb * ws, h))
        lines(c, hs, hd)
        a[:, :, :ws] = c.reshape(nb, ws, h).transpose(0, 2, 1)
    return a


def test_interp53_batch_model_is_the_model():
    rng = np.random.default_rng(3)
    imgs = F.finite_floats(rng, (3 * 7, 1541)).reshape(3, 7, 1541)
    f = interp53_batch(imgs, 3, False)
    i = interp53_batch(f, 3, True)
    for b in range(3):
        want = imgs[b].copy()
        assert M53.fwd2d(want, j_max=3) == 3 and np.array_equal(bits(f[b]), bits(want))
        M53.inv2d(want, j_max=3)
        assert np.array_equal(bits(i[b]), bits(want))


# ---- the in-place device entry where no copy may ride along ----------------------------------------------------------------
RIDE_SETTINGS = [dict(ring=16), dict(nt=15), dict(ring_inv=16), dict(waves=1), dict(ring=16, nt=15, ring_inv=16, waves=1)]


@pytest.mark.parametrize("opts", RIDE_SETTINGS, ids=lambda o: "+".join("%s%d" % kv for kv in o.items()))
def test_in_place_entry_under_settings_that_forbid_a_riding_copy(dwt, oracle, opts):
    """dwt_cdf97_2f_s / _2i_s in place on 771 x 517 at pitch 520, 3 levels, ride_copy = 1: under each setting the sweeps have
    no ride-along kernel (the deep rings, the wave-shift taps, a workgroup of one wave); the driver's sweep_ride_ok must say so
    or the launch refuses the copy and the call fails.  The oracle's bits either way."""
    h, w, pe, J = 771, 517, 520, 3
    rng = np.random.default_rng(771)
    buf = F.finite_floats(rng, (h, pe))
    want = buf.copy()
    assert checker_inplace(oracle, "cdf97_2f_s", want[:, :w], J) == J
    back = want.copy()
    oracle.inv("cdf97_2i_s", back[:, :w], J)
    d = dwt.DeviceImage(h, w, pitch_bytes=pe * 4).upload(buf)
    try:
        dwt.set_option("ride_copy", 1)
        for k, v in opts.items():
            dwt.set_option(k, v)
        assert dwt.dwt_cdf97_2f_s(d.ptr, pe * 4, 4, w, h, w, h, J) == J
        assert np.array_equal(bits(d.download(np.float32)), bits(want)), "forward"
        dwt.dwt_cdf97_2i_s(d.ptr, pe * 4, 4, w, h, w, h, J)
        assert np.array_equal(bits(d.download(np.float32)), bits(back)), "inverse"
    finally:
        restore(dwt)
        d.free()


def checker_inplace(oracle, name, view, j):
    with (oracle.reflected_ends() if PLAIN_BUILD else warnings.catch_warnings()):
        return oracle.fwd(name, view, j)


# ---- fuse01 = 2 where the fused pair has no kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt,val", [("cpt", 4), ("ring", 8), ("nt", 15)])
def test_fuse01_forced_under_settings_without_a_fused_kernel(dwt, oracle, opt, val):
    """132 x 1028, 3 levels, out of place, legal for the fused pair of levels 0 and 1: with 4 columns per lane, the shallow ring
    or the wave-shift taps set by hand the call stays level by level -- 3 launches -- and gives the oracle's bits."""
    h, w, J = 132, 1028, 3
    img = F.finite_floats(np.random.default_rng(132), (h, w))
    want = img.copy()
    assert checker_inplace(oracle, "cdf97_2f_s", want, J) == J
    src, dst = dwt.DeviceImage(h, w).upload(img), dwt.DeviceImage(h, w).upload(np.full_like(img, 7.0))
    try:
        dwt.set_option("fuse01", 2)
        dwt.set_option(opt, val)
        n0 = dwt.get_option("stat_launches")
        assert dwt.dwt_cdf97_2f_s2(src.ptr, dst.ptr, dst.stride_x, 4, w, h, w, h, J) == J
        assert dwt.get_option("stat_launches") - n0 == J
        assert np.array_equal(bits(dst.download(np.float32)), bits(want))
    finally:
        restore(dwt)
        src.free()
        dst.free()


# ---- 3-D knobs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 50, 256), (40, 33, 768), (33, 65, 129)], ids=lambda s: "%dx%dx%d" % s)
def test_3d_cache_policy_and_block_order_change_no_bit(dwt, oracle, shape):
    """vol_nt (the z pass's and the fused level's cache policy) and vol_swizzle (the fused level's block order): every value
    gives the default setting's bits and the oracle's -- out of place with the fused level wherever it can run, and in place,
    forward and inverse.  Random [0, 1) data: no line end near overflow, so the 3-D kernels' reflected ends do not show."""
    nz, ny, nx = shape
    v = np.random.default_rng(nz * 100 + nx).random(shape, dtype=np.float32)
    want_f = oracle.vol("cdf97_3f_s", v.copy())
    want_i = oracle.vol("cdf97_3i_s", want_f.copy())
    L = dwt.lib
    src, dst = L.dwt_hip_malloc(v.nbytes), L.dwt_hip_malloc(v.nbytes)
    got = np.empty_like(v)

    def op():
        assert L.dwt_hip_memcpy_h2d(src, v.ctypes.data, v.nbytes) == 0 and L.dwt_hip_memcpy_h2d(dst, np.full_like(v, 7.0).ctypes.data, v.nbytes) == 0
        dwt.transform3d_op(src, dst, nx * 4, nx * ny * 4, nx, ny, nz, 1)
        assert L.dwt_hip_memcpy_d2h(got.ctypes.data, dst, v.nbytes) == 0
        return got.copy()

    def ip(inverse, data):
        assert L.dwt_hip_memcpy_h2d(src, data.ctypes.data, v.nbytes) == 0
        dwt.transform3d(inverse, src, nx * 4, nx * ny * 4, nx, ny, nz, 1)
        assert L.dwt_hip_memcpy_d2h(got.ctypes.data, src, v.nbytes) == 0
        return got.copy()

    try:
        assert src and dst
        dwt.set_option("vol_fused", 2)
        base = op()
        assert np.array_equal(bits(base), bits(want_f))
        for nt, swz in itertools.product((0, 1, 2, 3, 7), (0, 1)):
            dwt.set_option("vol_nt", nt)
            dwt.set_option("vol_swizzle", swz)
            assert np.array_equal(bits(op()), bits(base)), ("op", nt, swz)
        restore(dwt)
        base_f, base_i = ip(0, v), ip(1, want_f)
        assert np.array_equal(bits(base_f), bits(want_f)) and np.array_equal(bits(base_i), bits(want_i))
        for nt, swz in itertools.product((1, 3), (0, 1)):
            dwt.set_option("vol_nt", nt)
            dwt.set_option("vol_swizzle", swz)
            assert np.array_equal(bits(ip(0, v)), bits(base_f)), ("ip forward", nt, swz)
            assert np.array_equal(bits(ip(1, want_f)), bits(base_i)), ("ip inverse", nt, swz)
    finally:
        restore(dwt)
        L.dwt_hip_free(src)
        L.dwt_hip_free(dst)
