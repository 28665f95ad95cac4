"""The ring depths of the fused pair of levels 0 and 1 (option fuse01_ring): the 16-row ring runs one workgroup
of four waves per CU, the 8-row ring two of them -- two waves per SIMD.  The depth is a scheduling choice only: every case
runs through dwt_hip_transform2d_batch with fuse01 = 2 and is compared bit for bit with fuse01 = 0 (level by level) and with
the oracle; the launch counter must show J - 1 launches; row padding and the padding between images come back untouched.

Shapes: one seam and four tile rows, the ring wrapping several times per tile (128 x 1024); the line end inside a right
phantom's window (128 x 1036); a single narrow tile (128 x 128); a padded batch whose last tile has 2 row pairs -- 13 iterations,
the shortest sweep against the 3 iterations of look-ahead of the shallow ring (132 x 1540); full-height tiles of 75
iterations and a last tile of 4 pairs (264 x 516 at 64 pairs); the launcher's own height rule (264 x 1036, tile_pairs 0).

Input classes as in test_hip_fuse01_seams.py: "finite" (every sample compared) and "range" (-0.0, subnormals, +-3e38, +-Inf
and NaN at the seams and borders, compared with conftest.same_floats; at most half of the oracle's result is NaN, asserted
from the oracle alone)."""
import numpy as np
import pytest

from conftest import bits, same_floats
from floatends import nan_share
from test_hip_fuse01_seams import finite_input, range_input

pytestmark = pytest.mark.gpu

RINGS = [8, 16]  # every depth the library ships a fused kernel for
SHAPES = [
    # h, w, images, row pitch, padding between images (elements), tile pairs
    (128, 1024, 1, None, 0, 16),
    (128, 1036, 1, None, 0, 16),
    (128, 128, 1, None, 0, 16),
    (132, 1540, 3, 1600, 192, 16),
    (264, 516, 1, None, 0, 64),
    (264, 1036, 1, None, 0, 0),
]
NAN_CAP = 0.5
OPTIONS = (("fuse01", 1), ("tile_pairs", 0), ("fuse01_ring", 0), ("ring", 0))


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    for k, v in OPTIONS:
        d.set_option(k, v)
    d.dwt_util_finish()


def run(dwt, imgs, J, pitch, pad, **options):
    """The batch through the device entry under `options`, rows `pitch` elements and images pitch * h + pad elements apart;
    returns (coefficients, kernel launches of the call).  Everything outside the images must come back untouched."""
    L = dwt.lib
    nb, h, w = imgs.shape
    pitch = pitch or w
    bstride = pitch * h + pad
    host = np.full((nb, bstride), 7.0, dtype=np.float32)
    view = host[:, :pitch * h].reshape(nb, h, pitch)
    view[:, :, :w] = imgs
    src, dst = L.dwt_hip_malloc(host.nbytes), L.dwt_hip_malloc(host.nbytes)
    try:
        assert L.dwt_hip_memcpy_h2d(src, host.ctypes.data, host.nbytes) == 0
        assert L.dwt_hip_memcpy_h2d(dst, host.ctypes.data, host.nbytes) == 0
        for k, v in options.items():
            dwt.set_option(k, v)
        before = dwt.get_option("stat_launches")
        assert dwt.transform2d_batch("cdf97_s", 0, src, dst, bstride * 4, nb, pitch * 4, w, h, J) == J
        launches = dwt.get_option("stat_launches") - before
        got = np.empty_like(host)
        assert L.dwt_hip_memcpy_d2h(got.ctypes.data, dst, got.nbytes) == 0
    finally:
        for k, v in OPTIONS:
            dwt.set_option(k, v)
        L.dwt_hip_free(src)
        L.dwt_hip_free(dst)
    out = got[:, :pitch * h].reshape(nb, h, pitch)
    assert np.array_equal(bits(out[:, :, w:]), bits(view[:, :, w:])), "row padding written"
    assert np.array_equal(bits(got[:, pitch * h:]), bits(host[:, pitch * h:])), "padding between the images written"
    return out[:, :, :w].copy(), launches


def check(dwt, oracle, imgs, J, pitch, pad, pairs, equal):
    """Every shipped depth against the level-by-level call and the oracle (both computed once per case)."""
    want = imgs.copy()
    for b in range(len(imgs)):
        assert oracle.fwd("cdf97_2f_s", want[b], J) == J
    got0, n0 = run(dwt, imgs, J, pitch, pad, fuse01=0, tile_pairs=pairs)
    assert n0 == J
    for ring in RINGS:
        got, n = run(dwt, imgs, J, pitch, pad, fuse01=2, tile_pairs=pairs, fuse01_ring=ring)
        assert n == J - 1, "ring %d: %d launches" % (ring, n)
        assert equal(got, got0), "ring %d differs from fuse01 = 0" % ring
        assert equal(got, want), "ring %d differs from the oracle" % ring
    return want


@pytest.mark.parametrize("J", [2, 3])
@pytest.mark.parametrize("h,w,nb,pitch,pad,pairs", SHAPES)
def test_ring_depths_on_finite_input(dwt, oracle, h, w, nb, pitch, pad, pairs, J):
    imgs = finite_input(3000 * J + h + w, nb, h, w)
    want = check(dwt, oracle, imgs, J, pitch, pad, pairs, lambda a, b: np.array_equal(bits(a), bits(b)))
    assert np.isfinite(want).all()


@pytest.mark.parametrize("J", [2, 3])
@pytest.mark.parametrize("h,w,nb,pitch,pad,pairs", SHAPES)
def test_ring_depths_over_the_float_range(dwt, oracle, h, w, nb, pitch, pad, pairs, J):
    imgs = range_input(3000 * J + h + w, nb, h, w)
    with np.errstate(all="ignore"):
        want = imgs.copy()
        for b in range(nb):
            assert oracle.fwd("cdf97_2f_s", want[b], J) == J
        share = nan_share(want)
        assert share <= NAN_CAP, "NaN share of the oracle's result %.3f" % share
        check(dwt, oracle, imgs, J, pitch, pad, pairs, same_floats)


def test_the_fused_depth_has_a_knob_of_its_own(dwt):
    """fuse01_ring = 8 keeps the call fused (J - 1 launches; the sweep option ring = 8 keeps it level by level, which
    test_hip_sweep_matrix.py holds); a depth without a kernel is refused and changes nothing."""
    imgs = finite_input(7, 1, 128, 1024)
    for J in (2, 3):
        _, n = run(dwt, imgs, J, None, 0, fuse01=2, tile_pairs=16, fuse01_ring=8)
        assert n == J - 1
    dwt.set_option("fuse01_ring", 8)
    try:
        for bad in (4, 10, 12, 24, 32, -8):
            if bad in RINGS:
                continue
            with pytest.raises(dwt.DwtError):
                dwt.set_option("fuse01_ring", bad)
            assert dwt.get_option("fuse01_ring") == 8
    finally:
        dwt.set_option("fuse01_ring", 0)
    assert dwt.get_option("fuse01_ring") == 0


def test_the_tuner_picks_among_the_depths(dwt):
    """dwt_hip_tune on the smallest batch it measures (32 images of 2048^2: 512 MiB) with the pair forced: the choice the fused
    launch then runs with is one of the candidates -- 64, 128 or 32 row pairs at 8 or 16 rows --, a transform call measures
    nothing, and its result has the bits of the level-by-level call."""
    L = dwt.lib
    nb, n, J = 32, 2048, 2
    imgs = np.random.default_rng(97).random((nb, n, n), dtype=np.float32)
    src, dst = L.dwt_hip_malloc(imgs.nbytes), L.dwt_hip_malloc(imgs.nbytes)
    try:
        assert L.dwt_hip_memcpy_h2d(src, imgs.ctypes.data, imgs.nbytes) == 0
        dwt.set_option("fuse01", 0)
        assert dwt.transform2d_batch("cdf97_s", 0, src, dst, n * n * 4, nb, n * 4, n, n, J) == J
        want = np.empty_like(imgs)
        assert L.dwt_hip_memcpy_d2h(want.ctypes.data, dst, want.nbytes) == 0
        dwt.set_option("fuse01", 2)
        dwt.tune("cdf97_s", 0, src, dst, n * n * 4, nb, n * 4, n, n, J)
        assert L.dwt_hip_memcpy_h2d(dst, imgs.ctypes.data, imgs.nbytes) == 0
        before = dwt.get_option("stat_launches")
        assert dwt.transform2d_batch("cdf97_s", 0, src, dst, n * n * 4, nb, n * 4, n, n, J) == J
        assert dwt.get_option("stat_launches") - before == J - 1
        choice = dwt.get_option("fuse01_last_choice")
        assert choice & 0xFFFF in (64, 128, 32) and (choice >> 16) & 0xFF == 0 and choice >> 24 in RINGS, hex(choice)
        got = np.empty_like(imgs)
        assert L.dwt_hip_memcpy_d2h(got.ctypes.data, dst, got.nbytes) == 0
        assert np.array_equal(bits(got), bits(want))
    finally:
        for k, v in OPTIONS:
            dwt.set_option(k, v)
        L.dwt_hip_free(src)
        L.dwt_hip_free(dst)
