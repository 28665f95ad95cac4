"""The seams of the fused pair of levels 0 and 1 (option fuse01): its tiles lie 512 columns apart and every
wave computes the 8 level-0 LL columns beyond its seams again for itself (phantom columns).  Every case runs through
dwt_hip_transform2d_batch with fuse01 = 2 and 16 row pairs per tile and is compared bit for bit with fuse01 = 0 (level by
level) and with the oracle; the launch counter must show J - 1 launches.

Widths: one seam (1024), a tile with phantoms on both sides (1536), the line end 4, 8 or 12 columns past a seam -- inside the
right phantoms' windows -- (516, 1028, 1032, 1036; 516 and 1028 put the last column in the middle of lane 0), the first
remainder whose phantom windows are whole (1040), the last column in a middle lane 4 columns before a seam (1020), a single
tile (512, 128), and a padded batch (132 x 1540, pitch 1600).

Two input classes: "finite" (floatends.finite_floats, nothing overflows: every sample is compared) with distinct large values
in the input columns seam - 12 .. seam + 11 of every seam, the columns a phantom window can read; "range": -0.0, subnormals,
+-3e38, +-Inf and NaN in those same columns and at the four borders, compared with conftest.same_floats -- sparse enough that
at most half of the oracle's result is NaN, which the test asserts from the oracle alone."""
import numpy as np
import pytest

from conftest import bits, same_floats
from floatends import finite_floats, nan_share

pytestmark = pytest.mark.gpu

SHAPES = [
    # h, w, images, row pitch, padding between images (elements)
    (128, 1024, 1, None, 0),
    (128, 1536, 1, None, 0),
    (128, 516, 1, None, 0),
    (128, 1028, 1, None, 0),
    (128, 1032, 1, None, 0),
    (128, 1036, 1, None, 0),
    (128, 1040, 1, None, 0),
    (128, 1020, 1, None, 0),
    (128, 512, 1, None, 0),
    (128, 128, 1, None, 0),
    (132, 1540, 3, 1600, 192),
]
NAN_CAP = 0.5


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.set_option("tile_pairs", 16)
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    for k, v in (("fuse01", 1), ("tile_pairs", 0)):
        d.set_option(k, v)
    d.dwt_util_finish()


def seam_columns(w):
    """The input columns a phantom window of some tile can read: seam - 12 .. seam + 11 of every seam inside the line."""
    return [c for s in range(512, w, 512) for c in range(s - 12, min(s + 12, w))]


def finite_input(seed, nb, h, w):
    rng = np.random.default_rng(seed)
    imgs = np.stack([finite_floats(rng, (h, w)) for _ in range(nb)])
    cols = seam_columns(w)
    for b in range(nb):
        for i, c in enumerate(cols):
            r = np.arange(h)
            n = (r * len(cols) + i + 7 * b) % 4093  # distinct per (row, seam column)
            imgs[b, :, c] = (1e28 * (1.0 + n / 4093.0) * np.where((r + i) & 1, -1.0, 1.0)).astype(np.float32)
    return imgs


def range_input(seed, nb, h, w):
    """Uniform [-1, 1) with hand-placed specials: one per seam column (the row moves with the column), and every 29th sample
    of the first and last two rows and columns."""
    rng = np.random.default_rng(seed)
    imgs = rng.random((nb, h, w), dtype=np.float32) * 2 - 1
    specials = np.array([-0.0, 1e-40, -1e-42, 3e38, -3e38, np.inf, -np.inf, np.nan, -0.0, 1e-45, 3e38, -1e-40], dtype=np.float32)
    n = 0
    for b in range(nb):
        for i, c in enumerate(seam_columns(w)):
            for r in ((5 * i + 3 * b) % h, (5 * i + 3 * b + h // 2 + 1) % h):
                imgs[b, r, c] = specials[n % len(specials)]
                n += 1
        for r in (0, 1, h - 2, h - 1):
            for c in range(n % 29, w, 29):
                imgs[b, r, c] = specials[n % len(specials)]
                n += 1
        for c in (0, 1, w - 2, w - 1):
            for r in range(n % 29, h, 29):
                imgs[b, r, c] = specials[n % len(specials)]
                n += 1
    return imgs


def run(dwt, imgs, J, fuse, pitch, pad):
    """The batch through the device entry, rows `pitch` elements and images pitch * h + pad elements apart; returns
    (coefficients, kernel launches of the call).  Everything outside the images must come back untouched."""
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
        dwt.set_option("fuse01", fuse)
        before = dwt.get_option("stat_launches")
        assert dwt.transform2d_batch("cdf97_s", 0, src, dst, bstride * 4, nb, pitch * 4, w, h, J) == J
        launches = dwt.get_option("stat_launches") - before
        got = np.empty_like(host)
        assert L.dwt_hip_memcpy_d2h(got.ctypes.data, dst, got.nbytes) == 0
    finally:
        dwt.set_option("fuse01", 1)
        L.dwt_hip_free(src)
        L.dwt_hip_free(dst)
    out = got[:, :pitch * h].reshape(nb, h, pitch)
    assert np.array_equal(bits(out[:, :, w:]), bits(view[:, :, w:])), "row padding written"
    assert np.array_equal(bits(got[:, pitch * h:]), bits(host[:, pitch * h:])), "padding between the images written"
    return out[:, :, :w].copy(), launches


def check(dwt, oracle, imgs, J, pitch, pad, equal):
    want = imgs.copy()
    for b in range(len(imgs)):
        assert oracle.fwd("cdf97_2f_s", want[b], J) == J
    got2, n2 = run(dwt, imgs, J, 2, pitch, pad)
    got0, n0 = run(dwt, imgs, J, 0, pitch, pad)
    assert n0 == J and n2 == J - 1, "launches: %d fused, %d level by level" % (n2, n0)
    assert equal(got2, got0), "fuse01 = 2 differs from fuse01 = 0"
    assert equal(got2, want), "fuse01 = 2 differs from the oracle"
    return want


@pytest.mark.parametrize("J", [2, 3])
@pytest.mark.parametrize("h,w,nb,pitch,pad", SHAPES)
def test_seams_on_finite_input(dwt, oracle, h, w, nb, pitch, pad, J):
    imgs = finite_input(1000 * J + h + w, nb, h, w)
    want = check(dwt, oracle, imgs, J, pitch, pad, lambda a, b: np.array_equal(bits(a), bits(b)))
    assert np.isfinite(want).all()


@pytest.mark.parametrize("J", [2, 3])
@pytest.mark.parametrize("h,w,nb,pitch,pad", SHAPES)
def test_seams_over_the_float_range(dwt, oracle, h, w, nb, pitch, pad, J):
    imgs = range_input(2000 * J + h + w, nb, h, w)
    with np.errstate(all="ignore"):
        want = imgs.copy()
        for b in range(nb):
            assert oracle.fwd("cdf97_2f_s", want[b], J) == J
        share = nan_share(want)
        assert share <= NAN_CAP, "NaN share of the oracle's result %.3f" % share
        check(dwt, oracle, imgs, J, pitch, pad, same_floats)
