"""Levels 0 and 1 of the out-of-place float 9/7 forward transform in ONE launch over overlapped tiles (option fuse01,
DESIGN.md s4): every case runs with fuse01 = 2 (wherever the geometry is legal) and is compared bit for bit with
fuse01 = 0 (level by level) and with the oracle; the launch counter shows which path ran."""
import numpy as np
import pytest

from conftest import bits, same_floats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    for k, v in (("fuse01", 1), ("tile_pairs", 0), ("nt", 7)):
        d.set_option(k, v)
    d.dwt_util_finish()


def run(dwt, wname, imgs, J, fuse, pitch=None, pad=0, in_place=False):
    """The batch `imgs` (nb, h, w) through the device entry with rows `pitch` elements and images pitch * h + pad elements
    apart; returns (coefficients, kernel launches of the call)."""
    L = dwt.lib
    nb, h, w = imgs.shape
    pitch = pitch or w
    bstride = pitch * h + pad
    host = np.full((nb, bstride), 7.0, dtype=imgs.dtype)
    view = host[:, :pitch * h].reshape(nb, h, pitch)
    view[:, :, :w] = imgs
    src, dst = L.dwt_hip_malloc(host.nbytes), L.dwt_hip_malloc(host.nbytes)
    try:
        assert L.dwt_hip_memcpy_h2d(src, host.ctypes.data, host.nbytes) == 0
        assert L.dwt_hip_memcpy_h2d(dst, host.ctypes.data, host.nbytes) == 0
        dwt.set_option("fuse01", fuse)
        before = dwt.get_option("stat_launches")
        assert dwt.transform2d_batch(wname, 0, src, src if in_place else dst, bstride * 4, nb, pitch * 4, w, h, J) == J
        launches = dwt.get_option("stat_launches") - before
        got = np.empty_like(host)
        assert L.dwt_hip_memcpy_d2h(got.ctypes.data, src if in_place else dst, got.nbytes) == 0
    finally:
        dwt.set_option("fuse01", 1)
        L.dwt_hip_free(src)
        L.dwt_hip_free(dst)
    out = got[:, :pitch * h].reshape(nb, h, pitch)
    assert np.array_equal(bits(out[:, :, w:]), bits(view[:, :, w:])) and np.array_equal(bits(got[:, pitch * h:]), bits(host[:, pitch * h:])), "padding written"
    return out[:, :, :w].copy(), launches


def check(dwt, oracle, imgs, J, pitch=None, pad=0, fused=True, wname="cdf97_s", ofn="cdf97_2f_s", equal=None, in_place=False):
    equal = equal or (lambda a, b: np.array_equal(bits(a), bits(b)))
    got2, n2 = run(dwt, wname, imgs, J, 2, pitch, pad, in_place)
    got0, n0 = run(dwt, wname, imgs, J, 0, pitch, pad, in_place)
    assert equal(got2, got0), "fuse01 = 2 differs from fuse01 = 0"
    for b in range(len(imgs)):
        want = imgs[b].copy()
        assert oracle.fwd(ofn, want, J) == J
        assert equal(got2[b], want), "fuse01 = 2 differs from the oracle (image %d)" % b
    if not in_place:
        assert n0 == J, n0
    assert n2 == (n0 - 1 if fused else n0), "launches %d against %d level by level" % (n2, n0)


@pytest.mark.parametrize("J", [2, 3])
@pytest.mark.parametrize("h,w,nb,pitch,pad", [
    (128, 1024, 1, None, 0),    # 3 tiles across: left-edge, interior, right-edge; 4 tiles down
    (132, 1028, 1, None, 0),    # the last column in a middle lane of the last tile; 66 row pairs: a short last tile with one pair of level 1
    (128, 1444, 3, 1500, 192),  # row pitch and image stride padded
])
def test_fused_pair_is_the_two_levels(dwt, oracle, h, w, nb, pitch, pad, J):
    imgs = np.random.default_rng(h + w + J).random((nb, h, w), dtype=np.float32) * 2 - 1
    dwt.set_option("tile_pairs", 16)
    try:
        check(dwt, oracle, imgs, J, pitch, pad)
    finally:
        dwt.set_option("tile_pairs", 0)


def test_fused_pair_with_every_store_non_temporal(dwt, oracle):
    """The cases above run k_fwd_sweep01<7> (level 1's LL band stored temporal, the default below 1 GiB of it); option
    nt = 3 takes the other instantiation, the one large batches run."""
    imgs = np.random.default_rng(23).random((2, 132, 1028), dtype=np.float32) * 2 - 1
    dwt.set_option("tile_pairs", 16)
    dwt.set_option("nt", 3)
    try:
        check(dwt, oracle, imgs, 3)
    finally:
        dwt.set_option("tile_pairs", 0)
        dwt.set_option("nt", 7)


def test_default_rule_leaves_small_calls_level_by_level(dwt):
    """fuse01 = 1 (the default) engages by size only: a 128 x 1024 call, legal for the pair, still takes J launches."""
    imgs = np.random.default_rng(29).random((1, 128, 1024), dtype=np.float32) * 2 - 1
    got1, n1 = run(dwt, "cdf97_s", imgs, 3, 1)
    got0, n0 = run(dwt, "cdf97_s", imgs, 3, 0)
    assert n1 == n0 == 3 and np.array_equal(bits(got1), bits(got0))


def test_fused_pair_on_a_row_of_17_tiles(dwt, oracle):
    """The headline's width with the library's own tile height."""
    imgs = np.random.default_rng(5).random((1, 256, 8192), dtype=np.float32) * 2 - 1
    check(dwt, oracle, imgs, 3)


@pytest.mark.parametrize("J", [2, 3])
def test_fused_pair_over_the_float_range(dwt, oracle, J):
    """-0.0, subnormals, +-3e38 (a doubled tap overflows), +-Inf and NaN at and next to all four borders and at the tile
    seams (input columns 479..482, 959..962): the same bits, NaN payloads left out (conftest.same_floats)."""
    h, w = 128, 1024
    rng = np.random.default_rng(17)
    img = rng.random((h, w), dtype=np.float32) * 2 - 1
    specials = np.array([-0.0, 1e-40, -1e-42, 3e38, -3e38, np.inf, -np.inf, np.nan], dtype=np.float32)
    n = 0
    for c in (0, 1, 2, w - 3, w - 2, w - 1, 479, 480, 481, 482, 959, 960, 961, 962):
        for r in range(n % 5, h, 5):
            img[r, c] = specials[n % len(specials)]
            n += 1
    for r in (0, 1, 2, h - 3, h - 2, h - 1):
        for c in range(n % 7, w, 7):
            img[r, c] = specials[n % len(specials)]
            n += 1
    dwt.set_option("tile_pairs", 16)
    try:
        with np.errstate(all="ignore"):
            check(dwt, oracle, img[None], J, equal=same_floats)
    finally:
        dwt.set_option("tile_pairs", 0)


@pytest.mark.parametrize("h,w,wname,ofn,in_place", [
    (64, 1024, "cdf97_s", "cdf97_2f_s", False),   # level 1 below the size of the select form
    (130, 1024, "cdf97_s", "cdf97_2f_s", False),  # a height that is no multiple of 4
    (128, 1024, "cdf53_s", "cdf53_2f_s", False),  # another wavelet
    (128, 1024, "cdf97_s", "cdf97_2f_s", True),   # source and destination the same image
])
def test_what_cannot_fuse_falls_back(dwt, oracle, h, w, wname, ofn, in_place):
    imgs = np.random.default_rng(h).random((1, h, w), dtype=np.float32) * 2 - 1
    check(dwt, oracle, imgs, 2, fused=False, wname=wname, ofn=ofn, in_place=in_place)
