"""The direction of the tile rows of the fused pair of levels 0 and 1 (option fuse01_updown): every second tile
row marches from its lower edge upward, so that vertically adjacent tiles read the rows around their common edge at the same
time.  The direction is a scheduling choice only: every step of an upward tile has its two vertical neighbours exchanged inside
a commutative sum.  So every case runs through dwt_hip_transform2d_batch with fuse01 = 2 under fuse01_updown = 1 (odd tile rows
upward) and 2 (even ones: an upward tile at the image's top edge), at both ring depths, and its coefficients are compared as
int32 words with those of fuse01 = 0 (level by level) and of fuse01_updown = 0; one direction per depth also with the oracle.

Shapes (width x height, row pairs per tile), a batch of 3 each:
  128 x 128, 16    four tile rows, the minimum: every tile touches an image edge or a partner
  1040 x 384, 64 / 32 / 16    3, 6 and 12 tile rows -- under value 1 the last row is a downward tile at the bottom (3) or an upward
                   one that starts there (6, 12); three tile columns, the last one ragged: phantom columns on both sides
  516 x 256, 16    the last column in the middle of a lane's columns
  520 x 132, 16    the last tile row (2 pairs) shorter than the tile, in both directions
J = 2: level 1's LL band goes to the destination; J = 3: to scratch, and feeds level 2.

Inputs: conftest.full_range_floats ("mixed": +-0, subnormals, the largest normals, overflowing taps, the specials forced onto the
borders and seams) and a plain uniform image."""
import numpy as np
import pytest

from conftest import bits, full_range_floats, same_floats
from test_hip_fuse01_ring import run

pytestmark = pytest.mark.gpu

RINGS = [8, 16]
SHAPES = [
    # w, h, tile pairs
    (128, 128, 16),
    (1040, 384, 64),
    (1040, 384, 32),
    (1040, 384, 16),
    (516, 256, 16),
    (520, 132, 16),
]
NB = 3


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("fuse01_updown", -1)
    d.dwt_util_finish()


def words(a):
    return np.ascontiguousarray(a).view(np.int32)


def inputs(seed, h, w):
    rng = np.random.default_rng(seed)
    return {"range": np.stack([full_range_floats(rng, (h, w)) for _ in range(NB)]),
            "plain": rng.random((NB, h, w), dtype=np.float32)}


@pytest.mark.parametrize("J", [2, 3])
@pytest.mark.parametrize("w,h,pairs", SHAPES)
def test_upward_tile_rows_give_the_same_bits(dwt, oracle, w, h, pairs, J):
    try:
        for kind, imgs in inputs(500 * J + w + h + pairs, h, w).items():
            with np.errstate(all="ignore"):
                want = imgs.copy()
                for b in range(NB):
                    assert oracle.fwd("cdf97_2f_s", want[b], J) == J
            levels, n = run(dwt, imgs, J, None, 0, fuse01=0, tile_pairs=pairs)
            assert n == J
            for ring in RINGS:
                down, n = run(dwt, imgs, J, None, 0, fuse01=2, tile_pairs=pairs, fuse01_ring=ring, fuse01_updown=0)
                assert n == J - 1 and dwt.get_option("fuse01_last_updown") == 0
                assert np.array_equal(words(down), words(levels)), (kind, ring)
                for updown in (1, 2):
                    got, n = run(dwt, imgs, J, None, 0, fuse01=2, tile_pairs=pairs, fuse01_ring=ring, fuse01_updown=updown)
                    assert n == J - 1, "%d launches" % n
                    assert dwt.get_option("fuse01_last_updown") == updown
                    diff = words(got) != words(levels)
                    assert not diff.any(), "%s, ring %d, updown %d: %d words differ from fuse01 = 0, first at %s" % (
                        kind, ring, updown, diff.sum(), np.argwhere(diff)[0])
                    assert np.array_equal(words(got), words(down)), (kind, ring, updown)
                    if updown == (1 if ring == 8 else 2):  # one direction per depth against the oracle
                        if kind == "plain":
                            assert np.array_equal(bits(got), bits(want)), (kind, ring, updown)
                        else:
                            assert same_floats(got, want), (kind, ring, updown)
    finally:
        dwt.set_option("fuse01_updown", -1)


def test_the_direction_is_an_option_of_its_own(dwt):
    """A value other than -1, 0, 1, 2 is refused and changes nothing; fuse01_last_updown shows what the last fused launch ran
    with; 0 after 1 is the launch with every tile row downward again; the rule leaves a small launch downward."""
    imgs = np.random.default_rng(3).random((1, 128, 1024), dtype=np.float32)
    levels, _ = run(dwt, imgs, 2, None, 0, fuse01=0, tile_pairs=16)
    try:
        dwt.set_option("fuse01_updown", 1)
        for bad in (3, -2, 4, 8, 100):
            with pytest.raises(dwt.DwtError):
                dwt.set_option("fuse01_updown", bad)
            assert dwt.get_option("fuse01_updown") == 1
        for updown, shown in ((1, 1), (0, 0), (2, 2), (-1, 0)):
            got, n = run(dwt, imgs, 2, None, 0, fuse01=2, tile_pairs=16, fuse01_updown=updown)
            assert n == 1 and dwt.get_option("fuse01_last_updown") == shown, updown
            assert np.array_equal(words(got), words(levels)), updown
    finally:
        dwt.set_option("fuse01_updown", -1)
    assert dwt.get_option("fuse01_updown") == -1
