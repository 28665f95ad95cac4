"""Levels (2, 3), (4, 5) ... of a forward float 9/7 call as fused pairs too (option fuse_deep): the launch of
the pair of levels 0 and 1 on the running LL band, read from one scratch band, its last band written to the other scratch
band or, where the pair ends the call, to the image.  The kernel is the one of the pair at 0; what is new is the driver's
path, so every case runs through dwt_hip_transform2d_batch with fuse01 = 2 and fuse_deep = 2 and its coefficients are
compared as int32 words with those of the same call under fuse_deep = 0 and with the oracle's; stat_launches and
fuse_deep_last must show the pairs; row padding and the padding between images come back untouched; the LL scratch is the
caller's, of exactly the documented size (dwt_hip_set_workspace), poisoned, between guards.

Shapes (the smallest at which the driver's new path can go wrong):
  512 x 512           level 2 is 128 x 128, the smallest the pair may take.  J = 4: the pair (2, 3) is last, its LL band goes
                      to the image; J = 5: level 4 follows from scratch; J = 3: there is no deeper pair
  528 rows x 2064 columns, 3 images, padded row pitch and image stride
                      level 2 is 132 x 516: two tile columns, the second 4 columns wide (the line end inside a right
                      phantom's window), 66 row pairs (two tile rows at 64 pairs), a scratch pitch of 516 and a scratch
                      stride per image; J = 4 and 5, every fuse01_updown in {0, 1, 2} at either fuse01_ring
  2048 x 2048, J = 6  pairs at (0, 1), (2, 3) and (4, 5)
  520 columns x 512 rows, J = 4
                      level 2 is 130 wide, no multiple of 4: the pair must not engage (J - 1 launches), same bits

Inputs: "plain" (uniform, every sample compared bit for bit with the oracle) and "seams" (test_hip_fuse01_seams.finite_input:
values of 1e28 of alternating sign on the tile seams' columns; compared with the oracle by conftest.same_floats)."""
import numpy as np
import pytest

import hipdev
from conftest import bits, same_floats
from test_hip_fuse01_seams import finite_input

pytestmark = pytest.mark.gpu

OPTIONS = (("fuse01", 1), ("fuse_deep", 1), ("tile_pairs", 0), ("fuse01_ring", 0), ("fuse01_updown", -1))
SENTINEL = 7.0

# id: rows, columns, images, row pitch, padding between images (elements), J, deeper pairs expected under fuse_deep = 2
CASES = {
    "512-J4": (512, 512, 1, None, 0, 4, 1),
    "512-J5": (512, 512, 1, None, 0, 5, 1),
    "512-J3": (512, 512, 1, None, 0, 3, 0),
    "528x2064-J4": (528, 2064, 3, 2112, 160, 4, 1),
    "528x2064-J5": (528, 2064, 3, 2112, 160, 5, 1),
    "2048-J6": (2048, 2048, 1, None, 0, 6, 2),
    "512x520-J4": (512, 520, 1, None, 0, 4, 0),
}
# the launch variants of a case: (fuse01_ring, fuse01_updown); (0, -1): the launcher's rule
VARIANTS = {k: [(0, -1)] for k in CASES}
VARIANTS["528x2064-J4"] = VARIANTS["528x2064-J5"] = [(ring, updown) for ring in (8, 16) for updown in (0, 1, 2)]


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    yield d
    for k, v in OPTIONS:
        d.set_option(k, v)
    d.lib.dwt_hip_set_workspace(None, 0, None, 0)
    d.dwt_util_finish()


def words(a):
    return np.ascontiguousarray(a).view(np.int32)


class Call:
    """One batch in device memory, rows `pitch` elements and images pitch * h + pad elements apart, under a guarded workspace
    of exactly the documented size; run(): the forward call under `options` -> (coefficients, launches, fuse_deep_last)."""

    def __init__(self, dwt, imgs, pitch, pad):
        self.dwt = dwt
        self.nb, self.h, self.w = imgs.shape
        self.pitch = pitch or self.w
        self.bstride = self.pitch * self.h + pad
        self.host = np.full((self.nb, self.bstride), SENTINEL, dtype=np.float32)
        self.view = self.host[:, :self.pitch * self.h].reshape(self.nb, self.h, self.pitch)
        self.view[:, :, :self.w] = imgs
        self.src, self.dst = hipdev.Dev(dwt, self.host), hipdev.Dev(dwt, self.host)
        self.ws = hipdev.GuardedWorkspace(dwt, "cdf97_s", self.nb, self.w, self.h)

    def run(self, J, **options):
        dwt = self.dwt
        assert dwt.lib.dwt_hip_memcpy_h2d(self.dst.ptr, self.host.ctypes.data, self.host.nbytes) == 0
        self.ws.arm()
        try:
            for k, v in options.items():
                dwt.set_option(k, v)
            before = dwt.get_option("stat_launches")
            assert dwt.transform2d_batch("cdf97_s", 0, self.src.ptr, self.dst.ptr, self.bstride * 4, self.nb, self.pitch * 4, self.w, self.h, J) == J
            launches = dwt.get_option("stat_launches") - before
            deep = dwt.get_option("fuse_deep_last")
        finally:
            for k, v in OPTIONS:
                dwt.set_option(k, v)
        got = self.dst.get()
        self.ws.check()  # every guard word intact
        out = got[:, :self.pitch * self.h].reshape(self.nb, self.h, self.pitch)
        assert np.array_equal(bits(out[:, :, self.w:]), bits(self.view[:, :, self.w:])), "row padding written"
        assert np.array_equal(bits(got[:, self.pitch * self.h:]), bits(self.host[:, self.pitch * self.h:])), "padding between the images written"
        assert np.array_equal(bits(self.src.get()), bits(self.host)), "source modified"
        return out[:, :, :self.w].copy(), launches, deep

    def close(self):
        self.ws.close()
        self.src.free()
        self.dst.free()


def inputs(seed, nb, h, w):
    rng = np.random.default_rng(seed)
    return {"plain": rng.random((nb, h, w), dtype=np.float32) * 2 - 1, "seams": finite_input(seed, nb, h, w)}


@pytest.mark.parametrize("case", list(CASES))
def test_deeper_pairs_give_the_same_bits(dwt, oracle, case):
    h, w, nb, pitch, pad, J, pairs = CASES[case]
    for kind, imgs in inputs(7000 + 10 * h + w + J, nb, h, w).items():
        with np.errstate(all="ignore"):
            want = imgs.copy()
            for b in range(nb):
                assert oracle.fwd("cdf97_2f_s", want[b], J) == J
        call = Call(dwt, imgs, pitch, pad)
        try:
            # every option at its default: what the call takes today
            got, n, deep = call.run(J)
            assert (n, deep) == (J, 0), "defaults: %d launches, %d deeper pairs" % (n, deep)
            assert np.array_equal(words(got), words(want)) if kind == "plain" else same_floats(got, want), (kind, "defaults")
            # the pair at 0 alone
            levels, n, deep = call.run(J, fuse01=2, fuse_deep=0)
            assert (n, deep) == (J - 1, 0), "fuse_deep = 0: %d launches, %d deeper pairs" % (n, deep)
            assert np.array_equal(words(levels), words(want)) if kind == "plain" else same_floats(levels, want), (kind, "fuse_deep = 0")
            for ring, updown in VARIANTS[case]:
                got, n, deep = call.run(J, fuse01=2, fuse_deep=2, fuse01_ring=ring, fuse01_updown=updown)
                assert deep == pairs, "%s, ring %d, updown %d: %d deeper pairs, not %d" % (kind, ring, updown, deep, pairs)
                assert n == J - 1 - pairs, "%s, ring %d, updown %d: %d launches, not %d" % (kind, ring, updown, n, J - 1 - pairs)
                diff = words(got) != words(levels)
                assert not diff.any(), "%s, ring %d, updown %d: %d words differ from fuse_deep = 0, first at %s" % (
                    kind, ring, updown, diff.sum(), np.argwhere(diff)[0])
                assert np.array_equal(words(got), words(want)) if kind == "plain" else same_floats(got, want), (kind, ring, updown, "oracle")
        finally:
            call.close()


RULE_SCRIPT = r"""
import sys
import torch                      # first: this process then shares torch's HIP runtime
sys.path.insert(0, ROOT)
import libdwt_amd as dwt
dwt.dwt_util_init()
nb, n, J = 32, 8192, 5
dev = torch.device("cuda:0")
src = torch.rand((nb, n, n), device=dev, dtype=torch.float32, generator=torch.Generator(device=dev).manual_seed(5))
want, got = torch.empty_like(src), torch.empty_like(src)
torch.cuda.synchronize()
def run(dst, images, **options):
    for k, v in options.items():
        dwt.set_option(k, v)
    before = dwt.get_option("stat_launches")
    assert dwt.transform2d_batch("cdf97_s", 0, src, dst, n * n * 4, images, n * 4, n, n, J) == J
    dwt.sync()
    for k, v in OPTIONS:
        dwt.set_option(k, v)
    return dwt.get_option("stat_launches") - before, dwt.get_option("fuse_deep_last")
def same():
    torch.cuda.synchronize()
    return torch.equal(got.view(torch.int32), want.view(torch.int32))
r = run(want, nb, fuse_deep=0)
assert r == (4, 0), r
r = run(got, nb)
assert r == (3, 1), r
assert same(), "the rule's launch differs from fuse_deep = 0"
got.zero_()
r = run(got, nb, fuse_deep=2, fuse01_ring=16, fuse01_updown=0, tile_pairs=64)
assert r == (3, 1) and same(), r
r = run(got, nb, fuse01=0)
assert r == (5, 0), r
r = run(got, 16)
assert r == (5, 0), r
dwt.dwt_util_finish()
print("deeper pair by the rule OK")
"""


def test_the_rule_engages_from_32_images_of_8192():
    """Every option at its default on the smallest batch the rule takes (32 images of 8192^2: 32768 tiles at level 0, 2048 at
    level 2), generated and compared on the device as int32 words: pairs at (0, 1) and (2, 3) and level 4 alone -- 3 launches,
    the deeper one with the rule's own ring, direction and height -- against fuse_deep = 0 (4 launches) and against the pair
    under the launcher's geometry; without the pair at 0 there is no deeper pair; 16 of the images stay at one launch per
    level.  Own process: the batch lives in torch tensors, and torch comes before the library (one HIP runtime)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\nOPTIONS = %r\n" % (root, OPTIONS) + RULE_SCRIPT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "deeper pair by the rule OK" in out.stdout, out.stderr[-2000:]


def test_the_deeper_pairs_have_an_option_of_their_own(dwt):
    """fuse_deep does not ride on fuse01: with fuse01 = 2 alone (fuse_deep at its default) a small call takes J - 1 launches as
    before; fuse_deep = 2 without the pair at 0 still takes the pairs below it; fuse_deep_last counts the last call's only."""
    imgs = np.random.default_rng(11).random((1, 512, 512), dtype=np.float32)
    call = Call(dwt, imgs, None, 0)
    try:
        assert dwt.get_option("fuse_deep") == 1
        levels, n, deep = call.run(5, fuse01=0, fuse_deep=0)
        assert (n, deep) == (5, 0)
        got, n, deep = call.run(5, fuse01=2)
        assert (n, deep) == (4, 0) and np.array_equal(words(got), words(levels))
        got, n, deep = call.run(5, fuse01=0, fuse_deep=2)
        assert (n, deep) == (4, 1) and np.array_equal(words(got), words(levels))
        got, n, deep = call.run(5, fuse01=2, fuse_deep=2)
        assert (n, deep) == (3, 1) and np.array_equal(words(got), words(levels))
        got, n, deep = call.run(2, fuse01=2, fuse_deep=2)
        assert (n, deep) == (1, 0)
    finally:
        call.close()
    assert dwt.get_option("fuse_deep") == 1
