"""GPU checks of the best-basis search over packet quadtrees and of pruned 2-D packet trees (dwt_hip_wp_best2d_batch,
dwt_hip_wp_tree2d_batch, wp_joint_qtree; libdwt_amd/packets.py) against tests/wp_basis2d_model.py.  Coefficients and trees
compare bit for bit (a NaN on both sides is not compared); the costs of the THRESHOLD kind and of all-zero images compare
exactly, those of the float kinds within (n + 16) 2^-52 sum|term| of the model's fsum, n the node's sample count -- the
derived bound of a double sum of n terms in any order plus a few ulp per log / pow, not a measured figure.  The trees are the
model's EXACTLY because no input holds a near-tie (tests/test_wp_basis2d.py asserts that for every case of the table in
wp_basis2d_model.py, and that no tree is trivial).  Every buffer is filled with a canary first and every word outside the
addressed ones must still hold it; src of an out-of-place call must come back as it was.  Every case runs on the fused
route (dense device images: 3 * levels + 2 launches with dst, 2 * levels + 2 without, `levels` for a transform in given
trees) and under option "wp_fused" = 0."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import wp_basis2d_model as qm
import wp_model as wp
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
CANARY = np.uint32(0xDEADBEEF)
CANARY64 = np.uint64(0xDEADBEEFDEADBEEF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QW = qm.QTREE_WORDS
TW = QW + 4  # words between the trees of two images: 16 bytes of gap
EPS = 2.0 ** -52
BIG_GUARD = (64 << 10) // 4  # words: 64 KiB on either side of an output


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d
    from libdwt_amd import packets

    d.dwt_util_init()
    d.packets = packets
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("wp_fused", 1)


# ---- runners ----------------------------------------------------------------------------------------------------
class Images:
    """batch x H x W floats laid out in a canary-filled word buffer: elements es bytes apart, `row_gap` extra words behind a
    row, `batch_gap` behind an image, `guard` words in front of and behind the batch"""

    def __init__(self, x, es=4, row_gap=0, batch_gap=0, guard=4):
        self.batch, self.H, self.W = x.shape
        step = es // 4
        self.es, self.guard = es, guard
        self.pitch = self.W * step + row_gap
        self.bs = self.H * self.pitch + batch_gap
        self.words = 2 * guard + self.batch * self.bs
        b, y, c = np.ogrid[0:self.batch, 0:self.H, 0:self.W]
        self.idx = (guard + b * self.bs + y * self.pitch + c * step).reshape(-1)
        self.filled = np.full(self.words, CANARY, np.uint32)
        self.filled[self.idx] = x.view(np.uint32).reshape(-1)
        self.dense = es == 4

    def geom(self, levels):
        return (4 * self.bs, self.batch, 4 * self.pitch, self.es, self.W, self.H, levels)

    def blank(self):
        return np.full(self.words, CANARY, np.uint32)

    def images_of(self, buf):
        rest = np.ones(self.words, bool)
        rest[self.idx] = False
        assert (buf[rest] == CANARY).all(), "bytes outside the images were written"
        return buf[self.idx].view(F32).reshape(self.batch, self.H, self.W)


class Mem:
    """a host array as the call sees it: in device memory (a copy) or where it is"""

    def __init__(self, dwt, arr, device):
        self.host, self.dev = arr, Dev(dwt, arr) if device else None
        self.ptr = self.dev.ptr if device else arr.ctypes.data

    def get(self):
        if self.dev is None:
            return self.host
        out = self.dev.get()
        self.dev.free()
        return out


def run_best(dwt, wavelet, cost, x, levels, in_place=False, device=True, with_dst=True, outputs=("tree", "total", "node_cost"), guard=4, **layout):
    """-> dict(coef, tree, total, node_cost, launches); what was not asked for is None"""
    batch = len(x)
    nq, cd, g2 = qm.nq(levels), qm.nq(levels) + 2, guard // 2
    lay = Images(x, guard=guard, **layout)
    src = Mem(dwt, lay.filled.copy(), device)
    dst = src if in_place else Mem(dwt, lay.blank(), device)
    tree = Mem(dwt, np.full(2 * guard + batch * TW, CANARY, np.uint32), device) if "tree" in outputs else None
    total = Mem(dwt, np.full(2 * g2 + batch, CANARY64, np.uint64), device) if "total" in outputs else None
    nc = Mem(dwt, np.full(2 * g2 + batch * cd, CANARY64, np.uint64), device) if "node_cost" in outputs else None
    k = launches(dwt, lambda: dwt.packets.wp_best2d_batch(
        wp.WAVELET_ID[wavelet], cost[0], cost[1], src.ptr + 4 * guard, dst.ptr + 4 * guard if with_dst else None, *lay.geom(levels),
        tree=tree and tree.ptr + 4 * guard, tree_stride=4 * TW, total=total and total.ptr + 8 * g2, node_cost=nc and nc.ptr + 8 * g2,
        cost_stride=8 * cd))
    dwt.sync()
    out = dict(launches=k, coef=None, tree=None, total=None, node_cost=None)
    s = src.get()
    d = s if in_place else dst.get()
    if not in_place or not with_dst:
        assert np.array_equal(s, lay.filled), "src was written"
    if with_dst:
        out["coef"] = lay.images_of(d)
    elif not in_place:
        assert (d == CANARY).all(), "dst == NULL, and something was stored"
    if tree:
        t = tree.get()
        rows = t[guard:guard + batch * TW].reshape(batch, TW)
        assert (rows[:, QW:] == CANARY).all() and (t[:guard] == CANARY).all() and (t[guard + batch * TW:] == CANARY).all(), "words outside the trees were written"
        out["tree"] = [[int(v) for v in r[:QW]] for r in rows]
    if total:
        t = total.get()
        assert (t[:g2] == CANARY64).all() and (t[g2 + batch:] == CANARY64).all(), "words outside the totals were written"
        out["total"] = t[g2:g2 + batch].view(np.float64).copy()
    if nc:
        t = nc.get()
        rows = t[g2:g2 + batch * cd].reshape(batch, cd)
        assert (rows[:, nq:] == CANARY64).all() and (t[:g2] == CANARY64).all() and (t[g2 + batch * cd:] == CANARY64).all(), "words outside the cost tables were written"
        out["node_cost"] = np.ascontiguousarray(rows[:, :nq]).view(np.float64)
    return out


def run_tree(dwt, wavelet, inverse, x, levels, trees, shared=False, in_place=True, device=True, guard=4, **layout):
    """-> (the images after the call, launches).  trees: one per image, or ONE tree with shared (tree_stride 0)"""
    lay = Images(x, guard=guard, **layout)
    src = Mem(dwt, lay.filled.copy(), device)
    dst = src if in_place else Mem(dwt, lay.blank(), device)
    words = np.full((1 if shared else len(x)) * TW + 4, CANARY, np.uint32)
    for b, t in enumerate([trees] if shared else trees):
        words[b * TW:b * TW + QW] = np.array(t, np.uint32)
    tree = Mem(dwt, words, device)
    k = launches(dwt, lambda: dwt.packets.wp_tree2d_batch(wp.WAVELET_ID[wavelet], inverse, src.ptr + 4 * guard, dst.ptr + 4 * guard, *lay.geom(levels),
                                                           tree.ptr, 0 if shared else 4 * TW))
    dwt.sync()
    assert np.array_equal(tree.get(), words), "the trees were written"
    s = src.get()
    d = s if in_place else dst.get()
    if not in_place:
        assert np.array_equal(s, lay.filled), "src was written"
    return lay.images_of(d), k


def both_routes(dwt, run, check, count=None):
    """run() under "wp_fused" = 1 and 0, check(result, fused) both times; `count`: the launches of the fused route"""
    try:
        for fused in (1, 0):
            dwt.set_option("wp_fused", fused)
            got = run()
            k = got["launches"] if isinstance(got, dict) else got[1]
            if fused and count is not None:
                assert k == count, ("launches", k, count)
            check(got, fused)
    finally:
        dwt.set_option("wp_fused", 1)


def search_launches(levels, with_dst=True):
    """a cost launch behind the source and behind each level of the full tree, the selection, and with dst the
    pruned transform"""
    return (3 if with_dst else 2) * levels + 2


def wp2d_on_device(dwt, wavelet, inverse, x, levels):
    batch, H, W = x.shape
    d = Dev(dwt, x)
    dwt.packets.wp2d_batch(wp.WAVELET_ID[wavelet], inverse, d.ptr, d.ptr, 4 * W * H, batch, 4 * W, 4, W, H, levels)
    out = d.get()
    d.free()
    return out


# ---- expectations -----------------------------------------------------------------------------------------------
def node_counts(size_y, size_x, levels):
    n = np.zeros(qm.nq(levels))
    for (j, ky, kx), (x0, y0, w, h) in qm.rects(size_y, size_x, levels).items():
        n[qm.qindex(j, ky, kx)] = w * h
    return n


def same_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


def check_search(e, got, shape, cost, images=None, what=""):
    """the outputs of one search against the model's expectation e; images: the model image of every image of the call"""
    size_y, size_x, levels, _ = shape
    images = range(len(e["x"])) if images is None else images
    exact = cost[0] == qm.THRESHOLD
    count = node_counts(size_y, size_x, levels)
    for i, m in enumerate(images):
        want_c, own = e["cost"][m], e["own"][m]
        bound = (count + 16) * EPS * own  # (zero where a node's terms are all zero: exact there)
        if got["node_cost"] is not None:
            c = got["node_cost"][i]
            print(what, "image", i, "max |cost - model| / bound:", float(np.nanmax(np.abs(c - want_c) / np.where(bound > 0, bound, np.inf), initial=0)))
            if exact:
                assert same_f64(c, want_c), (what, i)
            else:
                assert (np.abs(c - want_c) <= bound).all(), (what, i, int(np.argmax(np.abs(c - want_c) - bound)))
        if got["tree"] is not None:
            assert got["tree"][i] == e["trees"][m], (what, i, "tree")
        if got["total"] is not None:
            # the leaves' own bounds, and half an ulp of a partial sum for each of the at most 3 * levels additions over a leaf
            t, want_t = got["total"][i], e["totals"][m]
            lv = qm.leaves(size_x, size_y, levels, e["trees"][m])
            tb = sum((w * h + 16 + 3 * levels) * EPS * own[qm.qindex(j, ky, kx)] for j, ky, kx, _, _, w, h in lv)
            print(what, "image", i, "total", t, "model", want_t, "bound", tb)
            assert (t == want_t) if exact else abs(t - want_t) <= tb, (what, i, t, want_t, tb)
            if got["node_cost"] is not None:
                assert t <= got["node_cost"][i][0], (what, i, "the total exceeds the root's cost")
    if got["coef"] is not None:
        want = e["coef"][list(images)]
        assert wp.same(got["coef"], want), (what, "coefficients", int((got["coef"].view(np.uint32) != want.view(np.uint32)).sum()))


def same_as(want, what=""):
    def check(got, fused):
        assert wp.same(got[0], want), (what, "wp_fused", fused, int((got[0].view(np.uint32) != want.view(np.uint32)).sum()))
    return check


# ---- the shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet,shape", qm.cases())
def test_search_and_trees(dwt, wavelet, shape):
    """every shape, the three wavelets, the four costs: the search (every output; in place and out of place in turn, so at
    odd and at even `levels`), then the transform in the trees found, forward and inverse; every leaf against wp2d_batch of
    its depth; the full tree against wp2d_batch.  The padded shape: row pitch and batch stride with padding and 64 KiB of
    canaries around dst, tree, total and node_cost"""
    size_y, size_x, levels, batch = shape
    lay = dict(row_gap=3, batch_gap=5, guard=BIG_GUARD) if shape == qm.PADDED_SHAPE else {}
    for i, cost in enumerate(qm.COSTS):
        e = qm.expected(wavelet, shape, cost)
        for in_place in ((i & 1, 1 - (i & 1)) if levels <= 3 else (i & 1,)):
            both_routes(dwt, lambda: run_best(dwt, wavelet, cost, e["x"], levels, in_place=bool(in_place), **lay),
                        lambda got, fused: check_search(e, got, shape, cost, what="%s %s cost %s fused %d" % (wavelet, shape, cost, fused)),
                        search_launches(levels))
    cost = qm.COSTS[1]
    e = qm.expected(wavelet, shape, cost)
    x, trees = e["x"], e["trees"]
    back = np.stack([qm.inv_qtree(wavelet, e["coef"][b], levels, trees[b]) for b in range(batch)])
    # (64 ulp of the largest sample a level: what a float lifting level and its inverse lose at these sizes, with room)
    assert np.abs(back - x).max() <= levels * 2.0 ** -18 * np.abs(x).max()
    both_routes(dwt, lambda: run_tree(dwt, wavelet, False, x, levels, trees, in_place=False, **lay), same_as(e["coef"], "forward"), levels)
    both_routes(dwt, lambda: run_tree(dwt, wavelet, True, e["coef"], levels, trees, **lay), same_as(back, "inverse"), levels)
    # a leaf of depth j: what dwt_hip_wp2d_batch(levels = j) gives at its place
    full = [x] + [wp2d_on_device(dwt, wavelet, False, x, j) for j in range(1, levels + 1)]
    for b in range(batch):
        for j, ky, kx, x0, y0, w, h in qm.leaves(size_x, size_y, levels, trees[b]):
            assert wp.same(e["coef"][b, y0:y0 + h, x0:x0 + w], full[j][b, y0:y0 + h, x0:x0 + w]), (b, j, ky, kx)
    # the full tree: the bits of wp2d_batch of the same depth, forward and inverse
    for inverse in (False, True):
        want = wp2d_on_device(dwt, wavelet, inverse, x, levels)
        both_routes(dwt, lambda: run_tree(dwt, wavelet, inverse, x, levels, qm.full_tree(levels), shared=True, in_place=inverse, **lay),
                    same_as(want, "full tree"), levels)


# ---- layouts, trees, outputs ------------------------------------------------------------------------------------
LAYOUTS = (dict(device=False), dict(es=8), dict(es=8, row_gap=2, batch_gap=6, device=False), dict(row_gap=1))


@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_layouts_and_outputs(dwt, wavelet):
    """host memory, elements 8 bytes apart, a padded pitch; in place and out of place; dst == NULL; single outputs; shared
    trees and trees with bits that cannot be reached"""
    shape = qm.LAYOUT_SHAPE
    size_y, size_x, levels, batch = shape
    for i, cost in enumerate(qm.COSTS):
        e = qm.expected(wavelet, shape, cost)
        lay = LAYOUTS[i % len(LAYOUTS)]
        fused = lay.get("device", True) and lay.get("es", 4) == 4
        what = "%s cost %s %s" % (wavelet, cost, lay)
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, e["x"], levels, in_place=bool(i & 1), **lay),
                    lambda got, f: check_search(e, got, shape, cost, what=what), search_launches(levels) if fused else None)
        # costs and tree only: no coefficient is stored; one output at a time
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, e["x"], levels, with_dst=False, **lay),
                    lambda got, f: check_search(e, got, shape, cost, what=what + " dst NULL"), search_launches(levels, False) if fused else None)
        only = ("tree", "total", "node_cost")[i % 3]
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, e["x"], levels, with_dst=bool(i & 1), outputs=(only,), **lay),
                    lambda got, f: check_search(e, got, shape, cost, what=what + " " + only), search_launches(levels, bool(i & 1)) if fused else None)
    e = qm.expected(wavelet, shape, qm.COSTS[0])
    both_routes(dwt, lambda: run_best(dwt, wavelet, qm.COSTS[0], e["x"], levels, with_dst=False),
                lambda got, f: check_search(e, got, shape, qm.COSTS[0], what="dense, dst NULL"), search_launches(levels, False))
    # trees: per image (test_search_and_trees), shared, with unreachable bits
    x = qm.expected(wavelet, shape, qm.COSTS[1])["x"]
    shared = qm.tree_of([0, 1, 3, 4, qm.qindex(2, 0, 1), qm.qindex(2, 2, 0), qm.qindex(2, 3, 3)])
    dirty = [a | b for a, b in zip(shared, qm.tree_of([qm.qindex(2, 0, 2), qm.qindex(2, 1, 3), qm.qindex(3, 0, 0), qm.qindex(3, 7, 7), 90, 340, 511]))]
    assert qm.effective(dirty, levels) == shared  # under the clear (1, 0, 1); levels 3 and beyond
    fwd = np.stack([qm.fwd_qtree(wavelet, img, levels, shared) for img in x])
    inv = np.stack([qm.inv_qtree(wavelet, img, levels, shared) for img in fwd])
    for i, lay in enumerate(LAYOUTS + ({},)):
        count = levels if lay.get("device", True) and lay.get("es", 4) == 4 else None
        for tree in (shared, dirty):
            both_routes(dwt, lambda: run_tree(dwt, wavelet, False, x, levels, tree, shared=True, in_place=bool(i & 1), **lay), same_as(fwd, lay), count)
            both_routes(dwt, lambda: run_tree(dwt, wavelet, True, fwd, levels, tree, shared=True, in_place=not i & 1, **lay), same_as(inv, lay), count)
    per_image = [dirty, qm.tree_of([]), qm.tree_of([1, 2, 3, 4, 200])]  # (the third: the root is clear, nothing is split)
    want = x.copy()
    want[0] = fwd[0]
    both_routes(dwt, lambda: run_tree(dwt, wavelet, False, x, levels, per_image, in_place=False), same_as(want, "per image"), levels)


# ---- special images ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_all_zero_images(dwt, wavelet):
    """exact ties everywhere: every cost 0, the root-only tree, total 0, the images untouched"""
    x = np.zeros((2, 8, 8), F32)
    for cost in qm.COSTS:
        def check(got, fused):
            assert not got["node_cost"].any() and not np.signbit(got["node_cost"]).any() and not got["total"].any()
            assert all(t == qm.tree_of([]) for t in got["tree"]) and wp.same(got["coef"], x)
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, x, 3), check, search_launches(3))


@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_nan_image_position_and_determinism(dwt, wavelet):
    """an image with one NaN sample keeps its root whole (NaN total), its neighbours in the batch as if it were not there.
    The same image at positions 0 and 2 of the batch: the same bits in every output.  Two identical calls: identical bytes."""
    shape = qm.LAYOUT_SHAPE
    size_y, size_x, levels, batch = shape
    for cost in qm.COSTS:
        e = qm.expected(wavelet, shape, cost)
        x = e["x"].copy()
        x[1, 40, 70] = np.nan
        x[2] = x[0]

        def check(got, fused):
            assert got["tree"][1] == qm.tree_of([]) and math.isnan(got["total"][1]) and math.isnan(got["node_cost"][1, 0])
            assert wp.same(got["coef"][1], x[1])
            for key in ("node_cost", "total", "coef"):
                assert got[key][0].tobytes() == got[key][2].tobytes(), key
            assert got["tree"][0] == got["tree"][2]
            sub = dict(got, node_cost=got["node_cost"][[0, 2]], total=got["total"][[0, 2]], coef=got["coef"][[0, 2]], tree=[got["tree"][0], got["tree"][2]])
            check_search(e, sub, shape, cost, images=[0, 0], what="beside a NaN image")
            again = run_best(dwt, wavelet, cost, x, levels)
            for key in ("node_cost", "total", "coef"):
                assert again[key].tobytes() == got[key].tobytes(), ("two calls", key)
            assert again["tree"] == got["tree"]
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, x, levels), check, search_launches(levels))


def test_launch_count_does_not_depend_on_the_batch(dwt):
    """the fused route: DESIGN.md's formula, for batch 1 and batch 3 alike, for two shapes"""
    for shape in ((67, 130, 3, 3), (160, 96, 4, 2)):
        size_y, size_x, levels, _ = shape
        x = qm.expected("cdf53_s", shape, qm.COSTS[3])["x"]
        for batch in (1, 3):
            xb = np.ascontiguousarray(np.concatenate([x, x])[:batch])
            for with_dst in (True, False):
                got = run_best(dwt, "cdf53_s", qm.COSTS[3], xb, levels, with_dst=with_dst)
                assert got["launches"] == search_launches(levels, with_dst), (shape, batch, with_dst, got["launches"])
            assert run_tree(dwt, "cdf53_s", False, xb, levels, qm.full_tree(levels), shared=True)[1] == levels


@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_joint_qtree(dwt, wavelet):
    """wp_joint_qtree: the model's selection on the float64 sum of the model's tables; the batch then transforms in it"""
    size_y, size_x, levels, batch = qm.LAYOUT_SHAPE
    e = qm.expected(wavelet, qm.LAYOUT_SHAPE, qm.JOINT_COST)
    want = qm.select(qm.joint_tables(wavelet)[0], levels)[0]
    fwd = np.stack([qm.fwd_qtree(wavelet, img, levels, want) for img in e["x"]])
    geom = (4 * size_x * size_y, batch, 4 * size_x, 4, size_x, size_y, levels)
    try:
        for fused in (1, 0):
            dwt.set_option("wp_fused", fused)
            for device in (True, False):
                x = Mem(dwt, e["x"].copy(), device)
                tree = dwt.packets.wp_joint_qtree(wp.WAVELET_ID[wavelet], qm.JOINT_COST[0], qm.JOINT_COST[1], x.ptr, *geom)
                assert tree == want, (fused, device)
                dwt.packets.wp_tree2d_batch(wp.WAVELET_ID[wavelet], False, x.ptr, x.ptr, *geom, tree)
                dwt.sync()
                assert wp.same(x.get(), fwd), (fused, device)
    finally:
        dwt.set_option("wp_fused", 1)


# ---- errors -----------------------------------------------------------------------------------------------------
def test_errors(dwt):
    L = dwt.lib
    x = Dev(dwt, np.zeros(2 * 64 * 64, F32))
    t = Dev(dwt, np.zeros(64, np.uint32))
    c = Dev(dwt, np.zeros(4096, np.float64))
    host = np.zeros(2 * 64 * 64, F32)
    host_tree = np.zeros(64, np.uint32)

    def refused(rc):
        assert rc != 0 and len(dwt.last_error()) > 10

    def best(wavelet=0, cost=0, param=0.0, src=x.ptr, dst=x.ptr, W=64, H=64, levels=2, tree=t.ptr, tree_stride=64, total=c.ptr, node_cost=None,
             cost_stride=None, bs=None):
        return L.dwt_hip_wp_best2d_batch(wavelet, cost, param, src, dst, 4 * W * H if bs is None else bs, 2, 4 * W, 4, W, H, levels, tree, tree_stride,
                                         total, node_cost, 8 * qm.nq(max(min(levels, 6), 0)) if cost_stride is None else cost_stride)

    def tree(wavelet=0, src=x.ptr, dst=x.ptr, W=64, H=64, levels=2, tr=t.ptr, tree_stride=64):
        return L.dwt_hip_wp_tree2d_batch(wavelet, 0, src, dst, 4 * W * H, 2, 4 * W, 4, W, H, levels, tr, tree_stride)

    assert best() == 0 and tree() == 0 and tree(tree_stride=0) == 0 and best(levels=5) == 0 and tree(levels=5) == 0, dwt.last_error()
    for W, H, levels in ((64, 64, 0), (64, 64, 6), (64, 64, -1), (64, 16, 5), (31, 64, 5), (64, 2, 2), (1, 64, 1)):
        refused(best(W=W, H=H, levels=levels))
        refused(tree(W=W, H=H, levels=levels))
    for wavelet in (1, 3, 4, 5, 7, 8, 9, -1, 77):
        refused(best(wavelet=wavelet))
        refused(tree(wavelet=wavelet))
    for cost, param in ((-1, 0.0), (4, 0.0), (2, 0.0), (2, 2.0), (2, -1.0), (2, math.nan), (3, -0.5), (3, math.nan), (3, math.inf)):
        refused(best(cost=cost, param=param))
    assert best(cost=2, param=1.5) == 0 and best(cost=3, param=0.0) == 0, dwt.last_error()
    refused(best(dst=None, tree=None, total=None, node_cost=None))  # every output NULL
    assert best(dst=None, tree=None, total=None, node_cost=c.ptr) == 0, dwt.last_error()
    for stride in (32, 60, 66, 0):
        refused(best(tree_stride=stride))
    for stride in (32, 60, 66):
        refused(tree(tree_stride=stride))
    refused(tree(tr=None))
    refused(best(node_cost=c.ptr, cost_stride=8 * 20))  # 21 doubles a table at 2 levels
    refused(best(node_cost=c.ptr, cost_stride=8 * 21 + 4))
    assert best(node_cost=c.ptr, cost_stride=8 * 21) == 0, dwt.last_error()
    refused(best(bs=4 * 64 * 64 - 4))  # images that share samples
    # mixed host and device pointers
    refused(best(src=host.ctypes.data, dst=host.ctypes.data))
    refused(best(dst=host.ctypes.data))
    refused(best(tree=host_tree.ctypes.data))
    refused(tree(tr=host_tree.ctypes.data))
    refused(tree(src=host.ctypes.data, dst=host.ctypes.data))
    dwt.sync()
    for d in (x, t, c):
        d.free()


# ---- example ----------------------------------------------------------------------------------------------------
def test_example_texture_best_basis(dwt, tmp_path):
    """examples/texture_best_basis.c: two textures in a resident batch, the joint tree, the transform in it, its leaves, the
    round trip"""
    exe, libdir = tmp_path / "texture_best_basis", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "texture_best_basis.c"),
                           "-o", str(exe), "-L" + libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "texture best basis: success" in out.stdout + out.stderr, out.stdout + out.stderr


# ---- stream -----------------------------------------------------------------------------------------------------
def test_entries_run_on_the_callers_stream():
    """both device entries on both routes, once on a non-blocking stream behind a bounded delay, in a process of its own
    (tests/wp_basis2d_stream.py, on the harness of tests/stream_cases.py): the model's results, queued without waiting for
    the stream, the launch count of the warm-up"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wp_basis2d_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]
