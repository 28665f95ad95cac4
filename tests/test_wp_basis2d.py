"""CPU checks of the quadtree helpers (dwt_hip_wp_best_qtree, dwt_hip_wp_qtree_leaves; libdwt_amd/packets.py) and of the
model tests/wp_basis2d_model.py, and two conditions of every input that tests/test_hip_wp_basis2d.py sends to the GPU:

* no node of a float cost may lie within 1e-9 * S[q] of a tie.  The device's double sums are within about
  (n + 16) 2^-52 S[q] of the model's; n is at most 65536 in these cases, 1.5e-11 S[q], so the margin is more than 60 x that
  bound.  The cap on left-out nodes is ZERO, and a seed that has one is replaced in the case table of wp_basis2d_model.py,
  never skipped;
* the model tree of every input is neither the root alone nor the full tree, and at least one case has leaves on three
  different levels -- a search that always or never splits would pass the GPU tests on trivial trees."""
import math
import os
import subprocess

import numpy as np
import pytest

import wp_basis2d_model as qm
import wp_model as wp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def packets():
    from libdwt_amd import packets as p
    return p


def same_total(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


# ---- dwt_hip_wp_best_qtree --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", (1, 2))
def test_best_qtree_is_the_brute_force_minimum(packets, levels):
    """random integer tables with many ties: the total is the minimum over ALL quadtrees (2 at one level, 17 at two), and
    the chosen tree is the shallowest among the minima: a node is split only where that is strictly cheaper"""
    rng = np.random.default_rng(50 + levels)
    trees = qm.all_trees(levels)
    assert len(trees) == (2, 17)[levels - 1]
    for _ in range(40):
        cost = [float(v) for v in rng.integers(0, 4 + 8 * (levels - 1), qm.nq(levels))]
        tree, total = packets.wp_best_qtree(levels, cost)
        want_tree, want_total, best = qm.select(cost, levels)
        assert tree == want_tree and total == want_total
        assert total == min(qm.tree_cost(cost, t) for t in trees)
        splits = {q for q in range(qm.nq(levels - 1)) if qm.bit(tree, q)}
        assert qm.tree_cost(cost, splits) == total and qm.effective(tree, levels) == tree
        for j, ky, kx in qm.nodes(levels - 1):
            q = qm.qindex(j, ky, kx)
            kids = sum(min(cost[qm.qindex(*c)], best[qm.qindex(*c)]) for c in qm.children(j, ky, kx))
            if q in splits:
                assert kids < cost[q], (q, cost)
            elif j == 0 or qm.qindex(j - 1, ky >> 1, kx >> 1) in splits:
                assert not kids < cost[q], (q, cost)


def test_all_trees_counts():
    # T(0) = 1, T(d) = 1 + T(d-1)^4
    assert [len(qm.all_trees(d)) for d in (0, 1, 2)] == [1, 2, 17]


def test_best_qtree_equals_the_model_at_5_levels(packets):
    rng = np.random.default_rng(51)
    depth = np.concatenate([np.full(4 ** j, j) for j in range(6)])
    deepest = False
    for k in range(8):
        cost = (0.6 + rng.random(qm.nq(5))) * 4.0 ** -depth  # four children cost about what their parent does
        if k & 1:
            cost = np.round(cost * 4096)  # with ties
        tree, total, _ = qm.select(cost, 5)
        got_tree, got_total = packets.wp_best_qtree(5, cost)
        assert got_tree == tree and got_total == total
        deepest = deepest or any(qm.bit(tree, q) for q in range(qm.qbase(4), qm.qbase(5)))
    assert deepest  # the deepest level is reached


def test_tie_and_nan_keep_the_parent(packets):
    assert packets.wp_best_qtree(1, [4.0, 1.0, 1.0, 1.0, 1.0]) == (qm.tree_of([]), 4.0)  # a tie
    assert packets.wp_best_qtree(1, [4.5, 1.0, 1.0, 1.0, 1.0]) == (qm.tree_of([0]), 4.0)
    for bad in range(5):
        cost = [10.0, 1.0, 1.0, 1.0, 1.0]
        cost[bad] = math.nan
        tree, total = packets.wp_best_qtree(1, cost)
        assert tree == qm.tree_of([]) and same_total(total, cost[0])
    # a NaN two levels down: its parent keeps whole, the root still splits
    cost = [100.0, 4.0, 4.0, 4.0, 4.0] + [0.5] * 16
    cost[5 + 2] = math.nan  # node (2, 0, 2): a child of (1, 0, 1)
    tree, total = packets.wp_best_qtree(2, cost)
    want, want_total, _ = qm.select(cost, 2)
    assert tree == want and total == want_total == 4.0 + 2.0 * 3
    assert qm.bit(tree, 0) and qm.bit(tree, 1) and not qm.bit(tree, 2) and qm.bit(tree, 3) and qm.bit(tree, 4)


def test_best_qtree_refuses_bad_levels(packets):
    for levels in (0, 6, -1):
        with pytest.raises(Exception):
            packets.wp_best_qtree(levels, [0.0] * 6000)
    with pytest.raises(Exception):
        packets.wp_best_qtree(2, [0.0] * 20)  # a table of 21 costs


# ---- dwt_hip_wp_qtree_leaves, bitmaps ---------------------------------------------------------------------------------
def test_dirty_bitmaps_equal_their_effective_tree(packets):
    rng = np.random.default_rng(52)
    for levels in range(1, 6):
        for _ in range(6):
            dirty = [int(v) for v in rng.integers(0, 1 << 32, 16, dtype=np.uint64)]
            dirty[0] |= rng.integers(0, 2) * 0b11111  # often the root and level 1 split
            eff = qm.effective(dirty, levels)
            assert qm.effective(eff, levels) == eff
            assert packets.wp_qtree_leaves(70, 67, levels, dirty) == packets.wp_qtree_leaves(70, 67, levels, eff) == qm.leaves(70, 67, levels, eff)
    # set bits under a clear one, and bits of levels >= `levels`
    tree = qm.tree_of([0, 1, 5, 6, qm.qindex(2, 3, 3), qm.qindex(3, 0, 0), qm.qindex(3, 7, 7), 340, 400, 511])
    want = qm.tree_of([0, 1, 5, 6, qm.qindex(3, 0, 0)])  # (2, 3, 3) hangs under the clear (1, 1, 1); (3, 0, 0) under (2, 0, 0) = 5
    assert qm.effective(tree, 5) == want
    assert packets.wp_qtree_leaves(64, 64, 5, tree) == qm.leaves(64, 64, 5, want)
    assert packets.wp_qtree_leaves(64, 64, 2, tree) == qm.leaves(64, 64, 2, qm.tree_of([0, 1]))


def test_leaves_tile_the_image_and_agree_with_wp_nodes(packets):
    """sizes 2 .. 70 per axis (every x size against a few y sizes and the other way round), the full tree, the root, noise"""
    rng = np.random.default_rng(53)
    pairs = {(n, m) for n in range(2, 71) for m in (2, 3, 37, 64, 70, n)} | {(m, n) for n in range(2, 71) for m in (2, 5, 33, 70)}
    for size_x, size_y in sorted(pairs):
        levels = min(wp.floor_log2(min(size_x, size_y)), qm.QTREE_MAX_LEVELS)
        r = qm.rects(size_y, size_x, levels)
        for tree in (qm.full_tree(levels), qm.tree_of([]), [int(v) | 1 for v in rng.integers(0, 1 << 32, 16, dtype=np.uint64)]):
            got = packets.wp_qtree_leaves(size_x, size_y, levels, tree)
            assert got == qm.leaves(size_x, size_y, levels, tree)
            seen = np.zeros((size_y, size_x), np.int32)
            for j, ky, kx, x0, y0, w, h in got:
                assert (x0, y0, w, h) == r[(j, ky, kx)] and w >= 1 and h >= 1
                seen[y0:y0 + h, x0:x0 + w] += 1
            assert (seen == 1).all()
        assert len(packets.wp_qtree_leaves(size_x, size_y, levels, qm.full_tree(levels))) == 4 ** levels
        # the geometry is that of dwt_hip_wp_nodes along each axis
        xs, ys = packets.wp_nodes(size_x, levels), packets.wp_nodes(size_y, levels)
        for j, ky, kx, x0, y0, w, h in packets.wp_qtree_leaves(size_x, size_y, levels, qm.full_tree(levels)):
            assert (x0, w, y0, h) == (xs[0][kx], xs[1][kx], ys[0][ky], ys[1][ky])
    none = [None] * 7
    words = (packets.C.c_uint32 * 16)()
    assert packets.lib.dwt_hip_wp_qtree_leaves(100, 7, 3, words, *none) == -1
    assert packets.lib.dwt_hip_wp_qtree_leaves(4096, 4096, 6, words, *none) == -1
    assert packets.lib.dwt_hip_wp_qtree_leaves(64, 64, 0, words, *none) == -1


# ---- the model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_model_trees_against_wp_model(wavelet):
    """the full tree is wp_model.fwd2d; a pruned tree's leaf is the node of the full tree of its depth; the inverse undoes
    the forward, node by node"""
    x = qm.texture(77, 37, 50)
    for levels in (1, 3, 5):
        full = qm.full_tree(levels)
        assert wp.same(qm.fwd_qtree(wavelet, x, levels, full), wp.fwd2d(wavelet, x, levels))
        assert wp.same(qm.inv_qtree(wavelet, x, levels, full), wp.inv2d(wavelet, x, levels))
    tree = qm.tree_of([0, 1, 3, qm.qindex(2, 0, 1), qm.qindex(2, 2, 0), qm.qindex(3, 7, 7), qm.qindex(3, 0, 2)])  # ((3, 7, 7) cannot be reached)
    y = qm.fwd_qtree(wavelet, x, 5, tree)
    stages = qm.full_levels(wavelet, x[None], 5)
    lv = qm.leaves(50, 37, 5, tree)
    assert sorted({l[0] for l in lv}) == [1, 2, 3, 4]
    for j, ky, kx, x0, y0, w, h in lv:
        assert wp.same(y[y0:y0 + h, x0:x0 + w], stages[j][0, y0:y0 + h, x0:x0 + w])
    back = qm.inv_qtree(wavelet, y, 5, tree)
    assert np.abs(back - x).max() < 1e-4
    assert wp.same(qm.fwd_qtree(wavelet, x, 5, tree), qm.fwd_qtree(wavelet, x, 5, qm.effective(tree, 5)))


# ---- the conditions of every GPU input --------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet,shape", qm.cases())
def test_gpu_inputs_hold_no_near_tie_and_have_non_trivial_trees(wavelet, shape):
    size_y, size_x, levels, batch = shape
    for cost in qm.COSTS:
        e = qm.expected(wavelet, shape, cost)
        for b in range(batch):
            bad = qm.near_ties(e["cost"][b], e["mass"][b], levels, float_kind=cost[0] != qm.THRESHOLD)
            assert bad == [], (wavelet, shape, cost, b, bad)
            assert e["trees"][b] != qm.tree_of([]) and e["trees"][b] != qm.full_tree(levels), (wavelet, shape, cost, b)


def test_a_case_has_leaves_on_three_levels():
    e = qm.expected("cdf97_s", (67, 130, 3, 3), (qm.SHANNON, 0.0))
    assert len({l[0] for l in qm.leaves(130, 67, 3, e["trees"][0])}) >= 3


def test_joint_table_holds_no_near_tie_and_a_non_trivial_tree():
    levels = qm.LAYOUT_SHAPE[2]
    for wavelet in wp.WAVELETS:
        cost, mass = qm.joint_tables(wavelet)
        assert qm.near_ties(cost, mass, levels) == []
        assert qm.select(cost, levels)[0] not in (qm.tree_of([]), qm.full_tree(levels))


def test_stream_input_holds_no_near_tie():
    """the input that tests/wp_basis2d_stream.py compares (seed 0; the other one only fills buffers)"""
    import wp_basis2d_stream as st

    stages = qm.full_levels(st.WAVELET, st.images(0), st.LEVELS)
    cost, mass, _ = qm.cost_tables(st.LOG_ENERGY[0], st.LOG_ENERGY[1], stages, st.LEVELS)
    for b in range(st.BATCH):
        assert qm.near_ties(cost[b], mass[b], st.LEVELS) == []
        assert qm.select(cost[b], st.LEVELS)[0] not in (qm.tree_of([]), qm.full_tree(st.LEVELS))


def test_all_zero_images_are_exact_ties():
    stages = qm.full_levels("cdf97_s", np.zeros((1, 8, 8), np.float32), 3)
    for kind, param in qm.COSTS:
        cost, mass, _ = qm.cost_tables(kind, param, stages, 3)
        assert not cost.any() and not mass.any()
        assert qm.select(cost[0], 3)[:2] == (qm.tree_of([]), 0.0)


# ---- the host helpers under the sanitizers ----------------------------------------------------------------------------
def test_host_helpers_under_asan_ubsan(tmp_path):
    """tests/san/san_wp_qtree.c: a stand-alone program around libdwt_amd/csrc/dwt_wp_tree.c, built with
    -fsanitize=address,undefined and run on the CPU; any report aborts it"""
    exe = tmp_path / "san_wp_qtree"
    subprocess.check_call(["gcc", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g",
                           "-O1", os.path.join(ROOT, "tests", "san", "san_wp_qtree.c"), os.path.join(ROOT, "libdwt_amd", "csrc", "dwt_wp_tree.c"),
                           "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "san_wp_qtree: OK" in out.stdout, out.stdout + out.stderr
