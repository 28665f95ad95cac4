"""CPU checks of the best-basis helpers (dwt_hip_wp_best_tree, dwt_hip_wp_tree_leaves; libdwt_amd/packets.py) and of the
model tests/wp_basis_model.py, and the near-tie condition of every input that tests/test_hip_wp_basis.py sends to the GPU:
no node of a float cost may lie within 1e-9 * S[h] of a tie (the device's double sums are within about (N + 16) 2^-52 S[h] ~
2e-12 S[h] of the model's, so the margin has 500x headroom; the cap is ZERO, and a seed that has one is replaced in the case
table of wp_basis_model.py, never skipped)."""
import math

import numpy as np
import pytest

import wp_basis_model as bm
import wp_model as wp


@pytest.fixture(scope="module")
def packets():
    from libdwt_amd import packets as p
    return p


# ---- dwt_hip_wp_best_tree ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", (1, 2, 3))
def test_best_tree_is_the_brute_force_minimum(packets, levels):
    """random integer tables with many ties: the total is the minimum over ALL trees, and along every path the chosen tree
    is the shallowest among the minima (a node is split only where that is strictly cheaper than keeping it)"""
    rng = np.random.default_rng(40 + levels)
    trees = bm.all_trees(levels)
    for _ in range(60):
        cost = [0.0] + [float(v) for v in rng.integers(0, 4, (2 << levels) - 1)]
        tree, total = packets.wp_best_tree(levels, cost)
        assert total == min(bm.tree_cost(cost, t) for t in trees)
        splits = {h for h in range(1, 1 << levels) if bm.bit(tree, h)}
        assert bm.tree_cost(cost, splits) == total and bm.effective(tree, levels) == tree
        # the best cost of every subtree, by brute force over the subtree's own trees
        best = {}
        for h in range((2 << levels) - 1, 0, -1):
            best[h] = cost[h] if h >= (1 << levels) else min(cost[h], best[2 * h] + best[2 * h + 1])
        for h in splits:  # strictly cheaper than stopping here
            assert best[2 * h] + best[2 * h + 1] < cost[h], (h, cost)
        for h in range(1, 1 << levels):  # a reachable node that is kept: splitting is not strictly cheaper
            if h not in splits and (h == 1 or (h >> 1) in splits):
                assert not best[2 * h] + best[2 * h + 1] < cost[h], (h, cost)


def test_best_tree_equals_the_model_at_10_levels(packets):
    rng = np.random.default_rng(41)
    depth = np.floor(np.log2(np.maximum(np.arange(2 << 10), 1)))
    deepest = False
    for k in range(8):
        cost = (0.6 + rng.random(2 << 10)) * 2.0 ** -depth  # two children cost about what their parent does
        if k & 1:
            cost = np.round(cost * 4096)  # with ties
        tree, total, _ = bm.select(cost, 10)
        got_tree, got_total = packets.wp_best_tree(10, cost)
        assert got_tree == tree and got_total == total
        deepest = deepest or any(bm.bit(tree, h) for h in range(512, 1024))
    assert deepest  # the deepest level is reached


def test_nan_keeps_the_parent(packets):
    for bad in (1, 2, 3, 5):
        cost = [0.0, 10.0, 1.0, 1.0, 0.25, 0.25, 0.25, 0.25]
        cost[bad] = math.nan
        tree, total = packets.wp_best_tree(2, cost)
        want, want_total, _ = bm.select(cost, 2)
        assert tree == want and (total == want_total or (math.isnan(total) and math.isnan(want_total)))
        assert not bm.bit(tree, 1) if bad in (1, 2, 3) else bm.bit(tree, 1) and not bm.bit(tree, 2)
    assert packets.wp_best_tree(1, [0.0, math.nan, 0.0, 0.0]) == (bm.tree_of([]), pytest.approx(math.nan, nan_ok=True))


def test_best_tree_refuses_bad_levels(packets):
    for levels in (0, 11, -1):
        with pytest.raises(Exception):
            packets.wp_best_tree(levels, [0.0] * 4096)


# ---- dwt_hip_wp_tree_leaves -------------------------------------------------------------------------------------------
def test_leaves_tile_the_line_and_agree_with_wp_nodes(packets):
    rng = np.random.default_rng(42)
    for N in range(2, 301):
        levels = min(wp.floor_log2(N), 10)
        tables = [wp.nodes_recursive(N, j) for j in range(levels + 1)]
        for tree in (bm.full_tree(levels), bm.tree_of([]), [int(v) for v in rng.integers(0, 1 << 32, 32, dtype=np.uint64)]):
            got = packets.wp_tree_leaves(N, levels, tree)
            assert got == bm.leaves(N, levels, tree)
            pos = 0
            for j, k, s, n in got:
                assert (s, n) == tables[j][k] and s == pos and n >= 1
                pos += n
            assert pos == N
        assert len(packets.wp_tree_leaves(N, levels, bm.full_tree(levels))) == 1 << levels
    assert packets.lib.dwt_hip_wp_tree_leaves(100, 7, (packets.C.c_uint32 * 32)(), None, None, None, None) == -1
    assert packets.lib.dwt_hip_wp_tree_leaves(4096, 11, (packets.C.c_uint32 * 32)(), None, None, None, None) == -1


def test_unreachable_bits_are_ignored(packets):
    tree = bm.tree_of([1, 2, 4, 6, 7, 13, 100, 1023])  # 6, 7 hang under the clear bit 3; 13, 100, 1023 under clear ones too
    want = bm.tree_of([1, 2, 4])
    assert bm.effective(tree, 10) == want
    assert packets.wp_tree_leaves(1000, 9, tree) == packets.wp_tree_leaves(1000, 9, want) == bm.leaves(1000, 9, want)
    assert [l[:2] for l in packets.wp_tree_leaves(1000, 9, tree)] == [(3, 0), (3, 1), (2, 1), (1, 1)]
    # bit 0 and the bits of levels >= `levels` mean nothing
    assert packets.wp_tree_leaves(1000, 2, bm.tree_of([0, 1, 2, 4, 8])) == bm.leaves(1000, 2, bm.tree_of([1, 2]))


# ---- the model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_model_trees_against_wp_model(wavelet):
    """the full tree is wp_model.fwd1d; a pruned tree's leaf is the node of the full tree of its depth; the inverse undoes
    the forward to the bits of wp_model's one-level inverse"""
    x = wp.make_input(77, "normal", 3, 100)
    for levels in (1, 3, 6):
        full = bm.full_tree(levels)
        assert wp.same(bm.fwd_tree(wavelet, x, levels, full), wp.fwd1d(wavelet, x, levels))
        assert wp.same(bm.inv_tree(wavelet, x, levels, full), wp.inv1d(wavelet, x, levels))
    tree = bm.tree_of([1, 2, 5, 10, 3, 6, 40])  # (40 cannot be reached: 20 is clear)
    y = bm.fwd_tree(wavelet, x, 6, tree)
    stages = bm.full_levels(wavelet, x, 6)
    for j, k, s, n in bm.leaves(100, 6, tree):
        assert wp.same(y[:, s:s + n], stages[j][:, s:s + n])
    back = bm.inv_tree(wavelet, y, 6, tree)
    assert np.abs(back - x).max() < 1e-4
    # the mirror, node by node
    z = y.copy()
    for j, s, n in sorted(bm._split_nodes(100, 6, tree), reverse=True):
        z[:, s:s + n] = wp._line_inv(wavelet, z[:, s:s + n])
    assert wp.same(back, z)


def test_terms_scalar_and_vector_agree():
    v = np.concatenate([wp.make_input(5, "normal", 1, 200)[0], wp.make_input(6, "tiny", 1, 200)[0],
                        np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0], np.float32)])
    for kind, param in bm.COSTS:
        t = bm.terms(kind, param, v)
        for c, got in zip(v, t):
            want = bm.term(kind, param, c)
            assert (math.isnan(want) and math.isnan(got)) or abs(got - want) <= 4 * 2.0 ** -52 * abs(want), (kind, c, got, want)
    assert all(math.isnan(bm.term(k, p, c)) for k, p in bm.COSTS for c in (np.nan, np.inf, -np.inf))


# ---- the near-tie condition of every GPU input ------------------------------------------------------------------------
def _no_near_tie(wavelet, kind_name, shape, cost):
    e = bm.expected(wavelet, kind_name, shape, cost)
    for y in range(shape[0]):
        bad = bm.near_ties(e["cost"][y], e["mass"][y], shape[2], float_kind=cost[0] != bm.THRESHOLD)
        assert bad == [], (wavelet, kind_name, shape, cost, y, bad)


@pytest.mark.parametrize("wavelet,kind_name,shape,costs", bm.shape_cases() + bm.layout_cases() + bm.extra_cases())
def test_gpu_inputs_hold_no_near_tie(wavelet, kind_name, shape, costs):
    for cost in costs:
        _no_near_tie(wavelet, kind_name, shape, cost)


def test_stream_input_holds_no_near_tie():
    """the input that tests/wp_basis_stream.py compares (seed 0; the other one only fills buffers)"""
    import wp_basis_stream as st

    stages = bm.full_levels(st.WAVELET, st.lines(0), st.LEVELS)
    cost, mass, _ = bm.cost_tables(st.SHANNON[0], st.SHANNON[1], stages, st.LEVELS)
    for y in range(st.N_LINES):
        assert bm.near_ties(cost[y], mass[y], st.LEVELS) == []


def test_tones_keep_their_band():
    """what tests/test_hip_wp_basis.py asks of the device's tree holds for the model's"""
    perm = wp.freq_order(3)
    for f in range(8):
        e = bm.expected("cdf97_s", "tone%d" % f, bm.TONE_SHAPE, bm.JOINT_COST)
        assert (3, perm[f]) in [l[:2] for l in bm.leaves(256, 3, e["trees"][0])], (f, e["trees"][0][0])


def test_joint_table_holds_no_near_tie():
    for wavelet in wp.WAVELETS:
        cost, mass = bm.joint_tables(wavelet)
        assert bm.near_ties(cost, mass, bm.LAYOUT_SHAPE[2]) == []


def test_all_zero_lines_are_exact_ties():
    """every cost of an all-zero line is 0 (log-energy and Shannon by their e == 0 branch): the root-only tree, total 0"""
    stages = bm.full_levels("cdf97_s", np.zeros((1, 37), np.float32), 5)
    for kind, param in bm.COSTS:
        cost, mass, _ = bm.cost_tables(kind, param, stages, 5)
        assert not cost.any() and not mass.any()
        assert bm.select(cost[0], 5)[:2] == (bm.tree_of([]), 0.0)


# ---- the host helpers under the sanitizers ----------------------------------------------------------------------------
def test_host_helpers_under_asan_ubsan(tmp_path):
    """tests/san/san_wp_tree.c: a stand-alone program around libdwt_amd/csrc/dwt_wp_tree.c, built with
    -fsanitize=address,undefined and run on the CPU; any report aborts it"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "san_wp_tree"
    subprocess.check_call(["gcc", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g",
                           "-O1", os.path.join(root, "tests", "san", "san_wp_tree.c"), os.path.join(root, "libdwt_amd", "csrc", "dwt_wp_tree.c"),
                           "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "san_wp_tree: OK" in out.stdout, out.stdout + out.stderr
