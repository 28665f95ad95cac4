"""GPU checks of the best-basis search and of pruned wavelet packet trees (dwt_hip_wp_best1d_batch, dwt_hip_wp_tree1d_batch,
wp_joint_basis; libdwt_amd/packets.py) against tests/wp_basis_model.py.  Coefficients and trees compare bit for bit (a NaN on
both sides is not compared); the costs of the THRESHOLD kind and of all-zero lines compare exactly, those of the float kinds
within (n + 16) 2^-52 sum|term| of the model's fsum -- the derived bound of a double sum of n terms in any order plus a few
ulp per log / pow, not a measured figure.  The trees are the model's EXACTLY because no input holds a near-tie
(tests/test_wp_basis.py asserts that for every case of the tables in wp_basis_model.py).  Every buffer is filled with a canary
first and every word outside the addressed ones must still hold it; src of an out-of-place call must come back as it was.
Every case runs on the one-launch route (exactly 1 launch) and under option "wp_fused" = 0."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import wp_basis_model as bm
import wp_model as wp
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
CANARY = np.uint32(0xDEADBEEF)
CANARY64 = np.uint64(0xDEADBEEFDEADBEEF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N1D_MAX = 8192
TW = bm.TREE_WORDS + 4  # words between the trees of two lines: 16 bytes of gap
EPS = 2.0 ** -52


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
class Lines:
    """n_lines x N floats laid out in a canary-filled word buffer: elements es bytes apart, `gap` extra words between
    lines, the base `off` words past the allocation"""

    def __init__(self, x, es=4, gap=0, off=0):
        self.n_lines, self.N = x.shape
        step = es // 4
        self.es, self.off, self.pe = es, off, self.N * step + gap
        self.words = off + self.n_lines * self.pe + 8
        self.idx = (off + np.arange(self.n_lines)[:, None] * self.pe + np.arange(self.N)[None, :] * step).reshape(-1)
        self.filled = np.full(self.words, CANARY, np.uint32)
        self.filled[self.idx] = x.view(np.uint32).reshape(-1)

    def blank(self):
        return np.full(self.words, CANARY, np.uint32)

    def lines_of(self, buf):
        rest = np.ones(self.words, bool)
        rest[self.idx] = False
        assert (buf[rest] == CANARY).all(), "bytes outside the lines were written"
        return buf[self.idx].view(F32).reshape(self.n_lines, self.N)


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


def run_best(dwt, wavelet, cost, x, levels, es=4, gap=0, off=0, in_place=False, device=True, with_dst=True,
             outputs=("tree", "total", "node_cost")):
    """-> dict(coef, tree, total, node_cost, launches); what was not asked for is None"""
    n_lines, N = x.shape
    nt, cd = 2 << levels, (2 << levels) + 2
    lay = Lines(x, es, gap, off)
    src = Mem(dwt, lay.filled.copy(), device)
    dst = src if in_place else Mem(dwt, lay.blank(), device)
    tree = Mem(dwt, np.full(n_lines * TW + 4, CANARY, np.uint32), device) if "tree" in outputs else None
    total = Mem(dwt, np.full(n_lines + 2, CANARY64, np.uint64), device) if "total" in outputs else None
    nc = Mem(dwt, np.full(n_lines * cd + 2, CANARY64, np.uint64), device) if "node_cost" in outputs else None
    k = launches(dwt, lambda: dwt.packets.wp_best1d_batch(
        wp.WAVELET_ID[wavelet], cost[0], cost[1], src.ptr + 4 * off, dst.ptr + 4 * off if with_dst else None, lay.pe * 4, es, n_lines, N,
        levels, tree=tree and tree.ptr, tree_stride=4 * TW, total=total and total.ptr, node_cost=nc and nc.ptr, cost_stride=8 * cd))
    dwt.sync()
    out = dict(launches=k, coef=None, tree=None, total=None, node_cost=None)
    s = src.get()
    d = s if in_place else dst.get()
    if not in_place or not with_dst:
        assert np.array_equal(s, lay.filled), "src was written"
    if with_dst:
        out["coef"] = lay.lines_of(d)
    elif not in_place:
        assert (d == CANARY).all(), "dst == NULL, and something was stored"
    if tree:
        t = tree.get()
        rows = t[:n_lines * TW].reshape(n_lines, TW)
        assert (rows[:, bm.TREE_WORDS:] == CANARY).all() and (t[n_lines * TW:] == CANARY).all(), "words outside the trees were written"
        out["tree"] = [[int(v) for v in r[:bm.TREE_WORDS]] for r in rows]
    if total:
        t = total.get()
        assert (t[n_lines:] == CANARY64).all(), "words behind the totals were written"
        out["total"] = t[:n_lines].view(np.float64).copy()
    if nc:
        t = nc.get()
        rows = t[:n_lines * cd].reshape(n_lines, cd)
        assert (rows[:, nt:] == CANARY64).all() and (t[n_lines * cd:] == CANARY64).all(), "words outside the cost tables were written"
        out["node_cost"] = np.ascontiguousarray(rows[:, :nt]).view(np.float64)
    return out


def run_tree(dwt, wavelet, inverse, x, levels, trees, shared=False, es=4, gap=0, off=0, in_place=True, device=True):
    """-> (the lines after the call, launches).  trees: one per line, or ONE tree with shared (tree_stride 0)"""
    n_lines, N = x.shape
    lay = Lines(x, es, gap, off)
    src = Mem(dwt, lay.filled.copy(), device)
    dst = src if in_place else Mem(dwt, lay.blank(), device)
    words = np.full((1 if shared else n_lines) * TW + 4, CANARY, np.uint32)
    for y, t in enumerate([trees] if shared else trees):
        words[y * TW:y * TW + bm.TREE_WORDS] = np.array(t, np.uint32)
    tree = Mem(dwt, words, device)
    k = launches(dwt, lambda: dwt.packets.wp_tree1d_batch(wp.WAVELET_ID[wavelet], inverse, src.ptr + 4 * off, dst.ptr + 4 * off, lay.pe * 4, es,
                                                           n_lines, N, levels, tree.ptr, 0 if shared else 4 * TW))
    dwt.sync()
    assert np.array_equal(tree.get(), words), "the trees were written"
    s = src.get()
    d = s if in_place else dst.get()
    if not in_place:
        assert np.array_equal(s, lay.filled), "src was written"
    return lay.lines_of(d), k


def both_routes(dwt, run, check, N):
    """run() under "wp_fused" = 1 and 0, check(result) both times; the one-launch route's count where it applies"""
    try:
        for fused in (1, 0):
            dwt.set_option("wp_fused", fused)
            got = run()
            k = got["launches"] if isinstance(got, dict) else got[1]
            if fused and N <= N1D_MAX and k is not None:
                assert k == 1, ("launches", k)
            check(got, fused)
    finally:
        dwt.set_option("wp_fused", 1)


# ---- expectations -----------------------------------------------------------------------------------------------
def node_lengths(N, levels):
    n = np.zeros(2 << levels)
    for j in range(levels + 1):
        for k, (_, ln) in enumerate(wp.nodes_recursive(N, j)):
            n[(1 << j) + k] = ln
    return n


def same_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


def level_sums(cost, levels):
    """the costs of every full level 1 .. levels, each summed pairwise up the heap (the order in which the selection adds:
    rounding is monotonic, so the total can be no larger than any of them)"""
    out = []
    for j in range(1, levels + 1):
        v = np.array(cost[1 << j:2 << j], np.float64)
        while len(v) > 1:
            v = v[0::2] + v[1::2]
        out.append(float(v[0]))
    return out


def check_search(e, got, shape, cost, lines=None, what=""):
    """the outputs of one search against the model's expectation e; lines: the model line of every line of the call"""
    n_lines, N, levels = shape
    lines = range(n_lines) if lines is None else lines
    exact = cost[0] == bm.THRESHOLD
    nlen = node_lengths(N, levels)
    for y, m in enumerate(lines):
        want_c, own = e["cost"][m], e["own"][m]
        bound = (nlen + 16) * EPS * own  # (zero where a node's terms are all zero: exact there)
        if got["node_cost"] is not None:
            c = got["node_cost"][y]
            print(what, "line", y, "max |cost - model| / bound:", float(np.nanmax(np.abs(c[1:] - want_c[1:]) / np.where(bound[1:] > 0, bound[1:], np.inf), initial=0)))
            if exact:
                assert same_f64(c[1:], want_c[1:]), (what, y)
            else:
                assert (np.abs(c[1:] - want_c[1:]) <= bound[1:]).all(), (what, y, int(np.argmax(np.abs(c[1:] - want_c[1:]) - bound[1:])) + 1)
            # the properties, from the returned table alone
            total = c[0]
            assert total <= c[1] and all(total <= s for s in level_sums(c, levels)), (what, y, total, c[1])
            if got["total"] is not None:
                assert total.tobytes() == got["total"][y].tobytes(), (what, y, "node_cost[0] is not the total")
        if got["tree"] is not None:
            assert got["tree"][y] == e["trees"][m], (what, y, "tree")
        if got["total"] is not None:
            t, want_t = got["total"][y], e["totals"][m]
            tb = sum((n + 16) * EPS * own[(1 << j) + k] for j, k, _, n in bm.leaves(N, levels, e["trees"][m]))
            print(what, "line", y, "total", t, "model", want_t, "bound", tb)
            assert (t == want_t) if exact else abs(t - want_t) <= tb, (what, y, t, want_t, tb)
    if got["coef"] is not None:
        want = e["coef"][list(lines)]
        assert wp.same(got["coef"], want), (what, "coefficients", int((got["coef"].view(np.uint32) != want.view(np.uint32)).sum()))


# ---- the shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet,kind_name,shape,costs", bm.shape_cases())
def test_search_and_trees(dwt, wavelet, kind_name, shape, costs):
    """every shape, the three wavelets: the search (every output; in place and out of place in turn), then the transform in
    the trees found, forward and inverse, and in the full tree against wp1d_batch"""
    n_lines, N, levels = shape
    for i, cost in enumerate(costs):
        e = bm.expected(wavelet, kind_name, shape, cost)
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, e["x"], levels, in_place=bool(i & 1)),
                    lambda got, fused: check_search(e, got, shape, cost, what="%s %s %s cost %s fused %d" % (wavelet, kind_name, shape, cost, fused)), N)
    e = bm.expected(wavelet, kind_name, shape, costs[0])
    back = np.concatenate([bm.inv_tree(wavelet, e["coef"][y:y + 1], levels, e["trees"][y]) for y in range(n_lines)])

    def same_as(want):
        def check(got, fused):
            assert wp.same(got[0], want), ("wp_fused", fused, int((got[0].view(np.uint32) != want.view(np.uint32)).sum()))
        return check
    both_routes(dwt, lambda: run_tree(dwt, wavelet, False, e["x"], levels, e["trees"], in_place=False), same_as(e["coef"]), N)
    both_routes(dwt, lambda: run_tree(dwt, wavelet, True, e["coef"], levels, e["trees"]), same_as(back), N)
    # the full tree: the bits of wp1d_batch of the same depth, forward and inverse
    full = bm.full_tree(levels)
    for inverse in (False, True):
        d = Dev(dwt, e["x"])
        dwt.packets.wp1d_batch(wp.WAVELET_ID[wavelet], inverse, d.ptr, d.ptr, 4 * N, 4, n_lines, N, levels)
        want = d.get()
        d.free()
        both_routes(dwt, lambda: run_tree(dwt, wavelet, inverse, e["x"], levels, full, shared=True, in_place=inverse), same_as(want), N)


def test_many_lines_cross_check_route(dwt):
    """65539 lines under "wp_fused" = 0: the helper kernels past 65535 lines (the same 16 lines over and over)"""
    n_lines, N, levels = bm.MANY_LINES
    block = (bm.MANY_BLOCK, N, levels)
    lines = [y % bm.MANY_BLOCK for y in range(n_lines)]
    try:
        dwt.set_option("wp_fused", 0)
        for cost in bm.MANY_COSTS:
            e = bm.expected("cdf97_s", "normal", block, cost)
            x = np.ascontiguousarray(e["x"][lines])
            got = run_best(dwt, "cdf97_s", cost, x, levels)
            for key in ("node_cost", "total", "coef"):  # every repetition of a line: the bits of its first
                v = got[key].reshape(n_lines, -1).view(np.uint32 if key == "coef" else np.uint64)
                assert np.array_equal(v, v[lines]), key
            assert got["tree"] == [got["tree"][m] for m in lines]
            head = {k: (v[:2 * bm.MANY_BLOCK] if isinstance(v, (np.ndarray, list)) else v) for k, v in got.items()}
            tail = {k: (v[-bm.MANY_BLOCK:] if isinstance(v, (np.ndarray, list)) else v) for k, v in got.items()}
            check_search(e, head, (2 * bm.MANY_BLOCK, N, levels), cost, lines=lines[:2 * bm.MANY_BLOCK], what="many lines, head")
            check_search(e, tail, (bm.MANY_BLOCK, N, levels), cost, lines=lines[-bm.MANY_BLOCK:], what="many lines, tail")
            want = e["coef"][lines]
            assert wp.same(got["coef"], want)
            back, _ = run_tree(dwt, "cdf97_s", True, want, levels, got["tree"])
            model_back = np.concatenate([bm.inv_tree("cdf97_s", e["coef"][m:m + 1], levels, e["trees"][m]) for m in range(bm.MANY_BLOCK)])
            assert wp.same(back, model_back[lines])
    finally:
        dwt.set_option("wp_fused", 1)


# ---- layouts ----------------------------------------------------------------------------------------------------
LAYOUTS = (dict(es=8), dict(gap=3), dict(off=1), dict(device=False), dict(device=False, es=8, gap=1), dict(es=12, gap=1, off=1))


@pytest.mark.parametrize("wavelet,kind_name,shape,costs", bm.layout_cases())
def test_layouts(dwt, wavelet, kind_name, shape, costs):
    """elements 8 bytes apart, gaps between lines, a base 4 bytes off 16-byte alignment, host memory; in place and out of
    place; dst == NULL; single outputs; per-line trees, a shared tree, a tree with unreachable bits"""
    n_lines, N, levels = shape
    for i, cost in enumerate(costs):
        e = bm.expected(wavelet, kind_name, shape, cost)
        lay = LAYOUTS[i % len(LAYOUTS)]
        what = "%s %s cost %s %s" % (wavelet, kind_name, cost, lay)
        for in_place in (False, True):
            both_routes(dwt, lambda: run_best(dwt, wavelet, cost, e["x"], levels, in_place=in_place, **lay),
                        lambda got, fused: check_search(e, got, shape, cost, what=what), N if lay.get("device", True) else 2 * N1D_MAX)
        # costs and tree only; one output at a time
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, e["x"], levels, with_dst=False, **lay),
                    lambda got, fused: check_search(e, got, shape, cost, what=what + " dst NULL"), N if lay.get("device", True) else 2 * N1D_MAX)
        only = ("tree", "total", "node_cost")[i % 3]
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, e["x"], levels, with_dst=bool(i & 1), outputs=(only,), **lay),
                    lambda got, fused: check_search(e, got, shape, cost, what=what + " " + only), N if lay.get("device", True) else 2 * N1D_MAX)
    # trees: per line (above, in test_search_and_trees), shared, with unreachable bits
    e = bm.expected(wavelet, kind_name, shape, costs[0])
    shared = bm.tree_of([1, 2, 3, 5, 6, 11, 12, 24, 49])
    dirty = [a | b for a, b in zip(shared, bm.tree_of([0, 8, 9, 16, 17, 35, 40, 63, 64, 200, 1023]))]  # under clear bits, bit 0, level 6 and beyond
    assert bm.effective(dirty, levels) == shared
    fwd = bm.fwd_tree(wavelet, e["x"], levels, shared)
    inv = bm.inv_tree(wavelet, fwd, levels, shared)
    for i, lay in enumerate(LAYOUTS):
        for tree in (shared, dirty):
            def same_as(want):
                def check(got, fused):
                    assert wp.same(got[0], want), (lay, "wp_fused", fused)
                return check
            n = N if lay.get("device", True) else 2 * N1D_MAX
            both_routes(dwt, lambda: run_tree(dwt, wavelet, False, e["x"], levels, tree, shared=True, in_place=bool(i & 1), **lay), same_as(fwd), n)
            both_routes(dwt, lambda: run_tree(dwt, wavelet, True, fwd, levels, tree, shared=True, in_place=not i & 1, **lay), same_as(inv), n)
    per_line = [dirty if y & 1 else bm.tree_of([]) for y in range(n_lines)]
    want = e["x"].copy()
    want[1::2] = fwd[1::2]
    both_routes(dwt, lambda: run_tree(dwt, wavelet, False, e["x"], levels, per_line, in_place=False), same_as(want), N)


# ---- special lines ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_all_zero_lines(dwt, wavelet):
    """exact ties everywhere: every cost 0, the root-only tree, total 0, the lines untouched"""
    shape = (5, 37, 5)
    for cost in bm.COSTS:
        e = bm.expected(wavelet, "zeros", shape, cost)
        assert all(t == bm.tree_of([]) for t in e["trees"]) and not e["cost"].any()

        def check(got, fused):
            assert not got["node_cost"].any() and not np.signbit(got["node_cost"]).any() and not got["total"].any()
            assert all(t == bm.tree_of([]) for t in got["tree"]) and wp.same(got["coef"], e["x"])
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, e["x"], 5), check, 37)


@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_nan_sample_and_position_in_the_batch(dwt, wavelet):
    """a line with one NaN sample: the root-only tree and a NaN total; the lines around it as if it were not there.  The
    same line at positions 0 and 4 of the batch: the same bits in every output.  Two identical calls: identical bytes."""
    shape = bm.LAYOUT_SHAPE
    n_lines, N, levels = shape
    for cost in bm.COSTS:
        e = bm.expected(wavelet, "normal", shape, cost)
        x = e["x"].copy()
        x[1, 40] = np.nan
        x[4] = x[0]
        model = [0, None, 2, 3, 0]

        def check(got, fused):
            assert got["tree"][1] == bm.tree_of([]) and math.isnan(got["total"][1]) and np.isnan(got["node_cost"][1, :2]).all()
            assert wp.same(got["coef"][1], x[1])
            for key in ("node_cost", "total", "coef"):
                assert got[key][0].tobytes() == got[key][4].tobytes(), key
            assert got["tree"][0] == got["tree"][4]
            keep = [0, 2, 3, 4]
            sub = dict(got, node_cost=got["node_cost"][keep], total=got["total"][keep], coef=got["coef"][keep], tree=[got["tree"][y] for y in keep])
            check_search(e, sub, (4, N, levels), cost, lines=[model[y] for y in keep], what="beside a NaN line")
            again = run_best(dwt, wavelet, cost, x, levels)
            for key in ("node_cost", "total", "coef"):
                assert again[key].tobytes() == got[key].tobytes(), ("two calls", key)
            assert again["tree"] == got["tree"]
        both_routes(dwt, lambda: run_best(dwt, wavelet, cost, x, levels), check, N)


def test_tone_keeps_its_band(dwt):
    """a tone in the middle of band f of a 3-level tree of 256 samples, Shannon cost (the tones of tests/test_wp.py): the
    effective tree contains the leaf perm[f] of level 3"""
    perm = wp.freq_order(3)
    for f in range(8):
        e = bm.expected("cdf97_s", "tone%d" % f, bm.TONE_SHAPE, bm.JOINT_COST)

        def check(got, fused):
            assert got["tree"][0] == e["trees"][0]
            assert (3, perm[f]) in [l[:2] for l in dwt.packets.wp_tree_leaves(256, 3, got["tree"][0])], (f, got["tree"][0][0])
        both_routes(dwt, lambda: run_best(dwt, "cdf97_s", bm.JOINT_COST, e["x"], 3, with_dst=False, outputs=("tree",)), check, 256)


@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_joint_basis(dwt, wavelet):
    """wp_joint_basis: the model's selection on the float64 sum of the model's tables; the batch then transforms in it"""
    n_lines, N, levels = bm.LAYOUT_SHAPE
    e = bm.expected(wavelet, "normal", bm.LAYOUT_SHAPE, bm.JOINT_COST)
    want = bm.select(bm.joint_tables(wavelet)[0], levels)[0]
    fwd = bm.fwd_tree(wavelet, e["x"], levels, want)
    try:
        for fused in (1, 0):
            dwt.set_option("wp_fused", fused)
            for device in (True, False):
                x = Mem(dwt, e["x"].copy(), device)
                tree = dwt.packets.wp_joint_basis(wp.WAVELET_ID[wavelet], bm.JOINT_COST[0], bm.JOINT_COST[1], x.ptr, 4 * N, 4, n_lines, N, levels)
                assert tree == want, (fused, device)
                dwt.packets.wp_tree1d_batch(wp.WAVELET_ID[wavelet], False, x.ptr, x.ptr, 4 * N, 4, n_lines, N, levels, tree)
                dwt.sync()
                assert wp.same(x.get(), fwd), (fused, device)
    finally:
        dwt.set_option("wp_fused", 1)


# ---- errors -----------------------------------------------------------------------------------------------------
def test_errors(dwt):
    L = dwt.lib
    x = Dev(dwt, np.zeros(4096, F32))
    t = Dev(dwt, np.zeros(64 * 32, np.uint32))
    c = Dev(dwt, np.zeros(4096, np.float64))
    host = np.zeros(4096, F32)
    host_tree = np.zeros(64 * 32, np.uint32)

    def refused(rc):
        assert rc != 0 and len(dwt.last_error()) > 10

    def best(wavelet=0, cost=0, param=0.0, src=x.ptr, dst=x.ptr, N=100, levels=2, tree=t.ptr, tree_stride=128, total=c.ptr, node_cost=None):
        return L.dwt_hip_wp_best1d_batch(wavelet, cost, param, src, dst, 4 * N, 4, 2, N, levels, tree, tree_stride, total, node_cost, 8 * (2 << max(levels, 0)))

    def tree(wavelet=0, src=x.ptr, dst=x.ptr, N=100, levels=2, tr=t.ptr, tree_stride=128):
        return L.dwt_hip_wp_tree1d_batch(wavelet, 0, src, dst, 4 * N, 4, 2, N, levels, tr, tree_stride)

    assert best() == 0 and tree() == 0 and tree(tree_stride=0) == 0, dwt.last_error()
    for N, levels in ((100, 0), (100, 7), (100, -1), (2048, 11), (2048, 12), (2, 2)):
        refused(best(N=N, levels=levels))
        refused(tree(N=N, levels=levels))
    for wavelet in (1, 3, 4, 5, 7, 8, 9, -1, 77):
        refused(best(wavelet=wavelet))
        refused(tree(wavelet=wavelet))
    for cost, param in ((-1, 0.0), (4, 0.0), (2, 0.0), (2, 2.0), (2, -1.0), (2, math.nan), (3, -0.5), (3, math.nan), (3, math.inf)):
        refused(best(cost=cost, param=param))
    assert best(cost=2, param=1.5) == 0 and best(cost=3, param=0.0) == 0, dwt.last_error()
    refused(best(dst=None, tree=None, total=None, node_cost=None))  # every output NULL
    assert best(dst=None, tree=None, total=None, node_cost=c.ptr) == 0, dwt.last_error()
    refused(best(tree_stride=64))
    refused(best(tree_stride=130))
    refused(tree(tree_stride=64))
    refused(tree(tr=None))
    refused(L.dwt_hip_wp_best1d_batch(0, 0, 0.0, x.ptr, x.ptr, 400, 4, 2, 100, 2, None, 0, None, c.ptr, 8 * 4))  # cost tables too close
    # mixed host and device pointers
    refused(best(src=host.ctypes.data, dst=host.ctypes.data))
    refused(best(dst=host.ctypes.data))
    refused(best(tree=host_tree.ctypes.data))
    refused(tree(tr=host_tree.ctypes.data))
    refused(tree(src=host.ctypes.data, dst=host.ctypes.data))
    # lines that share samples
    refused(L.dwt_hip_wp_tree1d_batch(0, 0, x.ptr, x.ptr, 4 * 99, 4, 2, 100, 2, t.ptr, 0))
    dwt.sync()
    for d in (x, t, c):
        d.free()


# ---- example ----------------------------------------------------------------------------------------------------
def test_example_spectra_best_basis(dwt, tmp_path):
    """examples/spectra_best_basis.c: condition, per-row search, the joint tree, the transform in it, its leaves in
    frequency order, the round trip"""
    exe, libdir = tmp_path / "spectra_best_basis", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "spectra_best_basis.c"),
                           "-o", str(exe), "-L" + libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "best basis: success" in out.stdout + out.stderr, out.stdout + out.stderr


# ---- stream -----------------------------------------------------------------------------------------------------
def test_entries_run_on_the_callers_stream():
    """both device entries on both routes, once on a non-blocking stream behind a bounded delay, in a process of its own
    (tests/wp_basis_stream.py, on the harness of tests/stream_cases.py): the model's results, queued without waiting for the
    stream, the launch count of the warm-up"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wp_basis_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]
