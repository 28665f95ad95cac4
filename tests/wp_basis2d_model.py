"""Model of the best-basis search over packet QUADTREES and of pruned 2-D packet trees (include/libdwt_hip.h).

* `terms` -- tests/wp_basis_model.py's float64 terms;
* `qbase`, `qindex`, `nq`, `children` -- the index order: node (ky, kx) of level j at (4^j - 1)/3 + ky * 2^j + kx;
* `rects` -- {(j, ky, kx): (x0, y0, w, h)}, the product of wp_model.nodes_recursive along y and along x;
* `full_levels` -- the images after 0 .. levels levels of the full tree (wp_model._node2d per node);
* `cost_tables` -- per image (cost, S, own): cost[q] the `math.fsum` of the terms of node q over the full tree of its depth,
  own[q] the sum of |term| over the node's samples, S[q] that over all nodes of the subtree of q;
* `select` -- the selection rule: (tree, total, best), effective bits only; a tie and a NaN keep the parent;
* `effective`, `leaves`, `full_tree`, `tree_of` -- bitmaps;
* `fwd_qtree`, `inv_qtree` -- the transform in a tree, composed per split node from wp_model._node2d;
* `near_ties` -- the nodes whose decision a rounding error of the device's sums could turn;
* `all_trees`, `tree_cost` -- brute force over every quadtree of up to 2 levels;
* the case table of tests/test_hip_wp_basis2d.py and its seeded inputs: a smooth quadrant, an oscillating quadrant and noise.
"""
import math

import numpy as np

import wp_basis_model as bm
import wp_model as wp

F32 = np.float32
SHANNON, LOG_ENERGY, LP, THRESHOLD = bm.SHANNON, bm.LOG_ENERGY, bm.LP, bm.THRESHOLD
QTREE_WORDS, QTREE_MAX_LEVELS = 16, 5
NEAR_TIE = 1e-9  # a node is a near-tie if |cost[q] - (sum of its children's best)| <= NEAR_TIE * S[q], S[q] > 0
terms = bm.terms


# ---- index order ---------------------------------------------------------------------------------------------
def qbase(j):
    return ((1 << (2 * j)) - 1) // 3


def qindex(j, ky, kx):
    return qbase(j) + (ky << j) + kx


def nq(levels):
    return qbase(levels + 1)


def children(j, ky, kx):
    """LL, HL, LH, HH"""
    return [(j + 1, 2 * ky, 2 * kx), (j + 1, 2 * ky, 2 * kx + 1), (j + 1, 2 * ky + 1, 2 * kx), (j + 1, 2 * ky + 1, 2 * kx + 1)]


def nodes(levels):
    """every (j, ky, kx) of levels 0 .. levels, in index order"""
    return [(j, ky, kx) for j in range(levels + 1) for ky in range(1 << j) for kx in range(1 << j)]


def rects(size_y, size_x, levels):
    out = {}
    for j in range(levels + 1):
        ys, xs = wp.nodes_recursive(size_y, j), wp.nodes_recursive(size_x, j)
        for ky, (y0, h) in enumerate(ys):
            for kx, (x0, w) in enumerate(xs):
                out[(j, ky, kx)] = (x0, y0, w, h)
    return out


# ---- the full tree and its costs -----------------------------------------------------------------------------
def full_levels(wavelet, x, levels):
    """x: batch x H x W.  [the images after j levels of the full tree, j = 0 .. levels]"""
    out = [np.array(x, dtype=F32, copy=True)]
    H, W = out[0].shape[1:]
    for j in range(levels):
        a = out[-1].copy()
        for img in a:
            for y0, h in wp.nodes_recursive(H, j):
                for x0, w in wp.nodes_recursive(W, j):
                    wp._node2d(wavelet, img[y0:y0 + h, x0:x0 + w], False)
        out.append(a)
    return out


def cost_tables(kind, param, stages, levels):
    """-> (cost, S, own), each batch x nq(levels) float64 in index order"""
    batch, H, W = stages[0].shape
    r = rects(H, W, levels)
    cost, own = np.zeros((batch, nq(levels))), np.zeros((batch, nq(levels)))
    for j in range(levels + 1):
        t = terms(kind, param, stages[j])
        for (jj, ky, kx), (x0, y0, w, h) in r.items():
            if jj != j:
                continue
            q = qindex(j, ky, kx)
            for b in range(batch):
                v = t[b, y0:y0 + h, x0:x0 + w].reshape(-1)
                cost[b, q] = math.fsum(v)
                own[b, q] = math.fsum(np.abs(v))
    mass = own.copy()
    for j, ky, kx in reversed(nodes(levels - 1)):  # S: the subtree's
        for c in children(j, ky, kx):
            mass[:, qindex(j, ky, kx)] += mass[:, qindex(*c)]
    return cost, mass, own


# ---- trees ---------------------------------------------------------------------------------------------------
def bit(tree, q):
    return (int(tree[q >> 5]) >> (q & 31)) & 1


def tree_of(splits):
    t = [0] * QTREE_WORDS
    for q in splits:
        t[q >> 5] |= 1 << (q & 31)
    return t


def full_tree(levels):
    return tree_of(range(nq(levels - 1)))


def effective(tree, levels):
    """the bits of levels < `levels` that can be reached from the root through set bits"""
    out = []

    def walk(j, ky, kx):
        if j < levels and bit(tree, qindex(j, ky, kx)):
            out.append(qindex(j, ky, kx))
            for c in children(j, ky, kx):
                walk(*c)
    walk(0, 0, 0)
    return tree_of(out)


def select(cost, levels):
    """-> (tree, total, best): bottom-up, split iff ((best[LL] + best[HL]) + best[LH]) + best[HH] < cost[q]"""
    best = [float(c) for c in cost[:nq(levels)]]
    splits = []
    for j, ky, kx in reversed(nodes(levels - 1)):
        q = qindex(j, ky, kx)
        ll, hl, lh, hh = (best[qindex(*c)] for c in children(j, ky, kx))
        c = ((ll + hl) + lh) + hh
        if c < best[q]:
            best[q] = c
            splits.append(q)
    return effective(tree_of(splits), levels), best[0], best


def leaves(size_x, size_y, levels, tree):
    """[(level, ky, kx, x0, y0, w, h)] of the effective tree, depth first, the children in the order LL, HL, LH, HH"""
    out = []

    def walk(j, ky, kx, x0, y0, w, h):
        if j < levels and bit(tree, qindex(j, ky, kx)):
            wl, hl = (w + 1) // 2, (h + 1) // 2
            walk(j + 1, 2 * ky, 2 * kx, x0, y0, wl, hl)
            walk(j + 1, 2 * ky, 2 * kx + 1, x0 + wl, y0, w - wl, hl)
            walk(j + 1, 2 * ky + 1, 2 * kx, x0, y0 + hl, wl, h - hl)
            walk(j + 1, 2 * ky + 1, 2 * kx + 1, x0 + wl, y0 + hl, w - wl, h - hl)
        else:
            out.append((j, ky, kx, x0, y0, w, h))
    walk(0, 0, 0, 0, 0, size_x, size_y)
    return out


def _split_nodes(size_y, size_x, levels, tree):
    """[(level, x0, y0, w, h)] of the effectively split nodes, by level"""
    eff = effective(tree, levels)
    r = rects(size_y, size_x, levels - 1)
    return sorted((n[0],) + r[n] for n in nodes(levels - 1) if bit(eff, qindex(*n)))


def fwd_qtree(wavelet, a, levels, tree):
    """the image a in `tree`; returns a new array"""
    a = np.array(a, dtype=F32, copy=True)
    for j, x0, y0, w, h in _split_nodes(a.shape[0], a.shape[1], levels, tree):
        wp._node2d(wavelet, a[y0:y0 + h, x0:x0 + w], False)
    return a


def inv_qtree(wavelet, a, levels, tree):
    a = np.array(a, dtype=F32, copy=True)
    for j, x0, y0, w, h in reversed(_split_nodes(a.shape[0], a.shape[1], levels, tree)):
        wp._node2d(wavelet, a[y0:y0 + h, x0:x0 + w], True)
    return a


def near_ties(cost, mass, levels, float_kind=True):
    """the indices of the near-tie nodes of one image's tables"""
    if not float_kind:
        return []
    best = select(cost, levels)[2]
    out = []
    for j, ky, kx in nodes(levels - 1):
        q = qindex(j, ky, kx)
        ll, hl, lh, hh = (best[qindex(*c)] for c in children(j, ky, kx))
        d = abs(cost[q] - (((ll + hl) + lh) + hh))
        if mass[q] > 0 and d <= NEAR_TIE * mass[q]:  # (a NaN on either side keeps the parent whatever the rounding)
            out.append(q)
    return out


# ---- brute force ---------------------------------------------------------------------------------------------
def all_trees(levels):
    """every effective quadtree of depth <= levels, as sets of split indices"""
    def sub(j, ky, kx):
        if j == levels:
            return [frozenset()]
        out = [frozenset()]
        parts = [sub(*c) for c in children(j, ky, kx)]
        for a in parts[0]:
            for b in parts[1]:
                for c in parts[2]:
                    for d in parts[3]:
                        out.append(frozenset({qindex(j, ky, kx)}) | a | b | c | d)
        return out
    return sub(0, 0, 0)


def tree_cost(cost, splits):
    """the summed cost of the leaves of the tree whose split nodes are `splits`"""
    def walk(j, ky, kx):
        if qindex(j, ky, kx) in splits:
            return sum(walk(*c) for c in children(j, ky, kx))
        return cost[qindex(j, ky, kx)]
    return walk(0, 0, 0)


# ---- the cases of the GPU tests (tests/test_hip_wp_basis2d.py); tests/test_wp_basis2d.py holds every one to the near-tie cap
# and to the non-trivial-tree rule ----
COSTS = ((SHANNON, 0.0), (LOG_ENERGY, 0.0), (LP, 0.5), (THRESHOLD, 1.0))
# (rows, columns, levels, batch)
SHAPES = ((8, 8, 3, 2), (67, 130, 3, 3), (33, 257, 2, 1), (256, 256, 5, 2), (160, 96, 4, 2))
PADDED_SHAPE = (160, 96, 4, 2)  # row pitch and batch stride with padding, canaries around every output
LAYOUT_SHAPE = (67, 130, 3, 3)  # in place, dst == NULL, host memory, strided elements, NaN image, position, determinism
JOINT_COST = (SHANNON, 0.0)
SEED0 = 8100  # a case whose tables hold a near-tie or whose tree is trivial takes another seed HERE (never a skip)
REPLACED_SEEDS = {}


def case_seed(wavelet, shape):
    return REPLACED_SEEDS.get((wavelet, shape), SEED0 + 17 * wp.WAVELETS.index(wavelet) + shape[0] + 3 * shape[1])


def texture(seed, size_y, size_x):
    """one image: a smooth top-left quadrant, an oscillating top-right quadrant, noise below -- loud on the left, faint on
    the right -- so that a search splits some nodes and keeps others"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size_y, 0:size_x].astype(np.float64)
    hy, hx = (size_y + 1) // 2, (size_x + 1) // 2
    a = np.empty((size_y, size_x))
    f = rng.uniform(0.6, 1.4, 4)
    smooth = 6.0 * np.cos(f[0] * np.pi * x / size_x) * np.cos(f[1] * np.pi * y / size_y) + 2.0
    osc = 5.0 * np.cos(np.pi * (0.70 + 0.2 * f[2] / 1.4) * x) * np.cos(np.pi * (0.55 + 0.3 * f[3] / 1.4) * y)
    a[:hy, :hx] = smooth[:hy, :hx]
    a[:hy, hx:] = osc[:hy, hx:]
    a[hy:, :hx] = 3.0 * rng.standard_normal((size_y - hy, hx))
    a[hy:, hx:] = 0.4 * rng.standard_normal((size_y - hy, size_x - hx)) + smooth[hy:, hx:] * 0.5
    a += 0.05 * rng.standard_normal(a.shape)
    return a.astype(F32)


def amplitude(cost):
    """the Shannon term -e log(e) rewards concentration only where e < 1: its cases take the textures at 1/32 (a power of
    two: the same mantissas); the threshold at 1 needs them as they are"""
    return F32(1.0 / 32) if cost[0] == SHANNON else F32(1.0)


def case_input(wavelet, shape, cost):
    size_y, size_x, levels, batch = shape
    return np.stack([texture(case_seed(wavelet, shape) + 1000 * b, size_y, size_x) for b in range(batch)]) * amplitude(cost)


def cases():
    """(wavelet, shape) of every GPU case; each runs with every cost of COSTS"""
    return [(wavelet, shape) for shape in SHAPES for wavelet in wp.WAVELETS]


_memo = {}


def expected(wavelet, shape, cost, x=None, key=None):
    """-> dict(x, stages, cost, mass, own, trees, totals, best, coef) of a case (or of the images x under the memo key `key`),
    computed once and never modified"""
    size_y, size_x, levels, batch = shape
    k0 = (wavelet, shape, key, float(amplitude(cost)))
    if k0 not in _memo:
        x = case_input(wavelet, shape, cost) if x is None else np.array(x, F32)
        x.setflags(write=False)
        _memo[k0] = (x, full_levels(wavelet, x, levels))
    x, stages = _memo[k0]
    k1 = k0 + (cost,)
    if k1 not in _memo:
        c, m, own = cost_tables(cost[0], cost[1], stages, levels)
        sel = [select(c[b], levels) for b in range(len(x))]
        trees = [t for t, _, _ in sel]
        coef = np.empty_like(x)
        for b in range(len(x)):  # a leaf of a pruned tree is the node of the full tree of its depth
            for j, ky, kx, x0, y0, w, h in leaves(size_x, size_y, levels, trees[b]):
                coef[b, y0:y0 + h, x0:x0 + w] = stages[j][b, y0:y0 + h, x0:x0 + w]
        for a in (c, m, own, coef):
            a.setflags(write=False)
        _memo[k1] = dict(x=x, stages=stages, cost=c, mass=m, own=own, trees=trees, totals=[t for _, t, _ in sel], best=[b for _, _, b in sel],
                         coef=coef)
    return _memo[k1]


def joint_tables(wavelet):
    """the tables of wp_joint_qtree on LAYOUT_SHAPE: the model's tables summed over the images in float64, in batch order
    -> (cost, S)"""
    e = expected(wavelet, LAYOUT_SHAPE, JOINT_COST)
    cost, mass = np.zeros(e["cost"].shape[1]), np.zeros(e["cost"].shape[1])
    for b in range(LAYOUT_SHAPE[3]):
        cost += e["cost"][b]
        mass += e["mass"][b]
    return cost, mass
