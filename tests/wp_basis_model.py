"""Model of the best-basis search and of pruned wavelet packet trees (include/libdwt_hip.h).

* `term`, `terms` -- one coefficient's term of a cost, in float64 as the header states it (scalar / numpy);
* `full_levels` -- the lines after 0 .. levels levels of the full tree (tests/wp_model.py's one-level line functions);
* `cost_tables` -- per line (cost, S, own): cost[h] the `math.fsum` of the terms of node h over the full tree of its depth,
  S[h] the sum of |term| over all samples of all nodes of the subtree of h;
* `select` -- the selection rule: (tree, total, best), effective bits only; a tie and a NaN keep the parent;
* `effective`, `leaves`, `full_tree` -- tree bitmaps;
* `fwd_tree`, `inv_tree` -- the transform in a tree, composed from wp_model's one-level line functions per split node;
* `near_ties` -- the nodes whose decision a rounding error of the device's sums could turn;
* `all_trees`, `tree_cost` -- brute force over every tree of up to 3 levels.
"""
import math

import numpy as np

import wp_model as wp

F32 = np.float32
SHANNON, LOG_ENERGY, LP, THRESHOLD = 0, 1, 2, 3
TREE_WORDS, TREE_MAX_LEVELS = 32, 10
NEAR_TIE = 1e-9  # a node is a near-tie if |cost[h] - (best[2h] + best[2h+1])| <= NEAR_TIE * S[h], S[h] > 0


# ---- costs ---------------------------------------------------------------------------------------------------
def term(kind, param, c):
    c = F32(c)
    if not np.isfinite(c):
        return math.nan
    x = float(c)
    e = x * x
    if kind == SHANNON:
        return 0.0 if e == 0 else -e * math.log(e)
    if kind == LOG_ENERGY:
        return 0.0 if e == 0 else math.log(e)
    if kind == LP:
        p = float(F32(param))
        return abs(x) if p == 1.0 else abs(x) ** p
    assert kind == THRESHOLD
    return 1.0 if abs(c) > F32(param) else 0.0


def terms(kind, param, v):
    """the terms of an array of float32 coefficients, float64, elementwise as `term`"""
    v = np.asarray(v, F32)
    x = v.astype(np.float64)
    e = x * x
    with np.errstate(all="ignore"):
        if kind == SHANNON:
            t = np.where(e == 0, 0.0, -e * np.log(np.where(e == 0, 1.0, e)))
        elif kind == LOG_ENERGY:
            t = np.where(e == 0, 0.0, np.log(np.where(e == 0, 1.0, e)))
        elif kind == LP:
            p = float(F32(param))
            t = np.abs(x) if p == 1.0 else np.abs(x) ** p
        else:
            assert kind == THRESHOLD
            t = (np.abs(v) > F32(param)).astype(np.float64)
    return np.where(np.isfinite(v), t, np.nan)


def full_levels(wavelet, x, levels):
    """[the lines after j levels of the full tree, j = 0 .. levels]"""
    out = [np.array(x, dtype=F32, copy=True)]
    for j in range(levels):
        a = out[-1].copy()
        for s, n in wp.nodes_recursive(a.shape[1], j):
            a[:, s:s + n] = wp._line_fwd(wavelet, a[:, s:s + n])
        out.append(a)
    return out


def cost_tables(kind, param, stages, levels):
    """stages: full_levels(...).  -> (cost, S, own), each lines x 2^(levels+1) float64 in heap order, entry 0 is 0; own[h]:
    the sum of |term| over the samples of node h alone"""
    n_lines, N = stages[0].shape
    nt = 2 << levels
    cost, mass = np.zeros((n_lines, nt)), np.zeros((n_lines, nt))
    for j in range(levels + 1):
        t = terms(kind, param, stages[j])
        for k, (s, n) in enumerate(wp.nodes_recursive(N, j)):
            for y in range(n_lines):
                cost[y, (1 << j) + k] = math.fsum(t[y, s:s + n])
                mass[y, (1 << j) + k] = math.fsum(np.abs(t[y, s:s + n]))
    own = mass.copy()
    for h in range((1 << levels) - 1, 0, -1):  # S: the subtree's
        mass[:, h] += mass[:, 2 * h] + mass[:, 2 * h + 1]
    return cost, mass, own


# ---- trees ---------------------------------------------------------------------------------------------------
def bit(tree, h):
    return (int(tree[h >> 5]) >> (h & 31)) & 1


def tree_of(splits):
    t = [0] * TREE_WORDS
    for h in splits:
        t[h >> 5] |= 1 << (h & 31)
    return t


def full_tree(levels):
    return tree_of(range(1, 1 << levels))


def effective(tree, levels):
    """the bits that can be reached from the root through set bits"""
    out = []
    for h in range(1, 1 << levels):
        a, on = h, True
        while a >= 1 and on:
            on = bool(bit(tree, a))
            a >>= 1
        if on:
            out.append(h)
    return tree_of(out)


def select(cost, levels):
    """-> (tree, total, best): bottom-up, split iff best[2h] + best[2h+1] < cost[h]"""
    best = [float(c) for c in cost[:2 << levels]]
    splits = []
    for h in range((1 << levels) - 1, 0, -1):
        c = best[2 * h] + best[2 * h + 1]
        if c < best[h]:
            best[h] = c
            splits.append(h)
    return effective(tree_of(splits), levels), best[1], best


def leaves(N, levels, tree):
    """[(level, index, start, len)] of the effective tree, left to right"""
    out = []

    def walk(j, k, s, n):
        if j < levels and bit(tree, (1 << j) + k):
            nl = (n + 1) // 2
            walk(j + 1, 2 * k, s, nl)
            walk(j + 1, 2 * k + 1, s + nl, n - nl)
        else:
            out.append((j, k, s, n))
    walk(0, 0, 0, N)
    return out


def _split_nodes(N, levels, tree):
    """[(level, start, len)] of the effectively split nodes"""
    eff = effective(tree, levels)
    return [(j, s, n) for j in range(levels) for k, (s, n) in enumerate(wp.nodes_recursive(N, j)) if bit(eff, (1 << j) + k)]


def fwd_tree(wavelet, a, levels, tree):
    """every row of a (lines x N) in `tree`; returns a new array"""
    a = np.array(a, dtype=F32, copy=True)
    for j, s, n in sorted(_split_nodes(a.shape[1], levels, tree)):
        a[:, s:s + n] = wp._line_fwd(wavelet, a[:, s:s + n])
    return a


def inv_tree(wavelet, a, levels, tree):
    a = np.array(a, dtype=F32, copy=True)
    for j, s, n in sorted(_split_nodes(a.shape[1], levels, tree), reverse=True):
        a[:, s:s + n] = wp._line_inv(wavelet, a[:, s:s + n])
    return a


def near_ties(cost, mass, levels, float_kind=True):
    """the heap indices of the near-tie nodes of one line's tables"""
    if not float_kind:
        return []
    best = select(cost, levels)[2]
    out = []
    for h in range(1, 1 << levels):
        d = abs(cost[h] - (best[2 * h] + best[2 * h + 1]))
        if mass[h] > 0 and d <= NEAR_TIE * mass[h]:  # (a NaN on either side keeps the parent whatever the rounding)
            out.append(h)
    return out


# ---- brute force ---------------------------------------------------------------------------------------------
def all_trees(levels):
    """every effective tree of depth <= levels, as sets of split heap indices"""
    def sub(h, j):
        if j == levels:
            return [frozenset()]
        out = [frozenset()]
        for l in sub(2 * h, j + 1):
            for r in sub(2 * h + 1, j + 1):
                out.append(frozenset({h}) | l | r)
        return out
    return sub(1, 0)


def tree_cost(cost, splits):
    """the summed cost of the leaves of the tree whose split nodes are `splits`"""
    def walk(h):
        return walk(2 * h) + walk(2 * h + 1) if h in splits else cost[h]
    return walk(1)


# ---- the cases of the GPU tests (tests/test_hip_wp_basis.py); tests/test_wp_basis.py holds every one to the near-tie cap ----
COSTS = ((SHANNON, 0.0), (LOG_ENERGY, 0.0), (LP, 1.0), (LP, 0.5), (THRESHOLD, 1.0))
# (n_lines, N, levels)
SHAPES = ((1, 2, 1), (3, 3, 1), (5, 37, 5), (4, 64, 6), (5, 100, 6), (2, 512, 9), (5, 513, 9), (3, 2048, 10), (2, 2049, 10),
          (2, 8192, 10), (2, 8191, 10), (1, 8193, 3))
MANY_LINES = (65539, 4, 2)  # under "wp_fused" = 0 only: the helper kernels past 65535 lines
MANY_BLOCK = 16             # ... the lines of the case (16, 4, 2) over and over
MANY_COSTS = ((SHANNON, 0.0), (THRESHOLD, 1.0))
TONE_SHAPE = (1, 256, 3)    # input kinds "tone0" .. "tone7": a tone in the middle of band f of a 3-level tree
LAYOUT_SHAPE = (5, 100, 6)
JOINT_COST = (SHANNON, 0.0)
SEED0 = 7300  # a case whose tables hold a near-tie takes another seed HERE (never a skip): REPLACED_SEEDS
REPLACED_SEEDS = {}


def case_seed(wavelet, kind_name, n_lines, N, levels):
    key = (wavelet, kind_name, n_lines, N, levels)
    return REPLACED_SEEDS.get(key, SEED0 + 13 * wp.WAVELETS.index(wavelet) + N + 7 * n_lines + (101 if kind_name == "tiny" else 0))


def case_input(wavelet, kind_name, n_lines, N, levels):
    """the lines of a case: wp_model.make_input kinds, "zeros" (every line zero) and "with_zero_line" (line 1 zero)"""
    if kind_name == "zeros":
        return np.zeros((n_lines, N), F32)
    if kind_name.startswith("tone"):
        return np.cos(np.pi * (int(kind_name[4:]) + 0.5) / (1 << levels) * (np.arange(N) + 0.5)).astype(F32)[None]
    x = wp.make_input(case_seed(wavelet, kind_name, n_lines, N, levels), kind_name, n_lines, N)
    return x


def shape_cases():
    """(wavelet, input kind, (n_lines, N, levels), [costs]) of the shape sweep: every shape with the three wavelets; the
    inputs alternate, the short lines take every cost, the long ones two of the five in rotation"""
    out = []
    for i, shape in enumerate(SHAPES):
        for w, wavelet in enumerate(wp.WAVELETS):
            kind_name = ("normal", "tiny")[(i + w) & 1]
            costs = list(COSTS) if shape[1] <= 600 else [COSTS[(i + w) % 5], COSTS[(i + w + 2) % 5]]
            out.append((wavelet, kind_name, shape, costs))
    return out


def layout_cases():
    """every cost on both inputs, the three wavelets, on LAYOUT_SHAPE"""
    return [(wavelet, kind_name, LAYOUT_SHAPE, list(COSTS)) for wavelet in wp.WAVELETS for kind_name in ("normal", "tiny")]


def extra_cases():
    """the inputs of the GPU tests beside the shape and layout sweeps"""
    out = [("cdf97_s", "normal", (MANY_BLOCK,) + MANY_LINES[1:], list(MANY_COSTS))]
    out += [("cdf97_s", "tone%d" % f, TONE_SHAPE, [JOINT_COST]) for f in range(8)]
    return out


_memo = {}


def expected(wavelet, kind_name, shape, cost):
    """-> dict(x, cost, mass, trees, totals, coef) of a case, computed once and never modified"""
    n_lines, N, levels = shape
    k0 = (wavelet, kind_name, shape)
    if k0 not in _memo:
        x = case_input(wavelet, kind_name, n_lines, N, levels)
        x.setflags(write=False)
        _memo[k0] = (x, full_levels(wavelet, x, levels))
    x, stages = _memo[k0]
    k1 = k0 + (cost,)
    if k1 not in _memo:
        c, m, own = cost_tables(cost[0], cost[1], stages, levels)
        sel = [select(c[y], levels) for y in range(n_lines)]
        trees = [t for t, _, _ in sel]
        coef = np.empty_like(x)
        for y in range(n_lines):  # a leaf of a pruned tree is the node of the full tree of its depth
            for j, k, s, n in leaves(N, levels, trees[y]):
                coef[y, s:s + n] = stages[j][y, s:s + n]
        for a in (c, m, own, coef):
            a.setflags(write=False)
        _memo[k1] = dict(x=x, cost=c, mass=m, own=own, trees=trees, totals=[t for _, t, _ in sel], best=[b for _, _, b in sel], coef=coef)
    return _memo[k1]


def joint_tables(wavelet):
    """the tables of wp_joint_basis on LAYOUT_SHAPE: the model's tables of the "normal" case summed over the lines in
    float64, in line order -> (cost, S)"""
    e = expected(wavelet, "normal", LAYOUT_SHAPE, JOINT_COST)
    cost, mass = np.zeros(e["cost"].shape[1]), np.zeros(e["cost"].shape[1])
    for y in range(LAYOUT_SHAPE[0]):
        cost += e["cost"][y]
        mass += e["mass"][y]
    return cost, mass
