"""Model of the wavelet packet transforms: every node of every level is split again.  A packet level is
the reference's own one-level transform applied to each node, so the model composes the CPU oracle's one-level transforms
(tests/oraclelib.py; the interpolating 5/3 from tests/interp53_model.py) node by node on numpy views.

* `nodes_recursive`, `nodes_closed_form` -- the natural-order node table of one level of an N-sample line, by the
  recursion of the definition and by the closed form len(k) = (N - bitrev_j(k) + 2^j - 1) >> j;
* `freq_order` -- the Gray code: the natural index of the node with the f-th lowest band;
* `fwd1d`, `inv1d` -- packets of every row of a 2-D array (the lines of a batch).  A node of a line is handed to the
  oracle's one-level LINE function (the 2-D drivers are no stand-in for it on a 1 x n image: the 5/3 drivers run the column
  pass over lines of one sample too, which scales them);
* `fwd2d`, `inv2d` -- packets of an image: a node's rectangle is a numpy view passed to fwd(name, view, 1) / inv(...);
* `make_input` -- seeded inputs of the kinds of tests/swt2d_model.py;
* `CASES_1D`, `CASES_2D` -- what tests/golden/wp.npz holds, written by scripts/gen_wp_golden.py from the compiled reference.
"""
import os

import numpy as np

import interp53_model as i53
import swt2d_model as m2
import swt_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wp.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "wp_manifest.json")

F32 = np.float32
WAVELETS = ("cdf97_s", "cdf53_s", "interp53_s")
WAVELET_ID = {"cdf97_s": 0, "cdf53_s": 2, "interp53_s": 6}  # enum dwt_hip_wavelet
KINDS = m2.KINDS
MAX_LEVELS_2D = 8
NONFINITE_CAP = 0.25  # float_range: at most this share of the golden result may be non-finite

_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        import oraclelib
        _oracle = oraclelib.Oracle()
    return _oracle


def floor_log2(n):
    return n.bit_length() - 1


def max_levels_1d(N):
    return floor_log2(N)


def max_levels_2d(size_y, size_x):
    return min(floor_log2(min(size_y, size_x)), MAX_LEVELS_2D)


# ---- node geometry -------------------------------------------------------------------------------------------
def nodes_recursive(N, level):
    """[(start, len)] of the 2^level nodes of `level` in natural order: L child first, H child behind it"""
    nodes = [(0, N)]
    for _ in range(level):
        nxt = []
        for s, n in nodes:
            nl = (n + 1) // 2
            nxt += [(s, nl), (s + nl, n - nl)]
        nodes = nxt
    return nodes


def bitrev(k, j):
    r = 0
    for _ in range(j):
        r = (r << 1) | (k & 1)
        k >>= 1
    return r


def nodes_closed_form(N, level):
    out, s = [], 0
    for k in range(1 << level):
        n = (N - bitrev(k, level) + (1 << level) - 1) >> level
        out.append((s, n))
        s += n
    return out


def freq_order(level):
    """perm[f] = natural index of the node whose band is the f-th lowest"""
    return [f ^ (f >> 1) for f in range(1 << level)]


# ---- one level of one node -----------------------------------------------------------------------------------
def _line_fwd(wavelet, t):
    """the one-level forward line function on the rows of t (lines x n, n >= 2): L | H per row"""
    n = t.shape[1]
    if wavelet == "interp53_s":
        il = i53.fwd_lines(t)
    else:
        il = np.ascontiguousarray(t, F32).copy()
        for row in il:
            oracle().line(wavelet[:-2] + "_f_s", row)
    out = np.empty_like(il)
    out[:, :(n + 1) // 2] = il[:, 0::2]
    out[:, (n + 1) // 2:] = il[:, 1::2]
    return out


def _line_inv(wavelet, t):
    n = t.shape[1]
    il = np.empty(t.shape, F32)
    il[:, 0::2] = t[:, :(n + 1) // 2]
    il[:, 1::2] = t[:, (n + 1) // 2:]
    if wavelet == "interp53_s":
        return i53.inv_lines(il)
    for row in il:
        oracle().line(wavelet[:-2] + "_i_s", row)
    return il


def fwd1d(wavelet, a, levels):
    """forward packets of every row of a (lines x N); returns a new array: the 2^levels leaves in natural order"""
    a = np.array(a, dtype=F32, copy=True)
    N = a.shape[1]
    assert 1 <= levels <= max_levels_1d(N)
    for lev in range(levels):
        for s, n in nodes_recursive(N, lev):
            a[:, s:s + n] = _line_fwd(wavelet, a[:, s:s + n])
    return a


def inv1d(wavelet, a, levels):
    a = np.array(a, dtype=F32, copy=True)
    N = a.shape[1]
    assert 1 <= levels <= max_levels_1d(N)
    for lev in range(levels - 1, -1, -1):
        for s, n in nodes_recursive(N, lev):
            a[:, s:s + n] = _line_inv(wavelet, a[:, s:s + n])
    return a


def _node2d(wavelet, view, inverse):
    """one level of the 2-D driver, in place on the node's rectangle"""
    if wavelet == "interp53_s":
        (i53.inv2d if inverse else i53.fwd2d)(view, j_max=1)
    elif inverse:
        oracle().inv(wavelet[:-2] + "_2i_s", view, 1)
    else:
        assert oracle().fwd(wavelet[:-2] + "_2f_s", view, 1) == 1


def _packets2d(wavelet, a, levels, inverse):
    a = np.array(a, dtype=F32, copy=True)
    size_y, size_x = a.shape
    assert 1 <= levels <= max_levels_2d(size_y, size_x)
    for lev in (range(levels - 1, -1, -1) if inverse else range(levels)):
        for sy, h in nodes_recursive(size_y, lev):
            for sx, w in nodes_recursive(size_x, lev):
                _node2d(wavelet, a[sy:sy + h, sx:sx + w], inverse)
    return a


def fwd2d(wavelet, a, levels):
    """forward packets of the image a; returns a new array"""
    return _packets2d(wavelet, a, levels, False)


def inv2d(wavelet, a, levels):
    return _packets2d(wavelet, a, levels, True)


# ---- inputs --------------------------------------------------------------------------------------------------
def make_input(seed, kind, size_y, size_x, image=False):
    """seeded rows (image=False: size_y lines of size_x samples) or one image.  float_range: a few huge, infinite and NaN
    samples among finite ones, few enough that most of a transform of up to 3 levels stays finite -- every level spreads
    a non-finite sample over its neighbours, in an image along both axes, so there the special values lie together in one
    block of 2 x 3 samples at a seeded place"""
    if kind != "float_range":
        return m2.make_input(seed, kind, size_y, size_x)
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((size_y, size_x)).astype(F32)
    r = rng.random((size_y, size_x))
    a[r < 0.30] *= F32(m2.TINY / 4)  # subnormals and the smallest normals
    a[(r >= 0.30) & (r < 0.36)] = F32(0.0)
    a[(r >= 0.36) & (r < 0.42)] = F32(-0.0)
    big = (r >= 0.42) & (r < 0.52)
    a[big] = (np.sign(a[big]) * F32(1e30) * (F32(1) + np.abs(a[big]))).astype(F32)  # near 1e30: sums stay finite
    special = (F32(np.nan), F32(np.inf), F32(-np.inf), F32(3e38), F32(-3e38), F32(m2.TINY / 8))
    if image:
        y0, x0 = int(rng.integers(0, max(size_y - 1, 1))), int(rng.integers(0, max(size_x - 2, 1)))
        for i, v in enumerate(special):
            a[min(y0 + i // 3, size_y - 1), min(x0 + i % 3, size_x - 1)] = v
        return a
    flat = a.reshape(-1)
    # one special value per 512 samples (at least the six), at seeded places
    n = max(len(special), flat.size // 512)
    for i, p in enumerate(rng.choice(flat.size, size=min(n, flat.size), replace=False)):
        flat[p] = special[i % len(special)]
    return a


def same(a, b):
    """bit-equal float32 arrays, a NaN on both sides not compared"""
    return sm.same(a, b)


def nonfinite_share(a):
    return float((~np.isfinite(a)).sum()) / max(a.size, 1)


# ---- the golden cases ----------------------------------------------------------------------------------------
# (seed, wavelet, kind, n_lines, N, levels)
CASES_1D = [
    (5101, "cdf97_s", "normal", 2, 2, 1),
    (5102, "cdf53_s", "small_ints", 2, 3, 1),
    (5103, "interp53_s", "normal", 2, 5, 2),
    (5104, "cdf97_s", "small_ints", 3, 8, 3),
    (5105, "cdf53_s", "normal", 2, 63, 5),
    (5106, "interp53_s", "small_ints", 2, 64, 6),
    (5107, "cdf97_s", "normal", 2, 100, 6),
    (5108, "cdf97_s", "tiny", 2, 257, 4),
    (5109, "cdf53_s", "tiny", 2, 129, 7),
    (5110, "interp53_s", "tiny", 2, 100, 3),
    (5111, "cdf97_s", "float_range", 2, 1025, 3),
    (5112, "cdf53_s", "float_range", 2, 600, 3),
    (5113, "interp53_s", "float_range", 2, 513, 2),
    (5114, "cdf53_s", "normal", 1, 1025, 10),
    (5115, "cdf97_s", "normal", 1, 513, 9),
    (5116, "interp53_s", "normal", 1, 512, 9),
]
# (seed, wavelet, kind, size_y, size_x, levels)
CASES_2D = [
    (5201, "cdf97_s", "normal", 2, 2, 1),
    (5202, "cdf53_s", "small_ints", 3, 5, 1),
    (5203, "interp53_s", "normal", 8, 8, 3),
    (5204, "cdf97_s", "small_ints", 47, 33, 5),
    (5205, "cdf53_s", "normal", 33, 47, 5),
    (5206, "interp53_s", "small_ints", 21, 64, 4),
    (5207, "cdf97_s", "tiny", 40, 37, 3),
    (5208, "cdf53_s", "tiny", 16, 19, 4),
    (5209, "cdf97_s", "float_range", 64, 64, 2),
    (5210, "cdf53_s", "float_range", 48, 64, 3),
    (5211, "interp53_s", "float_range", 64, 40, 3),
    (5212, "cdf97_s", "normal", 64, 64, 6),
]


def case_key(dim, i):
    return "%dd_%d" % (dim, i)
