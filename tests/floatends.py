"""Two float input classes whose transforms stay (almost) free of NaN, and the cases built on them
(tests/test_float_ends.py, tests/test_hip_float_ends.py, tests/test_hip_sweep_matrix.py, oracle/gen_golden.py float_ends).

`conftest.same_floats` leaves out every sample that is a NaN on both sides.  On the overflowing classes of
`conftest.full_range_floats` ("huge", "mixed") most of a forward result and all of an inverse is NaN, so those classes say
little about a kernel's line ends above MAX/2 -- the one place where the reference's (2c)*x and plain reflection's c*(x+x)
differ.  The classes here keep the overflow local:

  finite_floats  nothing overflows at any depth: every sample of every result is compared bit for bit;
  ends_floats    a few finite values above MAX/2 next to the line ends (where both taps of an end fall) and a few isolated
                 +-Inf / NaN; the NaN share of a result stays below `NAN_CAP` and at least `TELLING_MIN` samples per (entry,
                 direction) differ between the two end forms (asserted with the oracle alone, tests/test_float_ends.py).

An inverse runs on an input of the class itself, read as a coefficient image -- not on a forward result."""
import contextlib

import numpy as np

from conftest import bits

NAN_CAP = 0.25     # condition (a): the largest NaN share of an expected result
TELLING_MIN = 8    # condition (b): samples per (entry, direction), summed over the shapes, that tell the two end forms apart

# the sweep kernels' edge shapes (tests/test_hip_sweep_matrix.py says why each) ...
SWEEP_SHAPES = [(131, 1030), (67, 259), (40, 513), (12, 256), (9, 257), (5, 1541)]
# ... two more with both sides odd / both a multiple of 16, and the degenerate ones of the CPU comparison
SHAPES = SWEEP_SHAPES + [(37, 53), (64, 80)]
TINY_SHAPES = [(2, 9), (9, 1), (1, 9)]
# interp53 has a doubled tap on even lines only (6 of the 16 sides above): two shapes even both ways on top
INTERP_SHAPES = SHAPES + [(66, 260), (132, 1028)]
# row batches of the 1-D entries (lines, samples): short, odd, multiples of 4 (an even line at level 2 too), past the one-launch cap of 8192
LINE_SHAPES = [(6, 9), (6, 64), (5, 257), (8, 512), (4, 1032), (3, 8197), (3, 8200)]
VOLUMES = [(9, 7, 6), (12, 40, 272), (33, 70, 300)]  # (z, y, x), those of the whole-range fixtures


def _specials(dtype, large):
    fi = np.finfo(dtype)
    tiny, sub = dtype(fi.tiny), dtype(fi.smallest_subnormal)
    v = [0.0, -0.0, sub, -sub, sub * 3, sub * 1000, tiny, -tiny, tiny * dtype(0.75), tiny * dtype(1.5), 1.0, -1.0, dtype(fi.eps)]
    if large:
        # 1e30 and 2^100 of float, the same fraction of the largest double: 12 levels of LL gain 2 stay finite
        s = float(fi.max) / float(np.finfo(np.float32).max)
        v += [1e30 * s, -1e30 * s, 2.0 ** 100 * s, -2.0 ** 100 * s]
    return np.array(v, dtype=dtype)


def _base(rng, shape, dtype, large):
    a = (rng.random(shape) * 2 - 1).astype(dtype)
    pick = rng.random(shape) < 0.25
    a[pick] = rng.choice(_specials(dtype, large), size=int(pick.sum()))
    return a


def finite_floats(rng, shape, dtype=np.float32):
    """Uniform [-1, 1), a quarter of the samples from +-0, subnormals, the smallest normal and its neighbours, +-1, eps,
    +-1e30 and +-2^100 (doubles: the same fractions of the largest double).  No transform of any depth overflows."""
    return _base(rng, shape, dtype, True)


def _near_positions(h, w, lines):
    """Where a value above MAX/2 meets a doubled tap: the sample next to a line end -- (row, column, kind).  Columns 1 and
    w-2 of three rows, rows 1 and h-2 of three columns and of the tile seams (kind 0) -- and, for an inverse, the Mallat
    positions that interleave to the same samples at levels 1 and 2: the first H coefficient (kind 1) and the last L
    coefficient of an even line or the last H of an odd one (kind 2 / 1).
    `lines`: the rows are lines of a 1-D batch -- every row, no column direction."""
    def ends(n):
        out = [(1, 0), (n - 2, 0)]
        for m in (n, (n + 1) // 2):  # the line of level 1, of level 2
            nl = (m + 1) // 2
            out += [(nl, 1), (nl - 1, 2) if m % 2 == 0 else (m - 1, 1)]
        return out
    if lines:
        return [(r, c, k) for r in range(h) for c, k in ends(w)]
    pos = [(r, c, k) for r in (h // 4, h // 2, 3 * h // 4) for c, k in ends(w)]
    pos += [(r, c, k) for c in (w // 5, w // 2, 4 * w // 5, 255, 256, 257, 511, 512, 513) for r, k in ends(h)]
    return pos


def _lone_positions(h, w):
    return [(h // 3, c, 0) for c in (0, w - 1, 255, 256, 511, 512, 1023, 1024)] + [(0, w // 3, 0), (h - 1, 2 * w // 3, 0)]


def _inside(pos, h, w):
    seen, out = set(), []
    for r, c, k in pos:
        if 0 <= r < h and 0 <= c < w and (r, c) not in seen:
            seen.add((r, c))
            out.append((r, c, k))
    return out


def ends_floats(rng, shape, dtype=np.float32, reach=81, lines=False):
    """The base of `finite_floats` without its large magnitudes; finite values of 0.59 .. 0.85 of the largest (float: 2e38 ..
    2.9e38) on the samples next to a line end; isolated +Inf, -Inf, NaN and 0.97 of the largest (3.3e38) on row h/3 and at
    (0, w/3), (h-1, 2w/3).  `reach`: the samples one special spreads to in a level (2-D 9 x 9, lines 9, volumes 9 x 9 x 9).
    Small images take every stride-th position of both lists (the first shuffled, so that no stride skips one kind of
    position), stride = positions * reach * 4 / samples, and none of the second list below 8 * reach samples: what the
    specials spread to stays a small share of the image.
    An inverse scales before it lifts -- the H coefficients by sqrt 2 (5/3) or 1.15 (9/7), the L ones by their inverses --:
    the H positions take 0.59 and 0.66 of the largest, the L positions 0.74 and more, so that both stay finite and above
    MAX/2 there."""
    h, w = shape
    a = _base(rng, shape, dtype, False)
    big = dtype(np.finfo(dtype).max)
    near = _inside(_near_positions(h, w, lines), h, w)
    near = [near[i] for i in rng.permutation(len(near))]
    lone = _inside(_lone_positions(h, w), h, w) if h * w >= 8 * reach else []
    stride = max(1, len(near) * reach * 4 // (h * w))
    frac = {0: (0.59, 0.85, 0.74, 0.66, 0.79, 0.82), 1: (0.59, 0.66), 2: (0.85, 0.74, 0.79, 0.82)}
    lonev = [dtype(np.inf), dtype(-np.inf), dtype(np.nan), big * dtype(0.97)]
    for n, (r, c, kind) in enumerate(near[::stride]):
        f = frac[kind]
        a[r, c] = big * dtype(f[(n // 2) % len(f)]) * dtype(-1 if n & 1 else 1)
    for n, (r, c, _) in enumerate(lone[::stride]):
        a[r, c] = lonev[n % len(lonev)]
    return a


def ends_volume(rng, shape, dtype=np.float32):
    """`ends_floats` on the (z*y, x) rows of a volume, plus (volumes of 16 * 729 samples and more) values above MAX/2 next to
    the ends of the z lines."""
    nz, ny, nx = shape
    v = ends_floats(rng, (nz * ny, nx), dtype, reach=729).reshape(shape).copy()
    big = dtype(np.finfo(dtype).max)
    if nz >= 3 and v.size >= 16 * 729:
        for k, (z, y, x) in enumerate([(1, ny // 2, nx // 3), (nz - 2, ny // 3, nx // 2), (1, ny - 1, nx - 1), (nz - 2, 0, 0)]):
            v[z, y, x] = big * dtype(0.6 + 0.05 * k) * dtype(-1 if k & 1 else 1)
    return v


def finite_volume(rng, shape, dtype=np.float32):
    return finite_floats(rng, (shape[0] * shape[1], shape[2]), dtype).reshape(shape).copy()


def class_input(klass, seed, shape, dtype=np.float32, lines=False):
    """The input of a case: class "finite" or "ends"; 2-D shapes, row batches of 1-D lines, (z, y, x) volumes."""
    rng = np.random.default_rng(seed)
    if len(shape) == 3:
        return (finite_volume if klass == "finite" else ends_volume)(rng, tuple(shape), dtype)
    if klass == "finite":
        return finite_floats(rng, tuple(shape), dtype)
    return ends_floats(rng, tuple(shape), dtype, reach=9 if lines else 81, lines=lines)


def telling(a, b):
    """The samples that differ under `conftest.same_floats`: a NaN on one side only, or other bits where neither is one."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (bits(a) != bits(b)))).sum())


def nan_share(a):
    return float(np.isnan(a).mean()) if a.size else 0.0


def nonfinite_share(a):
    return float((~np.isfinite(a)).mean()) if a.size else 0.0


# ---- the interpolating 5/3 (tests/interp53_model.py) with its one doubled tap written as reflection gives it ----
@contextlib.contextmanager
def interp53_reflected_ends():
    """Within the block interp53_model evaluates the last odd sample of an even line as p*(x+x) instead of the reference's
    (2p)*x: the form to count telling samples against (no kernel is held to it)."""
    import interp53_model as M

    M.REFLECTED_ENDS = True
    try:
        yield
    finally:
        M.REFLECTED_ENDS = False


# ---- the entries and how the checkers run them -------------------------------------------------------------------------
ENTRY2D = {
    "cdf97_s": ("cdf97_2f_s", "cdf97_2i_s"), "cdf53_s": ("cdf53_2f_s", "cdf53_2i_s"),
    "cdf97_d": ("cdf97_2f_d", "cdf97_2i_d"), "cdf53_d": ("cdf53_2f_d", "cdf53_2i_d"),
    "cdf97_il": ("cdf97_2f_inplace_s", "cdf97_2i_inplace_s"), "cdf53_il": ("cdf53_2f_inplace_s", "cdf53_2i_inplace_s"),
}  # (= test_float_range.ENTRY)
ENTRIES = list(ENTRY2D) + ["cdf97_1d", "cdf53_1d", "interp53_2d", "interp53_1d", "cdf97_3d"]


def entry_dtype(e):
    return np.float64 if e.endswith("_d") else np.float32


def entry_shapes(e):
    return VOLUMES if e == "cdf97_3d" else LINE_SHAPES if e.endswith("_1d") else INTERP_SHAPES if e == "interp53_2d" else SHAPES


def _vol_ref(b):
    import ctypes as C

    class Vol(C.Structure):
        _fields_ = [("size_x", C.c_int), ("size_y", C.c_int), ("size_z", C.c_int), ("stride_x", C.c_size_t),
                    ("stride_y", C.c_size_t), ("stride_z", C.c_size_t), ("data", C.c_void_p)]
    return C.byref(Vol(b.shape[2], b.shape[1], b.shape[0], b.strides[2], b.strides[1], b.strides[0], b.ctypes.data))


def transform(impl, e, inverse, a, j=-1, d1=0):
    """Entry `e` forward (inverse: on `a` as coefficients) by the checker `impl` -- an oraclelib.Oracle or .Reference -- on a
    copy of `a`; returns (result, level count).  3-D: one level.  1-D: every row of `a` a line."""
    import interp53_model as M
    from oraclelib import Oracle
    from test_oned import ref_call, ref_lib, restated

    is_oracle = isinstance(impl, Oracle)
    b = np.ascontiguousarray(a).copy()
    if e in ENTRY2D:
        name = ENTRY2D[e][1 if inverse else 0]
        return b, (impl.inv if inverse else impl.fwd)(name, b, j, decompose_one=d1)
    if e == "cdf97_3d":
        if is_oracle:
            return impl.vol("cdf97_3i_s" if inverse else "cdf97_3f_s", b), 1
        getattr(impl.lib, "cdf97_3%s_ip_sep_horizontal_s" % ("i" if inverse else "f"))(_vol_ref(b))
        return b, 1
    if e.startswith("interp53"):
        m = M if is_oracle else M.RefInterp53()
        if e == "interp53_2d":
            f = m.inv2d if inverse else m.fwd2d
            jo = f(b, j_max=j, decompose_one=d1)
        else:
            jo = (m.inv1d if inverse else m.fwd1d)(b, j_max=j)
        return b, (j if inverse else jo)
    wv = e[:5]
    jo = j
    for y in range(b.shape[0]):
        if is_oracle:
            jo = restated(impl, wv, inverse, b[y], b.shape[1], None, j)
        else:
            jo = ref_call(ref_lib(impl), wv, inverse, b[y], b.shape[1], None, j)
    return b, jo


@contextlib.contextmanager
def reflected_ends(oracle):
    """Every checker's line ends as reflection gives them, c*(x+x)."""
    with oracle.reflected_ends(), interp53_reflected_ends():
        yield


def ends_level(oracle, e, a, d1=0):
    """The depth an "ends" case runs at: 2 where the oracle's forward and inverse both keep the NaN share within NAN_CAP,
    else 1 (one level mixes the specials into a 9 x 9 neighbourhood, two into 25 x 25: too much of a small image)."""
    if e == "cdf97_3d" or e.startswith("interp53"):
        # (interp53: its one doubled tap, the last odd sample of an even line, takes an L coefficient, which an inverse has
        # scaled by 1/sqrt 2 per level: above MAX/2 and finite at one level only -- and level 1's position is where level 2
        # writes.  One level keeps level 1's ends telling.)
        return 1
    with np.errstate(all="ignore"):
        if all(nan_share(transform(oracle, e, inv, a, 2, d1)[0]) <= NAN_CAP for inv in (0, 1)):
            return 2
    return 1


# ---- the cases of tests/golden/float_ends.npz ---------------------------------------------------------------------------
FULL_SHAPES = {(37, 53), (6, 9), (6, 64), (9, 7, 6)} | set(TINY_SHAPES)  # stored in full; the others as hashes


def case_list():
    """(entry, class, shape, decompose_one, stored in full) of every fixture case, in the order of their seeds.  The tiny
    shapes go with the 2-D entries only and decompose to the longer side (a 1 x 9 image has no level otherwise)."""
    out = []
    for e in ENTRIES:
        shapes = list(entry_shapes(e))
        if e in ENTRY2D or e == "interp53_2d":
            shapes += TINY_SHAPES
        for klass in ("finite", "ends"):
            for shp in shapes:
                out.append((e, klass, tuple(shp), 1 if shp in TINY_SHAPES else 0, tuple(shp) in FULL_SHAPES))
    return out


def case_input(m):
    """The input of manifest case `m`, regenerated from its seed."""
    return class_input(m["klass"], m["seed"], tuple(m["shape"]), entry_dtype(m["entry"]), m["entry"].endswith("_1d"))


def is_tiny(shape):
    """Shapes of a few samples, where one overflow reaches every sample: compared with the reference like the others, left
    out of conditions (a) and (b)."""
    return tuple(shape) in TINY_SHAPES or tuple(shape) == (9, 7, 6)
