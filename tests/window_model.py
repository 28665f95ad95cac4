"""The numpy model of the windowed inverse (include/libdwt_hip.h, dwt_hip_window_regions / dwt_hip_inverse_window_batch;
DESIGN.md s30), shared by tests/test_window.py, tests/test_hip_window.py and tests/window_stream.py.

`regions` restates the rule of the header: per line the interleaved indices 2 floor(a/2) - K + 1 .. 2 floor((b-1)/2) + K + 1
folded into the line by whole-sample reflection, their least and greatest giving the L and the H indices; level by level
from the window up to LL(J).  `expected` is the crop of the full inverse -- the oracle's for the float 9/7, the float and
the int32 5/3, tests/interp53_model.py and tests/i16_model.py for the other two."""
import numpy as np

WAVELETS = ["cdf97_s", "cdf53_s", "interp53_s", "cdf53_i", "cdf53_i16"]
FLOAT_WAVELETS = WAVELETS[:3]
HALO = {"cdf97_s": 4, "cdf53_s": 2, "interp53_s": 1, "cdf53_i": 2, "cdf53_i16": 2}
DTYPE = {"cdf97_s": np.float32, "cdf53_s": np.float32, "interp53_s": np.float32, "cdf53_i": np.int32, "cdf53_i16": np.int16}
ORACLE_INVERSE = {"cdf97_s": "cdf97_2i_s", "cdf53_s": "cdf53_2i_s", "cdf53_i": "cdf53_2i_i"}
# the frames of the sweeps, (h, w): one row, one column, two rows, a small square, odd sizes at every level twice, more rows than columns
SHAPES = [(1, 9), (9, 1), (2, 7), (5, 5), (17, 33), (61, 131), (100, 37)]


def ceil_log2(x):
    n = 0
    while (1 << n) < x:
        n += 1
    return n


def band(size, level):
    """ceil(size / 2^level)"""
    return (size + (1 << level) - 1) >> level


def levels(h, w, j_max):
    J = ceil_log2(min(h, w))
    return j_max if 0 <= j_max < J else J


def reflect(i, n):
    period = 2 * (n - 1)
    i %= period
    return i if i < n else period - i


def need(a, b, n, k):
    """the samples [a, b) of a line of n: ((first L, last L), (first H, last H)), a pair with last < first being empty"""
    if n == 1:
        return (0, 0), (0, -1)
    folded = [reflect(i, n) for i in range(2 * (a // 2) - k + 1, 2 * ((b - 1) // 2) + k + 2)]
    lo, hi = min(folded), max(folded)
    return (-(-lo // 2), hi // 2), (lo // 2, (hi - 1) // 2)


def regions(wavelet, h, w, j_max, discard, x0, y0, ww, wh):
    """(3 J + 1, 4) int32 {x, y, size_x, size_y}; None for arguments the entry refuses"""
    if wavelet not in HALO or h < 1 or w < 1:
        return None
    J, k = levels(h, w, j_max), HALO[wavelet]
    if not 0 <= discard <= J:
        return None
    if x0 < 0 or y0 < 0 or ww < 1 or wh < 1 or x0 + ww > band(w, discard) or y0 + wh > band(h, discard):
        return None
    out = np.zeros((3 * J + 1, 4), np.int32)

    def put(slot, x, cols, y, rows):
        if cols[1] >= cols[0] and rows[1] >= rows[0]:
            out[slot] = (x + cols[0], y + rows[0], cols[1] - cols[0] + 1, rows[1] - rows[0] + 1)

    X, Y = (x0, x0 + ww - 1), (y0, y0 + wh - 1)
    for l in range(discard + 1, J + 1):
        Lx, Hx = need(X[0], X[1] + 1, band(w, l - 1), k)
        Ly, Hy = need(Y[0], Y[1] + 1, band(h, l - 1), k)
        put(3 * (l - 1) + 0, band(w, l), Hx, 0, Ly)
        put(3 * (l - 1) + 1, 0, Lx, band(h, l), Hy)
        put(3 * (l - 1) + 2, band(w, l), Hx, band(h, l), Hy)
        X, Y = Lx, Ly
    put(3 * J, 0, X, 0, Y)
    return out


def inside(reg, h, w):
    """bool (h, w): the elements of a frame that lie in one of the rectangles"""
    m = np.zeros((h, w), bool)
    for x, y, sx, sy in reg:
        m[y:y + sy, x:x + sx] = True
    return m


def full_inverse(oracle, wavelet, frame, j_max, discard):
    """the inverse at J - discard levels of the top-left LL(discard)-sized rectangle of `frame`, as a new array"""
    h, w = frame.shape
    J = levels(h, w, j_max)
    a = np.ascontiguousarray(frame[:band(h, discard), :band(w, discard)]).copy()
    if J == discard:
        return a
    with np.errstate(all="ignore"):
        if wavelet == "interp53_s":
            import interp53_model

            interp53_model.inv2d(a, j_max=J - discard)
        elif wavelet == "cdf53_i16":
            import i16_model

            i16_model.inv2d(a, j_max=J - discard)
        else:
            oracle.inv(ORACLE_INVERSE[wavelet], a, J - discard)
    return a


def expected(oracle, wavelet, frame, j_max, discard, x0, y0, ww, wh):
    return full_inverse(oracle, wavelet, frame, j_max, discard)[y0:y0 + wh, x0:x0 + ww].copy()


def make_frame(wavelet, seed, h, w):
    """a coefficient frame: normal floats, or integers over the whole range of the type"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(DTYPE[wavelet])
    if dt.kind == "f":
        return rng.standard_normal((h, w)).astype(dt)
    ii = np.iinfo(dt)
    return rng.integers(ii.min, ii.max + 1, (h, w), dtype=np.int64).astype(dt)


def masked(wavelet, frame, reg, seed):
    """`frame` with everything outside the rectangles replaced: NaN (floats), other random integers of the whole range"""
    keep = inside(reg, *frame.shape)
    if frame.dtype.kind == "f":
        junk = np.full(frame.shape, np.nan, frame.dtype)
    else:
        junk = make_frame(wavelet, seed + 7919, *frame.shape)
    return np.where(keep, frame, junk)


def sweep_windows(rng, bw, bh, n_random):
    """(x0, y0, w, h) in a band of bw x bh: the whole band, the four 1 x 1 corners, n_random random interiors"""
    out = [(0, 0, bw, bh), (0, 0, 1, 1), (bw - 1, 0, 1, 1), (0, bh - 1, 1, 1), (bw - 1, bh - 1, 1, 1)]
    for _ in range(n_random):
        x0, y0 = int(rng.integers(0, bw)), int(rng.integers(0, bh))
        out.append((x0, y0, int(rng.integers(1, bw - x0 + 1)), int(rng.integers(1, bh - y0 + 1))))
    return list(dict.fromkeys(out))


def border_windows(h, w, depth=16):
    """the four border windows of `depth` rows or columns: top, bottom, left, right"""
    dy, dx = min(depth, h), min(depth, w)
    return [(0, 0, w, dy), (0, h - dy, w, dy), (0, 0, dx, h), (w - dx, 0, dx, h)]


def same(got, want):
    """bit for bit, a NaN equal to a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    u = {4: np.uint32, 2: np.uint16, 8: np.uint64}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(u)[~gn], want.view(u)[~wn]))
