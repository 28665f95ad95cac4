"""The conditioning of spectra rows (dwt_util_shift21_med_s, dwt_util_center21_s, dwt_util_scale21_s and their primitives,
src/libdwt.c:25426-26055) restated in numpy, in the arithmetic the device uses: the model reproduces the
device bit for bit and is itself checked against the compiled reference (scripts/gen_condition_golden.py, which asserts
model == reference on every row when it writes tests/golden/condition.npz).

Everything but the centre is plain float32 arithmetic as the reference writes it.  The centre (get_center1, p = 10):
terms t = float32(a^2 ^2 ^2 * a^2) with a = float64(|x|) -- four IEEE double products, no pow --, every sum a chain of
float32 additions in index order, norm = float32(pow(float64(S), float64(float32(1)/float32(10)))), N = term(norm)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "condition.npz")
MANIFEST = os.path.join(HERE, "golden", "condition_manifest.json")

MED_SHIFT, CENTER, SCALE = 1, 2, 4
F = np.float32

KINDS = ("spectrum", "two_peaks", "edge", "zero", "tiny", "huge", "exact", "constant")
SIZES = (1, 2, 3, 5, 64, 65, 255, 1000, 4096, 8192, 8193, 10000)
DISPLACEMENTS = ("-n-1", "-3", "0", "2", "n")


def displacement(name, n):
    return {"-n-1": -n - 1, "-3": -3, "0": 0, "2": 2, "n": n}[name]


def _cases():
    """(seed, kind, n_lines, n).  Every kind at every small size with 2 rows and at 1000 with one; at the large sizes one
    row of the kinds whose golden rows stay small (noise does not compress); one batch of 5 and one of 67 rows.  A seed
    that the generator had to move off a near-tie row is recorded in the manifest (none so far)."""
    out = []
    seed = 100
    for n in SIZES:
        for kind in KINDS:
            if n <= 1000 or kind in ("spectrum", "exact", "zero", "constant") or (kind, n) == ("two_peaks", 4096):
                out.append((seed, kind, 2 if n < 1000 else 1, n))
            seed += 1
    out.append((seed, "spectrum", 5, 255))
    out.append((seed + 1, "two_peaks", 67, 64))
    return out


CASES = _cases()


def make_input(seed, kind, n_lines, n):
    rng = np.random.default_rng(seed)
    x = np.arange(n, dtype=np.float64)
    rows = np.zeros((n_lines, n), np.float64)
    for y in range(n_lines):
        if kind == "spectrum":
            r = 1.0 + 1e-2 * rng.standard_normal(n)
            for _ in range(3):
                r += rng.uniform(0.3, 2.0) * np.exp(-0.5 * ((x - rng.uniform(0.1, 0.9) * n) / max(1.0, 0.01 * n * rng.uniform(0.5, 2))) ** 2)
        elif kind == "two_peaks":
            r = 1e-2 * rng.standard_normal(n)
            w = max(1.0, 0.02 * n)
            r += np.exp(-0.5 * ((x - rng.uniform(0.05, 0.25) * n) / w) ** 2)
            r += rng.uniform(0.93, 1.07) * np.exp(-0.5 * ((x - rng.uniform(0.7, 0.95) * n) / w) ** 2)
        elif kind == "edge":
            r = 1e-3 * rng.standard_normal(n)
            r[0 if (y + seed) % 2 == 0 else n - 1] += 5.0
        elif kind == "zero":
            r = np.zeros(n)
        elif kind == "tiny":
            r = 1e-5 * rng.standard_normal(n)
        elif kind == "huge":
            r = 1e5 * (1.0 + rng.random(n))
        elif kind == "exact":
            r = rng.choice(np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0]), size=n, p=[0.4, 0.15, 0.15, 0.1, 0.1, 0.05, 0.05])
        elif kind == "constant":
            r = np.full(n, float(rng.integers(-3, 4)) * 0.25)
        else:
            raise ValueError(kind)
        rows[y] = r
    return rows.astype(F)


def term(x):
    """|x|^10 as the device forms it (float32 in, float32 out)."""
    with np.errstate(over="ignore", under="ignore"):
        a = np.abs(np.asarray(x, F)).astype(np.float64)
        a2 = a * a
        a4 = a2 * a2
        a8 = a4 * a4
        return (a8 * a2).astype(F)


WARN_NORM, WARN_INDEX = 1, 2


def get_center1(row):
    return get_center1_warn(row)[0]


def get_center1_warn(row):
    """-> (centre, what the reference warns about there: 0, WARN_NORM (zero norm) or WARN_INDEX (a crossing not found))"""
    row = np.asarray(row, F)
    n = row.shape[0]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        t = term(row)
        fwd = np.cumsum(t, dtype=F)  # (accumulate: sequential float32 additions in index order)
        S = fwd[-1]
        norm = F(np.power(np.float64(S), np.float64(F(1.0) / F(10.0))))
        if F(0.0) == norm:
            return n // 2, WARN_NORM
        half = term(norm) / F(2)
        bwd = np.cumsum(t[::-1], dtype=F)
        lidx = ridx = -1
        hit = np.nonzero(fwd > half)[0]
        if hit.size:
            ridx = int(hit[0]) - 1
        hit = np.nonzero(bwd > half)[0]
        if hit.size:
            lidx = (n - 1 - int(hit[0])) + 1
    warn = WARN_INDEX if lidx == -1 or ridx == -1 else 0
    if lidx == -1 and ridx == -1:
        return n // 2, warn
    if lidx == -1:
        lidx = ridx
    elif ridx == -1:
        ridx = lidx
    return int((lidx + ridx) / 2), warn  # C integer division (both are >= 0 here)


def displace1(row, d, zero_fill):
    row = np.asarray(row, F)
    n = row.shape[0]
    q = np.arange(n, dtype=np.int64) + d
    qc = np.clip(q, 0, n - 1)
    out = row[qc].copy()
    if zero_fill:
        out[q != qc] = F(0.0)
    return out


def median(row):
    row = np.asarray(row, F)
    return np.sort(row)[row.shape[0] // 2]


def shift_med(row):
    row = np.asarray(row, F)
    return (row + (-median(row))).astype(F)


def center1(row, max_iters):
    """-> (row, net offset, moves, last centre found or -1)"""
    row = np.asarray(row, F).copy()
    n = row.shape[0]
    off, moves, c = 0, 0, -1
    for _ in range(max_iters):
        c = get_center1(row)
        displ = n // 2 - c
        if displ == 0:
            break
        row = displace1(row, -displ, True)
        off += -displ
        moves += 1
    return row, off, moves, c


def center_warnings(rows, ops, max_iters=20):
    """-> (zero norms, missing indexes) over every centre evaluation that conditioning `rows` makes"""
    count = [0, 0, 0]
    if ops & CENTER:
        for row in np.asarray(rows, F):
            row = shift_med(row) if ops & MED_SHIFT else row.copy()
            for _ in range(max_iters):
                c, warn = get_center1_warn(row)
                count[warn] += 1
                if c == row.shape[0] // 2:
                    break
                row = displace1(row, c - row.shape[0] // 2, True)
    return count[WARN_NORM], count[WARN_INDEX]


def min_max(row):
    row = np.asarray(row, F)
    return row.min(), row.max()


def scale1(row, lo, hi):
    """-> (row, skipped)"""
    row = np.asarray(row, F)
    mn, mx = min_max(row)
    if mx == mn:
        return row.copy(), 1
    with np.errstate(over="ignore", invalid="ignore"):
        target = F(hi) - F(lo)
        diff = mx - mn
        out = (row + (F(lo) - mn)).astype(F)
        out = (out * (target / diff)).astype(F)
    return out, 0


def condition(rows, ops, max_iters=20, lo=0.0, hi=1.0):
    """-> (rows, info): info[y] = (net offset, moves, last centre or -1, scale skipped)"""
    rows = np.asarray(rows, F)
    out = np.empty_like(rows)
    info = np.zeros((rows.shape[0], 4), np.int32)
    for y, row in enumerate(rows):
        off, moves, c, skip = 0, 0, -1, 0
        if ops & MED_SHIFT:
            row = shift_med(row)
        if ops & CENTER:
            row, off, moves, c = center1(row, max_iters)
        if ops & SCALE:
            row, skip = scale1(row, lo, hi)
        out[y] = row
        info[y] = (off, moves, c, skip)
    return out, info


def reversing_row():
    """A row of 64 samples (found by a seed search) whose centring moves it one way and then back, so that samples lost to
    the zero fill stay lost: its result is NOT one shift of the original row by the net offset."""
    rng = np.random.default_rng(2847)
    return rng.choice(np.array([0, 0.5, -0.5, 1, -1, 2, -2.0]), size=64, p=[0.6, 0.1, 0.1, 0.06, 0.06, 0.04, 0.04]).astype(F)


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden
