"""The user-defined lifting wavelets (include/libdwt_hip.h) restated in numpy: the specification of
struct dwt_hip_lifting one operation at a time -- every float product and sum is a binary32 operation of its own, int
arithmetic wraps in uint32 and shifts arithmetically --, the built-in schemes from their own expressions, seeded random
schemes, and the multi-level Mallat transform of a batch of frames.  The device is held to this model bit for bit."""
import numpy as np

F32, I32 = 0, 1
MAX_STEPS, MAX_TERMS, MAX_OFFSET, FUSED_REACH = 8, 4, 7, 8
f32 = np.float32


class Step:
    def __init__(self, parity, terms, sign=1, add=0, shift=0):
        """terms: [(coefficient, off_a, off_b)]; the coefficient a float (float schemes) or an int (int schemes)"""
        self.parity, self.terms, self.sign, self.add, self.shift = parity, list(terms), sign, add, shift

    @property
    def reach(self):
        return max(max(abs(a), abs(b)) for _, a, b in self.terms)


class Scheme:
    def __init__(self, type_, steps, fwd_scale=(1, 1), inv_scale=(1, 1), inverse_cols_first=None):
        self.type, self.steps = type_, list(steps)
        self.fwd_scale = tuple(f32(v) for v in fwd_scale)
        self.inv_scale = tuple(f32(v) for v in inv_scale)
        self.inverse_cols_first = int(type_ == I32) if inverse_cols_first is None else int(inverse_cols_first)

    @property
    def dtype(self):
        return np.dtype(np.int32 if self.type == I32 else np.float32)

    @property
    def reach(self):
        return sum(s.reach for s in self.steps)

    def table(self):
        """the scheme as plain values: floats as their bits (what libdwt_amd.lifting.Scheme.table gives for the same scheme)"""
        bits = lambda v: int(np.array(v, np.float32).view(np.uint32))
        is_int = self.type == I32
        return (self.type, self.inverse_cols_first, tuple(bits(v) for v in self.fwd_scale), tuple(bits(v) for v in self.inv_scale),
                tuple((s.parity, s.sign if is_int else 1, s.add if is_int else 0, s.shift if is_int else 0,
                       tuple((0 if is_int else bits(c), int(c) if is_int else 0, a, b) for c, a, b in s.terms)) for s in self.steps))


# ---- the built-in schemes, each constant from its own expression -------------------------------------------------------

def _cdf97():
    zeta = f32(1.1496043988602)
    steps = [Step(1, [(f32(-1.58613434342059), -1, 1)]), Step(0, [(f32(-0.0529801185729), -1, 1)]),
             Step(1, [(f32(0.8829110755309), -1, 1)]), Step(0, [(f32(0.4435068520439), -1, 1)])]
    return Scheme(F32, steps, (zeta, f32(1) / zeta), (f32(1) / zeta, zeta), 0)


def _cdf53(update=True):
    s1, s2 = f32(1.41421356237309504880), f32(0.70710678118654752440)
    steps = [Step(1, [(f32(-0.5), -1, 1)])] + ([Step(0, [(f32(0.25), -1, 1)])] if update else [])
    return Scheme(F32, steps, (s1, s2), (s2, s1), 0)


def _cdf53_int():
    return Scheme(I32, [Step(1, [(1, -1, 1)], -1, 0, 1), Step(0, [(1, -1, 1)], +1, 2, 2)])


def _cdf97_int():
    return Scheme(I32, [Step(1, [(203, -1, 1)], -1, -64, 7), Step(0, [(-217, -1, 1)], +1, 2048, 12),
                        Step(1, [(-113, -1, 1)], -1, -64, 7), Step(0, [(1817, -1, 1)], +1, 2048, 12)])


def _haar():
    return Scheme(F32, [Step(1, [(f32(-1), -1, 0)]), Step(0, [(f32(0.5), 1, 0)])], inverse_cols_first=0)


def _haar_int():
    return Scheme(I32, [Step(1, [(1, -1, 0)], -1, 0, 0), Step(0, [(1, 1, 0)], +1, 0, 1)])


def _d4():
    r2, r3 = np.sqrt(f32(2)), np.sqrt(f32(3))  # binary32 square roots, correctly rounded
    three, four, six = f32(3), f32(4), f32(6)
    alpha = f32(-1.0 / float(r3))  # the quotient in double, rounded once
    beta, gamma, delta = (six - three * r3) / four, r3 / four, f32(-1) / three
    steps = [Step(1, [(alpha, 1, 0)]), Step(0, [(beta, -1, 0), (gamma, 1, 0)]), Step(1, [(delta, -1, 0)])]
    return Scheme(F32, steps, ((three + r3) / (three * r2), (three - r3) / (three * r2)),
                  ((three * r2) / (three + r3), (three * r2) / (three - r3)), 0)


BUILTINS = {"CDF97": _cdf97, "CDF53": _cdf53, "INTERP53": lambda: _cdf53(False), "CDF53_INT": _cdf53_int, "CDF97_INT": _cdf97_int,
            "HAAR": _haar, "HAAR_INT": _haar_int, "D4": _d4}
IDS = {name: k for k, name in enumerate(BUILTINS)}  # DWT_HIP_LIFT_*


def builtin(name):
    return BUILTINS[name]()


def random_scheme(type_, seed, reach=None, n_steps=None):
    """a seeded valid scheme; `reach`: the offsets are drawn until the scheme's reach is exactly that.  Float coefficients
    stay below 1 in magnitude with the sum of a step's magnitudes below 1, so a transform grows a sample by at most 2 a step."""
    rng = np.random.default_rng([77, type_, seed])
    while True:
        steps = []
        parity = int(rng.integers(0, 2))
        for _ in range(n_steps or int(rng.integers(1, MAX_STEPS + 1))):
            n_terms = int(rng.integers(1, MAX_TERMS + 1))
            terms = []
            for _ in range(n_terms):
                a = int(rng.choice([-7, -5, -3, -1, 1, 3, 5, 7], p=[.03, .05, .12, .3, .3, .12, .05, .03]))
                b = int(rng.choice([0, -7, -5, -3, -1, 1, 3, 5, 7], p=[.3, .02, .04, .09, .2, .2, .09, .04, .02]))
                c = int(rng.integers(-300, 301)) if type_ == I32 else f32(rng.uniform(-1, 1) / (2 * n_terms))
                terms.append((c, a, b))
            if type_ == I32:
                steps.append(Step(parity, terms, int(rng.choice([-1, 1])), int(rng.integers(-5000, 5001)), int(rng.integers(0, 32))))
            else:
                steps.append(Step(parity, terms))
            parity ^= int(rng.random() < 0.8)  # consecutive steps may share a parity
        s = Scheme(type_, steps)
        if type_ == F32:
            k = f32(rng.uniform(1.05, 1.5))
            s = Scheme(F32, steps, (k, f32(1) / k), (f32(1) / k, k), int(rng.integers(0, 2)))
        if reach is None or s.reach == reach:
            return s


# ---- one line pass -----------------------------------------------------------------------------------------------------

def reflect(i, N):
    """whole-sample symmetric reflection of the indices i into [0, N), bounce by bounce"""
    i = np.array(i, np.int64)
    assert N >= 2
    while ((i < 0) | (i >= N)).any():
        i = np.where(i < 0, -i, i)
        i = np.where(i >= N, 2 * (N - 1) - i, i)
    return i


def _wrap(v):
    return np.uint32(int(v) & 0xFFFFFFFF)


def step_lines(s, st, x, inverse):
    """step st on the lines along the last axis of x, in place (the step reads the other parity only)"""
    N = x.shape[-1]
    idx = np.arange(st.parity, N, 2)
    if N < 2 or not idx.size:
        return
    if s.type == F32:
        total = None
        for c, oa, ob in st.terms:
            a = x[..., reflect(idx + oa, N)]
            if ob:
                a = a + x[..., reflect(idx + ob, N)]
            t = f32(c) * a
            total = t if total is None else total + t
        assert total.dtype == np.float32
        x[..., idx] = x[..., idx] - total if inverse else x[..., idx] + total
    else:
        u = x.view(np.uint32)
        acc = np.zeros(u[..., idx].shape, np.uint32)
        for c, oa, ob in st.terms:
            a = u[..., reflect(idx + oa, N)]
            if ob:
                a = a + u[..., reflect(idx + ob, N)]
            acc = acc + _wrap(c) * a
        v = (acc + _wrap(st.add)).view(np.int32) >> np.int32(st.shift)
        d = v.view(np.uint32) if (st.sign > 0) != bool(inverse) else np.uint32(0) - v.view(np.uint32)
        u[..., idx] = u[..., idx] + d


def pass_lines(s, x, inverse):
    """one 1-D pass over the lines along the last axis of x, in place"""
    N = x.shape[-1]
    scale = s.inv_scale if inverse else s.fwd_scale

    def scaled():
        if s.type == F32:
            for p in (0, 1):
                if scale[p] != f32(1):
                    x[..., p::2] = x[..., p::2] * scale[p]

    with np.errstate(all="ignore"):
        if inverse:
            scaled()
        if N >= 2:
            for st in (reversed(s.steps) if inverse else s.steps):
                step_lines(s, st, x, inverse)
        if not inverse:
            scaled()


# ---- the 2-D transform ---------------------------------------------------------------------------------------------------

def ceil_log2(n):
    return max(0, (int(n) - 1).bit_length())


def levels(W, H, j_max):
    """dwt_hip_band_levels"""
    lo, hi = min(W, H), max(W, H)
    return ceil_log2(hi if lo <= 1 else lo) if j_max < 0 else min(j_max, ceil_log2(hi))


def level2d(s, r, inverse):
    """one level on the rectangles r (B, H, W) in SAMPLE order, in place"""
    rows = lambda: pass_lines(s, r, inverse)

    def cols():
        t = np.ascontiguousarray(r.transpose(0, 2, 1))
        pass_lines(s, t, inverse)
        r[...] = t.transpose(0, 2, 1)

    for p in ((cols, rows) if inverse and s.inverse_cols_first else (rows, cols)):
        p()


def deinterleave(r):
    out = np.empty_like(r)
    hl, wl = (r.shape[1] + 1) // 2, (r.shape[2] + 1) // 2
    out[:, :hl, :wl], out[:, :hl, wl:], out[:, hl:, :wl], out[:, hl:, wl:] = r[:, 0::2, 0::2], r[:, 0::2, 1::2], r[:, 1::2, 0::2], r[:, 1::2, 1::2]
    return out


def interleave(m):
    out = np.empty_like(m)
    hl, wl = (m.shape[1] + 1) // 2, (m.shape[2] + 1) // 2
    out[:, 0::2, 0::2], out[:, 0::2, 1::2], out[:, 1::2, 0::2], out[:, 1::2, 1::2] = m[:, :hl, :wl], m[:, :hl, wl:], m[:, hl:, :wl], m[:, hl:, wl:]
    return out


def fwd2d(s, frames, j_max=-1):
    """(B, H, W) frames -> (their Mallat planes, J)"""
    out = np.array(frames, s.dtype, ndmin=3, copy=True)
    H, W = out.shape[1:]
    J = levels(W, H, j_max)
    for k in range(J):
        h, w = -(-H >> k), -(-W >> k)
        r = np.ascontiguousarray(out[:, :h, :w])
        level2d(s, r, False)
        out[:, :h, :w] = deinterleave(r)
    return out, J


def inv2d(s, planes, j_max=-1):
    out = np.array(planes, s.dtype, ndmin=3, copy=True)
    H, W = out.shape[1:]
    J = levels(W, H, j_max)
    for k in reversed(range(J)):
        h, w = -(-H >> k), -(-W >> k)
        r = interleave(np.ascontiguousarray(out[:, :h, :w]))
        level2d(s, r, True)
        out[:, :h, :w] = r
    return out, J
