"""The user-defined lifting wavelets of LINE batches (dwt_hip_lifting1d_batch; include/libdwt_hip.h) restated
in numpy on top of tests/lifting_model.py: its line pass (pass_lines: one operation at a time, binary32 or wrapping int32)
under the 1-D level loop and the 1-D Mallat layout of dwt_hip_transform1d_batch, and the synthesis norms and quantizer step
tables of a float scheme in float64.  The device is held to the transforms bit for bit."""
import numpy as np

import lifting_model as lm

N1D_MAX = 8192  # the longest line whose every level runs in one launch
QUANT_MAX_LEVELS = 16
f64 = np.float64


def levels1d(size, j, inverse=False):
    """the level count of a call: forward, a j outside 0 .. ceil_log2(size) becomes that limit; inverse, a j inside
    0 .. limit - 1 is used as it is and any other stands for the limit"""
    limit = lm.ceil_log2(size)
    if inverse:
        return j if 0 <= j < limit else limit
    return limit if (j < 0 or j > limit) else j


def length(N, k):
    """samples of a line of N at level k"""
    return -(-N >> k)


def fwd1d(s, lines, j=-1):
    """(n_lines, N) lines -> (their 1-D Mallat lines, J)"""
    out = np.array(lines, s.dtype, ndmin=2, copy=True)
    N = out.shape[-1]
    J = levels1d(N, j)
    for k in range(J):
        n = length(N, k)
        r = out[:, :n].copy()
        lm.pass_lines(s, r, False)
        out[:, :(n + 1) // 2], out[:, (n + 1) // 2:n] = r[:, 0::2], r[:, 1::2]
    return out, J


def inv1d(s, coefs, j=-1):
    out = np.array(coefs, s.dtype, ndmin=2, copy=True)
    N = out.shape[-1]
    J = levels1d(N, j, True)
    for k in reversed(range(J)):
        n = length(N, k)
        r = np.empty((out.shape[0], n), s.dtype)
        r[:, 0::2], r[:, 1::2] = out[:, :(n + 1) // 2], out[:, (n + 1) // 2:n]
        lm.pass_lines(s, r, True)
        out[:, :n] = r
    return out, J


# ---- the synthesis norms, float64 ----------------------------------------------------------------------------------------

def _inverse_level64(s, low, high):
    """one inverse level of a float scheme in float64: the binary32 constants widened, coef * (a + b) and ((t0 + t1) + t2) + t3"""
    n = 2 * len(low)
    x = np.empty(n, f64)
    x[0::2], x[1::2] = low * f64(s.inv_scale[0]), high * f64(s.inv_scale[1])
    for st in reversed(s.steps):
        idx = np.arange(st.parity, n, 2)
        total = None
        for c, oa, ob in st.terms:
            a = x[lm.reflect(idx + oa, n)]
            if ob:
                a = a + x[lm.reflect(idx + ob, n)]
            t = f64(np.float32(c)) * a
            total = t if total is None else total + t
        x[idx] = x[idx] - total
    return x


def norms(s, levels):
    """dwt_hip_lifting_norms: (norm_l, norm_h), each `levels` float64 values.  A 1 at the middle L (H) coefficient of level
    j of a line with 2 (R + 2) coefficients a band there, inverted j levels: the span of nonzero samples stays more than R
    away from both ends, so no tap that reflects reads anything but a zero"""
    assert s.type == lm.F32 and 0 <= levels <= QUANT_MAX_LEVELS
    nc = 2 * (s.reach + 2)
    out = np.zeros((2, levels), f64)
    for j in range(1, levels + 1):
        for high in (0, 1):
            low, hi = np.zeros(nc, f64), np.zeros(nc, f64)
            (hi if high else low)[nc // 2] = 1.0
            for _ in range(j):
                low = _inverse_level64(s, low, hi)
                hi = np.zeros(len(low), f64)
            out[high, j - 1] = np.sqrt(np.sum(low * low))
    return out[0], out[1]


def quant_steps(s, levels, base_step):
    """dwt_hip_lifting_quant_steps: the 3 * levels + 1 binary32 steps in the layout of dwt_hip_quant_steps"""
    nl, nh = norms(s, levels)
    base = f64(np.float32(base_step))
    steps = np.empty(3 * levels + 1, np.float32)
    for j in range(levels):
        steps[3 * j:3 * j + 3] = [base / (nh[j] * nl[j]), base / (nl[j] * nh[j]), base / (nh[j] * nh[j])]
    steps[3 * levels] = base / (nl[levels - 1] * nl[levels - 1]) if levels else base
    return steps
