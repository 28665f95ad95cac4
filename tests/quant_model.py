"""numpy restatement of the deadzone quantizer that include/libdwt_hip.h specifies: quantize, dequantize,
the band counters, the synthesis norms, the step tables, the code-block layout and its bit-plane map.  float32 and int64
arithmetic with the roundings where the header puts them; the device code is held to these bits.  A plain module like
pixels_model.py: it imports nothing of the package."""
import numpy as np

F = np.float32
S, H = 0, 1  # coefficient types
I16, I32 = 0, 1  # index types
COEF_DTYPE = {S: np.dtype(np.float32), H: np.dtype(np.float16)}
INDEX_DTYPE = {I16: np.dtype(np.int16), I32: np.dtype(np.int32)}
LIMIT = {I16: F(32768.0), I32: F(2147483648.0)}
TOP = {I16: 32767, I32: 2147483647}
CDF97, CDF53, INTERP53 = "cdf97", "cdf53", "interp53"


# ---- geometry: the slots of dwt_hip_bands_apply_batch (dwt_util_subband_s over a dense frame) -----------------------
def ceil_log2(x):
    n = 0
    while n < 31 and (1 << n) < x:
        n += 1
    return n


def levels(size_x, size_y, j_max):
    lo, hi = min(size_x, size_y), max(size_x, size_y)
    if j_max < 0:
        return ceil_log2(hi if lo <= 1 else lo)
    return min(j_max, ceil_log2(hi))


def cdiv(i, j):
    return (i + (1 << j) - 1) >> j


def geometry(size_x, size_y, j_max):
    """(slots, 4) of x, y, w, h: HL, LH, HH of level 1 .. J, then LL(J)"""
    J = levels(size_x, size_y, j_max)
    out = []
    for j in range(1, J + 1):
        hx, hy = cdiv(size_x, j - 1) // 2, cdiv(size_y, j - 1) // 2
        lx, ly = cdiv(size_x, j), cdiv(size_y, j)
        out += [(lx, 0, hx, ly), (0, ly, lx, hy), (lx, ly, hx, hy)]
    out.append((0, 0, cdiv(size_x, J), cdiv(size_y, J)))
    return np.array(out, np.int64)


def slot_map(size_x, size_y, j_max):
    """(size_y, size_x) of the slot every position belongs to, painted from the rectangles; every position is painted once"""
    m = np.full((size_y, size_x), -1, np.int64)
    for k, (x, y, w, h) in enumerate(geometry(size_x, size_y, j_max)):
        assert (m[y:y + h, x:x + w] == -1).all()
        m[y:y + h, x:x + w] = k
    assert (m >= 0).all()
    return m


def per_sample(table, smap, batch):
    """table (slots,) or (batch, slots) -> (batch, size_y, size_x) of every position's entry"""
    t = np.asarray(table, F)
    if t.ndim == 1:
        t = np.broadcast_to(t, (batch,) + t.shape)
    return t[:, smap]


# ---- the arithmetic -------------------------------------------------------------------------------------------------
def quantize(coef, step, index_type):
    """coef: float32 / float16 array; step: float32, broadcast against it -> (index array, clipped mask)"""
    with np.errstate(all="ignore"):
        c = np.asarray(coef).astype(F)  # (binary16 widens exactly)
        inv = F(1.0) / np.asarray(step, F)  # an IEEE binary32 division
        m = (np.abs(c) * inv).astype(F)  # one rounded product
        nan = np.isnan(m)
        sat = m >= LIMIT[index_type]
        k = np.where(nan | sat, 0, m).astype(np.int64)  # truncation
        k = np.where(sat, TOP[index_type], k)
        q = np.where(np.signbit(c), -k, k)
    return q.astype(INDEX_DTYPE[index_type]), nan | sat


def dequantize(q, step, r, coef_type):
    """q: int16 / int32 array; step float32, broadcast; r float -> coefficient array"""
    with np.errstate(all="ignore"):
        q64 = np.asarray(q).astype(np.int64)
        a = np.abs(q64).astype(F)  # (2^31 is a float)
        v = ((a + F(r)).astype(F) * np.asarray(step, F)).astype(F)  # two roundings
        v = np.where(q64 < 0, -v, v)
        v = np.where(q64 == 0, F(0.0), v).astype(F)
        return v.astype(COEF_DTYPE[coef_type])  # binary16: one more rounding, to nearest even


def quantize_frames(coef, steps, j_max, index_type):
    """coef (batch, size_y, size_x); steps (slots,) or (batch, slots) -> (indices, stats (batch, slots, 3) int64)"""
    B, Hh, W = coef.shape
    smap = slot_map(W, Hh, j_max)
    ns = 3 * levels(W, Hh, j_max) + 1
    q, clipped = quantize(coef, per_sample(steps, smap, B), index_type)
    stats = np.zeros((B, ns, 3), np.int64)
    mag = np.abs(q.astype(np.int64))
    for b in range(B):
        for k in range(ns):
            sel = smap == k
            if sel.any():
                stats[b, k] = ((mag[b][sel] != 0).sum(), mag[b][sel].max(), clipped[b][sel].sum())
    return q, stats


def dequantize_frames(q, steps, j_max, r, coef_type):
    B, Hh, W = q.shape
    return dequantize(q, per_sample(steps, slot_map(W, Hh, j_max), B), r, coef_type)


def bit_length(v):
    v = np.asarray(v, np.int64)
    out = np.zeros(v.shape, np.int64)
    for b in range(33):
        out = np.where(v >> b, b + 1, out)
    return out


# ---- synthesis norms and steps --------------------------------------------------------------------------------------
def lifting(wavelet):
    """(inverse steps as (parity, coefficient), scaling of the even / L samples, of the odd / H samples): the binary32
    constants of the float kernels, widened"""
    if wavelet == CDF97:
        zeta = F(1.1496043988602)
        return [(0, F(-0.4435068520439)), (1, F(-0.8829110755309)), (0, F(0.0529801185729)), (1, F(1.58613434342059))], F(1.0) / zeta, zeta
    if wavelet == CDF53:
        return [(0, F(-0.25)), (1, F(0.5))], F(0.70710678118654752440), F(1.41421356237309504880)
    if wavelet == INTERP53:
        return [(1, F(0.5))], F(0.70710678118654752440), F(1.41421356237309504880)
    raise ValueError(wavelet)


def inverse_level(wavelet, lo, hi):
    steps, even, odd = lifting(wavelet)
    n = 2 * len(lo)
    x = np.zeros(n, np.float64)
    x[0::2] = lo * np.float64(even)
    x[1::2] = hi * np.float64(odd)
    for parity, c in steps:
        idx = np.arange(parity, n, 2)
        left = np.where(idx == 0, 1, idx - 1)
        right = np.where(idx == n - 1, n - 2, idx + 1)
        x[idx] += np.float64(c) * (x[left] + x[right])
    return x


def synthesis_norm(wavelet, j, high):
    lo, hi = np.zeros(64), np.zeros(64)
    (hi if high else lo)[32] = 1.0
    for _ in range(j):
        lo = inverse_level(wavelet, lo, hi)
        hi = np.zeros(len(lo))
    return float(np.sqrt(np.sum(lo * lo)))


def norms(wavelet, n_levels):
    return (np.array([synthesis_norm(wavelet, j, False) for j in range(1, n_levels + 1)]),
            np.array([synthesis_norm(wavelet, j, True) for j in range(1, n_levels + 1)]))


def steps(wavelet, n_levels, base_step):
    nl, nh = norms(wavelet, n_levels)
    base = np.float64(F(base_step))
    out = []
    for j in range(n_levels):
        out += [base / (nh[j] * nl[j]), base / (nl[j] * nh[j]), base / (nh[j] * nh[j])]
    last = nl[n_levels - 1] if n_levels else 1.0
    out.append(base / (last * last))
    return np.array(out, np.float64).astype(F)


# ---- code-blocks ----------------------------------------------------------------------------------------------------
def codeblock_layout(size_x, size_y, j_max, cbx, cby):
    """(first (slots + 1), blocks_x (slots)) from the rectangles"""
    first, blocks_x, total = [], [], 0
    for x, y, w, h in geometry(size_x, size_y, j_max):
        nx = -(-w // (1 << cbx)) if w > 0 and h > 0 else 0
        ny = -(-h // (1 << cby)) if nx else 0
        first.append(total)
        blocks_x.append(nx)
        total += nx * ny
    return np.array(first + [total], np.int64), np.array(blocks_x, np.int64)


def codeblock_bitplanes(q, j_max, cbx, cby):
    """q (batch, size_y, size_x) -> uint8 (batch, total)"""
    B, Hh, W = q.shape
    first, blocks_x = codeblock_layout(W, Hh, j_max, cbx, cby)
    out = np.zeros((B, first[-1]), np.uint8)
    mag = np.abs(q.astype(np.int64))
    for k, (x, y, w, h) in enumerate(geometry(W, Hh, j_max)):
        nx, n = int(blocks_x[k]), int(first[k + 1] - first[k])
        if n == 0:
            continue
        ny = n // nx
        band = np.zeros((B, ny << cby, nx << cbx), np.int64)  # partial blocks padded with zeros
        band[:, :h, :w] = mag[:, y:y + h, x:x + w]
        top = band.reshape(B, ny, 1 << cby, nx, 1 << cbx).max(axis=(2, 4))
        out[:, first[k]:first[k + 1]] = bit_length(top).reshape(B, n)
    return out
