"""GPU checks past the launch-grid caps.  Twelve kernels cap one grid dimension and cover the rest with a
loop, `for (y = blockIdx.y; y < n; y += gridDim.y)` or a slab loop of the same shape; every other GPU test stays below the
caps, so each of those loops runs exactly once there.  Every case here exceeds one cap by a little -- 65835 = 65535 + 300
lines, 16684 = 16384 + 300 rows -- states the cap and its source line, and asserts on its own sizes that the loop takes a
second trip.

Every comparison is bitwise on the uint32 / uint16 image (NaN == NaN where the family's own `same` says so).  Every output
lies in a buffer filled with a canary first: a skipped trip leaves canaries inside the result, a store one cap away from
where it belongs lands on a canary or on another line's data.  Where lines are independent the batch repeats 251 distinct
model lines (tests/gridlimits.py; tests/test_grid_limits_model.py holds the tiling to the full model on the CPU); where
rows interact (2-D transforms, SWT 2-D, EAW) the full model runs."""
import ctypes as C
import functools

import numpy as np
import pytest

import condition_model as cm
import eaw_model as em
import features_model as fm
import gridlimits as gl
import i16_model as im
import nterm_model as nm
import shape_model as shm
import swt2d_model as m2
import swt_model as sm
import timefreq_model as tm
from hipdev import Dev, launches
from test_hip_condition import frame as cond_frame, run as run_condition, same as cond_same
from test_hip_shape import frames as shape_frames, run as run_shape
from test_hip_swt import run_features as run_swt_features, run_swt
from test_hip_swt2d import run_swt2d
from test_hip_timefreq import run_batch as run_timefreq, run_plane_op

pytestmark = pytest.mark.gpu
F32 = np.float32
P = gl.P
LINES = 65535 + 300  # past every cap of 65535 (and of 65536)
ROWS = 16384 + 300   # past every cap of 16384
CANARY = np.uint32(0xDEADBEEF)
CANARY_F = np.array([CANARY], np.uint32).view(F32)[0]
CANARY_16 = np.uint16(0x5AA5)
HUGE = F32(3.0e38)   # the padding of the N-term groups (tests/test_hip_nterm.py)
U = 2.0 ** -24
DEFAULTS = (("swt_fused", 1), ("swt2d_fused", 1), ("cond_fused", -1), ("timefreq_tiled", 1), ("eaw_two_pass", 0))


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    for k, v in DEFAULTS:
        d.set_option(k, v)


class option:
    """`with option(dwt, name, value):` -- the option set, and back at its default whatever happens inside"""

    def __init__(self, dwt, name, value):
        self.dwt, self.name, self.value = dwt, name, value

    def __enter__(self):
        self.dwt.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.dwt.set_option(self.name, dict(DEFAULTS)[self.name])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ---- 1. SWT rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_swt_rows(dwt, wavelet):
    """cap: grid.y <= 65535 lines (launch_swt_level, dwt_swt1d.hip:156): k_swt_level walks lines y, y + 65535"""
    n, levels = 8, 3
    assert gl.trips(LINES, 65535) >= 2
    base = sm.make_input(101, "normal", P, n)
    x = gl.tile(base, LINES)
    L, H = sm.swt_levels(base, wavelet, levels)
    wantL, wantH = gl.tile(L, LINES, axis=1), gl.tile(H, LINES, axis=1)
    for fused, k_want in ((0, levels), (1, 1)):  # one launch per level through global memory; four lines per workgroup
        with option(dwt, "swt_fused", fused):
            gotH, gotL, k = run_swt(dwt, wavelet, x, levels, True, 3, 4, 2)
        assert k == k_want, (fused, k)
        assert sm.same(gotH, wantH) and sm.same(gotL, wantL), fused


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_swt_row_features(dwt, wavelet):
    """the same lines through dwt_hip_swt_features1d_batch (WPS, mean), under both routes.  Line i repeats line i % 251 and
    a line's sums depend on nothing but the line, so the batch equals the tiled result of the first 251 lines alone -- a
    call below every cap -- which is held, as tests/test_hip_swt.py holds it, to dwt_hip_band_feature over the planes the
    coefficient mode stores."""
    n, levels, names = 8, 3, ["wps", "mean"]
    assert gl.trips(LINES, 65535) >= 2
    base = sm.make_input(101, "normal", P, n)
    small, order = run_swt_features(dwt, wavelet, names, base, levels, 0, 2.0, True)
    src, h = Dev(dwt, base), Dev(dwt, np.zeros((levels, P, n), F32))
    dwt.swt1d_batch(wavelet, src.ptr, n * 4, 4, P, n, levels, h.ptr, None, 0, P * n * 4, n * 4)
    v = C.c_float()
    for y in range(P):
        for lev in range(levels):
            for i, name in enumerate(order):
                rc = dwt.lib.dwt_hip_band_feature(fm.NAMES.index(name), h.ptr + ((lev * P + y) * n) * 4, 0, 4, n, 1, lev, 2.0, C.byref(v))
                assert rc == 0, dwt.last_error()
                assert sm.same(small[y, i, lev], F32(v.value)), (name, y, lev)
    src.free()
    h.free()
    x = gl.tile(base, LINES)
    for fused in (1, 0):
        with option(dwt, "swt_fused", fused):
            big, _ = run_swt_features(dwt, wavelet, names, x, levels, 0, 2.0, True)
        assert sm.same(big, gl.tile(small, LINES)), fused


# ---- 2. SWT images ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_swt2d_passes(dwt, wavelet):
    """cap: grid.y <= 65535 of H * batch (pass_grid, dwt_swt2d.hip:153-157): k_swt2d_rows and k_swt2d_cols walk the
    lines q, q + 65535 of 3 images of 22000 rows.  The rows of an image interact: the full model."""
    batch, h, w, levels = 3, 22000, 5, 2
    assert gl.trips(batch * h, 65535) >= 2
    x = np.stack([m2.make_input(201 + b, "normal", h, w) for b in range(batch)])
    LL, D = m2.swt2d_levels(x, wavelet, levels)
    with option(dwt, "swt2d_fused", 0):
        gotD, gotL, k = run_swt2d(dwt, wavelet, x, levels, True, 1, 4, 2)
    assert k == 2 * levels, k
    assert sm.same(gotD, D) and sm.same(gotL, LL)


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_swt2d_fused_declined(dwt, wavelet):
    """cap: the fused kernel takes the batch as grid.z and is refused for batch > 65535 (swt2d_fused_fits,
    dwt_swt2d.hip:174-179): 65536 images take the two passes (2 launches, not 1), whose 131072 lines wrap as well"""
    batch, h, w = 65536, 2, 3
    assert batch > 65535 and gl.trips(batch * h, 65535) >= 2
    base = np.stack([m2.make_input(301 + b, "normal", h, w) for b in range(P)])
    LL, D = m2.swt2d_levels(base, wavelet, 1)  # (1, P, h, w), (1, 3, P, h, w)
    gotD, gotL, k = run_swt2d(dwt, wavelet, gl.tile(base, batch), 1, True, 1, 4, 2)
    assert k == 2, k
    assert sm.same(gotD, gl.tile(D, batch, axis=2)) and sm.same(gotL, gl.tile(LL, batch, axis=1))
    small = run_swt2d(dwt, wavelet, base, 1, True, 1, 4, 2)
    assert small[2] == 1 and sm.same(small[0], D)  # (the same images below the limit: the fused kernel, the same planes)


# ---- 3. conditioning --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cond_rows():
    base = cm.make_input(401, "spectrum", P, 5)
    base.setflags(write=False)
    return base


def test_condition_rows(dwt):
    """cap: grid.y <= 16384 rows (grid2, dwt_condition.hip:338): with cond_fused = 0 k_elem_op subtracts the medians
    (op 2) and scales (op 3, info[4y + 3] included) rows y, y + 16384; cond_fused = 1 is one launch without a cap"""
    assert gl.trips(ROWS, 16384) >= 2
    ops = cm.MED_SHIFT | cm.SCALE
    rows, info = cm.condition(cond_rows(), ops, 20, -1.0, 2.5)
    x = gl.tile(cond_rows(), ROWS)
    for fused in (0, 1):
        with option(dwt, "cond_fused", fused):
            got, got_info, k = run_condition(dwt, x, ops, 20, -1.0, 2.5)
        assert (k == 1) if fused else (k > 1), (fused, k)
        assert cond_same(got, gl.tile(rows, ROWS)), fused
        assert np.array_equal(got_info, gl.tile(info, ROWS)), fused


@pytest.mark.parametrize("zero_fill", [True, False])
def test_condition_displace(dwt, zero_fill):
    """cap: grid.y <= 16384 rows (grid2, dwt_condition.hip:338): k_rows_displace with one displacement per row.  Rows
    repeat with period 251 and displacements with period 5: the expected rows come from a 5 x 251 table"""
    n = 5
    assert gl.trips(ROWS, 16384) >= 2
    i = np.arange(ROWS)
    displ = np.array([cm.displacement(dn, n) for dn in cm.DISPLACEMENTS], np.int32)[i % 5]
    per = np.stack([[cm.displace1(r, cm.displacement(dn, n), zero_fill) for r in cond_rows()] for dn in cm.DISPLACEMENTS])
    buf = cond_frame(gl.tile(cond_rows(), ROWS), 3, 1)
    d, dd = Dev(dwt, buf), Dev(dwt, displ)
    dwt.rows_displace(d.ptr, buf.shape[1] * 4, 4, ROWS, n, dd, zero_fill=zero_fill)
    out = d.get()
    assert np.array_equal(dd.get(), displ)
    d.free()
    dd.free()
    assert np.array_equal(bits(out[:ROWS, :n]), bits(per[i % 5, i % P]))
    assert np.all(bits(out[:ROWS, n:]) == bits(buf[:ROWS, n:])) and np.all(bits(out[ROWS]) == bits(buf[ROWS]))


def test_condition_shift_and_scale(dwt):
    """cap: grid.y <= 16384 rows (grid2, dwt_condition.hip:338): dwt_util_shift_s and dwt_util_scale_s (k_elem_op ops 0
    and 1) on an image of 5 columns and 16684 rows"""
    n = 5
    assert gl.trips(ROWS, 16384) >= 2
    x = gl.tile(cond_rows(), ROWS)
    buf = cond_frame(x, 3, 1)
    d = Dev(dwt, buf)
    dwt.dwt_util_shift_s(d.ptr, n, ROWS, buf.shape[1] * 4, 4, 0.3)
    shifted = d.get()
    dwt.dwt_util_scale_s(d.ptr, n, ROWS, buf.shape[1] * 4, 4, 1.7)
    scaled = d.get()
    d.free()
    want = (x + F32(0.3)).astype(F32)
    assert np.array_equal(bits(shifted[:ROWS, :n]), bits(want))
    assert np.array_equal(bits(scaled[:ROWS, :n]), bits((want * F32(1.7)).astype(F32)))
    for out in (shifted, scaled):
        assert np.all(bits(out[:ROWS, n:]) == bits(buf[:ROWS, n:])) and np.all(bits(out[ROWS]) == bits(buf[ROWS]))


def test_condition_many_rows_without_a_cap(dwt):
    """rows_min_max and rows_center_index index the rows by grid.x, which has no cap here: a guard for many rows"""
    n = 5
    x = gl.tile(cond_rows(), ROWS)
    d = Dev(dwt, x)
    mn, mx = dwt.rows_min_max(d.ptr, n * 4, 4, ROWS, n)
    center = dwt.rows_center_index(d.ptr, n * 4, 4, ROWS, n)
    assert np.array_equal(bits(d.get()), bits(x))
    d.free()
    assert np.array_equal(bits(mn), bits(gl.tile(cond_rows().min(axis=1), ROWS)))
    assert np.array_equal(bits(mx), bits(gl.tile(cond_rows().max(axis=1), ROWS)))
    assert np.array_equal(center, gl.tile(np.array([cm.get_center1(r) for r in cond_rows()], np.int32), ROWS))


# ---- 4. dwt_hip_abs ---------------------------------------------------------------------------------------------------------
def test_abs(dwt):
    """cap: grid.y <= 16384 rows (launch_feat_abs, dwt_features.hip:303): k_feat_abs on 5 columns and 16684 rows; signs
    and both zeros from features_model.make_input, NaNs of either sign that carry their row in the payload"""
    n = 5
    assert gl.trips(ROWS, 16384) >= 2
    x = fm.make_input(501, "normal", n, ROWS)
    ties = fm.make_input(502, "small_ints", n, ROWS)
    x[3::7] = ties[3::7]
    assert np.any(bits(x) == 0x80000000) and np.any(bits(x) == 0)
    y = np.arange(5, ROWS, 11)
    x.view(np.uint32)[y, y % n] = (0x7fc00000 | ((y & 1) << 31) | y).astype(np.uint32)
    buf = np.full((ROWS + 1, n + 3), CANARY_F, F32)
    buf[:ROWS, :n] = x
    d = Dev(dwt, buf)
    dwt.dwt_hip_abs(d.ptr, buf.shape[1] * 4, 4, n, ROWS)
    out = d.get()
    d.free()
    assert np.array_equal(bits(out[:ROWS, :n]), bits(x) & np.uint32(0x7fffffff))
    assert np.all(bits(out[:ROWS, n:]) == CANARY) and np.all(bits(out[ROWS]) == CANARY)


# ---- 5. strided staging -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname", ["cdf97_s", "cdf53_i", "cdf53_i16"])
def test_strided_staging(dwt, oracle, wname):
    """cap: grid.y <= 16384 rows (strided_move_t, dwt_strided.hip:59): k_strided_move packs and spreads one channel of a
    two-channel device image of 4 columns and 16684 rows (elements 8 bytes apart; int16: 4 bytes), forward at 2 levels and
    back through dwt_hip_transform2d.  The other channel and the pitch padding keep their bits."""
    h, w, pad, ch, levels = ROWS, 4, 2, 1, 2
    assert gl.trips(h, 16384) >= 2
    rng = np.random.default_rng(601)
    if wname == "cdf53_i16":
        dt, canary = np.int16, np.array([CANARY_16], np.uint16).view(np.int16)[0]
        pix = rng.integers(-32768, 32768, size=(h, w, 2)).astype(dt)
    elif wname == "cdf53_i":
        dt, canary = np.int32, np.array([CANARY], np.uint32).view(np.int32)[0]
        pix = rng.integers(-(1 << 20), 1 << 20, size=(h, w, 2)).astype(dt)
    else:
        dt, canary = F32, CANARY_F
        pix = rng.standard_normal((h, w, 2)).astype(dt)
    es = np.dtype(dt).itemsize
    buf = np.full((h + 1, w + pad, 2), canary, dt)
    buf[:h, :w] = pix
    want_f = buf.copy()
    if wname == "cdf53_i16":
        a = np.ascontiguousarray(pix[:, :, ch])
        jw = im.fwd2d(a, j_max=levels)
        want_f[:h, :w, ch] = a
        im.inv2d(a, j_max=jw)
        want_i = buf.copy()
        want_i[:h, :w, ch] = a
        assert np.array_equal(a, pix[:, :, ch])
    else:
        ff = {"cdf97_s": "cdf97_2f_s", "cdf53_i": "cdf53_2f_i"}[wname]
        jw = oracle.call_channel(ff, want_f[:h, :w], ch, levels)
        want_i = want_f.copy()
        oracle.call_channel(ff.replace("2f", "2i"), want_i[:h, :w], ch, jw)
    assert jw == levels
    d = Dev(dwt, buf)
    ptr, jj = d.ptr + es * ch, C.c_int(levels)
    wid = dwt.WAVELET_ID[wname]
    rc = dwt.lib.dwt_hip_transform2d(wid, 0, ptr, ptr, buf.strides[0], buf.strides[1], w, h, w, h, C.byref(jj), 0, 0)
    assert rc == 0 and jj.value == jw, dwt.last_error()
    assert np.array_equal(bits(d.get()), bits(want_f)), "forward"
    rc = dwt.lib.dwt_hip_transform2d(wid, 1, ptr, ptr, buf.strides[0], buf.strides[1], w, h, w, h, C.byref(jj), 0, 0)
    assert rc == 0, dwt.last_error()
    assert np.array_equal(bits(d.get()), bits(want_i)), "inverse"
    d.free()


# ---- 6. time-frequency ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", [1, 0], ids=["tiled", "plain"])
def test_timefreq_many_lines(dwt, tiled):
    """cap: grid.y (k_tf_tiled) / grid.z (k_tf_plain) <= 65535 lines (capped, dwt_timefreq.hip:227-250): 65835 lines of
    16 samples against a bank of 3 short kernels, complex output"""
    n = 16
    assert gl.trips(LINES, 65535) >= 2
    rng = np.random.default_rng(701)
    kernels = [(rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64) for s in (3, 5, 2)]
    bank = dwt.timefreq_bank(kernels=kernels, centers=[1, 2, 0])
    sizes, centers, taps = bank.query()
    base = tm.make_input(702, "normal", P, n)
    want = np.stack([np.stack(tm.planes(row, sizes, centers, taps)[:2], axis=-1) for row in base])  # (P, bins, n, 2)
    try:
        with option(dwt, "timefreq_tiled", tiled):
            got, k = run_timefreq(dwt, bank, 3, gl.tile(base, LINES), "complex", True, 1)
    finally:
        bank.free()
    assert k == 1
    assert tm.same(got, gl.tile(want, LINES))


@pytest.mark.parametrize("tiled", [1, 0], ids=["tiled", "plain"])
def test_timefreq_many_bins(dwt, tiled):
    """cap: grid.z (k_tf_tiled) / grid.y (k_tf_plain) <= 65535 bins (capped, dwt_timefreq.hip:227-250): one line of 8
    samples against 65835 kernels of 1 to 3 taps, 251 of them distinct; bin y writes row bins - 1 - y"""
    n, bins = 8, LINES
    assert gl.trips(bins, 65535) >= 2
    rng = np.random.default_rng(711)
    distinct = [(rng.standard_normal(1 + b % 3) + 1j * rng.standard_normal(1 + b % 3)).astype(np.complex64) for b in range(P)]
    centers = [b % len(distinct[b]) for b in range(P)]
    x = tm.make_input(712, "normal", 1, n)
    dots = np.stack([np.stack(tm.cdots(x[0], len(distinct[b]), centers[b], distinct[b]), axis=-1) for b in range(P)])  # (P, n, 2)
    bank = dwt.timefreq_bank(kernels=[distinct[y % P] for y in range(bins)], centers=[centers[y % P] for y in range(bins)])
    try:
        with option(dwt, "timefreq_tiled", tiled):
            got, k = run_timefreq(dwt, bank, bins, x, "complex", True, 1)
    finally:
        bank.free()
    assert k == 1
    assert tm.same(got[0], gl.tile(dots, bins)[::-1])


def plane_operators(dwt, planes):
    """phase_derivative and detect_ridges 1, 2, 3 over the planes (p, rows, n) against the model"""
    limit = tm.LIMIT
    mag = np.abs(planes)
    got, k = run_plane_op(dwt, 0, planes, limit, True, 1)
    assert k == 1 and tm.same(got, tm.phase_derivative(planes, limit)), "phase_derivative"
    got, k = run_plane_op(dwt, 1, mag, 0.25, True, 1)
    assert k == 1 and tm.same(got, tm.ridges1(mag, 0.25)), "detect_ridges 1"
    got, k = run_plane_op(dwt, 2, planes, 0.25, True, 1)
    assert k == 1 and tm.same(got, tm.ridges2(planes, 0.25)), "detect_ridges 2"
    return run_plane_op(dwt, 3, mag, 0.25, True, 1)


def test_timefreq_operators_on_a_tall_plane(dwt):
    """cap: grid.y <= 65535 rows (launch_tf_plane_op, dwt_timefreq.hip:252-259): one plane of 8 columns and 65835 rows.
    detect_ridges 3 reads the rows above and below: the full model"""
    rows, n = LINES, 8
    assert gl.trips(rows, 65535) >= 2
    plane = tm.make_input(721, "normal", rows, n)
    got, k = plane_operators(dwt, plane[None])
    assert k == 1 and tm.same(got[0], tm.ridges3(np.abs(plane), 0.25)), "detect_ridges 3"


def test_timefreq_operators_on_many_planes(dwt):
    """cap: grid.z <= 65535 planes (launch_tf_plane_op, dwt_timefreq.hip:252-259): 65835 planes of 4 rows and 3 columns"""
    rows, n = 4, 3
    assert gl.trips(LINES, 65535) >= 2
    base = tm.make_input(731, "normal", P * rows, n).reshape(P, rows, n)
    got, k = plane_operators(dwt, gl.tile(base, LINES))
    want = np.stack([tm.ridges3(np.abs(p), 0.25) for p in base])
    assert k == 1 and tm.same(got, gl.tile(want, LINES)), "detect_ridges 3"


# ---- 7. band operators ------------------------------------------------------------------------------------------------------
EXACT_OPS = (shm.KEEP, shm.ZERO, shm.SCALE, shm.HARD, shm.SOFT)  # COMPRESS, LOG and EXP are 1-ulp operators


def test_band_operators(dwt):
    """cap: 256 * 64 = 16384 workgroups (launch_band_ops, dwt_bandops.hip:145): 2000 images of 8 x 8 at 3 levels have 10
    slots, none empty, so at least 10 chunks each: k_band_ops walks 20000 chunks or more.  One table per image
    (table_stride), the five exact operators in turn with parameters of the image's own"""
    batch, w, h, J = 2000, 8, 8, 3
    geometry = shm.slots(w, h, w, h, J)
    ns, ts = len(geometry), len(geometry) + 2
    assert ns == 10 and all(sw and sh for _, _, sw, sh in geometry)
    assert gl.trips(batch * ns, 16384) >= 2
    base = np.stack([shm.make_input(801 + t, h, w) for t in range(P)])
    ops = np.array([[EXACT_OPS[(t + k) % 5] for k in range(ns)] for t in range(P)], np.int32)
    params = np.array([[shm.PARAM[o] * (1 + t % 4) for o in row] for t, row in enumerate(ops)], F32)
    want = np.stack([shm.apply_table(base[t], w, h, w, h, J, ops[t], params[t]) for t in range(P)])
    tab_o, tab_p = np.full((batch, ts), 77, np.int32), np.full((batch, ts), np.nan, F32)  # (behind a table: never read)
    tab_o[:, :ns], tab_p[:, :ns] = gl.tile(ops, batch), gl.tile(params, batch)
    xs = list(gl.tile(base, batch))
    got, k = run_shape(dwt, lambda p, bs, sx, sy: dwt.bands_apply_batch(p, bs, batch, sx, w, h, J, tab_o, tab_p, ts), xs)
    assert k == 1
    assert shm.same(np.stack(got), gl.tile(want, batch))


def test_band_threshold(dwt):
    """dwt_hip_universal_threshold_batch on the same 2000 images (their HH(1) bands free of NaN): one threshold per
    image, the images only read"""
    batch, w, h = 2000, 8, 8
    base = np.stack([shm.threshold_input(shm.make_input(801 + t, h, w), w, h) for t in range(P)])
    want = np.array([shm.threshold(x, w, h) for x in base], F32)
    buf, _ = shape_frames(list(gl.tile(base, batch)), 1)
    d = Dev(dwt, buf)
    lam = dwt.universal_threshold_batch(d.ptr, buf.strides[0], batch, buf.strides[1], w, h, np.full(batch, CANARY_F, F32))
    assert np.array_equal(bits(d.get()), bits(buf))
    d.free()
    assert np.array_equal(bits(lam), bits(gl.tile(want, batch)))


# ---- 8. N-term --------------------------------------------------------------------------------------------------------------
NT_GROUPS, NT_W, NT_H, NT_PAD = 683, 16384, 4, 4


@functools.lru_cache(maxsize=None)
def nterm_groups():
    """683 distinct groups of one channel, (683, 4, 16384), laid into a buffer of 3e38 with 4 words behind every row and
    one row behind every group -> (groups, buffer, mask of the groups' words)"""
    x = np.stack([nm.make_input(seed, "normal", 1, NT_H, NT_W)[0] for seed in range(NT_GROUPS)])
    buf = np.full((NT_GROUPS, NT_H + 1, NT_W + NT_PAD), HUGE, F32)
    buf[:, :NT_H, :NT_W] = x
    mask = np.zeros(buf.shape, bool)
    mask[:, :NT_H, :NT_W] = True
    for a in (x, buf, mask):
        a.setflags(write=False)
    return x, buf, mask


def nterm_walk():
    """the geometry of fill_walk (dwt_backend_nterm.hip:59-62) for these sizes -> (slab_rows, slabs, bpg)"""
    slab_rows = max(1, 16384 // NT_W)
    slabs = -(-NT_H // slab_rows)
    return slab_rows, slabs, max(1, min(slabs, -(-2048 // NT_GROUPS)))


def test_nterm_keep_largest(dwt):
    """cap: bpg = min(slabs, ceil(2048 / batch)) workgroups per group, slabs of 16384 elements
    (dwt_backend_nterm.hip:59-62, dwt_nterm.hip:142): 683 groups of 4 rows of 16384 give slab_rows 1, slabs 4, bpg 3, so
    workgroup 0 of every group walks slabs 0 and 3 in the histogram passes and in the apply pass.  Every group distinct;
    thresholds, kept counts and coefficients exact; the buffer takes 224 MB"""
    slab_rows, slabs, bpg = nterm_walk()
    assert (slab_rows, slabs, bpg) == (1, 4, 3) and gl.trips(slabs, bpg) >= 2
    x, buf, mask = nterm_groups()
    M = NT_W * NT_H
    keep = np.array([(1, M // 10, M // 2, M - 1, M, 0)[g % 6] for g in range(NT_GROUPS)], np.int32)
    d = Dev(dwt, buf)
    bs, sx = buf.strides[0], buf.strides[1]
    thr, kept = dwt.keep_largest_batch(d.ptr, bs, NT_GROUPS, 1, bs, sx, NT_W, NT_H, keep)
    out = d.get()
    d.free()
    assert np.array_equal(bits(out)[~mask], bits(buf)[~mask]), "a word outside the groups was written"
    for g in range(NT_GROUPS):
        want, wthr, wkept = nm.keep_largest(x[g][None], int(keep[g]))
        assert bits(thr[g:g + 1])[0] == bits(wthr) and kept[g] == wkept, (g, keep[g], thr[g], wthr, kept[g], wkept)
        assert np.array_equal(bits(out[g, :NT_H, :NT_W]), bits(want[0])), (g, keep[g])


def test_nterm_magnitude(dwt):
    """the same groups through dwt_hip_magnitude_batch, whose workgroups walk the slabs the same way"""
    slab_rows, slabs, bpg = nterm_walk()
    assert gl.trips(slabs, bpg) >= 2
    x, buf, mask = nterm_groups()
    d, m = Dev(dwt, buf), Dev(dwt, np.full(buf.shape, HUGE, F32))
    bs, sx = buf.strides[0], buf.strides[1]
    k = launches(dwt, lambda: dwt.magnitude_batch(d.ptr, bs, NT_GROUPS, 1, bs, sx, NT_W, NT_H, m.ptr, bs, sx))
    got = m.get()
    assert np.array_equal(bits(d.get()), bits(buf)), "the source changed"
    d.free()
    m.free()
    assert k == 1
    assert np.all(bits(got)[~mask] == bits(HUGE)), "a word outside the maps was written"
    assert np.array_equal(bits(got[:, :NT_H, :NT_W]), bits(np.abs(x)))


# ---- 9. EAW line route ------------------------------------------------------------------------------------------------------
def test_eaw_line_route(dwt):
    """cap: 65536 workgroups of 256 threads (eaw_grid, dwt_eaw.hip:56-60): with eaw_two_pass = 1 one level of a
    4352 x 8192 image gives k_eaw_line 4096 pairs x 4352 rows and 2176 pairs x 8192 columns, 17.8 M threads' worth each,
    and k_eaw_place twice that, against 16 777 216 threads.  Forward against the model, coefficients and both weight
    planes; the inverse against the tile route (no cap; held to the model at small sizes by tests/test_hip_eaw.py)"""
    h, w, pad = 4352, 8192, 4
    assert gl.trips(((w + 1) // 2) * h, 65536 * 256) >= 2 and gl.trips(((h + 1) // 2) * w, 65536 * 256) >= 2
    x = sm.make_input(901, "normal", h, w)
    buf = np.full((h + 1, w + pad), CANARY_F, F32)
    buf[:h, :w] = x
    pitch = buf.strides[0]

    def padding_kept(out):
        return np.all(bits(out[:h, w:]) == CANARY) and np.all(bits(out[h]) == CANARY)

    d = Dev(dwt, buf)
    with option(dwt, "eaw_two_pass", 1):
        j, wH, wV = dwt.dwt_eaw53_2f_s(d.ptr, pitch, 4, w, h, w, h, 1, 0, 0, alpha=1.0)
    fwd = d.get()
    want = x.copy()
    jw, want_wH, want_wV = em.mallat_fwd(want, j_max=1, alpha=1.0)
    assert j == jw == 1 and padding_kept(fwd)
    assert np.array_equal(bits(fwd[:h, :w]), bits(want)), "coefficients"
    assert em.same_weights(wH[0], want_wH[0]) and em.same_weights(wV[0], want_wV[0]), "weights"
    del want, want_wH, want_wV
    back = []
    for two_pass in (1, 0):
        assert dwt.lib.dwt_hip_memcpy_h2d(d.ptr, fwd.ctypes.data, fwd.nbytes) == 0
        with option(dwt, "eaw_two_pass", two_pass):
            dwt.dwt_eaw53_2i_s(d.ptr, pitch, 4, w, h, w, h, 1, 0, 0, wH, wV)
        back.append(d.get())
        assert padding_kept(back[-1]), two_pass
    d.free()
    assert np.array_equal(bits(back[0]), bits(back[1])), "inverse: line route against tile route"


# ---- 10. the batch limit of the 2-D entries ---------------------------------------------------------------------------------
def batch_of_tiny_images(wname, oracle, batch):
    """`batch` images of 2 x 2 repeating 251 distinct ones, in a canary-filled buffer (rows of 4 elements, images 12
    elements apart) -> (source buffer, expected forward buffer, expected inverse buffer, levels)"""
    rng = np.random.default_rng(1001)
    if wname == "cdf53_i16":
        dt, canary = np.int16, np.array([CANARY_16], np.uint16).view(np.int16)[0]
        base = rng.integers(-32768, 32768, size=(P, 2, 2)).astype(dt)
    elif wname == "cdf53_i":
        dt, canary = np.int32, np.array([CANARY], np.uint32).view(np.int32)[0]
        base = rng.integers(-(1 << 20), 1 << 20, size=(P, 2, 2)).astype(dt)
    else:
        dt, canary = F32, CANARY_F
        base = rng.standard_normal((P, 2, 2)).astype(dt)
    fwd, inv = base.copy(), base.copy()
    for t in range(P):
        if wname == "cdf53_i16":
            jw = im.fwd2d(fwd[t], j_max=-1)
            inv[t] = fwd[t]
            im.inv2d(inv[t], j_max=jw)
        else:
            ff = {"cdf97_s": "cdf97_2f_s", "cdf53_i": "cdf53_2f_i"}[wname]
            jw = oracle.fwd(ff, fwd[t], -1)
            inv[t] = fwd[t]
            oracle.inv(ff.replace("2f", "2i"), inv[t], jw)
    assert jw == 1

    def lay(images):
        buf = np.full((batch, 3, 4), canary, dt)
        buf[:, :2, :2] = gl.tile(images, batch)
        return buf

    return lay(base), lay(fwd), lay(inv), jw


@pytest.mark.parametrize("wname", ["cdf97_s", "cdf53_i", "cdf53_i16"])
def test_batch_limit_of_the_2d_entries(dwt, oracle, wname):
    """cap: batch 1 .. 65535, the grid.y of the sweeps (dwt_hip_transform2d_batch, dwt_abi.hip:462; dwt_tuning.hip:308):
    65535 images of 2 x 2 forward and back -- the last block row of the largest grid -- and 65536 refused with a message,
    source and destination untouched"""
    batch = 65535
    src, want_f, want_i, jw = batch_of_tiny_images(wname, oracle, batch + 1)
    bs, sx = src.strides[0], src.strides[1]
    blank = np.full(src.shape, src[0, 2, 0], src.dtype)
    a, b, c = Dev(dwt, src), Dev(dwt, blank), Dev(dwt, blank)
    # the refusal first: 65536 images
    assert batch + 1 > 65535
    with pytest.raises(dwt.DwtError, match="batch must be 1..65535"):
        dwt.transform2d_batch(wname, 0, a.ptr, b.ptr, bs, batch + 1, sx, 2, 2, -1)
    assert np.array_equal(bits(a.get()), bits(src)) and np.array_equal(bits(b.get()), bits(blank))
    # the limit itself: image 65535 of the buffers stays as it is
    assert dwt.transform2d_batch(wname, 0, a.ptr, b.ptr, bs, batch, sx, 2, 2, -1) == jw
    got = b.get()
    assert np.array_equal(bits(a.get()), bits(src)), "the source changed"
    assert np.array_equal(bits(got[:batch]), bits(want_f[:batch])) and np.array_equal(bits(got[batch]), bits(blank[batch]))
    assert dwt.transform2d_batch(wname, 1, b.ptr, c.ptr, bs, batch, sx, 2, 2, jw) == jw
    back = c.get()
    assert np.array_equal(bits(b.get()), bits(got)), "the source of the inverse changed"
    assert np.array_equal(bits(back[:batch]), bits(want_i[:batch])) and np.array_equal(bits(back[batch]), bits(blank[batch]))
    for dv in (a, b, c):
        dv.free()


# ---- 11. many lines without a cap -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wv", ["cdf97", "cdf53"])
def test_many_lines_without_a_cap(dwt, oracle, wv):
    """transform1d_batch and features1d_batch index the lines by grid.x, which has no cap here: a guard for 70000 lines of
    16 samples at 2 levels, forward, features of the forward result, inverse.  Medians exact against the model; the sums
    of the first 251 lines within the derived bound of the float64 model (tests/test_hip_features.py) and their features
    the host's finish of the device's own sums; the batch the tiled result of those 251 lines, bit for bit"""
    lines, n, J, pad = 70000, 16, 2, 4
    assert lines > 65536
    wavelet = wv + "_s"
    base = sm.make_input(1101, "normal", P, n)
    fwd, jw = gl.oned(oracle, wv, 0, base, J)
    inv, _ = gl.oned(oracle, wv, 1, fwd, J)
    src = np.full((lines + 1, n + pad), CANARY_F, F32)
    src[:lines, :n] = gl.tile(base, lines)
    blank = np.full(src.shape, CANARY_F, F32)
    a, b, c = Dev(dwt, src), Dev(dwt, blank), Dev(dwt, blank)
    ls = src.strides[0]

    def check(got, want):
        assert np.array_equal(bits(got[:lines, :n]), bits(gl.tile(want, lines)))
        assert np.all(bits(got[:lines, n:]) == CANARY) and np.all(bits(got[lines]) == CANARY)

    assert dwt.transform1d_batch(wavelet, 0, a.ptr, b.ptr, ls, lines, n, J) == jw == J
    assert np.array_equal(bits(a.get()), bits(src)), "the source changed"
    check(b.get(), fwd)
    # features of the forward result: one band, H of level 1
    names = ["wps", "mean", "med"]
    (band,) = fm.bands(n, 1, n, 1, J)
    stride = len(names) + 2
    fv_small, fv_big = Dev(dwt, np.full((P, stride), np.nan, F32)), Dev(dwt, np.full((lines, stride), np.nan, F32))
    dwt.features1d_batch(names, b.ptr, ls, 4, P, n, J, fv_small.ptr, stride)
    raw = {q: dwt.features_raw_sums(i, P) for i, q in ((0, "S1"), (1, "S2"))}
    small = fv_small.get()
    dwt.features1d_batch(names, b.ptr, ls, 4, lines, n, J, fv_big.ptr, stride)
    big = fv_big.get()
    check(b.get(), fwd)  # the features only read
    assert np.isnan(small[:, len(names):]).all() and np.isnan(big[:, len(names):]).all()
    for y in range(P):
        v = fm.band_values(fwd[y][None], band)
        m = fm.model64_band(v, 2.0)
        for q in ("S1", "S2"):
            s, t, cnt = m[q]
            assert abs(raw[q][y] - s) <= U * abs(s) + cnt * 2.0 ** -53 * t, (q, y, raw[q][y], s)
        sums = {q: F32(raw[q][y]) for q in ("S1", "S2")}
        assert sm.same(small[y, 0], fm.finish("wps", sums, len(v), band[4], 2.0)), y
        assert sm.same(small[y, 1], fm.finish("mean", sums, len(v), band[4], 2.0)), y
        assert small[y, 2] == fm.order_stats(v)["med"], y
    assert np.array_equal(bits(big[:, :len(names)]), bits(gl.tile(small[:, :len(names)], lines)))
    # back
    assert dwt.transform1d_batch(wavelet, 1, b.ptr, c.ptr, ls, lines, n, J) == J
    check(c.get(), inv)
    for dv in (a, b, c, fv_small, fv_big):
        dv.free()
