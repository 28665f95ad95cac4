"""GPU checks of the row conditioning (dwt_hip_rows_condition and its primitives, the dwt_util_* mirrors) against the
numpy model of tests/condition_model.py and the reference-generated fixtures of tests/golden/condition.npz, which
tests/test_condition.py pins to each other.  Every comparison is bit for bit, zeros by value (which of +0 / -0 a median of
zeros is, is unspecified); every word around the rows must come back untouched."""
import numpy as np
import pytest

import condition_model as cm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
CANARY = F32(-7.5)
FUSED_SIZES = [n for n in cm.SIZES if n <= 8192]


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("cond_fused", -1)


def same(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))))


def all_kinds(n, rows_per_kind=1):
    """one batch with rows of every kind (and, at 64 samples, the row whose centring reverses)"""
    rows = [cm.make_input(1000 + 17 * k + n, kind, rows_per_kind, n) for k, kind in enumerate(cm.KINDS)]
    if n == 64:
        rows.append(cm.reversing_row()[None, :])
    return np.concatenate(rows)


def batch_of(n_lines, n):
    x = all_kinds(n, 1)
    return np.concatenate([x] * (n_lines // len(x) + 1))[:n_lines].copy()


def frame(x, pad, step):
    """x laid out with `pad` canary elements after each row and elements `step` floats apart -> the buffer, one canary row after the batch"""
    n_lines, n = x.shape
    buf = np.full((n_lines + 1, (n + pad) * step), CANARY, F32)
    buf[:n_lines, :n * step:step] = x
    return buf


def run(dwt, x, ops, max_iters=20, lo=0.0, hi=1.0, device=True, pad=3, step=1, want_info=True):
    """-> (rows, info, launches); the padding, the gaps between strided elements and the row after the batch untouched"""
    n_lines, n = x.shape
    buf = frame(x, pad, step)
    ls = buf.shape[1] * 4
    info = np.full((n_lines, 4), -99, np.int32)
    if device:
        d, di = Dev(dwt, buf), Dev(dwt, info)
        k = launches(dwt, lambda: dwt.rows_condition(ops, d.ptr, ls, 4 * step, n_lines, n, max_iters, lo, hi, di.ptr if want_info else None))
        out, info = d.get(), di.get()
        d.free()
        di.free()
    else:
        out = buf.copy()
        k = launches(dwt, lambda: dwt.rows_condition(ops, out, ls, 4 * step, n_lines, n, max_iters, lo, hi, info if want_info else None))
    mask = np.zeros(buf.shape, bool)
    mask[:n_lines, :n * step:step] = True
    assert np.all(out[~mask] == CANARY), "a word outside the rows was written"
    return out[:n_lines, :n * step:step], info, k


def check(dwt, x, ops, max_iters=20, lo=0.0, hi=1.0, fused_launch=True, **kw):
    want, winfo = cm.condition(x, ops, max_iters, lo, hi)
    got, info, k = run(dwt, x, ops, max_iters, lo, hi, **kw)
    assert same(got, want), "rows differ in %d of %d rows" % (np.sum(np.any(got != want, axis=1)), len(x))
    assert np.array_equal(info, winfo)
    if fused_launch:
        assert k == 1
    return got, info


# ---- the fused route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FUSED_SIZES)
def test_fused_every_kind_every_op(dwt, n):
    x = all_kinds(n, 2)
    for ops in (1, 2, 4, 3, 5, 6, 7):
        check(dwt, x, ops, 20, -1.0, 2.5)
    for iters in (0, 1):
        check(dwt, x, 7, iters)
        check(dwt, x, 2, iters)


@pytest.mark.parametrize("n", FUSED_SIZES)
@pytest.mark.parametrize("n_lines", [1, 3, 67])
def test_fused_batches(dwt, n_lines, n):
    """67 rows: more than one workgroup at every size, never a multiple of the rows a workgroup takes"""
    x = batch_of(n_lines, n)
    check(dwt, x, 7, 20, 0.0, 1.0)
    if n_lines == 67:
        check(dwt, x, 3, 20, pad=5)  # rows not 16-byte aligned: the scalar load / store path


def test_fused_without_info_and_aligned_rows(dwt):
    x = batch_of(67, 1000)
    want, _ = cm.condition(x, 7, 20)
    got, info, k = run(dwt, x, 7, 20, pad=4, want_info=False)  # (16-byte aligned rows: the vector path)
    assert same(got, want) and np.all(info == -99) and k == 1


def golden_cases(max_n=None, min_n=0):
    return [i for i, c in enumerate(cm.CASES) if min_n <= c[3] and (max_n is None or c[3] <= max_n)]


@pytest.mark.parametrize("i", golden_cases(8192), ids=lambda i: "%s-%dx%d" % cm.CASES[i][1:])
def test_fused_matches_reference_fixtures(dwt, i):
    seed, kind, n_lines, n = cm.CASES[i]
    g = cm.golden()
    x = cm.make_input(seed, kind, n_lines, n)
    got, _, k = run(dwt, x, 1)
    assert same(got, g["shift_%d" % i]) and k == 1
    got, info, k = run(dwt, x, 3, 20)
    assert same(got, g["centered_%d" % i]) and np.array_equal(info, g["info_%d" % i]) and k == 1
    got, _, k = run(dwt, x, 7, 20, 0.0, 1.0)
    assert same(got, g["scaled_%d" % i]) and k == 1


# ---- fused against per-operation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 64, 255, 4096])
def test_fused_equals_per_operation(dwt, n):
    x = batch_of(67 if n < 4096 else 11, n)
    for ops, iters in ((7, 20), (3, 20), (2, 1), (5, 0), (4, 0)):
        a, ia, ka = run(dwt, x, ops, iters, -3.0, 0.5)
        wa = dwt.rows_warnings()
        dwt.set_option("cond_fused", 0)
        try:
            b, ib, kb = run(dwt, x, ops, iters, -3.0, 0.5)
            wb = dwt.rows_warnings()
        finally:
            dwt.set_option("cond_fused", -1)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ia, ib)
        assert ka == 1 and kb > 1
        assert wa == wb == cm.center_warnings(x, ops, iters)


def test_route_follows_the_batch_size(dwt):
    """left to itself the library conditions a batch that one round of workgroups holds in one launch, a larger one
    kernel by kernel (from there on every row in flight beats what the LDS of the CUs holds); option
    "cond_fused" = 1 keeps one launch for any batch.  Same bits either way."""
    n = 8192
    per_round = 256 * (152 * 1024 // (4 * (n + 4)))  # 256 CUs x the rows of a workgroup
    x = batch_of(per_round + 1, n)
    a, ia, ka = run(dwt, x, 3, 2)
    b, ib, kb = run(dwt, x[:per_round], 3, 2)
    dwt.set_option("cond_fused", 1)
    try:
        c, ic, kc = run(dwt, x, 3, 2)
    finally:
        dwt.set_option("cond_fused", -1)
    assert ka > 1 and kb == 1 and kc == 1
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(ia, ic)
    assert np.array_equal(a[:per_round].view(np.uint32), b.view(np.uint32))


def test_displace_takes_numpy_integers(dwt):
    x = batch_of(3, 65)
    d = Dev(dwt, x)
    dwt.rows_displace(d.ptr, 260, 4, 3, 65, np.int32(-7))
    dwt.rows_displace(d.ptr, 260, 4, 3, 65, np.int64(2), zero_fill=False)
    want = np.stack([cm.displace1(cm.displace1(r, -7, True), 2, False) for r in x])
    assert np.array_equal(d.get().view(np.uint32), want.view(np.uint32))


def test_center_index_counts_the_warnings(dwt):
    x = all_kinds(255, 2)
    d = Dev(dwt, x)
    dwt.rows_center_index(d.ptr, 4 * 255, 4, len(x), 255)
    warns = [cm.get_center1_warn(r)[1] for r in x]
    assert dwt.rows_warnings() == (warns.count(cm.WARN_NORM), warns.count(cm.WARN_INDEX)) and warns.count(cm.WARN_NORM) >= 2


# ---- the other routes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", golden_cases(min_n=8193), ids=lambda i: "%s-%dx%d" % cm.CASES[i][1:])
def test_long_rows_match_reference_fixtures(dwt, i):
    seed, kind, n_lines, n = cm.CASES[i]
    g = cm.golden()
    x = cm.make_input(seed, kind, n_lines, n)
    got, info, k = run(dwt, x, 3, 20)
    assert same(got, g["centered_%d" % i]) and np.array_equal(info, g["info_%d" % i]) and k > 1
    got, _, _ = run(dwt, x, 7, 20, 0.0, 1.0)
    assert same(got, g["scaled_%d" % i])


@pytest.mark.parametrize("n", [8193, 10000])
def test_long_rows_every_kind(dwt, n):
    check(dwt, all_kinds(n), 7, 20, fused_launch=False)


@pytest.mark.parametrize("n", [5, 255, 4096])
def test_strided_elements_and_host_pointers(dwt, n):
    x = batch_of(9, n)
    check(dwt, x, 7, 20, step=2, fused_launch=False)  # elem_stride 8, device
    check(dwt, x, 7, 20, device=False, fused_launch=False)
    check(dwt, x, 3, 20, device=False, step=2, fused_launch=False)


def test_host_rows_at_a_prime_byte_pitch(dwt):
    n, n_lines, pitch = 255, 7, 1021
    x = batch_of(n_lines, n)
    raw = np.full(pitch * n_lines + 8, 0xA5, np.uint8)
    view = np.ndarray((n_lines, n), F32, buffer=raw, strides=(pitch, 4))
    view[...] = x
    info = np.zeros((n_lines, 4), np.int32)
    dwt.rows_condition(7, raw.ctypes.data, pitch, 4, n_lines, n, 20, 0.0, 1.0, info)
    want, winfo = cm.condition(x, 7, 20)
    assert same(np.ascontiguousarray(view), want) and np.array_equal(info, winfo)
    gaps = np.ones(raw.shape, bool)
    for y in range(n_lines):
        gaps[y * pitch:y * pitch + 4 * n] = False
    assert np.all(raw[gaps] == 0xA5)


# ---- primitives -----------------------------------------------------------------------------------------------------------
def test_center_index_matches_reference_fixtures(dwt):
    g = cm.golden()
    for i, (seed, kind, n_lines, n) in enumerate(cm.CASES):
        x = cm.make_input(seed, kind, n_lines, n)
        d = Dev(dwt, x)
        assert np.array_equal(dwt.rows_center_index(d.ptr, 4 * n, 4, n_lines, n), g["center_%d" % i]), cm.CASES[i]
        d.free()
    x = all_kinds(255)
    assert np.array_equal(dwt.rows_center_index(x, 4 * 255, 4, len(x), 255), [cm.get_center1(r) for r in x])  # host rows
    dc = Dev(dwt, np.zeros(len(x), np.int32))  # device result
    d = Dev(dwt, x)
    dwt.rows_center_index(d.ptr, 4 * 255, 4, len(x), 255, dc.ptr)
    assert np.array_equal(dc.get(), [cm.get_center1(r) for r in x])


def test_min_max(dwt):
    g = cm.golden()
    for i, (seed, kind, n_lines, n) in enumerate(cm.CASES):
        if n in (1, 3, 65, 1000, 10000):
            d = Dev(dwt, cm.make_input(seed, kind, n_lines, n))
            mn, mx = dwt.rows_min_max(d.ptr, 4 * n, 4, n_lines, n)
            assert np.array_equal(mn, g["min_%d" % i]) and np.array_equal(mx, g["max_%d" % i])
            d.free()


@pytest.mark.parametrize("n", [1, 5, 65, 8193])
def test_displace_per_row(dwt, n):
    ds = np.array([-n - 1, -3, 0, 2, n, 1, -1, n - 1, -(n - 1)], np.int32)
    x = batch_of(len(ds), n)
    for zero in (True, False):
        want = np.stack([cm.displace1(r, int(d), zero) for r, d in zip(x, ds)])
        buf = frame(x, 3, 1)
        d, dd = Dev(dwt, buf), Dev(dwt, ds)
        dwt.rows_displace(d.ptr, buf.shape[1] * 4, 4, len(ds), n, dd if zero else ds, zero_fill=zero)  # device / host array
        out = d.get()
        assert np.array_equal(out[:len(ds), :n].view(np.uint32), want.view(np.uint32))
        assert np.all(out[:len(ds), n:] == CANARY) and np.all(out[len(ds)] == CANARY)


def test_displace_matches_reference_fixtures(dwt):
    g = cm.golden()
    seen = 0
    for i, (seed, kind, n_lines, n) in enumerate(cm.CASES):
        if "displace1_%d" % i not in g:
            continue
        x = cm.make_input(seed, kind, n_lines, n)
        for zero in (0, 1):
            for k, dn in enumerate(cm.DISPLACEMENTS):
                d = Dev(dwt, x)
                dwt.rows_displace(d.ptr, 4 * n, 4, n_lines, n, cm.displacement(dn, n), zero_fill=bool(zero))
                assert np.array_equal(d.get().view(np.uint32), g["displace%d_%d" % (zero, i)][k].view(np.uint32))
                d.free()
                seen += 1
    assert seen >= 40


def test_libdwt_mirrors_on_device_pointers(dwt):
    n, n_lines = 255, 6
    x = batch_of(n_lines, n)
    d = Dev(dwt, x)
    sx = 4 * n
    dwt.dwt_util_shift21_med_s(d.ptr, n, n_lines, sx, 4)
    want, _ = cm.condition(x, 1)
    assert same(d.get(), want)
    assert dwt.dwt_util_get_center1_s(d.ptr + sx, n, 4) == cm.get_center1(want[1])
    dwt.dwt_util_center21_s(d.ptr, n, n_lines, sx, 4, 20)
    want, _ = cm.condition(x, 3, 20)
    assert same(d.get(), want)
    assert dwt.dwt_util_find_min_max_s(d.ptr, n, n_lines, sx, 4) == (float(want.min()), float(want.max()))
    dwt.dwt_util_scale21_s(d.ptr, n, n_lines, sx, 4, 0.0, 1.0)
    want, _ = cm.condition(x, 7, 20)
    assert same(d.get(), want)
    dwt.dwt_util_shift_s(d.ptr, n, n_lines, sx, 4, 0.3)
    want = (want + F32(0.3)).astype(F32)
    dwt.dwt_util_scale_s(d.ptr, n, n_lines, sx, 4, 1.7)
    want = (want * F32(1.7)).astype(F32)
    assert np.array_equal(d.get().view(np.uint32), want.view(np.uint32))
    dwt.dwt_util_displace1_s(d.ptr, n, 4, -4)
    dwt.dwt_util_displace1_zero_s(d.ptr + sx, n, 4, 9)
    got = d.get()
    assert np.array_equal(got[0], cm.displace1(want[0], -4, False)) and np.array_equal(got[1], cm.displace1(want[1], 9, True))
    dwt.dwt_util_center1_s(d.ptr + 2 * sx, n, 4, 3)
    assert np.array_equal(d.get()[2], cm.center1(want[2], 3)[0])
    # pointer arithmetic only (the reference's argument order: sizes before strides)
    assert dwt.dwt_util_crop21(d.ptr, n, n_lines, sx, 4, 100) == d.ptr + 4 * (n // 2 - 50)
    assert dwt.dwt_util_viewport(d.ptr, n, n_lines, sx, 4, 7, 2) == d.ptr + 2 * sx + 28
    # the C entries themselves, on the same device rows
    e = Dev(dwt, x)
    L = dwt.lib
    import ctypes as C
    L.dwt_util_shift21_med_s.argtypes = [C.c_void_p] + [C.c_int] * 4
    L.dwt_util_shift21_med_s.restype = None
    L.dwt_util_center21_s.argtypes = [C.c_void_p] + [C.c_int] * 5
    L.dwt_util_scale21_s.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_float] * 2
    L.dwt_util_get_center1_s.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.dwt_util_shift21_med_s(e.ptr, n, n_lines, sx, 4)
    L.dwt_util_center21_s(e.ptr, n, n_lines, sx, 4, 20)
    want3, _ = cm.condition(x, 3, 20)
    assert L.dwt_util_get_center1_s(e.ptr, n, 4) == cm.get_center1(want3[0])
    L.dwt_util_scale21_s(e.ptr, n, n_lines, sx, 4, 0.0, 1.0)
    assert same(e.get(), cm.condition(x, 7, 20)[0])


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors(dwt):
    x = batch_of(3, 64)
    d = Dev(dwt, x)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0)):
        with pytest.raises(dwt.DwtError, match="hi > lo"):
            dwt.rows_condition(4, d.ptr, 256, 4, 3, 64, 20, lo, hi)
    dwt.rows_condition(3, d.ptr, 256, 4, 3, 64, 20, 1.0, 1.0)  # (lo, hi are not read without SCALE)
    d.free()
    d = Dev(dwt, x)
    with pytest.raises(dwt.DwtError, match="bad sizes"):
        dwt.rows_condition(7, d.ptr, 256, 4, 3, 0)
    with pytest.raises(dwt.DwtError, match="bad sizes"):
        dwt.rows_center_index(d.ptr, 256, 4, 3, 0)
    with pytest.raises(dwt.DwtError, match="multiples of 4"):
        dwt.rows_condition(7, d.ptr, 258, 4, 3, 64)
    with pytest.raises(dwt.DwtError, match="multiples of 4"):
        dwt.rows_min_max(d.ptr + 2, 256, 4, 3, 60)
    with pytest.raises(dwt.DwtError, match="operation mask"):
        dwt.rows_condition(8, d.ptr, 256, 4, 3, 64)
    assert np.array_equal(d.get().view(np.uint32), x.view(np.uint32))  # nothing was written


def test_example_spectra_condition(dwt, tmp_path):
    """examples/spectra_condition.c: upload, condition in one launch, transform, features; only the matrix comes down"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = tmp_path / "spectra_condition", os.path.join(root, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "spectra_condition.c"),
                           "-o", str(exe), "-L" + libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "success" in out.stdout + out.stderr, out.stdout + out.stderr
