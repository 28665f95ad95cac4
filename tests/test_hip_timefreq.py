"""GPU checks of the time-frequency planes (dwt_hip_timefreq_batch, the gabor_*_s entries, dwt_hip_phase_derivative,
dwt_hip_detect_ridges) against the reference's outputs in tests/golden/timefreq.npz; lines the fixtures do not hold are
checked against the float32 restatement of tests/timefreq_model.py, which tests/test_timefreq.py pins to the fixtures.

Complex sums, magnitudes, phase derivative and the ridge detectors: bitwise, NaN == NaN.  Arguments: the device value
against float64 arctan2 of the same (re, im) bits, within the reference's own largest error over the fixtures (manifest)
plus 1 ulp -- the room for two faithful roundings to land on neighbouring floats.

Launches: a batch call on device memory takes 1 launch whatever n_lines, bins and the kernel sizes, under either kernel."""
import json
import os
import subprocess

import numpy as np
import pytest

import timefreq_model as tm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
CANARY = np.uint32(0xDEADBEEF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(tm.GOLDEN)
with open(tm.MANIFEST) as _f:
    INFO = json.load(_f)
IDS = ["-".join(str(v) for v in c[:5]) for c in tm.CASES]
LAUNCHES_PER_BATCH = 1


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("timefreq_tiled", 1)


def bank_of(dwt, i):
    sizes, centers = GOLD["sizes_%d" % i], GOLD["centers_%d" % i]
    taps = np.split(GOLD["taps_%d" % i], np.cumsum(sizes)[:-1])
    return dwt.timefreq_bank(kernels=taps, centers=centers), (sizes, centers, taps)


def run_batch(dwt, bank, bins, x, out_kind, device, pad=0, es=4, dstep=1):
    """-> (planes (lines, bins, n[, 2]), launches).  Lines `pad` elements longer than n, elements es bytes apart; the output in
    a canary-filled buffer -- rows padded, elements `dstep` outputs apart, a gap between planes -- whose every word
    outside the addressed outputs must come back untouched, and src must come back as it went."""
    lines, n = x.shape
    step = es // 4
    src = np.full((lines, (n + pad) * step), F32(-7.5), F32)
    src[:, :n * step:step] = x
    w = 2 if out_kind == "complex" else 1  # words per output
    row_e = (n + pad) * w * dstep
    plane_e = bins * row_e + 16
    out = np.full(lines * plane_e, CANARY, np.uint32)
    bufs = [Dev(dwt, a) for a in (src, out)] if device else None
    sp, op = [b.ptr for b in bufs] if device else [a.ctypes.data for a in (src, out)]
    k = launches(dwt, lambda: dwt.timefreq_batch(bank, sp, src.shape[1] * 4, es, lines, n, out_kind, op, plane_e * 4, row_e * 4,
                                                 None if dstep == 1 else w * dstep * 4))
    if device:
        assert np.array_equal(bufs[0].get(src.shape).view(np.uint32), src.view(np.uint32))
        out = bufs[1].get(out.shape, np.uint32)
        for b in bufs:
            b.free()
    v = out.reshape(lines, plane_e)
    assert (v[:, bins * row_e:] == CANARY).all()
    body = v[:, :bins * row_e].reshape(lines, bins, n + pad, dstep, w)
    assert (body[:, :, n:] == CANARY).all() and (body[:, :, :, 1:] == CANARY).all()
    got = np.ascontiguousarray(body[:, :, :n, 0, :]).view(F32)
    return (got if w == 2 else got[..., 0]), k


# (device, pad, elem_stride, dst step, extra lines)
LAYOUTS = [(True, 0, 4, 1, 0), (True, 3, 4, 1, 2), (True, 5, 8, 2, 1), (False, 0, 4, 1, 1), (False, 2, 8, 3, 0)]


@pytest.mark.parametrize("tiled", [1, 0], ids=["tiled", "plain"])
@pytest.mark.parametrize("i", range(len(tm.CASES)), ids=IDS)
def test_dots_and_magnitudes_bit_identical(dwt, i, tiled):
    seed, kind, inp, n, bins, _, _ = tm.CASES[i]
    bank, (sizes, centers, taps) = bank_of(dwt, i)
    dots, mag = GOLD["dots_%d" % i], GOLD["mag_%d" % i]
    dwt.set_option("timefreq_tiled", tiled)
    try:
        for device, pad, es, dstep, extra in LAYOUTS:
            # line 0 is the fixture's; the lines after it differ from it and from each other
            x = np.concatenate([GOLD["x_%d" % i][None]] + [tm.make_input(seed + 50 + e, inp, 1, n) for e in range(extra)])
            want = [(dots[..., 0], dots[..., 1], mag)] + [tm.planes(x[1 + e], sizes, centers, taps) for e in range(extra)]
            c, k1 = run_batch(dwt, bank, bins, x, "complex", device, pad, es, dstep)
            m, k2 = run_batch(dwt, bank, bins, x, "abs", device, pad, es, dstep)
            for y in range(1 + extra):
                what = (tm.CASES[i], "tiled" if tiled else "plain", device, pad, es, dstep, "line", y)
                assert tm.same(c[y, ..., 0], want[y][0]) and tm.same(c[y, ..., 1], want[y][1]), what
                assert tm.same(m[y], want[y][2]), what
            if device:
                assert k1 == k2 == LAUNCHES_PER_BATCH
    finally:
        dwt.set_option("timefreq_tiled", 1)
        bank.free()


def test_zero_padding_is_exact_under_nan_and_inf(dwt):
    """the tiled kernel runs every tap over a window that is zero outside the line; the plain kernel clips the taps as the
    reference does: the same bits on lines of the whole float range, kernels far longer than the line included"""
    n, bins = 200, 7
    x = tm.make_input(99, "float_range", 4, n)
    assert np.isnan(x).any() and np.isinf(x).any()
    bank = dwt.timefreq_bank("ft", bins, 40.0)
    sizes, centers, taps = bank.query()
    assert sizes.min() > n
    got = {}
    for tiled in (1, 0):
        dwt.set_option("timefreq_tiled", tiled)
        got[tiled] = run_batch(dwt, bank, bins, x, "complex", True)[0]
    dwt.set_option("timefreq_tiled", 1)
    bank.free()
    assert tm.same(got[1], got[0])
    for y in range(4):
        re, im, _ = tm.planes(x[y], sizes, centers, taps)
        assert tm.same(got[1][y, ..., 0], re) and tm.same(got[1][y, ..., 1], im)


def test_non_finite_taps_take_the_plain_kernel(dwt):
    """0 * Inf is NaN: a bank with such a tap is never run over zero padding"""
    n = 40
    x = tm.make_input(5, "normal", 1, n)
    k = (np.arange(9) - 4 + 1j).astype(np.complex64)
    k[2] = np.inf
    k[7] = complex(1.0, np.nan)
    bank = dwt.timefreq_bank(kernels=[k, k[:5]], centers=[4, 1])
    got, launched = run_batch(dwt, bank, 2, x, "complex", True)
    bank.free()
    re, im, _ = tm.planes(x[0], [9, 5], [4, 1], [k, k[:5]])
    assert launched == 1 and tm.same(got[0, ..., 0], re) and tm.same(got[0, ..., 1], im)


def test_long_kernels_and_many_tiles(dwt):
    """kernels longer than one staged window (512 taps) and lines longer than one tile (512 outputs): the S transform at 256
    bins (13 .. 2898 taps) over 1500 samples, the rows with the longest and the shortest kernels against the restatement,
    every row tiled == plain"""
    n, bins = 1500, 256
    x = tm.make_input(321, "normal", 2, n)
    bank = dwt.timefreq_bank("st", bins)
    sizes, centers, taps = bank.query()
    tiled, k = run_batch(dwt, bank, bins, x, "complex", True)
    dwt.set_option("timefreq_tiled", 0)
    plain, _ = run_batch(dwt, bank, bins, x, "complex", True)
    dwt.set_option("timefreq_tiled", 1)
    bank.free()
    assert k == 1 and tm.same(tiled, plain)
    for y in (0, 1, 100, bins - 1):
        re, im = tm.cdots(x[1], int(sizes[y]), int(centers[y]), taps[y])
        assert tm.same(tiled[1, bins - 1 - y, :, 0], re) and tm.same(tiled[1, bins - 1 - y, :, 1], im), y


MEASURED = {"arg_max_ulp": 0.0}


@pytest.mark.parametrize("i", range(len(tm.CASES)), ids=IDS)
def test_arguments(dwt, i):
    n, bins = tm.CASES[i][3], tm.CASES[i][4]
    bank, _ = bank_of(dwt, i)
    x = GOLD["x_%d" % i][None]
    d = GOLD["dots_%d" % i].astype(np.float64)
    with np.errstate(all="ignore"):
        exact = np.arctan2(d[..., 1], d[..., 0])
    limit = INFO["arg_ref_max_ulp"] + 1
    for device, tiled in ((True, 1), (True, 0), (False, 1)):
        dwt.set_option("timefreq_tiled", tiled)
        got = run_batch(dwt, bank, bins, x, "arg", device, 1)[0][0]
        dwt.set_option("timefreq_tiled", 1)
        assert np.array_equal(np.isnan(got), np.isnan(exact))
        ok = ~np.isnan(exact)
        e = tm.ulps(got[ok], exact[ok])
        worst = float(e.max()) if e.size else 0.0
        MEASURED["arg_max_ulp"] = max(MEASURED["arg_max_ulp"], worst)
        print("device arg: %.4f ulp of float64 atan2 (limit %.4f)" % (worst, limit))
        assert worst <= limit
        assert np.array_equal(np.signbit(got[ok]), np.signbit(exact[ok]))  # the side of the branch cut, and both zeros
    bank.free()


def test_argument_at_the_branch_cut(dwt):
    """im = +-0 with re < 0: a sum never is -0 (it starts at +0), so the argument of a negative real sum is +pi; -pi would
    need im = -0.  A real tap gives im = x * -0 summed into +0."""
    x = np.array([[-1.0, -0.0, 0.0, 2.0, -3e38, -1e-45]], F32)
    bank = dwt.timefreq_bank(kernels=[np.array([1 + 0j], np.complex64)], centers=[0])
    c = run_batch(dwt, bank, 1, x, "complex", True)[0][0, 0]
    a = run_batch(dwt, bank, 1, x, "arg", True)[0][0, 0]
    bank.free()
    assert not np.signbit(c[:, 1]).any()
    want = np.arctan2(c[:, 1].astype(np.float64), c[:, 0].astype(np.float64)).astype(F32)
    assert tm.same(a, want) and a[0] == F32(np.pi) and a[4] == F32(np.pi) and a[5] == F32(np.pi) and not np.signbit(a).any()


def run_plane_op(dwt, op, planes, param, device, pad=0, step=1):
    """planes (p, rows, n) -> the operator's output, the same layout on both sides: rows padded, elements `step` words
    apart, a gap between planes; canary everywhere else"""
    p, rows, n = planes.shape
    row_e = (n + pad) * step
    plane_e = rows * row_e + 8
    src = np.full((p, plane_e), F32(4.25), F32)
    src[:, :rows * row_e].reshape(p, rows, n + pad, step)[:, :, :n, 0] = planes
    out = np.full((p, plane_e), CANARY, np.uint32)
    bufs = [Dev(dwt, a) for a in (src, out)] if device else None
    sp, op_ = [b.ptr for b in bufs] if device else [a.ctypes.data for a in (src, out)]
    if op == 0:
        k = launches(dwt, lambda: dwt.phase_derivative(sp, op_, row_e * 4, step * 4, n, rows, param, p, plane_e * 4))
    else:
        k = launches(dwt, lambda: dwt.detect_ridges(op, sp, op_, row_e * 4, step * 4, n, rows, param, p, plane_e * 4))
    if device:
        out = bufs[1].get(out.shape, np.uint32)
        for b in bufs:
            b.free()
    assert (out[:, rows * row_e:] == CANARY).all()
    body = out[:, :rows * row_e].reshape(p, rows, n + pad, step)
    assert (body[:, :, n:] == CANARY).all() and (body[:, :, :, 1:] == CANARY).all()
    return np.ascontiguousarray(body[:, :, :n, 0]).view(F32), k


@pytest.mark.parametrize("i", range(len(tm.CASES)), ids=IDS)
def test_plane_operators_bit_identical(dwt, i):
    """fed the fixtures' planes.  detect_ridges3_s: the fixtures hold no point within 2^-20 of a direction threshold
    (manifest, tests/test_timefreq.py), so none is excused"""
    mag, arg, pd = GOLD["mag_%d" % i], GOLD["arg_%d" % i], GOLD["pd_%d" % i]
    limit = INFO["phase_limit"]
    with np.errstate(all="ignore"):
        mag2, arg2 = (mag[::-1] * F32(0.5)).astype(F32), (-arg).astype(F32)
    for device, pad, step in ((True, 0, 1), (True, 3, 2), (False, 0, 1), (False, 1, 3)):
        got, k = run_plane_op(dwt, 0, np.stack([arg, arg2]), limit, device, pad, step)
        assert tm.same(got[0], pd) and tm.same(got[1], tm.phase_derivative(arg2, limit)), ("pd", device, pad, step)
        got1, _ = run_plane_op(dwt, 1, np.stack([mag, mag2]), 0.0, device, pad, step)
        assert tm.same(got1[0], GOLD["r1_%d" % i]) and tm.same(got1[1], tm.ridges1(mag2, 0.0)), ("r1", device, pad, step)
        got2, _ = run_plane_op(dwt, 2, np.stack([pd, got[1]]), 0.0, device, pad, step)
        assert tm.same(got2[0], GOLD["r2_%d" % i]) and tm.same(got2[1], tm.ridges2(got[1], 0.0)), ("r2", device, pad, step)
        got3, _ = run_plane_op(dwt, 3, np.stack([mag, mag]), 0.0, device, pad, step)
        assert tm.same(got3[0], GOLD["r3_%d" % i]) and tm.same(got3[1], GOLD["r3_%d" % i]), ("r3", device, pad, step)
        if device:
            assert k == 1
    thr = float(np.nanmedian(mag[np.isfinite(mag)])) if np.isfinite(mag).any() else 0.0
    assert tm.same(run_plane_op(dwt, 1, mag[None], thr, True)[0][0], tm.ridges1(mag, thr))


@pytest.mark.parametrize("i", range(len(tm.CASES)), ids=IDS)
def test_reference_entries(dwt, i):
    """gabor_ft_s / gabor_wt_s / gabor_st_s with the reference's prototypes on host memory (and device memory): the
    fixtures' magnitude planes bitwise where this host's generators gave the fixtures' taps bitwise, else the restatement
    over the library's own bank; the _arg_ twins within the limit of test_arguments"""
    _, kind, _, n, bins, sigma, freq = tm.CASES[i]
    x = GOLD["x_%d" % i]
    bank = dwt.timefreq_bank(kind, bins, sigma, freq)
    sizes, centers, taps = bank.query()
    bank.free()
    if tm.same(np.concatenate(taps).view(F32), GOLD["taps_%d" % i].view(F32)):
        d, want = GOLD["dots_%d" % i], GOLD["mag_%d" % i]
        re, im = d[..., 0], d[..., 1]
    else:
        re, im, want = tm.planes(x, sizes, centers, taps)
    extra = {"ft": (sigma,), "wt": (sigma, freq), "st": ()}[kind]
    for device in (False, True):
        for step in (1, 2):  # stride_y: the distance of a row's elements
            plane = np.full((bins, n * step), CANARY, np.uint32)
            angle = plane.copy()
            bufs = [Dev(dwt, a) for a in (x, plane, angle)] if device else None
            xp, pp, ap = [b.ptr for b in bufs] if device else [a.ctypes.data for a in (x, plane, angle)]
            getattr(dwt, "gabor_%s_s" % kind)(xp, 4, n, pp, n * step * 4, step * 4, bins, *extra)
            getattr(dwt, "gabor_%s_arg_s" % kind)(xp, 4, n, ap, n * step * 4, step * 4, bins, *extra)
            if device:
                plane, angle = bufs[1].get(plane.shape, np.uint32), bufs[2].get(angle.shape, np.uint32)
                for b in bufs:
                    b.free()
            assert tm.same(plane[:, ::step].view(F32), want), (device, step)
            assert all((plane[:, s::step] == CANARY).all() and (angle[:, s::step] == CANARY).all() for s in range(1, step))
            with np.errstate(all="ignore"):
                exact = np.arctan2(im.astype(np.float64), re.astype(np.float64))
            got, ok = angle[:, ::step].view(F32), ~np.isnan(exact)
            assert np.array_equal(np.isnan(got), ~ok) and (tm.ulps(got[ok], exact[ok]) <= INFO["arg_ref_max_ulp"] + 1).all()


def test_line_and_dot_entries(dwt):
    """timefreq_line / timefreq_arg_line / dwt_util_cdot1_s through their dwt_hip_ functions: one kernel the caller brings,
    its taps 16 bytes apart"""
    i = 5
    n, bins = tm.CASES[i][3], tm.CASES[i][4]
    x, dots, mag = GOLD["x_%d" % i], GOLD["dots_%d" % i], GOLD["mag_%d" % i]
    sizes, centers = GOLD["sizes_%d" % i], GOLD["centers_%d" % i]
    taps = np.split(GOLD["taps_%d" % i], np.cumsum(sizes)[:-1])
    for y in (0, 7, bins - 1):
        k = np.zeros((int(sizes[y]), 2), np.complex64)
        k[:, 0] = taps[y]
        for device in (False, True):
            row = np.full(2 * n, CANARY, np.uint32)
            bufs = [Dev(dwt, a) for a in (x, row)] if device else None
            xp, rp = [b.ptr for b in bufs] if device else [a.ctypes.data for a in (x, row)]
            assert dwt.lib.dwt_hip_timefreq_line(0, rp, 8, xp, 4, n, k.ctypes.data, 16, int(sizes[y]), int(centers[y])) == 0, dwt.last_error()
            re_im = np.zeros(2, F32)
            for t in (0, n // 2, n - 1):
                assert dwt.lib.dwt_hip_cdot1(xp, n, 4, t, k.ctypes.data, int(sizes[y]), 16, int(centers[y]), re_im.ctypes.data) == 0, dwt.last_error()
                assert tm.same(re_im, dots[bins - 1 - y, t])
            if device:
                row = bufs[1].get(row.shape, np.uint32)
                for b in bufs:
                    b.free()
            assert tm.same(row[::2].view(F32), mag[bins - 1 - y]) and (row[1::2] == CANARY).all()


def test_launch_counts(dwt):
    """dense device lines: LAUNCHES_PER_BATCH launches, independent of n_lines, of bins and of the kernel sizes"""
    for kind, bins, n in (("ft", 16, 64), ("wt", 64, 700), ("st", 32, 2000)):
        bank = dwt.timefreq_bank(kind, bins, 3.0, 3.0)
        for lines in (1, 3, 300):
            src, dst = Dev(dwt, np.zeros((lines, n), F32)), Dev(dwt, np.zeros((lines, bins, n, 2), F32))
            for tiled in (1, 0):
                dwt.set_option("timefreq_tiled", tiled)
                for out, w in (("complex", 8), ("abs", 4), ("arg", 4)):
                    k = launches(dwt, lambda: dwt.timefreq_batch(bank, src.ptr, n * 4, 4, lines, n, out, dst.ptr, bins * n * w, n * w))
                    assert k == LAUNCHES_PER_BATCH, (kind, lines, tiled, out, k)
            dwt.set_option("timefreq_tiled", 1)
            src.free()
            dst.free()
        bank.free()


def test_refusals(dwt):
    x, out = np.zeros((3, 32), F32), np.zeros((3, 4, 32), F32)
    d, do = Dev(dwt, x), Dev(dwt, out)
    bank = dwt.timefreq_bank("st", 4)
    bad = [
        lambda: dwt.timefreq_batch(bank, d.ptr, 128, 4, 3, 32, "abs", out, 512, 128),  # device src, host dst
        lambda: dwt.timefreq_batch(bank, x, 128, 4, 3, 32, "abs", do.ptr, 512, 128),
        lambda: dwt.timefreq_batch(bank, d.ptr, 128, 6, 2, 16, "abs", do.ptr, 512, 128),  # device stride not a multiple of 4
        lambda: dwt.timefreq_batch(bank, d.ptr, 128, 4, 3, 32, "abs", d.ptr, 512, 128),  # overlap
        lambda: dwt.phase_derivative(do.ptr, out, 128, 4, 32, 4, 3.0),
        lambda: dwt.detect_ridges(3, out, do.ptr, 128, 4, 32, 4, 0.0),
        lambda: dwt.detect_ridges(1, do.ptr, do.ptr + 64, 128, 4, 32, 4, 0.0),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    bank.free()
    d.free()
    do.free()


def test_c_example(dwt, tmp_path):
    """examples/time_freq.c: the flow of the reference's spectra-tf program from C, one batch call per plane kind"""
    exe, libdir = tmp_path / "time_freq", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "time_freq.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    text = out.stderr + out.stdout
    assert text.count("success") == 3 and "FT: success" in text and "WT: success" in text and "ST: success" in text
