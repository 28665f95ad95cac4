"""GPU checks of the wavelet packet transforms (dwt_hip_wp1d_batch, dwt_hip_wp2d_batch and the two feature entries,
libdwt_amd/packets.py) against tests/wp_model.py, which tests/test_wp.py pins to the compiled reference's functions.  Every
comparison is bitwise (a NaN on both sides is not compared); every buffer is filled with a canary first and every word
outside the addressed samples must still hold it afterwards; src of an out-of-place call must come back as it was.  Every
case runs on the fused route and under option "wp_fused" = 0, and both must give the model's bits."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import wp_model as wp
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
CANARY = np.uint32(0xDEADBEEF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N1D_MAX = 8192


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d
    from libdwt_amd import packets

    d.dwt_util_init()
    d.packets = packets
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("wp_fused", 1)


# ---- expectations: computed once, shared, never modified --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lines_case(wavelet, inverse, kind, n_lines, N, levels):
    x = wp.make_input(1000 + N + 7 * n_lines, kind, n_lines, N)
    want = (wp.inv1d if inverse else wp.fwd1d)(wavelet, x, levels)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@functools.lru_cache(maxsize=None)
def images_case(wavelet, inverse, kind, batch, size_y, size_x, levels):
    x = np.stack([wp.make_input(2000 + size_x + 3 * size_y + b, kind, size_y, size_x, image=True) for b in range(batch)])
    want = np.stack([(wp.inv2d if inverse else wp.fwd2d)(wavelet, x[b], levels) for b in range(batch)])
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def check_kind(kind, want):
    share = wp.nonfinite_share(want)
    if kind == "float_range":
        assert 0 < share <= wp.NONFINITE_CAP, share
    else:
        assert share == 0, share


# ---- runners ----------------------------------------------------------------------------------------------------
def run_lines(dwt, wavelet, inverse, x, levels, es=4, gap=0, off=0, in_place=True, device=True):
    """-> (the lines after the call, launches).  Elements es bytes apart, `gap` extra words between lines, the base `off`
    words past its allocation."""
    n_lines, N = x.shape
    step = es // 4
    pe = N * step + gap
    words = off + n_lines * pe + 8
    src = np.full(words, CANARY, np.uint32)
    idx = (off + np.arange(n_lines)[:, None] * pe + np.arange(N)[None, :] * step).reshape(-1)
    src[idx] = x.view(np.uint32).reshape(-1)
    dst = src if in_place else np.full(words, CANARY, np.uint32)
    src0 = src.copy()
    if device:
        ds = Dev(dwt, src)
        dd = ds if in_place else Dev(dwt, dst)
        sp, dp = ds.ptr + 4 * off, dd.ptr + 4 * off
    else:
        sp, dp = src.ctypes.data + 4 * off, dst.ctypes.data + 4 * off
    k = launches(dwt, lambda: dwt.packets.wp1d_batch(wp.WAVELET_ID[wavelet], inverse, sp, dp, pe * 4, es, n_lines, N, levels))
    if device:
        src = ds.get()
        dst = src if in_place else dd.get()
        ds.free()
        if not in_place:
            dd.free()
    if not in_place:
        assert np.array_equal(src, src0), "src was written"
    rest = np.ones(words, bool)
    rest[idx] = False
    assert (dst[rest] == CANARY).all(), "bytes outside the lines were written"
    return dst[idx].view(F32).reshape(n_lines, N), k


def run_images(dwt, wavelet, inverse, x, levels, es=4, pad=0, bgap=0, in_place=True, device=True):
    """-> (the images after the call, launches).  Rows `pad` elements longer than the image, `bgap` words between images,
    elements es bytes apart."""
    batch, h, w = x.shape
    step = es // 4
    pitch = (w + pad) * step
    img = h * pitch + bgap
    words = batch * img + 8
    src = np.full(words, CANARY, np.uint32)
    idx = (np.arange(batch)[:, None, None] * img + np.arange(h)[None, :, None] * pitch + np.arange(w)[None, None, :] * step).reshape(-1)
    src[idx] = x.view(np.uint32).reshape(-1)
    dst = src if in_place else np.full(words, CANARY, np.uint32)
    src0 = src.copy()
    if device:
        ds = Dev(dwt, src)
        dd = ds if in_place else Dev(dwt, dst)
        sp, dp = ds.ptr, dd.ptr
    else:
        sp, dp = src.ctypes.data, dst.ctypes.data
    k = launches(dwt, lambda: dwt.packets.wp2d_batch(wp.WAVELET_ID[wavelet], inverse, sp, dp, img * 4, batch, pitch * 4, es, w, h, levels))
    if device:
        src = ds.get()
        dst = src if in_place else dd.get()
        ds.free()
        if not in_place:
            dd.free()
    if not in_place:
        assert np.array_equal(src, src0), "src was written"
    rest = np.ones(words, bool)
    rest[idx] = False
    assert (dst[rest] == CANARY).all(), "bytes outside the images were written"
    return dst[idx].view(F32).reshape(batch, h, w), k


def both_routes(dwt, run, want, fused_launches):
    """the call under "wp_fused" = 1 and 0: the model's bits both times; the fused route's launch count where it is fixed"""
    try:
        for fused in (1, 0):
            dwt.set_option("wp_fused", fused)
            got, k = run()
            assert wp.same(got, want), ("wp_fused", fused, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            if fused and fused_launches is not None:
                assert k == fused_launches, (k, fused_launches)
    finally:
        dwt.set_option("wp_fused", 1)


# ---- 1-D --------------------------------------------------------------------------------------------------------
SIZES_1D = (2, 3, 5, 8, 63, 64, 100, 257, 512, 513, 2048, 2049, 4096, 8192, 8193, 10000)


def level_set(N):
    J = wp.floor_log2(N)
    return sorted({1, min(2, J), max(1, J // 2), J})


CASES_1D = []
for _i, _N in enumerate(SIZES_1D):
    for _j, _L in enumerate(level_set(_N)):
        # the deepest trees of the long lines: one line (the model walks thousands of nodes); otherwise 3 or 5 lines
        _n = 1 if (_N >= 4096 and _L > 8) else (3, 5)[(_i + _j) & 1]
        for _w, _wavelet in enumerate(wp.WAVELETS):
            for _inv in (False, True):
                _v = _i + _j + _w + _inv
                CASES_1D.append((_wavelet, _inv, _n, _N, _L, (4, 12)[_v % 3 == 0], (0, 1, 3)[_v % 3], _v & 1, bool((_v >> 1) & 1)))


@pytest.mark.parametrize("wavelet,inverse,n_lines,N,levels,es,gap,off,in_place", CASES_1D)
def test_lines(dwt, wavelet, inverse, n_lines, N, levels, es, gap, off, in_place):
    """every size, depth, wavelet and direction; element stride 4 and 12 (one channel of three), line pitches and bases
    that break 16-byte alignment, in place and out of place.  A fused call on device lines of up to 8192 samples is
    exactly one launch."""
    x, want = lines_case(wavelet, inverse, "normal", n_lines, N, levels)
    check_kind("normal", want)
    both_routes(dwt, lambda: run_lines(dwt, wavelet, inverse, x, levels, es, gap, off, in_place), want, 1 if N <= N1D_MAX else None)


@pytest.mark.parametrize("N,levels", [(64, 2), (64, 6), (513, 2), (2049, 2)])
@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_many_lines(dwt, wavelet, N, levels):
    """1030 lines: partial workgroups at 4, 2 and 1 lines per workgroup"""
    for inverse in (False, True):
        x, want = lines_case(wavelet, inverse, "small_ints", 1030, N, levels)
        both_routes(dwt, lambda: run_lines(dwt, wavelet, inverse, x, levels, in_place=not inverse), want, 1)


@pytest.mark.parametrize("wavelet", wp.WAVELETS)
@pytest.mark.parametrize("n_lines,N,levels", [(1, 2, 1), (3, 100, 6), (2, 4096, 12), (1, 8193, 3)])
def test_lines_host_pointers(dwt, wavelet, n_lines, N, levels):
    for inverse in (False, True):
        x, want = lines_case(wavelet, inverse, "normal", n_lines, N, levels)
        both_routes(dwt, lambda: run_lines(dwt, wavelet, inverse, x, levels, es=(4, 8)[inverse], gap=1, in_place=inverse, device=False), want, None)


@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_interleaved_lines(dwt, wavelet):
    """the lines as the channels of an (N, 3) array: line stride 4, element stride 12; in place, both routes"""
    n_lines, N, levels = 3, 100, 6
    for inverse in (False, True):
        x, want = lines_case(wavelet, inverse, "normal", n_lines, N, levels)

        def run():
            d = Dev(dwt, np.ascontiguousarray(x.T))
            k = launches(dwt, lambda: dwt.packets.wp1d_batch(wp.WAVELET_ID[wavelet], inverse, d.ptr, d.ptr, 4, 4 * n_lines, n_lines, N, levels))
            got = d.get().T
            d.free()
            return np.ascontiguousarray(got), k
        both_routes(dwt, run, want, 1)


# ---- 2-D --------------------------------------------------------------------------------------------------------
SIZES_2D = ((2, 2), (5, 3), (8, 8), (33, 47), (64, 64), (130, 66), (257, 129))  # (size_x, size_y)
CASES_2D = []
for _i, (_sx, _sy) in enumerate(SIZES_2D):
    for _L in range(1, wp.max_levels_2d(_sy, _sx) + 1):
        for _w, _wavelet in enumerate(wp.WAVELETS):
            # both directions of every (size, depth, wavelet); batch, pitch, batch gap and in place / out of place vary on
            # bits of their own
            _c = _i + _L + _w
            for _inv in (False, True):
                CASES_2D.append((_wavelet, _inv, (1, 3)[_c & 1], _sx, _sy, _L, (0, 5)[(_c >> 1) & 1], (0, 24)[(_c // 3) & 1],
                                 bool(((_c >> 1) + _inv) & 1)))
for _w, _wavelet in enumerate(wp.WAVELETS):
    for _inv in (False, True):
        CASES_2D.append((_wavelet, _inv, 1, 512, 96, 3, 0, 0, _inv))
# 8 levels, the most the entry takes (level index 7, the fused kernel's last): the smallest image that has them
for _wavelet, _inv in (("cdf97_s", False), ("cdf97_s", True), ("cdf53_s", False), ("interp53_s", True)):
    CASES_2D.append((_wavelet, _inv, 1, 256, 256, 8, 0, 0, not _inv))


@pytest.mark.parametrize("wavelet,inverse,batch,size_x,size_y,levels,pad,bgap,in_place", CASES_2D)
def test_images(dwt, wavelet, inverse, batch, size_x, size_y, levels, pad, bgap, in_place):
    """every size at levels 1 .. max, the three wavelets, both directions of each; batches of 3 with a batch stride
    larger than the image, pitches wider than the row, in place and out of place.  A fused call on a dense device batch
    is exactly `levels` launches, whatever the batch."""
    x, want = images_case(wavelet, inverse, "normal", batch, size_y, size_x, levels)
    check_kind("normal", want)
    both_routes(dwt, lambda: run_images(dwt, wavelet, inverse, x, levels, 4, pad, bgap, in_place), want, levels)


@pytest.mark.parametrize("wavelet", wp.WAVELETS)
@pytest.mark.parametrize("size_x,size_y,levels", [(5, 3, 1), (33, 47, 5), (130, 66, 3)])
def test_images_strided_elements_and_host(dwt, wavelet, size_x, size_y, levels):
    """stride_y 8 (the line-pass route whatever the option) on device memory, and host pointers"""
    for inverse in (False, True):
        x, want = images_case(wavelet, inverse, "normal", 2, size_y, size_x, levels)
        both_routes(dwt, lambda: run_images(dwt, wavelet, inverse, x, levels, es=8, pad=1, bgap=8, in_place=inverse), want, None)
        both_routes(dwt, lambda: run_images(dwt, wavelet, inverse, x, levels, pad=3, bgap=8, in_place=not inverse, device=False), want, None)


# ---- float classes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("float_range", "tiny"))
@pytest.mark.parametrize("wavelet", wp.WAVELETS)
def test_float_classes(dwt, wavelet, kind):
    """the whole float range (at most 25 % of the expected samples non-finite) and all-subnormal inputs: one 1-D and one
    2-D shape per wavelet, both directions, both routes"""
    for inverse in (False, True):
        x, want = lines_case(wavelet, inverse, kind, 3, 1000, 3)
        check_kind(kind, want)
        both_routes(dwt, lambda: run_lines(dwt, wavelet, inverse, x, 3, in_place=inverse), want, 1)
        x, want = images_case(wavelet, inverse, kind, 2, 66, 130, 2)
        check_kind(kind, want)
        both_routes(dwt, lambda: run_images(dwt, wavelet, inverse, x, 2, in_place=not inverse), want, 2)


# ---- geometry helpers of the library ----------------------------------------------------------------------------
def test_nodes_and_freq_order(dwt):
    for N in (2, 3, 100, 257, 8193):
        for level in range(wp.floor_log2(N) + 1):
            start, length = dwt.packets.wp_nodes(N, level)
            assert list(zip(start, length)) == wp.nodes_recursive(N, level)
        assert dwt.lib.dwt_hip_wp_nodes(N, wp.floor_log2(N) + 1, None, None) == -1
    for level in range(8):
        assert dwt.packets.wp_freq_order(level) == wp.freq_order(level)


# ---- features ---------------------------------------------------------------------------------------------------
def band_feature(dwt, f, ptr, stride_x, w, h, j, p):
    v = C.c_float()
    assert dwt.lib.dwt_hip_band_feature(f, ptr, stride_x, 4, w, h, j, p, C.byref(v)) == 0, dwt.last_error()
    return np.float32(v.value)


@pytest.mark.parametrize("order", (0, 1))
def test_features_of_lines(dwt, order):
    """level 5 of a batch of transformed lines: every feature of every node equals dwt_hip_band_feature on the node's span
    of the stored result, in natural and in frequency order"""
    n_lines, N, level, p = 3, 301, 5, 1.5
    x, packets_ = lines_case("cdf97_s", False, "normal", n_lines, N, level)
    d = Dev(dwt, packets_)
    nf, nb = len(dwt.FEATURE_NAMES), 1 << level
    fv = np.zeros((n_lines, nf * nb + 3), F32)
    dfv = Dev(dwt, fv)
    dwt.packets.wp_features1d_batch(list(dwt.FEATURE_NAMES), d.ptr, 4 * N, 4, n_lines, N, level, order, dfv.ptr, fv.shape[1], p)
    got = dfv.get()
    nodes = wp.nodes_recursive(N, level)
    perm = wp.freq_order(level) if order else list(range(nb))
    for y in range(n_lines):
        for f in range(nf):
            for k in range(nb):
                s, n = nodes[perm[k]]
                want = band_feature(dwt, f, d.ptr + 4 * (y * N + s), 4 * n, n, 1, level, p)
                assert got[y, f * nb + k].view(np.uint32) == want.view(np.uint32), (y, dwt.FEATURE_NAMES[f], k, got[y, f * nb + k], want)
    assert (got[:, nf * nb:] == 0).all()
    d.free()
    dfv.free()


@pytest.mark.parametrize("order", (0, 1))
def test_features_of_images(dwt, order):
    batch, size_x, size_y, level, p = 2, 47, 33, 2, 3.0
    x, packets_ = images_case("cdf53_s", False, "normal", batch, size_y, size_x, level)
    d = Dev(dwt, packets_)
    nf, nn = len(dwt.FEATURE_NAMES), 1 << level
    nb = nn * nn
    fv = np.zeros((batch, nf * nb), F32)
    dfv = Dev(dwt, fv)
    dwt.packets.wp_features2d_batch(list(dwt.FEATURE_NAMES), d.ptr, 4 * size_x * size_y, batch, 4 * size_x, size_x, size_y, level, order,
                                    dfv.ptr, fv.shape[1], p)
    got = dfv.get()
    nx, ny = wp.nodes_recursive(size_x, level), wp.nodes_recursive(size_y, level)
    perm = wp.freq_order(level) if order else list(range(nn))
    for b in range(batch):
        for f in range(nf):
            for ky in range(nn):
                for kx in range(nn):
                    (sx, w), (sy, h) = nx[perm[kx]], ny[perm[ky]]
                    want = band_feature(dwt, f, d.ptr + 4 * ((b * size_y + sy) * size_x + sx), 4 * size_x, w, h, level, p)
                    g = got[b, f * nb + ky * nn + kx]
                    assert g.view(np.uint32) == want.view(np.uint32), (b, dwt.FEATURE_NAMES[f], ky, kx, g, want)
    d.free()
    dfv.free()


# ---- errors -----------------------------------------------------------------------------------------------------
def test_errors(dwt):
    x = Dev(dwt, np.zeros(64 * 64, F32))
    fv = Dev(dwt, np.zeros(4096, F32))
    L = dwt.lib

    def refused(rc):
        assert rc != 0 and len(dwt.last_error()) > 10

    for N in (2, 100, 64):
        for levels in (0, wp.floor_log2(N) + 1, -1):
            refused(L.dwt_hip_wp1d_batch(0, 0, x.ptr, x.ptr, 4 * N, 4, 1, N, levels))
    # lines that share samples: neither apart nor interleaved within an element step
    refused(L.dwt_hip_wp1d_batch(0, 0, x.ptr, x.ptr, 4, 4, 2, 100, 2))
    refused(L.dwt_hip_wp1d_batch(0, 0, x.ptr, x.ptr, 4 * 99, 4, 2, 100, 2))
    refused(L.dwt_hip_wp1d_batch(0, 0, x.ptr, x.ptr, 4, 8, 3, 100, 2))
    for levels in (0, 7, 9):
        refused(L.dwt_hip_wp2d_batch(0, 0, x.ptr, x.ptr, 0, 1, 4 * 64, 4, 64, 64, levels))
    refused(L.dwt_hip_wp2d_batch(0, 0, x.ptr, x.ptr, 0, 1, 4 * 64, 4, 64, 33, 6))
    for wavelet in (1, 3, 4, 5, 7, 8, 9, -1, 77):  # int, double, none, int16, binary16
        refused(L.dwt_hip_wp1d_batch(wavelet, 0, x.ptr, x.ptr, 400, 4, 1, 100, 2))
        refused(L.dwt_hip_wp2d_batch(wavelet, 1, x.ptr, x.ptr, 0, 1, 4 * 64, 4, 64, 64, 2))
    one = dwt.FEATURE["wps"]
    refused(L.dwt_hip_wp_features1d_batch(one, x.ptr, 4 * 4096, 4, 1, 4096, 7, 0, 2.0, fv.ptr, 4096))  # 128 nodes
    refused(L.dwt_hip_wp_features2d_batch(one, x.ptr, 0, 1, 4 * 64, 64, 64, 4, 0, 2.0, fv.ptr, 4096))  # 256 nodes
    assert L.dwt_hip_wp_features1d_batch(one, x.ptr, 4 * 4096, 4, 1, 4096, 6, 1, 2.0, fv.ptr, 4096) == 0, dwt.last_error()
    assert L.dwt_hip_wp_features2d_batch(one, x.ptr, 0, 1, 4 * 64, 64, 64, 3, 1, 2.0, fv.ptr, 4096) == 0, dwt.last_error()
    x.free()
    fv.free()


# ---- example ----------------------------------------------------------------------------------------------------
def test_example_spectra_packets(dwt, tmp_path):
    """examples/spectra_packets.c: condition, packets in one launch, node energies in frequency order, round trip"""
    exe, libdir = tmp_path / "spectra_packets", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "spectra_packets.c"),
                           "-o", str(exe), "-L" + libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "packets: success" in out.stdout + out.stderr, out.stdout + out.stderr


# ---- stream -----------------------------------------------------------------------------------------------------
def test_entries_run_on_the_callers_stream():
    """every new device entry once on a non-blocking stream behind a bounded delay, in a process of its own
    (tests/wp_stream.py, on the harness of tests/stream_cases.py): the model's bits, and the transform entries queue
    without waiting for the stream"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wp_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]
