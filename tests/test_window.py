"""CPU checks of the windowed inverse (include/libdwt_hip.h): dwt_hip_window_regions against the rule as
tests/window_model.py restates it, the rule against the full inverse -- everything outside the rectangles can hold anything
--, the border windows that put the float line-end forms to the test, and the geometry file under the sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import floatends
import window_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENDS_SHAPES = [(37, 53), (64, 80), (67, 131), (66, 130), (38, 54)]
ENDS_ENTRY = {"cdf97_s": "cdf97_s", "cdf53_s": "cdf53_s", "interp53_s": "interp53_2d"}  # the entries of tests/floatends.py


@pytest.fixture(scope="module")
def window():
    from libdwt_amd import window as w

    return w


@pytest.fixture(scope="module")
def orc():
    from oraclelib import Oracle

    return Oracle()


def sweep(seed, n_random):
    """(h, w, j_max, discard, window) over SHAPES, every level count, every discard"""
    rng = np.random.default_rng(seed)
    for h, w in wm.SHAPES:
        for j_max in range(wm.ceil_log2(min(h, w)) + 1):
            for r in range(j_max + 1):
                for win in wm.sweep_windows(rng, wm.band(w, r), wm.band(h, r), n_random):
                    yield h, w, j_max, r, win


def test_names_stay_out_of_the_package_namespace(window):
    import libdwt_amd

    for name in ("window_regions", "inverse_window_batch", "window_route", "region_bytes", "ROUTE_KERNELS", "ROUTE_INVERSE", "HALO", "TILE"):
        assert hasattr(window, name) and name not in vars(libdwt_amd), name
    assert window.HALO == {libdwt_amd.WAVELET_ID[k]: v for k, v in wm.HALO.items()} and window.TILE == 64
    # the route query is host arithmetic too: the default takes the kernels for a small window of a large band only
    assert window.window_route("cdf97_s", 1, 8192, 8192, 5, 0, 1, 1, 512, 512) == window.ROUTE_KERNELS
    assert window.window_route("cdf97_s", 1, 8192, 8192, 5, 0, 0, 0, 8192, 8192) == window.ROUTE_INVERSE
    assert window.region_bytes("cdf97_s", window.window_regions("cdf97_s", 64, 64, 1, 0, 0, 0, 64, 64)) == 4 * 64 * 64


@pytest.mark.parametrize("wavelet", wm.WAVELETS)
def test_regions_equal_the_model(window, wavelet):
    n = 0
    for h, w, j_max, r, (x0, y0, ww, wh) in sweep(4100, 4):
        want = wm.regions(wavelet, h, w, j_max, r, x0, y0, ww, wh)
        got = window.window_regions(wavelet, w, h, j_max, r, x0, y0, ww, wh)
        assert got.dtype == np.int32 and np.array_equal(got, want), (wavelet, h, w, j_max, r, x0, y0, ww, wh, got.tolist(), want.tolist())
        n += 1
    assert n > 700
    # j_max < 0 and j_max past the limit: the full depth
    for j_max in (-1, 40):
        assert np.array_equal(window.window_regions(wavelet, 131, 61, j_max, 1, 3, 2, 9, 5), wm.regions(wavelet, 61, 131, -1, 1, 3, 2, 9, 5))


@pytest.mark.parametrize("wavelet", wm.WAVELETS)
def test_whole_band_window_gives_the_whole_bands(window, wavelet):
    import libdwt_amd as dwt

    for h, w in wm.SHAPES:
        J = wm.levels(h, w, -1)
        geom = np.zeros((3 * J + 1, 4), np.int32)
        assert dwt.lib.dwt_hip_band_geometry(w, h, w, h, J, geom.ctypes.data) == 3 * J + 1
        for r in range(J + 1):
            got = window.window_regions(wavelet, w, h, J, r, 0, 0, wm.band(w, r), wm.band(h, r))
            want = geom.copy()
            want[:3 * r] = 0
            want[(want[:, 2] == 0) | (want[:, 3] == 0)] = 0  # (an empty band has zero sizes here)
            if r == J:
                want[3 * J] = (0, 0, wm.band(w, J), wm.band(h, J))
            assert np.array_equal(got, want), (wavelet, h, w, r, got.tolist(), want.tolist())


@pytest.mark.parametrize("wavelet", wm.WAVELETS)
def test_a_window_inside_another_needs_regions_inside_the_others(window, wavelet):
    rng = np.random.default_rng(4200)
    for h, w in wm.SHAPES[3:]:
        for j_max in range(wm.ceil_log2(min(h, w)) + 1):
            for r in range(j_max + 1):
                bw, bh = wm.band(w, r), wm.band(h, r)
                for _ in range(4):
                    x0, y0 = int(rng.integers(0, bw)), int(rng.integers(0, bh))
                    ww, wh = int(rng.integers(1, bw - x0 + 1)), int(rng.integers(1, bh - y0 + 1))
                    ix, iy = x0 + int(rng.integers(0, ww)), y0 + int(rng.integers(0, wh))
                    iw, ih = int(rng.integers(1, x0 + ww - ix + 1)), int(rng.integers(1, y0 + wh - iy + 1))
                    outer = window.window_regions(wavelet, w, h, j_max, r, x0, y0, ww, wh)
                    inner = window.window_regions(wavelet, w, h, j_max, r, ix, iy, iw, ih)
                    for o, i in zip(outer, inner):
                        if i[2] and i[3]:
                            assert o[0] <= i[0] and o[1] <= i[1] and i[0] + i[2] <= o[0] + o[2] and i[1] + i[3] <= o[1] + o[3], (h, w, j_max, r, o, i)


def test_bad_arguments_are_refused(window):
    import libdwt_amd as dwt

    table = np.full((94, 4), -5, np.int32)

    def rc(*a):
        return dwt._cdll.dwt_hip_window_regions(*a, table.ctypes.data)

    good = (dwt.CDF97_S, 40, 24, 3, 1, 2, 3, 4, 5)
    assert rc(*good) == 10
    table[:] = -5
    for bad in ((dwt.CDF97_H,) + good[1:], (dwt.CDF97_I,) + good[1:], (dwt.CDF97_D,) + good[1:], (dwt.CDF53_D,) + good[1:], (7,) + good[1:], (-1,) + good[1:],
                (0, 0, 24, 3, 0, 0, 0, 1, 1), (0, 40, -1, 3, 0, 0, 0, 1, 1), (0, 40, 24, 3, 4, 0, 0, 1, 1), (0, 40, 24, 3, -1, 0, 0, 1, 1),
                (0, 40, 24, -1, 6, 0, 0, 1, 1), (0, 40, 24, 3, 1, 0, 0, 21, 1), (0, 40, 24, 3, 1, 0, 0, 1, 13), (0, 40, 24, 3, 1, 20, 0, 1, 1),
                (0, 40, 24, 3, 1, -1, 0, 2, 2), (0, 40, 24, 3, 1, 0, -1, 2, 2), (0, 40, 24, 3, 1, 0, 0, 0, 2), (0, 40, 24, 3, 1, 0, 0, 2, 0),
                (0, 40, 24, 3, 1, 2**31 - 1, 0, 2**31 - 1, 1)):
        assert rc(*bad) == -1, bad
    assert (table == -5).all()
    assert dwt._cdll.dwt_hip_window_regions(*good, None) == -1
    with pytest.raises(dwt.DwtError):
        window.window_regions("cdf97_s", 40, 24, 3, 1, 0, 0, 21, 1)
    assert wm.regions("cdf97_s", 24, 40, 3, 1, 0, 0, 21, 1) is None


@pytest.mark.parametrize("wavelet", wm.WAVELETS)
def test_nothing_outside_the_regions_is_needed(orc, wavelet):
    """the rule is sufficient: with everything outside the rectangles NaN (floats) or other random integers of the whole range,
    the window of the full inverse keeps every bit"""
    n = 0
    clean = {}
    # (the numpy models take milliseconds per inverse: fewer random windows)
    for h, w, j_max, r, (x0, y0, ww, wh) in sweep(4300, 1 if wavelet in ("interp53_s", "cdf53_i16") else 3):
        key = (h, w, j_max, r)
        frame = wm.make_frame(wavelet, 4301 + 13 * h + w, h, w)
        if key not in clean:
            clean = {key: wm.full_inverse(orc, wavelet, frame, j_max, r)}
        want = clean[key][y0:y0 + wh, x0:x0 + ww]
        reg = wm.regions(wavelet, h, w, j_max, r, x0, y0, ww, wh)
        dirty = wm.masked(wavelet, frame, reg, n)
        got = wm.expected(orc, wavelet, dirty, j_max, r, x0, y0, ww, wh)
        assert not (got.dtype.kind == "f" and np.isnan(want).any())
        assert got.tobytes() == want.tobytes(), (wavelet, h, w, j_max, r, x0, y0, ww, wh)
        n += 1
    assert n > 400


def ends_cases(orc, wavelet):
    """(input, depth, faithful inverse, inverse with reflected ends) of the "ends" class at the border-window shapes"""
    shapes = list(ENDS_SHAPES)
    if wavelet == "interp53_s":
        # its one doubled tap is the last odd sample of an EVEN line: the shapes above tell at 7 samples, one short of the
        # minimum, so the even shapes of floatends.INTERP_SHAPES join them
        shapes += [s for s in floatends.INTERP_SHAPES if s[0] % 2 == 0 and s[1] % 2 == 0 and s not in shapes]
    for k, shp in enumerate(shapes):
        a = floatends.class_input("ends", 4400 + k, shp)
        depth = floatends.ends_level(orc, ENDS_ENTRY[wavelet], a)
        faithful = wm.full_inverse(orc, wavelet, a, depth, 0)
        with floatends.reflected_ends(orc):
            plain = wm.full_inverse(orc, wavelet, a, depth, 0)
        yield a, depth, faithful, plain


@pytest.mark.parametrize("wavelet", wm.FLOAT_WAVELETS)
def test_border_windows_put_the_end_forms_to_the_test(orc, wavelet):
    """the oracle alone: inside the four 16-wide border windows the faithful inverse and the one with reflected line ends
    differ at TELLING_MIN samples or more, and at most NAN_CAP of the windows' samples are NaN"""
    tell = nans = total = 0
    for a, depth, faithful, plain in ends_cases(orc, wavelet):
        h, w = a.shape
        for x0, y0, ww, wh in wm.border_windows(h, w):
            f, p = faithful[y0:y0 + wh, x0:x0 + ww], plain[y0:y0 + wh, x0:x0 + ww]
            tell += floatends.telling(f, p)
            nans += int(np.isnan(f).sum())
            total += f.size
    print("%s: %d telling samples, NaN share %.3f" % (wavelet, tell, nans / total))
    assert tell >= floatends.TELLING_MIN, (wavelet, tell)
    assert nans / total <= floatends.NAN_CAP, (wavelet, nans / total)


def test_geometry_under_asan_ubsan(tmp_path):
    """tests/san/san_window.c: a stand-alone program around libdwt_amd/csrc/dwt_window_geom.c, built with
    -fsanitize=address,undefined and run on the CPU; any report aborts it"""
    exe = tmp_path / "san_window"
    subprocess.check_call(["gcc", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g",
                           "-O1", os.path.join(ROOT, "tests", "san", "san_window.c"), os.path.join(ROOT, "libdwt_amd", "csrc", "dwt_window_geom.c"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "san_window: OK" in out.stdout, out.stdout + out.stderr
