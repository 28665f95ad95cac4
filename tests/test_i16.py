"""The reversible int16 CDF 5/3 in JPEG 2000 order (DWT_HIP_CDF53_I16), without a GPU: the restatement of
tests/i16_model.py against the golden of the reference's cores (tests/golden/cdf53_i16.npz, scripts/gen_i16_golden.py),
its exact reversibility over the whole int16 range, its tie to the existing int32 oracle through the rows-first variant,
and the declarations of the public interface."""
import hashlib
import json
import os

import numpy as np
import pytest

import i16_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cdf53_i16.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "cdf53_i16_manifest.json")


def golden():
    with open(MANIFEST) as f:
        man = json.load(f)
    z = np.load(GOLDEN)
    return man, z


def test_manifest_matches_the_fixture():
    man, _ = golden()
    with open(GOLDEN, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == man["files"]["cdf53_i16.npz"]["sha256"]
    cases = man["files"]["cdf53_i16.npz"]["cases"]
    fwd1 = {(c["rows"], c["columns"]) for c in cases if c["kind"] == "forward" and c["levels"] == 1}
    assert fwd1 == {(2, 2), (3, 3), (2, 5), (9, 14), (13, 7), (16, 12), (32, 32), (67, 130)}
    assert {c["levels"] for c in cases if c["kind"] == "forward"} == {1, 2, 3}
    for c in cases:
        if c["kind"] == "inverse":  # the shapes the reference's inverse gets wrong are left out by rule
            assert c["rows"] % 2 == 0 and c["columns"] % 2 == 0 and min(c["rows"], c["columns"]) >= 4
        assert c["amplitude"] <= (4096 if c["levels"] == 1 else 1024)
    assert set(man["left_out_by_rule"]) == {"inverse", "one_line", "range"}


def test_model_equals_the_golden_bit_for_bit():
    man, z = golden()
    for i, c in enumerate(man["files"]["cdf53_i16.npz"]["cases"]):
        cur = z["in_%d" % i]
        assert cur.dtype == np.int16 and cur.shape == (c["rows"], c["columns"])
        for l in range(c["levels"]):
            want = z["out_%d_%d" % (i, l)]
            got = M.core_inv(cur) if c["kind"] == "inverse" else M.core_fwd(cur)
            assert np.array_equal(got, want), (c, l)
            cur = np.ascontiguousarray(want[0::2, 0::2])


def test_mallat_levels_are_the_cores_levels():
    """fwd2d's multi-level Mallat result holds, level by level, what the core leaves interleaved."""
    man, z = golden()
    for i, c in enumerate(man["files"]["cdf53_i16.npz"]["cases"]):
        if c["kind"] != "forward":
            continue
        a = z["in_%d" % i].copy()
        assert M.fwd2d(a, j_max=c["levels"]) == c["levels"]
        h, w = a.shape
        for l in range(c["levels"]):
            m = M.mallat_of(z["out_%d_%d" % (i, l)])
            hd, wd = (h + 1) // 2, (w + 1) // 2
            if l + 1 == c["levels"]:
                assert np.array_equal(a[:h, :w], m), (c, l)
            else:  # the LL quarter is transformed further
                assert np.array_equal(a[:h, wd:w], m[:, wd:]) and np.array_equal(a[hd:h, :wd], m[hd:, :wd]), (c, l)
            h, w = hd, wd


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (3, 5), (64, 64), (67, 131)])
@pytest.mark.parametrize("j_max", [-1, 1, 3])
def test_inverse_restores_full_range_images(shape, j_max):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + j_max)
    img = rng.integers(-32768, 32768, size=shape).astype(np.int16)
    a = img.copy()
    j = M.fwd2d(a, j_max=j_max)
    if min(shape) > 1 and j:
        assert not np.array_equal(a, img)
    M.inv2d(a, j_max=j)
    assert np.array_equal(a, img)


@pytest.mark.parametrize("value", [32767, -32767, -32768])
def test_constants_and_checkerboard_round_trip(value):
    img = np.full((9, 14), value, np.int16)
    a = img.copy()
    M.inv2d(a, j_max=M.fwd2d(a))
    assert np.array_equal(a, img)
    yy, xx = np.mgrid[0:12, 0:10]
    cb = np.where((yy + xx) & 1, 32767, -32768).astype(np.int16)  # sums leave 16 bits
    a = cb.copy()
    M.inv2d(a, j_max=M.fwd2d(a))
    assert np.array_equal(a, cb)


def test_line_steps_are_int_arithmetic_truncated_on_store():
    """One line by the formulas, sample by sample, in Python integers: the vectorised model is that arithmetic."""
    def narrow(v):
        return ((v + 32768) & 0xFFFF) - 32768

    rng = np.random.default_rng(7)
    for n in (2, 3, 4, 7, 16):
        x = [int(v) for v in rng.integers(-32768, 32768, size=n)]
        refl = lambda i: -i if i < 0 else (2 * (n - 1) - i if i >= n else i)  # noqa: E731
        t = list(x)
        for i in range(1, n, 2):
            t[i] = narrow(t[i] - ((t[refl(i - 1)] + t[refl(i + 1)]) >> 1))
        for i in range(0, n, 2):
            t[i] = narrow(t[i] + ((t[refl(i - 1)] + t[refl(i + 1)] + 2) >> 2))
        got = M.fwd_lines(np.array([x], np.int16))
        assert [int(v) for v in got[0]] == t
        assert np.array_equal(M.inv_lines(got)[0], np.array(x))


def test_rows_first_variant_is_the_int32_oracle(oracle):
    """Where every int32 coefficient fits 16 bits, truncation never acts and the int32 path's end forms equal the reflected
    ones: the rows-first variant of the model is the narrowed dwt_cdf53_2f_i result.  This ties the formulas to the oracle."""
    rng = np.random.default_rng(53)
    for shape, j in (((32, 32), 3), ((9, 14), -1), ((67, 131), 2), ((2, 2), 1), ((3, 5), -1)):
        img = rng.integers(-2048, 2049, size=shape).astype(np.int16)
        want = img.astype(np.int32)
        jw = oracle.fwd("cdf53_2f_i", want, j)
        assert np.abs(want).max() < 32768
        a = img.copy()
        assert M.fwd2d(a, j_max=j, rows_first=True) == jw
        assert np.array_equal(a.astype(np.int32), want), shape
        M.inv2d(a, j_max=jw, rows_first=True)
        assert np.array_equal(a, img)


def test_column_first_order_differs_from_the_int32_order(oracle):
    """With integer rounding the two orders are different transforms: this documents the order."""
    rng = np.random.default_rng(32)
    img = rng.integers(-4096, 4097, size=(32, 32)).astype(np.int16)
    want = img.astype(np.int32)
    oracle.fwd("cdf53_2f_i", want, 1)
    a = img.copy()
    M.fwd2d(a, j_max=1)
    differ = int((a.astype(np.int32) != want).sum())
    assert 0 < differ < a.size


def test_headers_declare_the_interface():
    h = open(os.path.join(ROOT, "include", "libdwt.h")).read()
    for name in ("dwt_cdf53_2f_i16", "dwt_cdf53_2i_i16", "dwt_util_load_from_pgm_i16", "dwt_util_save_to_pgm_i16",
                 "dwt_util_conv_show_i16", "dwt_util_test_image_fill2_i16"):
        assert name + "(" in h, name
    assert "DWT_HIP_CDF53_I16 = 8" in open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()


def test_python_names():
    import libdwt_amd as dwt

    assert dwt.CDF53_I16 == 8 and dwt.WAVELET_ID["cdf53_i16"] == 8
    assert dwt.FORWARD["cdf53_i16"] is dwt.dwt_cdf53_2f_i16 and dwt.INVERSE["cdf53_i16"] is dwt.dwt_cdf53_2i_i16
    for name in ("dwt_cdf53_2f_i16", "dwt_cdf53_2i_i16", "dwt_util_load_from_pgm_i16", "dwt_util_save_to_pgm_i16",
                 "dwt_util_conv_show_i16", "dwt_util_test_image_fill2_i16"):
        assert hasattr(dwt.lib, name), name


def test_host_utilities(tmp_path):
    """The int16 twins of the image utilities: pattern, view, PGM writer and reader (host C, no GPU)."""
    import ctypes as C

    import libdwt_amd as dwt

    lib = dwt.lib
    I, P = C.c_int, C.c_void_p
    lib.dwt_util_test_image_fill2_i16.argtypes = [P, I, I, I, I, I, I]
    lib.dwt_util_conv_show_i16.argtypes = [P, P, I, I, I, I]
    lib.dwt_util_save_to_pgm_i16.argtypes = [C.c_char_p, C.c_int16, P, I, I, I, I]
    lib.dwt_util_load_from_pgm_i16.argtypes = [C.c_char_p, C.c_int16, C.POINTER(P), C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I)]
    h, w = 9, 14
    a = np.zeros((h, w + 3), np.int16)  # padded pitch
    lib.dwt_util_test_image_fill2_i16(a.ctypes.data, a.strides[0], 2, w, h, 0, 2)
    yy, xx = np.mgrid[0:h, 0:w]
    assert np.array_equal(a[:, :w], ((xx ^ yy) & 0xFF).astype(np.int16)) and not a[:, w:].any()
    lib.dwt_util_test_image_fill2_i16(a.ctypes.data, a.strides[0], 2, w, h, 1, 0)
    x2 = xx >> 1
    assert np.array_equal(a[:, :w], (255 * (2 * x2 * yy) // (x2 * x2 + yy * yy + 1)).astype(np.int16))
    b = (a[:, :w] - 100).copy()
    v = np.zeros_like(b)
    lib.dwt_util_conv_show_i16(b.ctypes.data, v.ctypes.data, b.strides[0], 2, w, h)
    assert np.array_equal(v, np.abs(b))
    path = str(tmp_path / "t.pgm").encode()
    img = np.ascontiguousarray(a[:, :w])
    assert lib.dwt_util_save_to_pgm_i16(path, 255, img.ctypes.data, img.strides[0], 2, w, h) == 0
    p, sx, sy, nx, ny = P(), I(), I(), I(), I()
    assert lib.dwt_util_load_from_pgm_i16(path, 255, C.byref(p), C.byref(sx), C.byref(sy), C.byref(nx), C.byref(ny)) == 0
    assert (sy.value, nx.value, ny.value) == (2, w, h) and sx.value >= 2 * w
    rows = np.frombuffer(C.string_at(p.value, (h - 1) * sx.value + 2 * w), np.uint8)
    got = np.stack([rows[y * sx.value:y * sx.value + 2 * w].view(np.int16) for y in range(h)])
    assert np.array_equal(got, img)
    lib.dwt_util_free_image.argtypes = [C.POINTER(P)]
    lib.dwt_util_free_image(C.byref(p))
