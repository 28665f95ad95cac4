"""CPU-only checks of the shipped shared library: it loads, exports every symbol the
public headers declare, and its host-side helpers behave like the reference's.  No
compute entry is called here (there is no GPU in the build container)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def dwt():
    import __graft_entry__ as g

    if not os.path.exists(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")):
        g.build()
    import libdwt_amd

    return libdwt_amd


def declared_functions(header):
    text = open(os.path.join(INCLUDE, header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"enum\s+\w+\s*\{.*?\};", "", text, flags=re.S)
    # static inline helpers of volume.h are not exports
    text = re.sub(r"static\s+inline[^{;]*\{.*?\n\}", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b((?:dwt_|fdwt|volume_|cdf97_3)\w+)\s*\(", text)))


@pytest.mark.parametrize("header", ["libdwt.h", "libdwt_hip.h", "dwt-simple.h", "volume.h", "volume-dwt.h"])
def test_exports_every_declared_symbol(dwt, header):
    names = declared_functions(header)
    assert len(names) > {"dwt-simple.h": 5, "volume.h": 8, "volume-dwt.h": 15}.get(header, 15)
    if header == "volume-dwt.h":  # what the reference's 3-D perf test and its callers bind (src/volume-dwt.h:21,38,208,227,234)
        for n in ("cdf97_3f_ip_sep_horizontal_s", "cdf97_3f_op_sep_horizontal_s", "cdf97_3i_ip_sep_horizontal_s",
                  "cdf97_3f_op_wrapper_s", "volume_perftest_fwd97op_s", "volume_measure_fwd97op_s"):
            assert n in names
    if header == "volume.h":
        for n in ("volume_alloc_realiably", "volume_alloc_realiably_locked", "volume_free", "volume_fill_s", "volume_copy_s",
                  "volume_compare_s", "volume_save_to_pgm_s", "volume_save_log_to_pgm_s", "volume_invalidate_cache"):
            assert n in names
    missing = [n for n in names if not hasattr(dwt.lib, n)]
    assert not missing, missing


def test_exports_nothing_the_headers_do_not_declare(dwt):
    """Every C function the library exports is declared in a public header: no diagnosis entry or
    internal helper leaks out as a plain C symbol (C++ mangled names are not the C-ABI)."""
    if not shutil.which("nm"):
        pytest.skip("nm is not installed")
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")]).decode()
    exported = {f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] in ("T", "W") and not f[2].startswith("_Z")}
    declared = set()
    for header in os.listdir(INCLUDE):
        if header.endswith(".h"):
            declared.update(declared_functions(header))
    assert len(exported) > 100
    undeclared = sorted(exported - declared)
    assert not undeclared, undeclared


def test_exports_every_function_the_opencv_wrapper_calls(dwt):
    """src/cvdwt.cpp (the reference's OpenCV wrapper) cannot be built here
    (no OpenCV); every libdwt function it calls must be exported and declared, so that it links
    against this library unchanged.  The list is a fixture (oracle/gen_cvdwt_symbols.py)."""
    import json

    with open(os.path.join(ROOT, "tests", "golden", "cvdwt_symbols.json")) as f:
        calls = json.load(f)["calls"]
    assert len(calls) >= 17 and "dwt_cdf97_2f_s" in calls and "dwt_util_subband" in calls
    declared = set(declared_functions("libdwt.h"))
    assert not [n for n in calls if not hasattr(dwt.lib, n)], "not exported"
    assert not [n for n in calls if n not in declared], "not declared in include/libdwt.h"
    src = "/root/reference/src/cvdwt.cpp"
    if os.path.exists(src):  # in the build container the fixture is re-derived from the wrapper itself
        import importlib.util

        spec = importlib.util.spec_from_file_location("gen_cvdwt_symbols", os.path.join(ROOT, "oracle", "gen_cvdwt_symbols.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert mod.called_functions(open(src).read()) == calls


def test_headers_compile_as_c99_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "libdwt.h"\n#include "libdwt_hip.h"\n#include "dwt-simple.h"\n#include "volume.h"\n#include "volume-dwt.h"\n'
                   'int main(void){int j=-1;struct volume_t v;v.data=0;(void)j;(void)v;return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")])
    subprocess.check_call(["g++", "-x", "c++", "-std=c++11", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t2.o")])


def test_product_never_references_the_oracle():
    """The product path must not route through oracle/ (tier rule 3)."""
    pkg = os.path.join(ROOT, "libdwt_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".c", ".h", ".hip", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oraclelib" not in text and "dwt_oracle" not in text and "libdwt_ref" not in text, f
    out = subprocess.check_output(["ldd", os.path.join(pkg, "libdwt_hip.so")]).decode()
    assert "oracle" not in out and "libdwt_ref" not in out


def test_transform_fails_loudly_without_gpu(dwt):
    if dwt.device_count() > 0:
        pytest.skip("a GPU is present")
    img = np.zeros((16, 16), np.float32)
    with pytest.raises(dwt.DwtError) as e:
        dwt.dwt_cdf97_2f_s(img, 64, 4, 16, 16, 16, 16, -1)
    assert "no CPU fallback" in str(e.value) or "HIP" in str(e.value)
    assert not img.any()  # nothing was computed behind our back


def test_strides_match_reference(dwt, reference):
    for n in [1, 2, 3, 64, 2048, 2052, 32768, 4 * 1000, 340, 341 * 4, 561 * 4 + 1]:
        assert dwt.lib.dwt_util_get_opt_stride(n) == reference.lib.dwt_util_get_opt_stride(n), n
        for opt in range(9):
            assert dwt.lib.dwt_util_get_stride(n, opt) == reference.lib.dwt_util_get_stride(n, opt), (n, opt)
    assert dwt.lib.dwt_util_get_opt_stride(2048) == 2053  # examples/simple: 512 floats


def test_test_images_and_compare(dwt, oracle):
    a = np.zeros((37, 41), np.float32)
    b = np.zeros((37, 41), np.float32)
    dwt.lib.dwt_util_test_image_fill_s(a.ctypes.data, a.strides[0], 4, 41, 37, 0)
    oracle.fill_s(b)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ai = np.zeros((37, 41), np.int32)
    bi = np.zeros((37, 41), np.int32)
    dwt.lib.dwt_util_test_image_fill_i(ai.ctypes.data, ai.strides[0], 4, 41, 37, 1)
    oracle.fill_i(bi, 1)
    assert np.array_equal(ai, bi)
    # compare: float eps 1e-3 absolute, NaN/Inf => differ; int exact
    c = a.copy()
    assert dwt.lib.dwt_util_compare_s(a.ctypes.data, c.ctypes.data, a.strides[0], 4, 41, 37) == 0
    c[3, 4] += 5e-4
    assert dwt.lib.dwt_util_compare_s(a.ctypes.data, c.ctypes.data, a.strides[0], 4, 41, 37) == 0
    c[3, 4] += 1e-2
    assert dwt.lib.dwt_util_compare_s(a.ctypes.data, c.ctypes.data, a.strides[0], 4, 41, 37) == 1
    c = a.copy()
    c[0, 0] = np.nan
    assert dwt.lib.dwt_util_compare_s(c.ctypes.data, c.ctypes.data, a.strides[0], 4, 41, 37) == 1
    ci = ai.copy()
    assert dwt.lib.dwt_util_compare_i(ai.ctypes.data, ci.ctypes.data, ai.strides[0], 4, 41, 37) == 0
    ci[36, 40] += 1
    assert dwt.lib.dwt_util_compare_i(ai.ctypes.data, ci.ctypes.data, ai.strides[0], 4, 41, 37) == 1


def test_conv_show_copy_pgm(dwt, tmp_path):
    a = (np.arange(12, dtype=np.float32).reshape(3, 4) - 5) / 4
    out = np.zeros_like(a)
    dwt.lib.dwt_util_conv_show_s(a.ctypes.data, out.ctypes.data, 16, 4, 4, 3)
    want = (np.log(1.0 + np.abs(a).astype(np.float32) * np.float32(100.0)).astype(np.float32) / np.float32(10)).astype(np.float32)
    assert np.allclose(out, want, rtol=1e-6)
    i = np.array([[-3, 4], [0, -7]], np.int32)
    oi = np.zeros_like(i)
    dwt.lib.dwt_util_conv_show_i(i.ctypes.data, oi.ctypes.data, 8, 4, 2, 2)
    assert np.array_equal(oi, np.abs(i))
    cp = np.zeros_like(a)
    dwt.lib.dwt_util_copy_s(a.ctypes.data, cp.ctypes.data, 16, 4, 4, 3)
    assert np.array_equal(cp, a)
    p = tmp_path / "x.pgm"
    img = np.array([[0.0, 0.5], [1.0, 0.25]], np.float32)
    assert dwt.lib.dwt_util_save_to_pgm_s(str(p).encode(), 1.0, img.ctypes.data, 8, 4, 2, 2) == 0
    toks = p.read_text().split()
    assert toks[:4] == ["P2", "2", "2", "255"] and [int(t) for t in toks[4:]] == [0, 127, 255, 63]


def test_reference_examples_link_unchanged(dwt, tmp_path):
    """The reference's own programs around the path -- examples/simple, simple-int,
    simple-perf, subbands, perf-plot, simple-newapi, simple-double and the self-test `test` -- compile against include/*.h and link against
    libdwt_hip.so without modification."""
    ref = "/root/reference/examples"
    if not os.path.isdir(ref):
        pytest.skip("reference sources not present on this machine")
    libdir = os.path.join(ROOT, "libdwt_amd")
    import glob

    for ex in ("simple", "simple-int", "simple-perf", "subbands", "perf-plot", "simple-newapi", "simple-double", "test", "cdf97-test", "start",
               "load", "load-int", "subbands-int", "simple-single-loop", "simple-perf-int", "simple-perf-line"):
        exe = tmp_path / (ex + ".bin")
        src = sorted(glob.glob(os.path.join(ref, ex, "*.c")))[0]
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", INCLUDE, src,
                               "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
        assert exe.exists()


def _io_sigs(lib):
    import ctypes as C
    P, I = C.c_void_p, C.c_int
    PI = C.POINTER(I)
    lib.dwt_util_load_from_pgm_s.argtypes = [C.c_char_p, C.c_float, C.POINTER(P), PI, PI, PI, PI]
    lib.dwt_util_load_from_pgm_i.argtypes = [C.c_char_p, I, C.POINTER(P), PI, PI, PI, PI]
    lib.dwt_util_save_to_mat_s.argtypes = [C.c_char_p, P, I, I, I, I]
    lib.dwt_util_load_from_mat_s.argtypes = [C.c_char_p, C.POINTER(P), PI, PI, PI, PI]
    lib.dwt_util_load_from_mat_i.argtypes = [C.c_char_p, C.POINTER(P), PI, PI, PI, PI]
    lib.dwt_util_save_to_pgm_s.argtypes = [C.c_char_p, C.c_float, P, I, I, I, I]
    lib.dwt_util_free_image.argtypes = [C.POINTER(P)]
    for n in ("dwt_util_load_from_pgm_s", "dwt_util_load_from_pgm_i", "dwt_util_save_to_mat_s", "dwt_util_load_from_mat_s",
              "dwt_util_load_from_mat_i", "dwt_util_save_to_pgm_s"):
        getattr(lib, n).restype = I


def _load(lib, fn, path, dtype, *lead, mat=False):
    """Call a loader; returns (rc, array copy or None, (stride_x, stride_y))."""
    import ctypes as C
    ptr = C.c_void_p()
    a, b, c, d = (C.c_int() for _ in range(4))
    rc = getattr(lib, fn)(path.encode(), *lead, C.byref(ptr), C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    if rc or not ptr.value:
        return rc, None, None
    # PGM loaders: stride_x, stride_y, size_x, size_y; MAT loaders: size_x, size_y, stride_x, stride_y
    sx, sy, w, h = (c.value, d.value, a.value, b.value) if mat else (a.value, b.value, c.value, d.value)
    raw = (C.c_char * (sx * h)).from_address(ptr.value)
    buf = np.frombuffer(raw, dtype=np.uint8).copy()
    img = np.stack([np.frombuffer(buf[y * sx:y * sx + w * 4].tobytes(), dtype=dtype) for y in range(h)]) if h and w else np.zeros((h, w), dtype)
    lib.dwt_util_free_image(C.byref(ptr))
    return rc, img, (sx, sy)


def test_pgm_and_mat_io_match_reference(dwt, reference, tmp_path):
    """File IO around the path: same bytes out, same images in."""
    import ctypes as C
    _io_sigs(dwt.lib)
    _io_sigs(reference.lib)
    rng = np.random.default_rng(9)
    a = (rng.random((13, 17), dtype=np.float32) * 3 - 1).astype(np.float32)
    outs = []
    for tag, lib in (("ours", dwt.lib), ("ref", reference.lib)):
        p = str(tmp_path / f"{tag}.mat")
        assert lib.dwt_util_save_to_mat_s(p.encode(), a.ctypes.data, 17, 13, a.strides[0], 4) == 0
        outs.append(open(p, "rb").read())
    assert outs[0] == outs[1]
    mat = tmp_path / "hand.mat"
    mat.write_text("1.5,2;3\t4 5\n-1e1,+2.25,7,8\n\n9;10;11\n12,13,14\n")  # ragged rows, empty line, mixed delimiters
    mati = tmp_path / "hand_i.mat"
    mati.write_text("1,2;3\t4 5\n-10,225,7,8\n\n9;10;11\n12,13,14\n")
    pgm = tmp_path / "hand.pgm"
    pgm.write_text("P2\n# a comment\n5 3 # width height\n1000\n" + " ".join(str((i * 77) % 1001) for i in range(15)) + "\n")
    for fn, path, dt, lead, is_mat in (("dwt_util_load_from_mat_s", str(tmp_path / "ref.mat"), np.float32, (), True),
                                       ("dwt_util_load_from_mat_s", str(mat), np.float32, (), True),
                                       ("dwt_util_load_from_mat_i", str(mati), np.int32, (), True),
                                       ("dwt_util_load_from_pgm_s", str(pgm), np.float32, (C.c_float(2.5),), False),
                                       ("dwt_util_load_from_pgm_i", str(pgm), np.int32, (255,), False)):
        r0, i0, s0 = _load(dwt.lib, fn, path, dt, *lead, mat=is_mat)
        r1, i1, s1 = _load(reference.lib, fn, path, dt, *lead, mat=is_mat)
        assert r0 == r1 == 0, fn
        assert s0 == s1 and i0.shape == i1.shape, (fn, s0, s1, i0.shape, i1.shape)
        assert np.array_equal(i0.view(np.uint32), i1.view(np.uint32)), fn
    # a last line without a newline is not counted as a row (the reference writes past the image there)
    cut = tmp_path / "cut.mat"
    cut.write_text("1,2\n3,4")
    rc, img, _ = _load(dwt.lib, "dwt_util_load_from_mat_s", str(cut), np.float32, mat=True)
    assert rc == 0 and img.shape == (1, 2) and img.tolist() == [[1.0, 2.0]]
    # error codes
    bad = tmp_path / "bad.pgm"
    bad.write_text("P5\n1 1\n255\n0\n")
    assert _load(dwt.lib, "dwt_util_load_from_pgm_s", str(bad), np.float32, C.c_float(1.0))[0] == 2
    assert _load(dwt.lib, "dwt_util_load_from_pgm_s", str(tmp_path / "missing.pgm"), np.float32, C.c_float(1.0))[0] == 1
    deep = tmp_path / "deep.pgm"
    deep.write_text("P2\n1 1\n70000\n0\n")
    assert _load(dwt.lib, "dwt_util_load_from_pgm_i", str(deep), np.int32, 255)[0] == 3
    badm = tmp_path / "bad.mat"
    badm.write_text("1,2\nx,3\n")
    assert _load(dwt.lib, "dwt_util_load_from_mat_s", str(badm), np.float32, mat=True)[0] == 2


def test_dummy_driver_level_count(dwt, reference):
    """dwt_cdf53_2f_dummy_s (src/libdwt.c:16780): the level clamp every driver applies."""
    import ctypes as C
    sig = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    for lib in (dwt.lib, reference.lib):
        lib.dwt_cdf53_2f_dummy_s.argtypes = sig
        lib.dwt_cdf53_2f_dummy_s.restype = None
    for (w, h) in [(1, 1), (2, 2), (512, 300), (37, 1000), (8192, 8192)]:
        for j in (-1, 0, 3, 40):
            for d1 in (0, 1):
                a, b = C.c_int(j), C.c_int(j)
                dwt.lib.dwt_cdf53_2f_dummy_s(None, 0, 0, w, h, w, h, C.byref(a), d1)
                reference.lib.dwt_cdf53_2f_dummy_s(None, 0, 0, w, h, w, h, C.byref(b), d1)
                assert a.value == b.value


def test_fill2_patterns_match_reference(dwt, reference):
    import ctypes as C
    sig = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    for lib in (dwt.lib, reference.lib):
        for n in ("dwt_util_test_image_fill2_s", "dwt_util_test_image_fill2_i"):
            getattr(lib, n).argtypes = sig
            getattr(lib, n).restype = None
    for t in (0, 1, 2, 3):
        for rnd in (0, 2):
            a, b = np.zeros((37, 53), np.float32), np.zeros((37, 53), np.float32)
            dwt.lib.dwt_util_test_image_fill2_s(a.ctypes.data, a.strides[0], 4, 53, 37, rnd, t)
            reference.lib.dwt_util_test_image_fill2_s(b.ctypes.data, b.strides[0], 4, 53, 37, rnd, t)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t, rnd)
    for t in (0, 2):
        a, b = np.zeros((37, 53), np.int32), np.zeros((37, 53), np.int32)
        dwt.lib.dwt_util_test_image_fill2_i(a.ctypes.data, a.strides[0], 4, 53, 37, 1, t)
        reference.lib.dwt_util_test_image_fill2_i(b.ctypes.data, b.strides[0], 4, 53, 37, 1, t)
        assert np.array_equal(a, b), t


def test_volume_header_layout_matches_the_reference(tmp_path):
    """struct volume_t must have the reference's field layout (src/volume.h:14-24) -- callers fill it
    by hand -- and enum volume_approach its values (src/volume-dwt.h:210-225)."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volume-dwt.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(struct volume_t), offsetof(struct volume_t,size_x),'
                   'offsetof(struct volume_t,size_y), offsetof(struct volume_t,size_z), offsetof(struct volume_t,stride_x),'
                   'offsetof(struct volume_t,stride_y), offsetof(struct volume_t,stride_z), offsetof(struct volume_t,data),'
                   '(int)VOL_SEP_HORIZONTAL, (int)VOL_SEP_HORIZONTAL_Z, (int)VOL_LAST);return 0;}\n')
    outs = []
    incs = [INCLUDE] + (["/root/reference/src"] if os.path.exists("/root/reference/src/volume-dwt.h") else [])
    for k, inc in enumerate(incs):
        exe = tmp_path / f"layout{k}"
        subprocess.check_call(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe)])
        outs.append(subprocess.check_output([str(exe)]).decode().split())
    assert outs[0] == ["48", "0", "4", "8", "16", "24", "32", "40", "0", "12", "13"]
    assert all(o == outs[0] for o in outs)


def test_volume_housekeeping_on_host(dwt, tmp_path):
    """volume_alloc_realiably / fill / copy / compare / save on host volumes need no GPU; the fill is the
    reference's pattern (fixture generated by the reference's own volume_fill_s)."""
    L = dwt.lib
    v = L.volume_alloc_realiably(4, 21, 9, 13, 1)
    assert v.contents.size_x == 21 and v.contents.stride_x == 4
    assert v.contents.stride_y == L.dwt_util_get_stride(84, 1) and v.contents.stride_z == L.dwt_util_get_stride(v.contents.stride_y * 9, 1)
    L.volume_fill_s(v)
    raw = (C.c_uint8 * (v.contents.stride_z * 13)).from_address(v.contents.data)
    # libdwt's "optimal" strides are odd byte counts: rows are not 4-byte aligned (numpy copes)
    view = np.ndarray((13, 9, 21), np.float32, buffer=raw, strides=(v.contents.stride_z, v.contents.stride_y, 4))
    want = np.load(os.path.join(ROOT, "tests", "golden", "cdf97_3d_wide.npz"))["vol_fill_13x9x21"]
    assert np.array_equal(np.ascontiguousarray(view).view(np.uint32), want.view(np.uint32))
    w = L.volume_alloc_realiably(4, 21, 9, 13, 0)  # dense strides: a copy across different strides
    assert L.volume_copy_s(w, v) == 0 and L.volume_compare_s(v, w) == 0
    C.cast(w.contents.data, C.POINTER(C.c_float))[5] += 0.5
    assert L.volume_compare_s(v, w) != 0
    L.volume_save_to_pgm_s(v, str(tmp_path / "s%02d.pgm").encode())
    assert sorted(os.listdir(tmp_path)) == ["s%02d.pgm" % z for z in range(13)]
    # volume_save_log_to_pgm_s (src/volume.h:70): byte-identical to the reference's files where it is built
    L.volume_save_log_to_pgm_s(v, str(tmp_path / "l%02d.pgm").encode())
    assert len([f for f in os.listdir(tmp_path) if f.startswith("l")]) == 13
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libdwt_ref.so")
    if os.path.exists(ref_so):
        R = C.CDLL(ref_so)
        R.volume_save_log_to_pgm_s.argtypes = [C.c_void_p, C.c_char_p]
        R.volume_save_log_to_pgm_s(C.cast(v, C.c_void_p), str(tmp_path / "r%02d.pgm").encode())
        for z in range(13):
            assert open(tmp_path / ("l%02d.pgm" % z), "rb").read() == open(tmp_path / ("r%02d.pgm" % z), "rb").read(), z
    L.volume_free(v)
    L.volume_free(w)
