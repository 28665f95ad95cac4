"""CPU checks of the edge-avoiding 9/7 feature: the numpy restatement of tests/eaw97_model.py pinned bit for bit to the
fixtures of tests/golden/eaw97.npz (made from libdwt's own dwt_eaw97_2f_s / _2i_s by scripts/gen_eaw97_golden.py) --
coefficients, every weight the reference writes and the inverse's output; the manifest's checksum and its two measured
tolerances; the exported entries; the drop-in header in a C99 translation unit."""
import hashlib
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import eaw97_model as M

warnings.filterwarnings("ignore", category=RuntimeWarning)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = M.load_golden()
MANIFEST = M.load_manifest()


def same_bits(a, b):
    """equal bits, NaNs at the same places (their payloads are the platform's choice)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def test_fixture_holds_the_cases_of_the_model():
    assert len(CASES) == len(M.CASES)
    for c, (shape, si, j_max, d1, zp, alpha, kind) in zip(CASES, M.CASES):
        assert c["img"].shape == shape and c["size_i"] == si and (c["j_max"], c["d1"], c["zp"], c["kind"]) == (j_max, d1, zp, kind)
        assert c["alpha"] == np.float32(alpha)
        assert c["j"] == M.levels(False, shape[1], shape[0], j_max, d1)


@pytest.mark.parametrize("n", range(len(CASES)))
def test_model_matches_fixture(n):
    """Forward at alpha 1 and 0 (coefficients and weights), inverse at every alpha (it takes the weights as input)."""
    c = CASES[n]
    kw = dict(size_i=c["size_i"], j_max=c["j_max"], decompose_one=c["d1"], zero_padding=c["zp"])
    if c["alpha"] in (0.0, 1.0):
        a = c["img"].copy()
        j, wH, wV = M.mallat_fwd(a, alpha=c["alpha"], **kw)
        assert j == c["j"]
        assert same_bits(a, c["out"])
        assert all(M.same_weights(g, w) for g, w in zip(wH + wV, c["wH"] + c["wV"]))
    back = c["out"].copy()
    kw["j_max"] = c["j"]
    M.mallat_inv(back, [np.nan_to_num(w) for w in c["wH"]], [np.nan_to_num(w) for w in c["wV"]], **kw)
    assert same_bits(back, c["back"])


def test_manifest_checksum():
    with open(M.GOLDEN, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == MANIFEST["files"]["eaw97.npz"]["sha256"]
    assert len(MANIFEST["files"]["eaw97.npz"]["cases"]) == len(CASES)


def test_alpha_08_forward_deviation_is_the_recorded_one():
    """alpha 0.8: the model with pow-in-double weights against the reference's powf coefficients.  The deviation,
    relative to the largest coefficient, is the base of the GPU tolerance (tests/test_hip_eaw97.py)."""
    dev = M.alpha_deviation(CASES)
    print("alpha_dev_model", dev)
    assert sum(1 for c in CASES if c["alpha"] not in (0.0, 1.0)) == 2
    assert 0 < dev == MANIFEST["alpha_dev_model"]


def test_reference_round_trip_error_is_the_recorded_one():
    dev = M.roundtrip_deviation(CASES)
    print("roundtrip_ref", dev)
    assert 0 < dev == MANIFEST["roundtrip_ref"]


EAW97_ENTRIES = ["dwt_eaw97_2f_s", "dwt_eaw97_2i_s", "dwt_hip_eaw97_2d", "dwt_hip_eaw97_2d_batch"]


def test_entries_exported_and_declared():
    if not shutil.which("nm"):
        pytest.skip("nm is not installed")
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")]).decode()
    exported = {f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] == "T"}
    headers = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("eaw-experimental.h", "libdwt_hip.h"))
    for name in EAW97_ENTRIES:
        assert name in exported, name
        assert name + "(" in headers, name


def test_python_entries_exist():
    import libdwt_amd as dwt

    for name in ("dwt_eaw97_2f_s", "dwt_eaw97_2i_s", "eaw97_2d_batch"):
        assert callable(getattr(dwt, name)), name


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "tu.c"
    src.write_text('#include "eaw-experimental.h"\n#include "libdwt.h"\n'
                   "void f(void *p, float **h, float **v) { int j = -1; dwt_eaw97_2f_s(p, 16, 4, 4, 4, 4, 4, &j, 0, 0, h, v, 1.f);\n"
                   " dwt_eaw97_2i_s(p, 16, 4, 4, 4, 4, 4, j, 0, 0, h, v); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "tu.o")])
