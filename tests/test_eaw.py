"""CPU checks of the edge-avoiding 5/3 (EAW) feature: the numpy restatement of tests/eaw_model.py pinned bit for bit to
libdwt's own dwt_eaw53_* (oracle/_ref/libdwt_ref.so where it was built, the fixtures of tests/golden/eaw53.npz -- made
from it by scripts/gen_eaw_golden.py -- everywhere), coefficients and every weight the reference writes, forward and
inverse; the level clamp of dwt_eaw53_2f_dummy_s; the exported entries and the weight buffer layout."""
import ctypes as C
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import eaw_model as M

warnings.filterwarnings("ignore", category=RuntimeWarning)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eaw53.npz")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def restated(img, size_i, j_max, d1, zp, alpha, il):
    a = img.copy()
    if il:
        j, wH, wV = M.interleaved_fwd(a, size_i=size_i, j_max=j_max, decompose_one=d1, alpha=alpha)
    else:
        j, wH, wV = M.mallat_fwd(a, size_i=size_i, j_max=j_max, decompose_one=d1, zero_padding=zp, alpha=alpha)
    return a, j, wH, wV


def restated_inv(coef, wH, wV, size_i, j, d1, zp, il):
    a = coef.copy()
    if il:
        M.interleaved_inv(a, wH, wV, size_i=size_i, j_max=j, decompose_one=d1)
    else:
        M.mallat_inv(a, wH, wV, size_i=size_i, j_max=j, decompose_one=d1, zero_padding=zp)
    return a


def _golden():
    z = np.load(GOLDEN)
    n = 0
    cases = []
    while "c%d_meta" % n in z:
        h, w, siy, six, j_max, d1, zp, il, j = (int(v) for v in z["c%d_meta" % n])
        cases.append(dict(img=z["c%d_in" % n], out=z["c%d_out" % n], size_i=None if siy < 0 else (siy, six), j_max=j_max, d1=d1,
                          zp=zp, il=bool(il), j=j, alpha=float(z["c%d_alpha" % n]),
                          wH=[z["c%d_wH%d" % (n, k)] for k in range(j)], wV=[z["c%d_wV%d" % (n, k)] for k in range(j)]))
        n += 1
    return cases


GOLDEN_CASES = _golden()


@pytest.mark.parametrize("n", range(len(GOLDEN_CASES)))
def test_restatement_matches_golden(n):
    c = GOLDEN_CASES[n]
    coef, j, wH, wV = restated(c["img"], c["size_i"], c["j_max"], c["d1"], c["zp"], c["alpha"], c["il"])
    assert j == c["j"]
    assert bits_equal(coef, c["out"])
    assert all(M.same_weights(g, w) for g, w in zip(wH + wV, c["wH"] + c["wV"]))
    # the inverse with the reference's weights (the unwritten entries are never read)
    wHr = [np.nan_to_num(a) for a in c["wH"]]
    wVr = [np.nan_to_num(a) for a in c["wV"]]
    back = restated_inv(c["out"], wHr, wVr, c["size_i"], j, c["d1"], c["zp"], c["il"])
    assert np.all(np.isfinite(back))
    if c["size_i"] is None:
        assert np.abs(back - c["img"]).max() <= 1e-5 * max(1.0, np.abs(c["img"]).max())


LIVE = [((h, w), None, j, d1, 0) for (h, w) in [(1, 1), (1, 1000), (1000, 1), (2, 2), (3, 5), (37, 1000), (511, 513)]
        for j, d1 in [(-1, 0), (0, 0), (1, 0), (3, 1), (40, 0), (-1, 1)]]
LIVE += [((90, 120), (61, 77), 3, 0, zp) for zp in (0, 1)]


@pytest.mark.parametrize("alpha", [1.0, 0.0])
@pytest.mark.parametrize("il", [False, True], ids=["mallat", "interleaved"])
@pytest.mark.parametrize("case", LIVE, ids=lambda c: "%dx%d-si%s-j%d-d%d-zp%d" % (c[0] + (c[1] is not None, c[2], c[3], c[4])))
def test_restatement_matches_reference(case, il, alpha):
    """Against the compiled reference itself: forward coefficients and weights, then the inverse of the same data.
    Where the reference is not built, the golden fixtures (test_restatement_matches_golden) carry the pin."""
    if not M.have_ref():
        c = GOLDEN_CASES[0]
        assert bits_equal(restated(c["img"], c["size_i"], c["j_max"], c["d1"], c["zp"], c["alpha"], c["il"])[0], c["out"])
        return
    shape, si, j_max, d1, zp = case
    img = np.random.default_rng(shape[0] * 31 + shape[1]).random(shape, dtype=np.float32) * 8 - 4
    ref = M.RefEaw()
    want = img.copy()
    jw, wHw, wVw = ref.fwd(want, size_i=si, j_max=j_max, decompose_one=d1, zero_padding=zp, alpha=alpha, interleaved=il)
    coef, j, wH, wV = restated(img, si, j_max, d1, zp, alpha, il)
    assert j == jw and bits_equal(coef, want)
    assert all(M.same_weights(g, w) for g, w in zip(wH + wV, wHw + wVw))
    back = want.copy()
    ref.inv(back, wHw, wVw, size_i=si, j_max=jw, decompose_one=d1, zero_padding=zp, interleaved=il)
    assert bits_equal(restated_inv(want, [np.nan_to_num(a) for a in wHw], [np.nan_to_num(a) for a in wVw], si, jw, d1, zp, il), back)


@pytest.mark.parametrize("sox,soy", [(0, 0), (1, 1), (1024, 1), (1, 1024), (640, 480), (513, 7)])
@pytest.mark.parametrize("j_max", [-5, -1, 0, 1, 3, 9, 10, 11, 40])
@pytest.mark.parametrize("decompose_one", [0, 1])
def test_dummy_clamps_levels(sox, soy, j_max, decompose_one):
    import libdwt_amd as dwt

    got = dwt.dwt_eaw53_2f_dummy_s(None, 0, 0, sox, soy, sox, soy, j_max, decompose_one)
    assert got == M.levels(False, sox, soy, j_max, decompose_one)
    if M.have_ref():
        assert got == M.RefEaw().dummy(sox, soy, j_max, decompose_one)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("sizes", [(5, 3, 5, 3), (120, 90, 77, 61), (1, 1024, 1, 1024), (1920, 1080, 1920, 1080)])
def test_weights_layout(layout, sizes):
    """The per-level offsets and shapes of dwt_hip_eaw53_weights_layout follow the reference's allocations."""
    import libdwt_amd as dwt

    sox, soy, six, siy = sizes
    J = M.levels(False, sox, soy, -1, 1)
    total, hs, vs = dwt.eaw53_weights_layout(layout, sox, soy, six, siy, J)
    at = 0
    for k in range(J):
        cd = M.ceil_div_pow2
        want_h = (cd(soy, k), cd(six, k)) if layout == 0 else (cd(siy, k), cd(six, k))
        want_v = (cd(sox, k), cd(siy, k)) if layout == 0 else (cd(six, k), cd(siy, k))
        assert hs[k] == (at, want_h)
        at += want_h[0] * want_h[1]
        assert vs[k] == (at, want_v)
        at += want_v[0] * want_v[1]
    assert total == at
    assert dwt.lib.dwt_hip_eaw53_weights_layout(2, 4, 4, 4, 4, 1, None, None) == -1


EAW_ENTRIES = ["dwt_eaw53_2f_s", "dwt_eaw53_2i_s", "dwt_eaw53_2f_inplace_s", "dwt_eaw53_2i_inplace_s", "dwt_eaw53_2f_dummy_s",
               "dwt_util_alloc", "dwt_hip_eaw53_2d", "dwt_hip_eaw53_2d_batch", "dwt_hip_eaw53_weights_layout"]


def test_entries_exported_and_declared():
    if not shutil.which("nm"):
        pytest.skip("nm is not installed")
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")]).decode()
    exported = {f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] == "T"}
    headers = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("libdwt.h", "libdwt_hip.h"))
    for name in EAW_ENTRIES:
        assert name in exported, name
        assert name + "(" in headers, name


def test_util_alloc_is_malloc():
    import libdwt_amd as dwt

    dwt.lib.dwt_util_alloc.restype = C.c_void_p
    dwt.lib.dwt_util_alloc.argtypes = [C.c_int, C.c_size_t]
    p = dwt.lib.dwt_util_alloc(1000, 4)
    assert p
    C.memset(p, 0x5A, 4000)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(p)  # allocated with malloc: free() takes it
