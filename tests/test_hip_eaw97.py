"""GPU parity of the edge-avoiding 9/7 transforms (dwt_eaw97_2f_s / _2i_s, dwt_hip_eaw97_2d / _batch): bit for bit
against the fixtures of tests/golden/eaw97.npz where a case is in them, otherwise against the restatement of
tests/eaw97_model.py (which tests/test_eaw97.py pins to those fixtures).  Host and device pointers, byte pitches, one
channel of interleaved data, sparse frames, the whole float range, the fused one-launch-per-level path against the
two-pass route, batches, other alphas, and the two tolerances the fixture's manifest records."""
import ctypes as C
import warnings

import numpy as np
import pytest

import eaw97_model as M
from conftest import full_range_floats, same_floats
from hipdev import Dev

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

PAIRS = [(-1, 0), (-1, 1), (0, 0), (1, 0), (3, 1), (40, 0)]
HOST_SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (2, 3), (3, 5), (4, 5), (65, 67), (130, 257)]


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("eaw_two_pass", 0)
    d.dwt_util_finish()


@pytest.fixture(scope="module")
def golden():
    return M.load_golden()


def expect_fwd(img, **kw):
    a = np.ascontiguousarray(img, dtype=np.float32).copy()
    j, wH, wV = M.mallat_fwd(a, **kw)
    return a, j, wH, wV


def expect_inv(coef, wH, wV, **kw):
    a = np.ascontiguousarray(coef, dtype=np.float32).copy()
    M.mallat_inv(a, [np.nan_to_num(w) for w in wH], [np.nan_to_num(w) for w in wV], **kw)
    return a


def weights_ok(got, want):
    return len(got) == len(want) and all(M.same_weights(g, w) for g, w in zip(got, want))


def to_device(arr):
    import libdwt_amd as d

    return Dev(d, arr)


@pytest.mark.parametrize("where", ["host", "device"])
def test_fixture_cases_bit_exact(dwt, golden, where):
    """Every fixture case at alpha 1 and 0, forward and inverse, against the reference's recorded results."""
    n = 0
    for c in golden:
        if c["alpha"] not in (0.0, 1.0):
            continue
        h, w = c["img"].shape
        siy, six = c["size_i"] or (h, w)
        d = c["img"].copy() if where == "host" else to_device(c["img"])
        p = d.ctypes.data if where == "host" else d.ptr
        j, wH, wV = dwt.dwt_eaw97_2f_s(p, w * 4, 4, w, h, six, siy, c["j_max"], c["d1"], c["zp"], alpha=c["alpha"])
        got = d if where == "host" else d.get()
        assert j == c["j"] and same_floats(got, c["out"]), (n, c["img"].shape)
        assert weights_ok(wH, c["wH"]) and weights_ok(wV, c["wV"]), n
        dwt.dwt_eaw97_2i_s(p, w * 4, 4, w, h, six, siy, j, c["d1"], c["zp"], wH, wV)
        assert same_floats(d if where == "host" else d.get(), c["back"]), n
        n += 1
    assert n == len(golden) - 2


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("j_max,decompose_one", PAIRS)
def test_host_bit_exact(dwt, shape, j_max, decompose_one):
    h, w = shape
    img = np.random.default_rng(h * 7919 + w).random((h, w), dtype=np.float32) * 8 - 4
    want, jw, wHw, wVw = expect_fwd(img, j_max=j_max, decompose_one=decompose_one)
    got = img.copy()
    jg, wH, wV = dwt.dwt_eaw97_2f_s(got, w * 4, 4, w, h, w, h, j_max, decompose_one, 0)
    assert jg == jw
    assert same_floats(got, want)
    assert weights_ok(wH, wHw) and weights_ok(wV, wVw)
    dwt.dwt_eaw97_2i_s(got, w * 4, 4, w, h, w, h, jg, decompose_one, 0, wH, wV)
    assert same_floats(got, expect_inv(want, wHw, wVw, j_max=jw, decompose_one=decompose_one))


@pytest.mark.parametrize("shape", [(3, 5), (65, 67), (130, 257), (511, 513), (1080, 1920)], ids=lambda s: "%dx%d" % s)
def test_device_bit_exact(dwt, shape):
    h, w = shape
    img = np.random.default_rng(w).random((h, w), dtype=np.float32)
    want, jw, wHw, wVw = expect_fwd(img, j_max=5)
    d = to_device(img)
    jg, wH, wV = dwt.dwt_eaw97_2f_s(d.ptr, w * 4, 4, w, h, w, h, 5, 0, 0)
    assert jg == jw and same_floats(d.get(), want)
    assert weights_ok(wH, wHw) and weights_ok(wV, wVw)
    dwt.dwt_eaw97_2i_s(d.ptr, w * 4, 4, w, h, w, h, jg, 0, 0, wH, wV)
    assert same_floats(d.get(), expect_inv(want, wHw, wVw, j_max=jw))


SEAM_SIDES = [63, 64, 65, 66, 127, 129]


@pytest.mark.parametrize("w", SEAM_SIDES)
@pytest.mark.parametrize("h", SEAM_SIDES)
def test_tile_seam_bit_exact(dwt, h, w):
    """The last column and row on every place relative to the end of a 64-wide tile and its halo (4 samples before, 3
    after; the inverse 3 and 4), at level 0 and, with 32 .. 65 samples, at level 1: the fused tiles and the line route."""
    img = np.random.default_rng(h * 131 + w).random((h, w), dtype=np.float32)
    want, jw, wHw, wVw = expect_fwd(img, j_max=2)
    back = expect_inv(want, wHw, wVw, j_max=jw)
    for two_pass in (0, 1):
        dwt.set_option("eaw_two_pass", two_pass)
        try:
            d = to_device(img)
            jg, wH, wV = dwt.dwt_eaw97_2f_s(d.ptr, w * 4, 4, w, h, w, h, 2, 0, 0)
            assert jg == jw and same_floats(d.get(), want), two_pass
            assert weights_ok(wH, wHw) and weights_ok(wV, wVw), two_pass
            dwt.dwt_eaw97_2i_s(d.ptr, w * 4, 4, w, h, w, h, jg, 0, 0, wH, wV)
            assert same_floats(d.get(), back), two_pass
        finally:
            dwt.set_option("eaw_two_pass", 0)


@pytest.mark.parametrize("where", ["host", "device"])
def test_prime_pitch(dwt, where):
    """Rows 2053 bytes apart: every float is unaligned in all rows but one in four."""
    h, w, pitch = 67, 300, 2053
    img = np.random.default_rng(5).random((h, w), dtype=np.float32)
    buf = np.full(pitch * h + 16, 0xA5, dtype=np.uint8)
    for y in range(h):
        buf[y * pitch:y * pitch + 4 * w] = img[y].view(np.uint8)
    want, jw, wHw, wVw = expect_fwd(img, j_max=3)
    if where == "device":
        d = to_device(buf)
        jg, wH, wV = dwt.dwt_eaw97_2f_s(d.ptr, pitch, 4, w, h, w, h, 3, 0, 0)
        out = d.get()
    else:
        out = buf.copy()
        jg, wH, wV = dwt.dwt_eaw97_2f_s(out.ctypes.data, pitch, 4, w, h, w, h, 3, 0, 0)
    got = np.stack([out[y * pitch:y * pitch + 4 * w].view(np.float32) for y in range(h)])
    assert jg == jw and same_floats(got, want) and weights_ok(wH, wHw) and weights_ok(wV, wVw)
    pad = np.concatenate([out[y * pitch + 4 * w:(y + 1) * pitch] for y in range(h)])
    assert (pad == 0xA5).all(), "bytes between the rows were written"


@pytest.mark.parametrize("where", ["host", "device"])
def test_one_channel_of_three(dwt, where):
    h, w = 97, 130
    rgb = np.random.default_rng(9).random((h, w, 3), dtype=np.float32)
    want, jw, wHw, wVw = expect_fwd(rgb[:, :, 1], j_max=-1)
    if where == "device":
        d = to_device(rgb)
        jg, wH, wV = dwt.dwt_eaw97_2f_s(d.ptr + 4, w * 12, 12, w, h, w, h, -1, 0, 0)
        out = d.get()
    else:
        out = rgb.copy()
        jg, wH, wV = dwt.dwt_eaw97_2f_s(out.ctypes.data + 4, w * 12, 12, w, h, w, h, -1, 0, 0)
    assert jg == jw and same_floats(out[:, :, 1], want) and weights_ok(wH, wHw) and weights_ok(wV, wVw)
    assert np.array_equal(out[:, :, 0], rgb[:, :, 0]) and np.array_equal(out[:, :, 2], rgb[:, :, 2])


@pytest.mark.parametrize("zero_padding", [0, 1])
def test_sparse_frame(dwt, zero_padding):
    img = np.random.default_rng(2).random((90, 120), dtype=np.float32)
    kw = dict(size_i=(61, 77), j_max=3, zero_padding=zero_padding)
    want, jw, wHw, wVw = expect_fwd(img, **kw)
    got = img.copy()
    jg, wH, wV = dwt.dwt_eaw97_2f_s(got, 480, 4, 120, 90, 77, 61, 3, 0, zero_padding)
    assert jg == jw and same_floats(got, want) and weights_ok(wH, wHw) and weights_ok(wV, wVw)
    dwt.dwt_eaw97_2i_s(got, 480, 4, 120, 90, 77, 61, jg, 0, zero_padding, wH, wV)
    assert same_floats(got, expect_inv(want, wHw, wVw, **kw))


@pytest.mark.parametrize("klass", ["subnormal", "tiny", "huge", "mixed"])
@pytest.mark.parametrize("two_pass", [0, 1])
def test_full_float_range(dwt, klass, two_pass):
    h, w = 130, 257
    img = full_range_floats(np.random.default_rng(3), (h, w), klass=klass)
    want, jw, wHw, wVw = expect_fwd(img, j_max=3)
    d = to_device(img)
    dwt.set_option("eaw_two_pass", two_pass)
    try:
        jg, wH, wV = dwt.dwt_eaw97_2f_s(d.ptr, w * 4, 4, w, h, w, h, 3, 0, 0)
        assert jg == jw and same_floats(d.get(), want)
        # no line of this frame has one sample, so every weight is written: NaN weights (a difference of infinities)
        # must be NaN on the device too, every other weight has the model's bits
        assert all(b.shape[1] > 1 and same_floats(a, b) for a, b in zip(wH + wV, wHw + wVw))
        dwt.dwt_eaw97_2i_s(d.ptr, w * 4, 4, w, h, w, h, jg, 0, 0, wH, wV)
        assert same_floats(d.get(), expect_inv(want, wHw, wVw, j_max=jw))
    finally:
        dwt.set_option("eaw_two_pass", 0)


@pytest.mark.parametrize("shape", [(511, 513), (1080, 1920), (1024, 1)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("decompose_one", [0, 1])
def test_fused_equals_two_pass(dwt, shape, decompose_one):
    h, w = shape
    img = np.random.default_rng(11).random((h, w), dtype=np.float32)
    res = []
    for two in (0, 1):
        dwt.set_option("eaw_two_pass", two)
        try:
            d = to_device(img)
            j, wH, wV = dwt.dwt_eaw97_2f_s(d.ptr, w * 4, 4, w, h, w, h, -1, decompose_one, 0, alpha=0.8)
            f = d.get()
            dwt.dwt_eaw97_2i_s(d.ptr, w * 4, 4, w, h, w, h, j, decompose_one, 0, wH, wV)
            res.append((j, f, wH, wV, d.get()))
        finally:
            dwt.set_option("eaw_two_pass", 0)
    (j0, f0, h0, v0, i0), (j1, f1, h1, v1, i1) = res
    assert j0 == j1 and same_floats(f0, f1) and same_floats(i0, i1)
    assert all(M.same_weights(a, np.where(M.written(b), b, np.nan)) for a, b in zip(h0 + v0, h1 + v1))


def test_dense_device_call_makes_one_launch_per_level(dwt):
    h, w, J = 1000, 1500, 5
    d = to_device(np.random.default_rng(1).random((h, w), dtype=np.float32))
    total, _, _ = dwt.eaw53_weights_layout(dwt.EAW_MALLAT, w, h, w, h, J)
    wb = to_device(np.zeros(total, dtype=np.float32))
    j = C.c_int(J)
    n0 = dwt.get_option("stat_launches")
    assert dwt.lib.dwt_hip_eaw97_2d(0, d.ptr, w * 4, 4, w, h, w, h, C.byref(j), 0, 0, wb.ptr, 1.0) == 0
    assert dwt.get_option("stat_launches") - n0 == J
    n0 = dwt.get_option("stat_launches")
    assert dwt.lib.dwt_hip_eaw97_2d(1, d.ptr, w * 4, 4, w, h, w, h, C.byref(j), 0, 0, wb.ptr, 1.0) == 0
    assert dwt.get_option("stat_launches") - n0 == J


@pytest.mark.parametrize("where", ["device", "host"])
def test_batch_equals_single(dwt, where):
    B, h, w, J = 5, 200, 333, 4
    imgs = np.random.default_rng(4).random((B, h, w), dtype=np.float32)
    total, _, _ = dwt.eaw53_weights_layout(dwt.EAW_MALLAT, w, h, w, h, J)
    ws = total + 7
    if where == "device":
        d, wb = to_device(imgs), to_device(np.zeros(B * ws, dtype=np.float32))
    else:
        d, wb = imgs.copy(), np.zeros(B * ws, dtype=np.float32)
    assert dwt.eaw97_2d_batch(0, d, h * w * 4, B, w * 4, w, h, wb, ws, J, alpha=0.8) == J
    got = d.get() if where == "device" else d.copy()
    gw = wb.get() if where == "device" else wb
    singles = []
    for b in range(B):
        one = imgs[b].copy()
        j, wH, wV = dwt.dwt_eaw97_2f_s(one, w * 4, 4, w, h, w, h, J, 0, 0, alpha=0.8)
        assert same_floats(got[b], one)
        flat = np.concatenate([a.reshape(-1) for k in range(J) for a in (wH[k], wV[k])])
        assert same_floats(gw[b * ws:b * ws + total], flat)
        dwt.dwt_eaw97_2i_s(one, w * 4, 4, w, h, w, h, J, 0, 0, wH, wV)
        singles.append(one)
    dwt.eaw97_2d_batch(1, d, h * w * 4, B, w * 4, w, h, wb, ws, J)
    back = d.get() if where == "device" else d
    assert same_floats(back, np.stack(singles))


@pytest.mark.parametrize("alpha", [0.3, 0.8, 2.0])
def test_inverse_exact_for_any_alpha(dwt, alpha):
    """The inverse takes the weights as input: exact for every alpha, fed forwards computed by the model."""
    h, w = 301, 457
    img = np.random.default_rng(6).random((h, w), dtype=np.float32)
    coef, j, wH, wV = expect_fwd(img, j_max=4, alpha=alpha)
    want = expect_inv(coef, wH, wV, j_max=j)
    for where in ("host", "device"):
        d = coef.copy() if where == "host" else to_device(coef)
        dwt.dwt_eaw97_2i_s(d if where == "host" else d.ptr, w * 4, 4, w, h, w, h, j, 0, 0,
                           [np.nan_to_num(a) for a in wH], [np.nan_to_num(a) for a in wV])
        assert same_floats(d if where == "host" else d.get(), want), where


def test_alpha_08_forward_within_tolerance(dwt, golden):
    """alpha 0.8 on the device against the reference's coefficients of the fixture: within 4 x alpha_dev_model of the
    largest coefficient.  alpha_dev_model is what pow in double rounded once (the model, numpy) differs from glibc's
    powf by on these cases; the factor 4 is for the device's double pow rounding a rare value the other way from
    numpy's, and for later levels amplifying a one-ulp weight change.  The level-0 wH comes from the input itself:
    pow within 1 ulp, then + 1e-5 and 1 / x each rounded once -- within 2 ulp."""
    bound = 4 * M.load_manifest()["alpha_dev_model"]
    n = 0
    for c in golden:
        if c["alpha"] in (0.0, 1.0):
            continue
        h, w = c["img"].shape
        d = to_device(c["img"])
        j, wH, wV = dwt.dwt_eaw97_2f_s(d.ptr, w * 4, 4, w, h, w, h, c["j_max"], c["d1"], c["zp"], alpha=c["alpha"])
        assert j == c["j"]
        ulp = np.abs(wH[0].view(np.int32).astype(np.int64) - c["wH"][0].view(np.int32).astype(np.int64))
        dev = np.abs(d.get().astype(np.float64) - c["out"].astype(np.float64)).max() / np.abs(c["out"]).max()
        print("alpha", c["alpha"], c["img"].shape, "wH[0] ulp", ulp.max(), "coefficients", dev, "bound", bound)
        assert ulp.max() <= 2
        assert dev <= bound
        n += 1
    assert n == 2


@pytest.mark.parametrize("alpha", [1.0, 0.8])
def test_round_trip(dwt, alpha):
    """Within twice the reference's own round-trip error on the fixture cases, relative to max|input| (the manifest's
    roundtrip_ref), on inputs of the fixture's range [-4, 4)."""
    bound = 2 * M.load_manifest()["roundtrip_ref"]
    h, w = 777, 1025
    img = np.random.default_rng(13).random((h, w), dtype=np.float32) * 8 - 4
    d = to_device(img)
    j, wH, wV = dwt.dwt_eaw97_2f_s(d.ptr, w * 4, 4, w, h, w, h, -1, 1, 0, alpha=alpha)
    dwt.dwt_eaw97_2i_s(d.ptr, w * 4, 4, w, h, w, h, j, 1, 0, wH, wV)
    err = np.abs(d.get().astype(np.float64) - img).max() / np.abs(img).max()
    print("alpha", alpha, "levels", j, "round trip", err, "bound", bound)
    assert err <= bound
