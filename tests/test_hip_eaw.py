"""GPU parity of the edge-avoiding 5/3 transforms (dwt_eaw53_2f_s / _2i_s, the interleaved _inplace_s pair,
dwt_hip_eaw53_2d / _batch): bit for bit against the compiled reference where it was built, otherwise against the
restatement of tests/eaw_model.py (which tests/test_eaw.py pins to the reference).  Host and device pointers, byte
pitches, one channel of interleaved data, the whole float range, the fused one-launch-per-level path against the
two-pass route, batches, other alphas and an HDR-style detail edit."""
import ctypes as C
import warnings

import numpy as np
import pytest

import eaw_model as M
from conftest import full_range_floats, same_floats
from hipdev import Dev

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (3, 5), (37, 1000), (511, 513), (1080, 1920)]


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
def ref():
    return M.RefEaw() if M.have_ref() else None


def expect_fwd(ref, img, interleaved=False, **kw):
    """(coefficients, j, wH, wV) of the forward on a copy of img: the reference where built, else the restatement."""
    a = np.ascontiguousarray(img, dtype=np.float32).copy()
    if ref is not None:
        j, wH, wV = ref.fwd(a, interleaved=interleaved, **kw)
    else:
        kw.pop("zero_padding", None) if interleaved else None
        j, wH, wV = (M.interleaved_fwd if interleaved else M.mallat_fwd)(a, **kw)
    return a, j, wH, wV


def expect_inv(ref, coef, wH, wV, interleaved=False, **kw):
    a = np.ascontiguousarray(coef, dtype=np.float32).copy()
    if ref is not None:
        ref.inv(a, wH, wV, interleaved=interleaved, **kw)
    else:
        kw.pop("zero_padding", None) if interleaved else None
        (M.interleaved_inv if interleaved else M.mallat_inv)(a, wH, wV, **kw)
    return a


def fwd_fn(dwt, interleaved):
    return dwt.dwt_eaw53_2f_inplace_s if interleaved else dwt.dwt_eaw53_2f_s


def inv_fn(dwt, interleaved):
    return dwt.dwt_eaw53_2i_inplace_s if interleaved else dwt.dwt_eaw53_2i_s


def weights_ok(got, want):
    return len(got) == len(want) and all(M.same_weights(g, w) for g, w in zip(got, want))


def to_device(arr):
    import libdwt_amd as d

    return Dev(d, arr)


@pytest.mark.parametrize("interleaved", [False, True], ids=["mallat", "interleaved"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("j_max,decompose_one", [(-1, 0), (-1, 1), (0, 0), (1, 0), (3, 1), (40, 0)])
def test_host_bit_exact(dwt, ref, shape, interleaved, j_max, decompose_one):
    h, w = shape
    img = np.random.default_rng(h * 7919 + w).random((h, w), dtype=np.float32) * 8 - 4
    want, jw, wHw, wVw = expect_fwd(ref, img, interleaved, j_max=j_max, decompose_one=decompose_one)
    got = img.copy()
    jg, wH, wV = fwd_fn(dwt, interleaved)(got, w * 4, 4, w, h, w, h, j_max, decompose_one, 0)
    assert jg == jw
    assert same_floats(got, want)
    assert weights_ok(wH, wHw) and weights_ok(wV, wVw)
    inv_fn(dwt, interleaved)(got, w * 4, 4, w, h, w, h, jg, decompose_one, 0, wH, wV)
    assert same_floats(got, expect_inv(ref, want, wHw, wVw, interleaved, j_max=jw, decompose_one=decompose_one))


@pytest.mark.parametrize("interleaved", [False, True], ids=["mallat", "interleaved"])
@pytest.mark.parametrize("shape", [(1, 37), (3, 5), (511, 513), (1080, 1920), (4096, 4096)], ids=lambda s: "%dx%d" % s)
def test_device_bit_exact(dwt, ref, shape, interleaved):
    h, w = shape
    img = np.random.default_rng(w).random((h, w), dtype=np.float32)
    want, jw, wHw, wVw = expect_fwd(ref, img, interleaved, j_max=5)
    d = to_device(img)
    jg, wH, wV = fwd_fn(dwt, interleaved)(d.ptr, w * 4, 4, w, h, w, h, 5, 0, 0)
    assert jg == jw and same_floats(d.get(), want)
    assert weights_ok(wH, wHw) and weights_ok(wV, wVw)
    inv_fn(dwt, interleaved)(d.ptr, w * 4, 4, w, h, w, h, jg, 0, 0, wH, wV)
    assert same_floats(d.get(), expect_inv(ref, want, wHw, wVw, interleaved, j_max=jw))


SEAM_SIDES = [63, 64, 65, 66, 127, 129]


@pytest.mark.parametrize("w", SEAM_SIDES)
@pytest.mark.parametrize("h", SEAM_SIDES)
def test_tile_seam_bit_exact(dwt, ref, h, w):
    """The last column and row on every place relative to the end of a 64-wide tile and its halo (2 samples before, 1
    after; the inverse 1 and 2), at level 0 and, with 32 .. 65 samples, at level 1: the fused tiles and the line route."""
    img = np.random.default_rng(h * 131 + w).random((h, w), dtype=np.float32)
    want, jw, wHw, wVw = expect_fwd(ref, img, j_max=2)
    back = expect_inv(ref, want, wHw, wVw, j_max=jw)
    for two_pass in (0, 1):
        dwt.set_option("eaw_two_pass", two_pass)
        try:
            d = to_device(img)
            jg, wH, wV = dwt.dwt_eaw53_2f_s(d.ptr, w * 4, 4, w, h, w, h, 2, 0, 0)
            assert jg == jw and same_floats(d.get(), want), two_pass
            assert weights_ok(wH, wHw) and weights_ok(wV, wVw), two_pass
            dwt.dwt_eaw53_2i_s(d.ptr, w * 4, 4, w, h, w, h, jg, 0, 0, wH, wV)
            assert same_floats(d.get(), back), two_pass
        finally:
            dwt.set_option("eaw_two_pass", 0)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["mallat", "interleaved"])
def test_prime_pitch(dwt, ref, where, interleaved):
    """Rows 2053 bytes apart: every float is unaligned in all rows but one in four."""
    h, w, pitch = 67, 300, 2053
    img = np.random.default_rng(5).random((h, w), dtype=np.float32)
    buf = np.full(pitch * h + 16, 0xA5, dtype=np.uint8)
    for y in range(h):
        buf[y * pitch:y * pitch + 4 * w] = img[y].view(np.uint8)
    want, jw, wHw, wVw = expect_fwd(ref, img, interleaved, j_max=3)
    if where == "device":
        d = to_device(buf)
        jg, wH, wV = fwd_fn(dwt, interleaved)(d.ptr, pitch, 4, w, h, w, h, 3, 0, 0)
        out = d.get()
    else:
        out = buf.copy()
        jg, wH, wV = fwd_fn(dwt, interleaved)(out.ctypes.data, pitch, 4, w, h, w, h, 3, 0, 0)
    got = np.stack([out[y * pitch:y * pitch + 4 * w].view(np.float32) for y in range(h)])
    assert jg == jw and same_floats(got, want) and weights_ok(wH, wHw) and weights_ok(wV, wVw)
    pad = np.concatenate([out[y * pitch + 4 * w:(y + 1) * pitch] for y in range(h)])
    assert (pad == 0xA5).all(), "bytes between the rows were written"


@pytest.mark.parametrize("where", ["host", "device"])
def test_one_channel_of_three(dwt, ref, where):
    h, w = 97, 130
    rgb = np.random.default_rng(9).random((h, w, 3), dtype=np.float32)
    want, jw, wHw, wVw = expect_fwd(ref, rgb[:, :, 1], j_max=-1)
    if where == "device":
        d = to_device(rgb)
        jg, wH, wV = dwt.dwt_eaw53_2f_s(d.ptr + 4, w * 12, 12, w, h, w, h, -1, 0, 0)
        out = d.get()
    else:
        out = rgb.copy()
        jg, wH, wV = dwt.dwt_eaw53_2f_s(out.ctypes.data + 4, w * 12, 12, w, h, w, h, -1, 0, 0)
    assert jg == jw and same_floats(out[:, :, 1], want) and weights_ok(wH, wHw) and weights_ok(wV, wVw)
    assert np.array_equal(out[:, :, 0], rgb[:, :, 0]) and np.array_equal(out[:, :, 2], rgb[:, :, 2])


@pytest.mark.parametrize("klass", ["subnormal", "tiny", "huge", "mixed"])
@pytest.mark.parametrize("two_pass", [0, 1])
def test_full_float_range(dwt, ref, klass, two_pass):
    h, w = 130, 257
    img = full_range_floats(np.random.default_rng(3), (h, w), klass=klass)
    want, jw, wHw, wVw = expect_fwd(ref, img, j_max=3)
    d = to_device(img)
    dwt.set_option("eaw_two_pass", two_pass)
    try:
        jg, wH, wV = dwt.dwt_eaw53_2f_s(d.ptr, w * 4, 4, w, h, w, h, 3, 0, 0)
        assert jg == jw and same_floats(d.get(), want)
        assert all(same_floats(np.where(np.isnan(b), 0, a), np.nan_to_num(b, nan=0.0)) for a, b in zip(wH + wV, wHw + wVw))
        dwt.dwt_eaw53_2i_s(d.ptr, w * 4, 4, w, h, w, h, jg, 0, 0, wH, wV)
        assert same_floats(d.get(), expect_inv(ref, want, wHw, wVw, j_max=jw))
    finally:
        dwt.set_option("eaw_two_pass", 0)


@pytest.mark.parametrize("zero_padding", [0, 1])
@pytest.mark.parametrize("interleaved", [False, True], ids=["mallat", "interleaved"])
def test_sparse_frame(dwt, ref, zero_padding, interleaved):
    img = np.random.default_rng(2).random((90, 120), dtype=np.float32)
    kw = dict(size_i=(61, 77), j_max=3, zero_padding=zero_padding)
    want, jw, wHw, wVw = expect_fwd(ref, img, interleaved, **kw)
    got = img.copy()
    jg, wH, wV = fwd_fn(dwt, interleaved)(got, 480, 4, 120, 90, 77, 61, 3, 0, zero_padding)
    assert jg == jw and same_floats(got, want) and weights_ok(wH, wHw) and weights_ok(wV, wVw)
    inv_fn(dwt, interleaved)(got, 480, 4, 120, 90, 77, 61, jg, 0, zero_padding, wH, wV)
    assert same_floats(got, expect_inv(ref, want, wHw, wVw, interleaved, **kw))


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
            j, wH, wV = dwt.dwt_eaw53_2f_s(d.ptr, w * 4, 4, w, h, w, h, -1, decompose_one, 0, alpha=0.8)
            f = d.get()
            dwt.dwt_eaw53_2i_s(d.ptr, w * 4, 4, w, h, w, h, j, decompose_one, 0, wH, wV)
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
    assert dwt.lib.dwt_hip_eaw53_2d(0, 0, d.ptr, w * 4, 4, w, h, w, h, C.byref(j), 0, 0, wb.ptr, 1.0) == 0
    assert dwt.get_option("stat_launches") - n0 == J
    n0 = dwt.get_option("stat_launches")
    assert dwt.lib.dwt_hip_eaw53_2d(1, 0, d.ptr, w * 4, 4, w, h, w, h, C.byref(j), 0, 0, wb.ptr, 1.0) == 0
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
    assert dwt.eaw53_2d_batch(0, d, h * w * 4, B, w * 4, w, h, wb, ws, J, alpha=0.8) == J
    got = d.get() if where == "device" else d
    gw = wb.get() if where == "device" else wb
    for b in range(B):
        one = imgs[b].copy()
        j, wH, wV = dwt.dwt_eaw53_2f_s(one, w * 4, 4, w, h, w, h, J, 0, 0, alpha=0.8)
        assert same_floats(got[b], one)
        flat = np.concatenate([a.reshape(-1) for k in range(J) for a in (wH[k], wV[k])])
        assert same_floats(gw[b * ws:b * ws + total], flat)
    dwt.eaw53_2d_batch(1, d, h * w * 4, B, w * 4, w, h, wb, ws, J)
    back = d.get() if where == "device" else d
    assert np.abs(back - imgs).max() <= 1e-5 * np.abs(imgs).max()


@pytest.mark.parametrize("alpha", [0.3, 0.8, 2.0])
def test_inverse_exact_for_any_alpha(dwt, ref, alpha):
    """The inverse takes the weights as input: exact for every alpha, fed the reference's own forward."""
    h, w = 301, 457
    img = np.random.default_rng(6).random((h, w), dtype=np.float32)
    coef, j, wH, wV = expect_fwd(ref, img, j_max=4, alpha=alpha)
    want = expect_inv(ref, coef, wH, wV, j_max=j)
    for where in ("host", "device"):
        d = coef.copy() if where == "host" else to_device(coef)
        dwt.dwt_eaw53_2i_s(d if where == "host" else d.ptr, w * 4, 4, w, h, w, h, j, 0, 0,
                           [np.nan_to_num(a) for a in wH], [np.nan_to_num(a) for a in wV])
        assert same_floats(d if where == "host" else d.get(), want), where


def test_alpha_08_forward_within_tolerance(dwt, ref):
    """alpha 0.8: |d|^alpha in double rounded once to float against glibc's powf (within 1 ulp of each other), then
    + 1e-5 and 1 / x, each rounded: the weights of the input's own rows (level 0, horizontal) are within 2 ulp.  Every
    later weight is computed from coefficients that already differ by a few ulp, so only its statistics are pinned.
    Coefficients: within 1e-5 of the largest one (a weight error of 2^-22 moves a weighted average by at most that
    share of its neighbours' spread; ten passes of that stay far inside 1e-5)."""
    h, w = 512, 640
    img = np.random.default_rng(8).random((h, w), dtype=np.float32) * 100
    want, jw, wHw, wVw = expect_fwd(ref, img, j_max=5, alpha=0.8)
    d = to_device(img)
    jg, wH, wV = dwt.dwt_eaw53_2f_s(d.ptr, w * 4, 4, w, h, w, h, 5, 0, 0, alpha=0.8)
    assert jg == jw
    ulp = np.abs(wH[0].view(np.int32).astype(np.int64) - wHw[0].view(np.int32).astype(np.int64))
    assert ulp.max() <= 2
    for g, r in zip(wH[1:] + wV, wHw[1:] + wVw):
        m = ~np.isnan(r) & (r != 0)  # (each line's last weight is 0)
        rel = np.abs(g[m] - r[m]) / r[m]
        assert np.median(rel) <= 1e-6 and np.mean(rel > 1e-3) <= 1e-3, (np.median(rel), np.mean(rel > 1e-3), rel.max())
    got = d.get()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("where", ["host", "device"])
def test_hdr_detail_edit(dwt, ref, where):
    """The reference's tone-mapping pattern at alpha 1: forward, halve every detail subband, inverse."""
    h, w, J = 480, 640, 4
    img = np.log1p(np.random.default_rng(12).random((h, w), dtype=np.float32) * 1000).astype(np.float32)
    coef, jw, wHw, wVw = expect_fwd(ref, img, j_max=J)

    def halve(a):
        a = a.copy()
        keep = a[:(h + (1 << J) - 1) >> J, :(w + (1 << J) - 1) >> J].copy()
        a *= np.float32(0.5)
        a[:keep.shape[0], :keep.shape[1]] = keep
        return a
    want = expect_inv(ref, halve(coef), wHw, wVw, j_max=jw)
    d = img.copy() if where == "host" else to_device(img)
    p = d.ctypes.data if where == "host" else d.ptr
    j, wH, wV = dwt.dwt_eaw53_2f_s(p, w * 4, 4, w, h, w, h, J, 0, 0)
    c = d if where == "host" else d.get()
    c = halve(c)
    d = c if where == "host" else to_device(c)
    p = d.ctypes.data if where == "host" else d.ptr
    dwt.dwt_eaw53_2i_s(p, w * 4, 4, w, h, w, h, j, 0, 0, wH, wV)
    assert same_floats(d if where == "host" else d.get(), want)


@pytest.mark.parametrize("alpha", [1.0, 0.8])
def test_round_trip(dwt, alpha):
    h, w = 777, 1025
    img = np.random.default_rng(13).random((h, w), dtype=np.float32) + 0.5
    d = to_device(img)
    j, wH, wV = dwt.dwt_eaw53_2f_s(d.ptr, w * 4, 4, w, h, w, h, -1, 1, 0, alpha=alpha)
    dwt.dwt_eaw53_2i_s(d.ptr, w * 4, 4, w, h, w, h, j, 1, 0, wH, wV)
    assert np.abs(d.get() - img).max() <= 1e-5 * np.abs(img).max()
