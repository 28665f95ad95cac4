"""GPU parity of the float CDF 9/7 on IEEE binary16 storage (DWT_HIP_CDF97_H, dwt_cdf97_2f_h / _2i_h): bit for bit against
the restatement of tests/f16_model.py (the float oracle's one-level transform and numpy's rounding, level by level).
Host pointers, dense device images, padded pitches, pitches that are 2 mod 4 (the line-pass route), src != dst, the batch
entry with sentinels, the golden cases, option "generic", launch counts, dwt_hip_alloc_batch, dwt_hip_tune and the calls
that must refuse the wavelet.

Inputs: 8-bit integers, uniform [0, 1), random bit patterns over the whole finite binary16 range (subnormals included),
12-bit integers -- which overflow to Inf from level 4 on, and Inf - Inf to NaN, in the model's places -- and an 8-bit image
with +-Inf and NaN sprinkled in.  The comparison is on 16-bit patterns: identical bits wherever the model has no NaN, NaNs
at identical positions."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import f16_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WID = 9  # DWT_HIP_CDF97_H
SENT = 0x5AA5  # sentinel sample of the paddings (a finite binary16 pattern)

SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (3, 5), (9, 14), (64, 64), (67, 131), (130, 67), (257, 511), (40, 1023), (40, 1024),
          (40, 1025), (33, 2049), (515, 300)]
LEVELS = [-1, 0, 1, 2, 40]
KINDS = ("8bit", "unit", "bits", "12bit", "special")


def same16(got, want):
    """binary16 arrays: every sample that is no NaN in `want` has identical bits in `got`; NaNs sit at identical positions."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float16 and want.dtype == np.float16
    if got.shape != want.shape:
        return False
    ng, nw = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(ng, nw) and np.array_equal(got.view(np.uint16)[~nw], want.view(np.uint16)[~nw]))


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    for k, v in (("generic", 0), ("tile_pairs", 0), ("waves", 4), ("xcd_swizzle", 1), ("fuse01", 1), ("fma", 0)):
        d.set_option(k, v)
    d.dwt_util_finish()


_inputs = {}


def inputs(shape):
    """{kind: image} of the five kinds of input, deterministic per shape, computed once."""
    if shape not in _inputs:
        rng = np.random.default_rng(shape[0] * 4099 + shape[1])
        bits = rng.integers(0, 0x7C00, size=shape).astype(np.uint16) | (rng.integers(0, 2, size=shape).astype(np.uint16) << 15)
        special = rng.integers(0, 256, size=shape).astype(np.float16)
        flat = special.reshape(-1)
        for k, v in enumerate((np.inf, -np.inf, np.nan)):
            flat[rng.integers(0, flat.size, size=max(1, flat.size // 997))] = v
        out = {"8bit": rng.integers(0, 256, size=shape).astype(np.float16),
               "unit": rng.random(shape, dtype=np.float32).astype(np.float16),
               "bits": bits.view(np.float16),
               "12bit": rng.integers(0, 4096, size=shape).astype(np.float16),
               "special": special}
        for a in out.values():
            a.setflags(write=False)
        _inputs[shape] = out
    return _inputs[shape]


_want = {}


def want(shape, kind, j_max):
    """(forward result, level count, inverse of the forward result) of the model, computed once per case and shared."""
    key = (shape, kind, j_max)
    if key not in _want:
        a = inputs(shape)[kind].copy()
        j = M.fwd2d(a, j_max=j_max)
        back = a.copy()
        M.inv2d(back, j_max=j)
        a.setflags(write=False)
        back.setflags(write=False)
        _want[key] = (a, j, back)
    return _want[key]


def t2d(dwt, inverse, src, dst, stride_x, shape, j, size_i=None, decompose_one=0, zero_padding=0):
    jj = C.c_int(j)
    six, siy = size_i if size_i else (shape[1], shape[0])
    rc = dwt.lib.dwt_hip_transform2d(WID, int(inverse), src, dst, stride_x, 2, shape[1], shape[0], six, siy, C.byref(jj), decompose_one,
                                     zero_padding)
    assert rc == 0, dwt.last_error()
    return jj.value


class Padded:
    """A device image of binary16 samples with a pitch of its own; the padding holds sentinels."""

    def __init__(self, dwt, img, pitch):
        h, w = img.shape
        assert pitch >= 2 * w and pitch % 2 == 0
        self.h, self.w, self.pitch = h, w, pitch
        self.d = dwt.DeviceImage(h, w, itemsize=2, pitch_bytes=pitch)
        host = np.full((h, pitch // 2), SENT, np.uint16)
        host[:, :w] = img.view(np.uint16)
        self.d.upload(host)
        self.ptr = self.d.ptr

    def read(self):
        a = self.d.download(np.uint16)
        assert (a[:, self.w:] == SENT).all(), "pitch padding overwritten"
        return np.ascontiguousarray(a[:, :self.w]).view(np.float16)

    def free(self):
        self.d.free()


def pitches(w):
    dense = 2 * w
    padded = (dense + 3) // 4 * 4 + 64         # a multiple of 4: the fused route
    odd = dense + 2 if dense % 4 == 0 else dense + 4  # 2 mod 4: the line passes
    assert padded % 4 == 0 and odd % 4 == 2
    return dense, padded, odd


@pytest.mark.parametrize("shape", SHAPES)
def test_host_and_device_images(dwt, shape):
    """Host entry, dense device image, padded pitch, a pitch that is 2 mod 4, and src != dst: the forward equals the model
    bit for bit and the inverse of that result equals the model's inverse, with no tolerance, at every level count and for
    every kind of input."""
    h, w = shape
    for kind in KINDS:
        img = inputs(shape)[kind]
        for j_max in LEVELS:
            wf, jw, wb = want(shape, kind, j_max)
            a = img.copy()
            assert dwt.dwt_cdf97_2f_h(a, a.strides[0], 2, w, h, w, h, j_max) == jw
            assert same16(a, wf), ("host forward", kind, j_max)
            dwt.dwt_cdf97_2i_h(a, a.strides[0], 2, w, h, w, h, jw)
            assert same16(a, wb), ("host inverse", kind, j_max)
            for pitch in pitches(w):
                d = Padded(dwt, img, pitch)
                assert t2d(dwt, 0, d.ptr, d.ptr, pitch, shape, j_max) == jw
                assert same16(d.read(), wf), ("device forward", kind, j_max, pitch)
                t2d(dwt, 1, d.ptr, d.ptr, pitch, shape, jw)
                assert same16(d.read(), wb), ("device inverse", kind, j_max, pitch)
                d.free()
            if not jw:
                continue
            # src != dst (every level fused: the padded pitch)
            pitch = pitches(w)[1]
            s, d = Padded(dwt, img, pitch), Padded(dwt, np.zeros_like(img), pitch)
            assert t2d(dwt, 0, s.ptr, d.ptr, pitch, shape, j_max) == jw
            assert same16(d.read(), wf), ("out of place forward", kind, j_max)
            assert np.array_equal(s.read().view(np.uint16), img.view(np.uint16)), "source changed"
            t2d(dwt, 1, d.ptr, s.ptr, pitch, shape, jw)
            assert same16(s.read(), wb), ("out of place inverse", kind, j_max)
            assert same16(d.read(), wf), "coefficients changed"
            s.free()
            d.free()


@pytest.mark.parametrize("shape", [(2, 2), (9, 14), (67, 131), (40, 1025), (515, 300)])
def test_batch_entry_keeps_sentinels(dwt, shape):
    """batch = 3, a padded batch stride, sentinels between and after the images (and in the pitch padding) that survive."""
    h, w = shape
    batch = 3
    kinds = ("bits", "8bit", "12bit")
    imgs = [inputs(shape)[k] for k in kinds]
    for pitch in pitches(w)[1:]:  # the fused route, and the line passes image by image
        bstride = pitch * h + 128 + (pitch % 4)  # (keeps the stride's alignment class that of the pitch)
        total = bstride * batch + 64
        host = np.full(total // 2, SENT, np.uint16)
        mask = np.zeros(total // 2, bool)
        for b, im in enumerate(imgs):
            for y in range(h):
                o = (b * bstride + y * pitch) // 2
                host[o:o + w] = im[y].view(np.uint16)
                mask[o:o + w] = True
        src = dwt.DeviceImage(1, total // 2, itemsize=2).upload(host)
        dst = dwt.DeviceImage(1, total // 2, itemsize=2).upload(np.full(total // 2, SENT, np.uint16))
        for j_max in (-1, 2):
            jw = dwt.transform2d_batch(WID, 0, src.ptr, dst.ptr, bstride, batch, pitch, w, h, j_max)
            got = dst.download(np.uint16)[0]
            for b, kind in enumerate(kinds):
                wf, jm, _ = want(shape, kind, j_max)
                assert jm == jw
                rows = np.stack([got[(b * bstride + y * pitch) // 2:][:w] for y in range(h)]).view(np.float16)
                assert same16(rows, wf), ("batch forward", b, j_max, pitch)
            assert (got[~mask] == SENT).all(), "sentinels of the destination overwritten"
            assert np.array_equal(src.download(np.uint16)[0], host), "source batch changed"
            back = dwt.DeviceImage(1, total // 2, itemsize=2).upload(np.full(total // 2, SENT, np.uint16))
            dwt.transform2d_batch(WID, 1, dst.ptr, back.ptr, bstride, batch, pitch, w, h, jw)
            gb = back.download(np.uint16)[0]
            for b, kind in enumerate(kinds):
                rows = np.stack([gb[(b * bstride + y * pitch) // 2:][:w] for y in range(h)]).view(np.float16)
                assert same16(rows, want(shape, kind, j_max)[2]), ("batch inverse", b, j_max, pitch)
            assert (gb[~mask] == SENT).all(), "sentinels of the inverse's destination overwritten"
            back.free()
        src.free()
        dst.free()


def test_golden_cases(dwt):
    """The reference's one-level transforms with numpy's rounding (scripts/gen_h16_golden.py) through the GPU: sparse frames,
    zero_padding and decompose_one included."""
    with open(os.path.join(ROOT, "tests", "golden", "cdf97_h_manifest.json")) as f:
        cases = json.load(f)["files"]["cdf97_h.npz"]["cases"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "cdf97_h.npz"))
    for i, c in enumerate(cases):
        so, si = tuple(c["size_o"]), tuple(c["size_i"])
        a = z["in_%d" % i].view(np.float16).copy()
        j = dwt.dwt_cdf97_2f_h(a, a.strides[0], 2, so[0], so[1], si[0], si[1], c["j_max"], c["decompose_one"], c["zero_padding"])
        assert j == c["levels"] and same16(a, z["fwd_%d" % i].view(np.float16)), ("forward", c)
        dwt.dwt_cdf97_2i_h(a, a.strides[0], 2, so[0], so[1], si[0], si[1], j, c["decompose_one"], c["zero_padding"])
        assert same16(a, z["inv_%d" % i].view(np.float16)), ("inverse", c)


@pytest.mark.parametrize("shape", [(64, 64), (130, 68), (257, 512), (40, 1026), (67, 131)])
def test_generic_option_gives_the_fused_bits(dwt, shape):
    """The line passes (binary32 copy of the level's frame, Cdf97S with the reference's end forms, one rounding) and the fused
    sweeps (reflected line ends) give the same bits, which are the model's."""
    h, w = shape
    for kind in ("bits", "12bit", "special"):
        img = inputs(shape)[kind]
        wf, jw, wb = want(shape, kind, -1)
        src, dst = Padded(dwt, img, 2 * w), Padded(dwt, np.zeros_like(img), 2 * w)
        res = []
        try:
            for generic in (0, 1):
                dwt.set_option("generic", generic)
                assert t2d(dwt, 0, src.ptr, dst.ptr, 2 * w, shape, -1) == jw  # out of place
                res.append(dst.read().copy())
                t2d(dwt, 1, dst.ptr, dst.ptr, 2 * w, shape, jw)  # in place
                assert same16(dst.read(), wb), (kind, generic)
        finally:
            dwt.set_option("generic", 0)
        assert same16(res[0], wf) and same16(res[1], wf), kind
        nn = ~np.isnan(wf)
        assert np.array_equal(res[0].view(np.uint16)[nn], res[1].view(np.uint16)[nn])
        src.free()
        dst.free()


@pytest.mark.parametrize("shape", [(515, 300), (130, 2049), (67, 131)])
def test_tile_variants_agree(dwt, shape):
    """Every tile height, wave count and block order gives the model's bits (left alone the launcher picks 2 row pairs per
    tile for images of this size; option "tile_pairs" forces the taller tiles, 64 and 128 pairs one tile taller than the
    image).  Forward out of place, inverse in place, dense and padded pitch, sentinels kept."""
    h, w = shape
    try:
        for tp in (2, 4, 8, 64, 128):
            for waves in (1, 4):
                for swz in (0, 1):
                    for k, v in (("tile_pairs", tp), ("waves", waves), ("xcd_swizzle", swz)):
                        dwt.set_option(k, v)
                    kind = "bits" if (tp + waves + swz) & 1 else "8bit"
                    img = inputs(shape)[kind]
                    wf, jw, wb = want(shape, kind, -1)
                    for pitch in pitches(w)[:2]:
                        src, dst = Padded(dwt, img, pitch), Padded(dwt, np.zeros_like(img), pitch)
                        assert t2d(dwt, 0, src.ptr, dst.ptr, pitch, shape, -1) == jw
                        assert same16(dst.read(), wf), ("forward", tp, waves, swz, kind, pitch)
                        t2d(dwt, 1, dst.ptr, dst.ptr, pitch, shape, jw)
                        assert same16(dst.read(), wb), ("inverse", tp, waves, swz, kind, pitch)
                        src.free()
                        dst.free()
    finally:
        for k, v in (("tile_pairs", 0), ("waves", 4), ("xcd_swizzle", 1)):
            dwt.set_option(k, v)


def test_one_launch_per_level(dwt):
    """A dense 4-byte-aligned 256 x 512 device image at J = 3: stat_launches grows by exactly J, forward and inverse."""
    shape = (256, 512)
    img = inputs(shape)["8bit"]
    wf, jw, wb = want(shape, "8bit", 3)
    assert jw == 3
    src, dst = Padded(dwt, img, 1024), Padded(dwt, np.zeros_like(img), 1024)
    n0 = dwt.get_option("stat_launches")
    assert t2d(dwt, 0, src.ptr, dst.ptr, 1024, shape, 3) == jw
    assert dwt.get_option("stat_launches") - n0 == jw
    assert same16(dst.read(), wf)
    n0 = dwt.get_option("stat_launches")
    t2d(dwt, 1, dst.ptr, src.ptr, 1024, shape, jw)
    assert dwt.get_option("stat_launches") - n0 == jw
    assert same16(src.read(), wb)
    src.free()
    dst.free()


def test_options_fma_and_fuse01_do_not_apply(dwt):
    shape = (128, 128)
    img = inputs(shape)["8bit"]
    wf, jw, wb = want(shape, "8bit", 3)
    try:
        dwt.set_option("fuse01", 2)
        dwt.set_option("fma", 1)
        a, b = Padded(dwt, img, 256), Padded(dwt, np.zeros_like(img), 256)
        n0 = dwt.get_option("stat_launches")
        assert t2d(dwt, 0, a.ptr, b.ptr, 256, shape, 3) == jw and same16(b.read(), wf)
        assert dwt.get_option("stat_launches") - n0 == jw
        t2d(dwt, 1, b.ptr, a.ptr, 256, shape, jw)
        assert same16(a.read(), wb)
        a.free()
        b.free()
    finally:
        dwt.set_option("fuse01", 1)
        dwt.set_option("fma", 0)


def test_calls_that_refuse_the_wavelet(dwt):
    """Every entry that takes a wavelet id, but transform2d, transform2d_batch, alloc_batch and tune, refuses the wavelet and
    leaves the data alone -- the 1-D, interleaved, sharded, multi-device and SWT entries, the SWT's feature and one-level
    entries among them; so does a batch of 65536.  (The 2-D feature, band, N-term and EAW entries take float images and no
    wavelet id: there is nothing to pass them.)"""
    h, w, pitch = 64, 64, 256
    sent = np.full((h, pitch // 2), SENT, np.uint16)
    d = dwt.DeviceImage(h, w, itemsize=2, pitch_bytes=pitch).upload(sent)
    o = dwt.DeviceImage(4 * h, w, itemsize=2, pitch_bytes=pitch).upload(np.tile(sent, (4, 1)))
    j = C.c_int(-1)
    lib = dwt.lib
    assert lib.dwt_hip_transform1d_batch(WID, 0, d.ptr, d.ptr, pitch, 4, h, w, w, C.byref(j), 0) != 0
    assert lib.dwt_hip_transform1d(WID, 0, d.ptr, d.ptr, 4, w, w, C.byref(j), 0) != 0
    with pytest.raises(dwt.DwtError):
        dwt.transform2d_interleaved(WID, 0, 0, d.ptr, d.ptr, pitch, 4, w, h)
    with pytest.raises(dwt.DwtError):
        dwt.transform2d_batch_sharded(WID, 0, d.ptr, o.ptr, pitch * h, 1, pitch, w, h, -1, [0])
    with pytest.raises(dwt.DwtError):
        dwt.transform2d_batch_multi(WID, 0, [d.ptr], [o.ptr], [1], [0], pitch * h, pitch, w, h)
    with pytest.raises(dwt.DwtError):
        dwt.tune_batch_multi(WID, 0, [d.ptr], [o.ptr], [1], [0], pitch * h, pitch, w, h)
    with pytest.raises(dwt.DwtError):
        dwt.swt1d_batch(WID, d.ptr, pitch, 4, h, w // 2, 2, o.ptr, None, 0, pitch * h, pitch)
    fv = np.full(h * 2, -7.0, np.float32)
    assert lib.dwt_hip_swt_features1d_batch(WID, 1, d.ptr, pitch, 4, h, w // 2, 2, 0, 2.0, fv.ctypes.data, 2) != 0
    assert lib.dwt_hip_swt1d_level(WID, d.ptr, o.ptr, o.ptr, w // 2, 4, 0) != 0
    assert (fv == -7.0).all()
    with pytest.raises(dwt.DwtError):
        dwt.swt2d_batch(WID, d.ptr, pitch * h, 1, pitch, 4, w // 2, h, 1, o.ptr)
    with pytest.raises(dwt.DwtError):
        dwt.swt2d_level(WID, d.ptr, pitch, 4, w // 2, h, 0, o.ptr, o.ptr, o.ptr, o.ptr, pitch)
    with pytest.raises(dwt.DwtError):
        dwt.transform2d_batch(WID, 0, d.ptr, o.ptr, 0, 65536, pitch, w, h, 1)
    with pytest.raises(dwt.DwtError):
        dwt.tune(WID, 0, d.ptr, o.ptr, 0, 65536, pitch, w, h, 1)
    assert (d.download(np.uint16) == SENT).all() and (o.download(np.uint16) == SENT).all()
    d.free()
    o.free()


@pytest.mark.parametrize("shape", [(67, 130), (130, 67)])
def test_alloc_batch(dwt, shape):
    """Buffers of 2 * W * H bytes per image, dense: a batch laid out so transforms to the model's bits, the last image to its
    last sample."""
    h, w = shape
    n = 3
    kinds = ("bits", "8bit", "12bit")
    src, dst = dwt.alloc_batch("cdf97_h", n, w, h, -1)
    host = np.stack([inputs(shape)[k] for k in kinds])
    img_bytes = 2 * w * h
    dwt._check(dwt.lib.dwt_hip_memcpy_h2d(src, host.ctypes.data, n * img_bytes), "h2d")
    jw = dwt.transform2d_batch("cdf97_h", 0, src, dst, img_bytes, n, 2 * w, w, h, -1)
    got = np.empty_like(host)
    dwt._check(dwt.lib.dwt_hip_memcpy_d2h(got.ctypes.data, dst, n * img_bytes), "d2h")
    for b, kind in enumerate(kinds):
        wf, jm, _ = want(shape, kind, -1)
        assert jm == jw and same16(got[b], wf), b
    dwt.transform2d_batch("cdf97_h", 1, dst, src, img_bytes, n, 2 * w, w, h, jw)
    dwt._check(dwt.lib.dwt_hip_memcpy_d2h(got.ctypes.data, src, n * img_bytes), "d2h")
    for b, kind in enumerate(kinds):
        assert same16(got[b], want(shape, kind, -1)[2]), b
    dwt.lib.dwt_hip_free(src)
    dwt.lib.dwt_hip_free(dst)


def test_tune_accepts_the_wavelet(dwt):
    shape = (130, 68)
    h, w = shape
    img = inputs(shape)["8bit"]
    wf, jw, _ = want(shape, "8bit", -1)
    src, dst = Padded(dwt, img, 2 * w), Padded(dwt, np.zeros_like(img), 2 * w)
    dwt.tune("cdf97_h", 0, src.ptr, dst.ptr, 2 * w * h, 1, 2 * w, w, h, -1)
    assert same16(dst.read(), wf)
    src.free()
    dst.free()


def test_strided_device_image(dwt):
    """One channel of an interleaved three-channel binary16 image: only that channel's samples are written."""
    h, w = 37, 53
    rng = np.random.default_rng(3)
    pix = rng.integers(0, 256, size=(h, w, 3)).astype(np.float16)
    d = dwt.DeviceImage(h, 3 * w, itemsize=2).upload(pix.reshape(h, 3 * w).view(np.uint16))
    jj = C.c_int(2)
    rc = dwt.lib.dwt_hip_transform2d(WID, 0, d.ptr + 2, d.ptr + 2, 6 * w, 6, w, h, w, h, C.byref(jj), 0, 0)
    assert rc == 0, dwt.last_error()
    got = d.download(np.uint16).view(np.float16).reshape(h, w, 3)
    a = np.ascontiguousarray(pix[:, :, 1])
    M.fwd2d(a, j_max=2)
    assert same16(np.ascontiguousarray(got[:, :, 1]), a)
    assert np.array_equal(got[:, :, 0], pix[:, :, 0]) and np.array_equal(got[:, :, 2], pix[:, :, 2])
    d.free()


def test_sparse_frame_and_decompose_one(dwt):
    """size_i != size_o with and without zero_padding, and decompose_one on shapes with a short side: the exact line passes,
    geometry as dwt_cdf97_2f_s."""
    so, si = (40, 50), (29, 37)
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=so).astype(np.float16)
    for zp in (0, 1):
        a = img.copy()
        M.fwd2d(a, size_i=(si[1], si[0]), j_max=3, zero_padding=zp)
        g = img.copy()
        assert dwt.dwt_cdf97_2f_h(g, g.strides[0], 2, so[1], so[0], si[1], si[0], 3, 0, zp) == 3
        assert same16(g, a), zp
        M.inv2d(a, size_i=(si[1], si[0]), j_max=3, zero_padding=zp)
        dwt.dwt_cdf97_2i_h(g, g.strides[0], 2, so[1], so[0], si[1], si[0], 3, 0, zp)
        assert same16(g, a), zp
    for shape in ((1, 37), (37, 1), (5, 70), (67, 9)):
        h, w = shape
        img = inputs((67, 131))["8bit"][:h, :w].copy()
        a = img.copy()
        jw = M.fwd2d(a, j_max=-1, decompose_one=1)
        g = img.copy()
        assert dwt.dwt_cdf97_2f_h(g, g.strides[0], 2, w, h, w, h, -1, 1, 0) == jw and same16(g, a), shape
        d = Padded(dwt, img, pitches(w)[1])
        assert t2d(dwt, 0, d.ptr, d.ptr, d.pitch, shape, -1, decompose_one=1) == jw and same16(d.read(), a), shape
        M.inv2d(a, j_max=jw, decompose_one=1)
        t2d(dwt, 1, d.ptr, d.ptr, d.pitch, shape, jw, decompose_one=1)
        assert same16(d.read(), a), shape
        d.free()


def test_c_example(dwt, tmp_path):
    """examples/half97.c: fill, convert, forward and inverse on a resident binary16 image, convert back, from C."""
    import subprocess

    exe = tmp_path / "half97"
    libdir = os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "half97.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "round trip: maximum error" in out.stderr
