"""GPU parity of the reversible int16 CDF 5/3 in JPEG 2000 order (DWT_HIP_CDF53_I16, dwt_cdf53_2f_i16 / _2i_i16): bit for
bit against the restatement of tests/i16_model.py (which the CPU suite pins to the reference's cores).  Host pointers, dense
device images, padded pitches, pitches that are 2 mod 4 (the line-pass route), the batch entry with sentinels, the golden
cases, option "generic", launch counts, dwt_hip_alloc_batch and the calls that must refuse the wavelet.

Inputs: 12-bit random, full-range random int16, the constants +-32767 and -32768, and a checkerboard of -32768 and 32767
whose sums leave 16 bits (a packed 16-bit add would wrap before the shift)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import i16_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WID = 8  # DWT_HIP_CDF53_I16
SENT = 0x5AA5  # sentinel sample of the paddings

SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (3, 5), (9, 14), (64, 64), (67, 131), (130, 67), (257, 511), (40, 1023), (40, 1024),
          (40, 1025), (33, 2049), (515, 300)]
LEVELS = [-1, 0, 1, 2, 40]


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    for k, v in (("generic", 0), ("tile_pairs", 0), ("waves", 4), ("xcd_swizzle", 1)):
        d.set_option(k, v)
    d.dwt_util_finish()


def inputs(shape):
    """(name, image) of the four kinds of input, deterministic per shape."""
    rng = np.random.default_rng(shape[0] * 4099 + shape[1])
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    out = [("12bit", rng.integers(-2048, 2048, size=shape).astype(np.int16)),
           ("full", rng.integers(-32768, 32768, size=shape).astype(np.int16)),
           ("checker", np.where((yy + xx) & 1, 32767, -32768).astype(np.int16))]
    for v in (32767, -32767, -32768):
        out.append(("const%d" % v, np.full(shape, v, np.int16)))
    return out


_want = {}


def want(shape, name, img, j_max):
    """(forward result, level count) of the model, computed once per case and shared."""
    key = (shape, name, j_max)
    if key not in _want:
        a = img.copy()
        j = M.fwd2d(a, j_max=j_max)
        back = a.copy()
        M.inv2d(back, j_max=j)
        assert np.array_equal(back, img)  # the model's own round trip, full range included
        a.setflags(write=False)
        _want[key] = (a, j)
    return _want[key]


def t2d(dwt, inverse, src, dst, stride_x, shape, j):
    jj = C.c_int(j)
    rc = dwt.lib.dwt_hip_transform2d(WID, int(inverse), src, dst, stride_x, 2, shape[1], shape[0], shape[1], shape[0], C.byref(jj), 0, 0)
    assert rc == 0, dwt.last_error()
    return jj.value


class Padded:
    """A device image of int16 samples with a pitch of its own; the padding holds sentinels."""

    def __init__(self, dwt, img, pitch):
        h, w = img.shape
        assert pitch >= 2 * w and pitch % 2 == 0
        self.h, self.w, self.pitch = h, w, pitch
        self.d = dwt.DeviceImage(h, w, itemsize=2, pitch_bytes=pitch)
        host = np.full((h, pitch // 2), SENT, np.uint16).view(np.int16)
        host[:, :w] = img
        self.d.upload(host)
        self.ptr = self.d.ptr

    def read(self):
        a = self.d.download(np.int16)
        assert (a[:, self.w:].view(np.uint16) == SENT).all(), "pitch padding overwritten"
        return a[:, :self.w]

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
    """Host entry, dense device image, padded pitch and a pitch that is 2 mod 4: the forward equals the model bit for bit,
    the inverse restores the input bit for bit, at every level count and for every kind of input."""
    h, w = shape
    for name, img in inputs(shape):
        for j_max in LEVELS:
            if name.startswith("const") and j_max not in (-1, 1):
                continue
            wf, jw = want(shape, name, img, j_max)
            a = img.copy()
            assert dwt.dwt_cdf53_2f_i16(a, a.strides[0], 2, w, h, w, h, j_max) == jw
            assert np.array_equal(a, wf), ("host forward", name, j_max)
            dwt.dwt_cdf53_2i_i16(a, a.strides[0], 2, w, h, w, h, jw)
            assert np.array_equal(a, img), ("host inverse", name, j_max)
            for pitch in pitches(w):
                d = Padded(dwt, img, pitch)
                assert t2d(dwt, 0, d.ptr, d.ptr, pitch, shape, j_max) == jw
                assert np.array_equal(d.read(), wf), ("device forward", name, j_max, pitch)
                t2d(dwt, 1, d.ptr, d.ptr, pitch, shape, jw)
                assert np.array_equal(d.read(), img), ("device inverse", name, j_max, pitch)
                d.free()


@pytest.mark.parametrize("shape", SHAPES)
def test_batch_entry_keeps_sentinels(dwt, shape):
    """batch = 3, a padded batch stride, sentinels between and after the images (and in the pitch padding) that survive."""
    h, w = shape
    batch = 3
    ins = inputs(shape)
    imgs = [ins[1][1], ins[0][1], ins[2][1]]  # full range, 12 bit, checkerboard
    for pitch in pitches(w)[1:]:  # the fused route, and the line passes image by image
        bstride = pitch * h + 128 + (pitch % 4)  # (keeps the stride's alignment class that of the pitch)
        total = bstride * batch + 64
        host = np.full(total // 2, SENT, np.uint16).view(np.int16)
        mask = np.zeros(total // 2, bool)
        for b, im in enumerate(imgs):
            for y in range(h):
                o = (b * bstride + y * pitch) // 2
                host[o:o + w] = im[y]
                mask[o:o + w] = True
        src = dwt.DeviceImage(1, total // 2, itemsize=2).upload(host)
        dst = dwt.DeviceImage(1, total // 2, itemsize=2).upload(np.full(total // 2, SENT, np.uint16).view(np.int16))
        for j_max in (-1, 2):
            jw = dwt.transform2d_batch(WID, 0, src.ptr, dst.ptr, bstride, batch, pitch, w, h, j_max)
            got = dst.download(np.int16)[0]
            for b, im in enumerate(imgs):
                wf, jm = want(shape, ("full", "12bit", "checker")[b], im, j_max)
                assert jm == jw
                rows = np.stack([got[(b * bstride + y * pitch) // 2:][:w] for y in range(h)])
                if jw:
                    assert np.array_equal(rows, wf), ("batch forward", b, j_max, pitch)
            if jw:
                assert (got[~mask].view(np.uint16) == SENT).all(), "sentinels of the destination overwritten"
            assert np.array_equal(src.download(np.int16)[0], host), "source batch changed"
            if not jw:
                continue
            back = dwt.DeviceImage(1, total // 2, itemsize=2).upload(np.full(total // 2, SENT, np.uint16).view(np.int16))
            dwt.transform2d_batch(WID, 1, dst.ptr, back.ptr, bstride, batch, pitch, w, h, jw)
            assert np.array_equal(back.download(np.int16)[0], host), ("batch inverse", j_max, pitch)
            back.free()
        src.free()
        dst.free()


def test_golden_cases(dwt):
    """The reference's cores through the GPU: one level in Mallat order is the core's interleaved level; several levels are
    the core re-applied to the LL band; the inverse cases restore the reference's result."""
    with open(os.path.join(ROOT, "tests", "golden", "cdf53_i16_manifest.json")) as f:
        cases = json.load(f)["files"]["cdf53_i16.npz"]["cases"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "cdf53_i16.npz"))
    for i, c in enumerate(cases):
        h, w = c["rows"], c["columns"]
        if c["kind"] == "inverse":
            a = np.ascontiguousarray(M.mallat_of(z["in_%d" % i]))
            dwt.dwt_cdf53_2i_i16(a, a.strides[0], 2, w, h, w, h, 1)
            assert np.array_equal(a, z["out_%d_0" % i]), c
            continue
        a = z["in_%d" % i].copy()
        d = Padded(dwt, a, pitches(w)[1])
        assert t2d(dwt, 0, d.ptr, d.ptr, d.pitch, (h, w), c["levels"]) == c["levels"]
        got = d.read().copy()
        d.free()
        hh, ww = h, w
        for l in range(c["levels"]):
            m = M.mallat_of(z["out_%d_%d" % (i, l)])
            hd, wd = (hh + 1) // 2, (ww + 1) // 2
            if l + 1 == c["levels"]:
                assert np.array_equal(got[:hh, :ww], m), (c, l)
            else:
                assert np.array_equal(got[:hh, wd:ww], m[:, wd:]) and np.array_equal(got[hd:hh, :wd], m[hd:, :wd]), (c, l)
            hh, ww = hd, wd


@pytest.mark.parametrize("shape", [(64, 64), (130, 68), (257, 512), (40, 1026)])
def test_generic_option_gives_the_fused_bits(dwt, shape):
    h, w = shape
    name, img = inputs(shape)[1]
    wf, jw = want(shape, name, img, -1)
    src, dst = Padded(dwt, img, 2 * w), Padded(dwt, np.zeros_like(img), 2 * w)
    res = []
    for generic in (0, 1):
        dwt.set_option("generic", generic)
        n0 = dwt.get_option("stat_launches")
        assert t2d(dwt, 0, src.ptr, dst.ptr, 2 * w, shape, -1) == jw  # out of place
        res.append((dst.read().copy(), dwt.get_option("stat_launches") - n0))
        t2d(dwt, 1, dst.ptr, dst.ptr, 2 * w, shape, jw)  # in place
        assert np.array_equal(dst.read(), img), generic
    dwt.set_option("generic", 0)
    assert np.array_equal(res[0][0], wf) and np.array_equal(res[1][0], wf)
    assert res[0][1] == jw and res[1][1] == 2 * jw  # one fused launch per level; a column pass and a row pass per level
    src.free()
    dst.free()


@pytest.mark.parametrize("shape", [(515, 300), (130, 2049), (67, 131)])
def test_tile_variants_agree(dwt, shape):
    """Every tile height, wave count and block order gives the model's bits: the int16 twin of test_tile_variants_agree
    and test_double_tile_variants_agree in tests/test_hip_parity.py.  Left alone the launcher picks 2 row pairs per tile
    for calls of up to 2 Mi samples, 4 up to 8 Mi and up to 64 (forward) or 32 (inverse) beyond (i16_tile_pairs,
    dwt_sweep2d_i16.hip:181-195), so no image of this file's size ever meets the taller tiles; option "tile_pairs" forces
    them.  515 x 300: several tile rows, the last one short; 130 x 2049: three forward tiles across, an odd width;
    67 x 131: fewer than 64 rows, odd both ways.  64 and 128 pairs exceed the Hd of the smaller shapes on purpose: one
    tile taller than the image.  Forward out of place, inverse in place, dense and padded pitch, sentinels kept."""
    h, w = shape
    ins = dict(inputs(shape))
    try:
        for tp in (2, 4, 8, 64, 128):
            for waves in (1, 4):
                for swz in (0, 1):
                    for k, v in (("tile_pairs", tp), ("waves", waves), ("xcd_swizzle", swz)):
                        dwt.set_option(k, v)
                    for name in ("full", "checker"):
                        img = ins[name]
                        wf, jw = want(shape, name, img, -1)
                        for pitch in pitches(w)[:2]:
                            src, dst = Padded(dwt, img, pitch), Padded(dwt, np.zeros_like(img), pitch)
                            assert t2d(dwt, 0, src.ptr, dst.ptr, pitch, shape, -1) == jw
                            assert np.array_equal(dst.read(), wf), ("forward", tp, waves, swz, name, pitch)
                            assert np.array_equal(src.read(), img), ("source", tp, waves, swz, name, pitch)
                            t2d(dwt, 1, dst.ptr, dst.ptr, pitch, shape, jw)
                            assert np.array_equal(dst.read(), img), ("inverse", tp, waves, swz, name, pitch)
                            src.free()
                            dst.free()
    finally:
        for k, v in (("tile_pairs", 0), ("waves", 4), ("xcd_swizzle", 1)):
            dwt.set_option(k, v)


def test_one_launch_per_level(dwt):
    shape = (256, 512)
    name, img = inputs(shape)[0]
    wf, jw = want(shape, name, img, -1)
    assert jw == 8
    src, dst = Padded(dwt, img, 1024), Padded(dwt, np.zeros_like(img), 1024)
    n0 = dwt.get_option("stat_launches")
    assert t2d(dwt, 0, src.ptr, dst.ptr, 1024, shape, -1) == jw
    assert dwt.get_option("stat_launches") - n0 == jw
    assert np.array_equal(dst.read(), wf)
    n0 = dwt.get_option("stat_launches")
    t2d(dwt, 1, dst.ptr, src.ptr, 1024, shape, jw)
    assert dwt.get_option("stat_launches") - n0 == jw
    assert np.array_equal(src.read(), img)
    src.free()
    dst.free()


def test_calls_that_refuse_the_wavelet(dwt):
    """Every entry but transform2d, transform2d_batch, alloc_batch and tune refuses the wavelet and leaves the data alone."""
    h, w, pitch = 64, 64, 256
    sent = np.full((h, pitch // 2), SENT, np.uint16).view(np.int16)
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
    with pytest.raises(dwt.DwtError):
        dwt.swt2d_batch(WID, d.ptr, pitch * h, 1, pitch, 4, w // 2, h, 1, o.ptr)
    with pytest.raises(dwt.DwtError):
        dwt.swt2d_level(WID, d.ptr, pitch, 4, w // 2, h, 0, o.ptr, o.ptr, o.ptr, o.ptr, pitch)
    # "fuse01" asks for the fused pair of levels of the float 9/7: the int16 wavelet is not affected by it
    dwt.set_option("fuse01", 2)
    img = inputs((64, 64))[1][1]
    wf, jw = want((64, 64), "full", img, 3)
    a = Padded(dwt, img, pitch)
    b = Padded(dwt, np.zeros_like(img), pitch)
    assert t2d(dwt, 0, a.ptr, b.ptr, pitch, (64, 64), 3) == jw and np.array_equal(b.read(), wf)
    dwt.set_option("fuse01", 1)
    a.free()
    b.free()
    assert (d.download(np.int16).view(np.uint16) == SENT).all() and (o.download(np.int16).view(np.uint16) == SENT).all()
    d.free()
    o.free()


@pytest.mark.parametrize("shape", [(67, 130), (130, 67)])
def test_alloc_batch(dwt, shape):
    """Buffers of 2 * W * H bytes per image, dense: a batch laid out so round-trips, the last image to its last sample."""
    h, w = shape
    n = 3
    src, dst = dwt.alloc_batch("cdf53_i16", n, w, h, -1)
    ins = inputs(shape)
    host = np.stack([ins[1][1], ins[0][1], ins[2][1]])
    img_bytes = 2 * w * h
    dwt._check(dwt.lib.dwt_hip_memcpy_h2d(src, host.ctypes.data, n * img_bytes), "h2d")
    jw = dwt.transform2d_batch("cdf53_i16", 0, src, dst, img_bytes, n, 2 * w, w, h, -1)
    got = np.empty_like(host)
    dwt._check(dwt.lib.dwt_hip_memcpy_d2h(got.ctypes.data, dst, n * img_bytes), "d2h")
    for b, nm in enumerate(("full", "12bit", "checker")):
        wf, jm = want(shape, nm, host[b], -1)
        assert jm == jw and np.array_equal(got[b], wf), b
    dwt.transform2d_batch("cdf53_i16", 1, dst, src, img_bytes, n, 2 * w, w, h, jw)
    dwt._check(dwt.lib.dwt_hip_memcpy_d2h(got.ctypes.data, src, n * img_bytes), "d2h")
    assert np.array_equal(got, host)
    dwt.lib.dwt_hip_free(src)
    dwt.lib.dwt_hip_free(dst)


def test_tune_accepts_the_wavelet(dwt):
    shape = (130, 68)
    h, w = shape
    name, img = inputs(shape)[1]
    wf, jw = want(shape, name, img, -1)
    src, dst = Padded(dwt, img, 2 * w), Padded(dwt, np.zeros_like(img), 2 * w)
    dwt.tune("cdf53_i16", 0, src.ptr, dst.ptr, 2 * w * h, 1, 2 * w, w, h, -1)
    assert np.array_equal(dst.read(), wf)
    src.free()
    dst.free()


def test_strided_device_image(dwt):
    """One channel of an interleaved three-channel int16 image: only that channel's samples are written."""
    h, w = 37, 53
    rng = np.random.default_rng(3)
    pix = rng.integers(-32768, 32768, size=(h, w, 3)).astype(np.int16)
    d = dwt.DeviceImage(h, 3 * w, itemsize=2).upload(pix.reshape(h, 3 * w))
    jj = C.c_int(2)
    rc = dwt.lib.dwt_hip_transform2d(WID, 0, d.ptr + 2, d.ptr + 2, 6 * w, 6, w, h, w, h, C.byref(jj), 0, 0)
    assert rc == 0, dwt.last_error()
    got = d.download(np.int16).reshape(h, w, 3)
    a = np.ascontiguousarray(pix[:, :, 1])
    M.fwd2d(a, j_max=2)
    assert np.array_equal(got[:, :, 1], a) and np.array_equal(got[:, :, 0], pix[:, :, 0]) and np.array_equal(got[:, :, 2], pix[:, :, 2])
    d.free()


def test_sparse_frame(dwt):
    """size_i != size_o: the exact line passes, geometry as dwt_cdf53_2f_i."""
    so, si = (40, 50), (29, 37)
    rng = np.random.default_rng(11)
    img = rng.integers(-32768, 32768, size=so).astype(np.int16)
    for zp in (0, 1):
        a = img.copy()
        M.fwd2d(a, size_i=si, j_max=3, zero_padding=zp)
        g = img.copy()
        assert dwt.dwt_cdf53_2f_i16(g, g.strides[0], 2, so[1], so[0], si[1], si[0], 3, 0, zp) == 3
        assert np.array_equal(g, a), zp
        M.inv2d(a, size_i=si, j_max=3, zero_padding=zp)
        dwt.dwt_cdf53_2i_i16(g, g.strides[0], 2, so[1], so[0], si[1], si[0], 3, 0, zp)
        assert np.array_equal(g, a), zp


def test_c_example(dwt, tmp_path):
    """examples/lossless16.c: fill, forward, view, inverse, compare on the host and on a device image, from C."""
    import subprocess

    exe = tmp_path / "lossless16"
    libdir = os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lossless16.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "host round trip: success" in out.stderr and "device round trip: success" in out.stderr
