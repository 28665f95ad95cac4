"""GPU parity of the interpolating 5/3 wavelet (dwt_interp53_2f_s / _2i_s / _1f_s / _1i_s, DWT_HIP_INTERP53_S): bit for
bit against the compiled reference where it was built, otherwise against the restatement of tests/interp53_model.py
(which the CPU suite pins to the reference).  Host pointers, dense, strided and out-of-place device images, the batch
API, 1-D batches, the exact line-pass route (accel 1 / option "generic"), the whole float range, launch counts, the
C example and the calls that must refuse the wavelet."""
import ctypes as C
import os
import subprocess
import warnings

import numpy as np
import pytest

import interp53_model as M
from conftest import full_range_floats, same_floats

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WID = 6  # DWT_HIP_INTERP53_S
REF = M.RefInterp53() if os.path.exists(M.REF_SO) else None


def want2d(img, inverse, size_i=None, j_max=-1, d1=0, zp=0):
    """(expected image, level count) of the reference's call on a copy of img."""
    a = np.ascontiguousarray(img, np.float32).copy()
    impl = REF or M
    if inverse:
        (impl.inv2d)(a, size_i=size_i, j_max=j_max, decompose_one=d1, zero_padding=zp)
        return a, j_max
    return a, (impl.fwd2d)(a, size_i=size_i, j_max=j_max, decompose_one=d1, zero_padding=zp)


def want1d(x, inverse, size_i=None, j_max=-1, zp=0):
    a = np.ascontiguousarray(x, np.float32).copy()
    if REF is not None and a.shape[0] <= 64:
        impl = REF
    else:
        impl = M
    if inverse:
        impl.inv1d(a, size_i=size_i, j_max=j_max, zero_padding=zp)
        return a, j_max
    return a, impl.fwd1d(a, size_i=size_i, j_max=j_max, zero_padding=zp)


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("generic", 0)
    d.dwt_util_set_accel(0)
    d.dwt_util_finish()


def t2d(dwt, inverse, src, dst, stride_x, stride_y, so, si=None, j=-1, d1=0, zp=0):
    jj = C.c_int(j)
    siy, six = si or so
    rc = dwt.lib.dwt_hip_transform2d(WID, int(inverse), src, dst, stride_x, stride_y, so[1], so[0], six, siy, C.byref(jj), d1, zp)
    assert rc == 0, dwt.last_error()
    return jj.value


def on_device(dwt, arr):
    d = dwt.DeviceImage(arr.shape[0], arr.shape[1])
    d.upload(np.ascontiguousarray(arr, np.float32))
    return d


SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (3, 5), (9, 14), (64, 64), (67, 130), (130, 67), (256, 512), (257, 511),
          (100, 1030), (515, 300)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("j_max,d1", [(-1, 0), (-1, 1), (0, 0), (2, 1), (40, 0)])
def test_host_entries(dwt, shape, j_max, d1):
    rng = np.random.default_rng(hash((shape, j_max, d1)) & 0xFFFF)
    img = rng.random(shape, dtype=np.float32) * 8 - 4
    want, jw = want2d(img, False, j_max=j_max, d1=d1)
    a = img.copy()
    assert dwt.dwt_interp53_2f_s(a, a.strides[0], 4, shape[1], shape[0], shape[1], shape[0], j_max, d1) == jw
    assert same_floats(a, want)
    wi, _ = want2d(want, True, j_max=jw, d1=d1)
    dwt.dwt_interp53_2i_s(a, a.strides[0], 4, shape[1], shape[0], shape[1], shape[0], jw, d1)
    assert same_floats(a, wi)


@pytest.mark.parametrize("zp", [0, 1])
@pytest.mark.parametrize("d1", [0, 1])
@pytest.mark.parametrize("so,si", [((40, 50), (29, 37)), ((1, 33), (1, 20)), ((300, 260), (299, 131))])
def test_sparse_frames(dwt, so, si, zp, d1):
    rng = np.random.default_rng(5)
    img = rng.random(so, dtype=np.float32) * 8 - 4
    for where in ("host", "device"):
        want, jw = want2d(img, False, size_i=si, j_max=3, d1=d1, zp=zp)
        wi, _ = want2d(want, True, size_i=si, j_max=jw, d1=d1, zp=zp)
        if where == "host":
            a = img.copy()
            assert t2d(dwt, 0, a.ctypes.data, a.ctypes.data, a.strides[0], 4, so, si, 3, d1, zp) == jw
            assert same_floats(a, want)
            t2d(dwt, 1, a.ctypes.data, a.ctypes.data, a.strides[0], 4, so, si, jw, d1, zp)
            assert same_floats(a, wi)
        else:
            d = on_device(dwt, img)
            t2d(dwt, 0, d.ptr, d.ptr, d.stride_x, 4, so, si, 3, d1, zp)
            assert same_floats(d.download(np.float32), want)
            t2d(dwt, 1, d.ptr, d.ptr, d.stride_x, 4, so, si, jw, d1, zp)
            assert same_floats(d.download(np.float32), wi)
            d.free()


@pytest.mark.parametrize("shape", [(64, 64), (67, 130), (512, 512), (1000, 1500), (2048, 2048), (1, 4096), (4096, 3), (2, 4096)])
def test_dense_device_images_and_generic_route(dwt, shape):
    """Fused route (accel 0) and exact line passes (accel 1 and option "generic") give the reference's bits, in place and
    out of place (src != dst)."""
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    img = rng.random(shape, dtype=np.float32) * 8 - 4
    want, jw = want2d(img, False)
    wi, _ = want2d(want, True, j_max=jw)
    got = {}
    for route in ("fused", "accel1", "generic"):
        dwt.dwt_util_set_accel(1 if route == "accel1" else 0)
        dwt.set_option("generic", 1 if route == "generic" else 0)
        try:
            d = on_device(dwt, img)
            o = dwt.DeviceImage(*shape)
            assert t2d(dwt, 0, d.ptr, o.ptr, d.stride_x, 4, shape) == jw
            f = o.download(np.float32)
            t2d(dwt, 1, o.ptr, d.ptr, d.stride_x, 4, shape, None, jw)
            i_ = d.download(np.float32)
            d.upload(img)
            t2d(dwt, 0, d.ptr, d.ptr, d.stride_x, 4, shape)
            fi = d.download(np.float32)
            d.free()
            o.free()
        finally:
            dwt.dwt_util_set_accel(0)
            dwt.set_option("generic", 0)
        assert same_floats(fi, want), route
        if jw > 0:  # (no level: the out-of-place call leaves dst as it is)
            assert same_floats(f, want), route
            assert same_floats(i_, wi), route
        got[route] = fi
    assert np.array_equal(got["fused"].view(np.uint32), got["generic"].view(np.uint32))
    assert np.array_equal(got["fused"].view(np.uint32), got["accel1"].view(np.uint32))


def test_strided_device_image(dwt):
    """One channel of an interleaved 3-channel image with a padded pitch (byte strides): only its samples change."""
    h, w, ch = 130, 200, 3
    pitch = (w * ch + 8) * 4
    rng = np.random.default_rng(3)
    buf = rng.random((h, pitch // 4), dtype=np.float32)
    img = buf[:, 1:1 + w * ch:ch].copy()
    want, jw = want2d(img, False, j_max=4)
    wi, _ = want2d(want, True, j_max=jw)
    d = dwt.DeviceImage(h, pitch // 4)
    d.upload(buf)
    base = d.ptr + 4
    assert t2d(dwt, 0, base, base, pitch, 4 * ch, (h, w), None, 4) == jw
    got = d.download(np.float32)
    assert same_floats(got[:, 1:1 + w * ch:ch], want)
    rest = np.ones(got.shape, bool)
    rest[:, 1:1 + w * ch:ch] = False
    assert np.array_equal(got[rest].view(np.uint32), buf[rest].view(np.uint32))
    t2d(dwt, 1, base, base, pitch, 4 * ch, (h, w), None, jw)
    got = d.download(np.float32)
    assert same_floats(got[:, 1:1 + w * ch:ch], wi)
    d.free()


def test_batch_of_8(dwt):
    n, h, w = 8, 300, 520
    rng = np.random.default_rng(8)
    imgs = rng.random((n, h, w), dtype=np.float32) * 8 - 4
    src = dwt.DeviceImage(n * h, w).upload(imgs.reshape(n * h, w))
    dst = dwt.DeviceImage(n * h, w)
    bs = h * w * 4
    j = dwt.transform2d_batch("interp53_s", 0, src.ptr, dst.ptr, bs, n, w * 4, w, h, 5)
    out = dst.download(np.float32).reshape(n, h, w)
    for k in range(n):
        want, jw = want2d(imgs[k], False, j_max=5)
        assert j == jw and same_floats(out[k], want), k
    dwt.transform2d_batch("interp53_s", 1, dst.ptr, src.ptr, bs, n, w * 4, w, h, j)
    back = src.download(np.float32).reshape(n, h, w)
    for k in range(n):
        wi, _ = want2d(out[k], True, j_max=j)
        assert same_floats(back[k], wi), k
    src.free()
    dst.free()


@pytest.mark.parametrize("n_lines,size", [(100, 5000), (37, 8192), (300, 7), (3, 20000), (2, 65536 + 3)])
def test_1d_dense_batches(dwt, n_lines, size):
    rng = np.random.default_rng(size)
    x = rng.random((n_lines, size), dtype=np.float32) * 8 - 4
    want, jw = want1d(x, False)
    wi, _ = want1d(want, True, j_max=jw)
    d = dwt.DeviceImage(n_lines, size).upload(x)
    assert dwt.transform1d_batch("interp53_s", 0, d.ptr, d.ptr, size * 4, n_lines, size) == jw
    assert same_floats(d.download(np.float32), want)
    dwt.transform1d_batch("interp53_s", 1, d.ptr, d.ptr, size * 4, n_lines, size, jw)
    assert same_floats(d.download(np.float32), wi)
    d.free()
    # host pointers through the drop-in 1-D entries
    a = x[0].copy()
    assert dwt.dwt_interp53_1f_s(a, 4, size, size) == jw
    assert same_floats(a, want[0])
    dwt.dwt_interp53_1i_s(a, 4, size, size, jw)
    assert same_floats(a, wi[0])


@pytest.mark.parametrize("es", [8, 12])
def test_1d_element_strides(dwt, es):
    n_lines, size = 20, 3000
    k = es // 4
    rng = np.random.default_rng(es)
    buf = rng.random((n_lines, size * k), dtype=np.float32)
    x = buf[:, ::k].copy()
    want, jw = want1d(x, False, j_max=6)
    d = dwt.DeviceImage(n_lines, size * k).upload(buf)
    assert dwt.transform1d_batch("interp53_s", 0, d.ptr, d.ptr, size * es, n_lines, size, 6, elem_stride=es) == jw
    got = d.download(np.float32)
    assert same_floats(got[:, ::k], want)
    assert np.array_equal(got[:, 1::k].view(np.uint32), buf[:, 1::k].view(np.uint32))
    d.free()


@pytest.mark.parametrize("so,si,zp", [(50, 29, 0), (50, 29, 1), (33, 1, 1), (1, 1, 0), (1, 0, 1)])
def test_1d_sparse_and_single_sample(dwt, so, si, zp):
    rng = np.random.default_rng(so * 3 + si)
    x = rng.random((4, so), dtype=np.float32) * 8 - 4
    want, jw = want1d(x, False, size_i=si, j_max=-1, zp=zp)
    wi, _ = want1d(want, True, size_i=si, j_max=jw, zp=zp)
    d = dwt.DeviceImage(4, so).upload(x)
    j = C.c_int(-1)
    assert dwt.lib.dwt_hip_transform1d_batch(WID, 0, d.ptr, d.ptr, so * 4, 4, 4, so, si, C.byref(j), zp) == 0, dwt.last_error()
    assert j.value == jw and same_floats(d.download(np.float32), want)
    j = C.c_int(jw)
    assert dwt.lib.dwt_hip_transform1d_batch(WID, 1, d.ptr, d.ptr, so * 4, 4, 4, so, si, C.byref(j), zp) == 0
    assert same_floats(d.download(np.float32), wi)
    d.free()


@pytest.mark.parametrize("klass,nonfinite", [("subnormal", False), ("tiny", False), ("huge", False), ("mixed", True)])
@pytest.mark.parametrize("shape", [(130, 260), (300, 520), (67, 129)])
def test_whole_float_range(dwt, shape, klass, nonfinite):
    rng = np.random.default_rng(hash((shape, klass)) & 0xFFFF)
    img = full_range_floats(rng, shape, klass=klass, nonfinite=nonfinite)
    want, jw = want2d(img, False)
    d = on_device(dwt, img)
    t2d(dwt, 0, d.ptr, d.ptr, d.stride_x, 4, shape)
    assert same_floats(d.download(np.float32), want)
    # the inverse of the whole range too (its own input, not the forward's output)
    wi, _ = want2d(img, True, j_max=jw)
    d.upload(img)
    t2d(dwt, 1, d.ptr, d.ptr, d.stride_x, 4, shape, None, jw)
    assert same_floats(d.download(np.float32), wi)
    d.free()
    x = full_range_floats(rng, (8, 1000), klass=klass, nonfinite=nonfinite)
    w1, j1 = want1d(x, False)
    d = on_device(dwt, x)
    dwt.transform1d_batch("interp53_s", 0, d.ptr, d.ptr, 4000, 8, 1000)
    assert same_floats(d.download(np.float32), w1)
    d.free()


def test_launch_counts(dwt):
    """A dense device 2-D call launches what the CDF 5/3 float call does; a dense 1-D batch of at most 8192 samples one."""
    for shape in [(512, 512), (1000, 1500), (4096, 4096)]:
        img = np.random.default_rng(1).random(shape, dtype=np.float32)
        counts = []
        for wid in (2, WID):
            for inverse in (0, 1):
                d = on_device(dwt, img)
                o = dwt.DeviceImage(*shape)
                j = C.c_int(5)
                n0 = dwt.get_option("stat_launches")
                assert dwt.lib.dwt_hip_transform2d(wid, inverse, d.ptr, o.ptr, d.stride_x, 4, shape[1], shape[0], shape[1], shape[0],
                                                   C.byref(j), 0, 0) == 0
                counts.append(dwt.get_option("stat_launches") - n0)
                d.free()
                o.free()
        assert counts[:2] == counts[2:], (shape, counts)
    x = np.random.default_rng(2).random((64, 8192), dtype=np.float32)
    d = on_device(dwt, x)
    for inverse in (0, 1):
        n0 = dwt.get_option("stat_launches")
        dwt.transform1d_batch("interp53_s", inverse, d.ptr, d.ptr, 8192 * 4, 64, 8192, 13)
        assert dwt.get_option("stat_launches") - n0 == 1
    d.free()


def test_tune_and_alloc_batch_accept_the_wavelet(dwt):
    n, h, w = 2, 256, 256
    src, dst = dwt.DeviceImage(n * h, w), dwt.DeviceImage(n * h, w)
    src.upload(np.random.default_rng(4).random((n * h, w), dtype=np.float32))
    assert dwt.lib.dwt_hip_tune(WID, 0, src.ptr, dst.ptr, h * w * 4, n, w * 4, w, h, 3) == 0, dwt.last_error()
    s_, d_ = C.c_void_p(), C.c_void_p()
    assert dwt.lib.dwt_hip_alloc_batch(WID, n, w, h, 3, C.byref(s_), C.byref(d_)) == 0, dwt.last_error()
    dwt.lib.dwt_hip_free(s_.value)
    dwt.lib.dwt_hip_free(d_.value)
    src.free()
    dst.free()


def test_calls_that_refuse_the_wavelet(dwt):
    a = np.zeros((64, 64), np.float32)
    with pytest.raises(dwt.DwtError):
        dwt.transform2d_interleaved(WID, 0, 0, a, a, 256, 4, 64, 64)
    assert not a.any()
    d = on_device(dwt, a)
    j = C.c_int(-1)
    assert dwt.lib.dwt_hip_transform2d(7, 0, d.ptr, d.ptr, 256, 4, 64, 64, 64, 64, C.byref(j), 0, 0) != 0
    assert dwt.lib.dwt_hip_transform1d_batch(7, 0, d.ptr, d.ptr, 256, 4, 64, 64, 64, C.byref(j), 0) != 0
    assert dwt.lib.dwt_hip_transform2d_batch(7, 0, d.ptr, d.ptr, 64 * 256, 1, 256, 64, 64, C.byref(j)) != 0
    assert not d.download(np.float32).any()
    d.free()


def test_c_example(dwt, tmp_path):
    """examples/interp53.c: the reference's simple-interpl flow plus a device round trip, from C."""
    exe = tmp_path / "interp53"
    libdir = os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "interp53.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "host round trip: success" in out.stderr and "device round trip: success" in out.stderr
