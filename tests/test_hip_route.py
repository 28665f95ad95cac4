"""A call's route depends only on that call.

Whether a level of a 2-D Mallat call takes a fused sweep or the exact line passes is decided from the call's own
wavelet, addresses and strides.  The same calls made in different orders on one context and one thread -- every
element size, the 2-byte wavelets on a pitch the fused sweeps take and on one they do not, with a 1-D call and an
EAW call in between -- give the same bytes and the same number of kernel launches as each call made alone, first
after a fresh init.  The expected launch counts are those of the "alone" runs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, J = 64, 48, 2  # the smallest size at which two levels are both >= 2 and dense
# (name, wavelet, dtype, pitch in bytes); pitch 130 is 2 mod 4: the line passes
CALLS = [("s", "cdf97_s", np.float32, 256), ("d", "cdf97_d", np.float64, 512), ("i", "cdf53_i", np.int32, 256),
         ("i16", "cdf53_i16", np.int16, 128), ("i16u", "cdf53_i16", np.int16, 130),
         ("h", "cdf97_h", np.float16, 128), ("hu", "cdf97_h", np.float16, 130),
         ("1d", None, None, None), ("eaw", None, None, None)]
UNALIGNED, WIDE = {"i16u", "hu"}, {"s", "d", "i"}
MIXED = ["s", "i16u", "d", "hu", "i", "i16", "h", "1d", "eaw"]


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.dwt_util_finish()


def _image(dtype, pitch, n, seed):
    """n images of H rows of `pitch` bytes, the padding zero."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n * H, pitch // np.dtype(dtype).itemsize), dtype)
    if np.issubdtype(dtype, np.integer):
        a[:, :W] = rng.integers(-2048, 2048, size=(n * H, W))
    else:
        a[:, :W] = rng.random((n * H, W))
    return a


def _run(dwt, name):
    """One entry of CALLS, forward then inverse -> (every buffer it wrote, as bytes; the launches of every call)."""
    out, launches = [], []

    def counted(f, *a):
        n0 = dwt.get_option("stat_launches")
        r = f(*a)
        launches.append(dwt.get_option("stat_launches") - n0)
        return r

    def t2d(wavelet, inverse, s, d, pitch, es, j):
        import ctypes as C

        jj = C.c_int(j)
        rc = dwt.lib.dwt_hip_transform2d(dwt.WAVELET_ID[wavelet], inverse, s.ptr, d.ptr, pitch, es, W, H, W, H, C.byref(jj), 0, 0)
        assert rc == 0, dwt.last_error()
        return jj.value

    if name == "1d":
        x = _image(np.float32, 256, 1, 11)[:4]
        s, d = dwt.DeviceImage(4, W).upload(x), dwt.DeviceImage(4, W).upload(np.zeros_like(x))
        j = counted(dwt.transform1d_batch, "cdf97_s", 0, s.ptr, d.ptr, 256, 4, W, J)
        out.append(d.download(np.float32).tobytes())
        counted(dwt.transform1d_batch, "cdf97_s", 1, d.ptr, s.ptr, 256, 4, W, j)
        out.append(s.download(np.float32).tobytes())
        s.free(), d.free()
    elif name == "eaw":
        d = dwt.DeviceImage(H, W).upload(_image(np.float32, 256, 1, 12))
        j, wh, wv = counted(dwt.dwt_eaw53_2f_s, d.ptr, 256, 4, W, H, W, H, J)
        out += [d.download(np.float32).tobytes()] + [np.asarray(a).tobytes() for a in wh + wv]
        counted(dwt.dwt_eaw53_2i_s, d.ptr, 256, 4, W, H, W, H, j, 0, 0, wh, wv)
        out.append(d.download(np.float32).tobytes())
        d.free()
    else:
        _, wavelet, dtype, pitch = next(c for c in CALLS if c[0] == name)
        es = np.dtype(dtype).itemsize
        for n in (1, 2):  # the one-image entry, the batch entry with 2 images
            x = _image(dtype, pitch, n, 13 + n)
            bufs = [dwt.DeviceImage(n * H, W, itemsize=es, pitch_bytes=pitch).upload(a) for a in (x, np.zeros_like(x), np.zeros_like(x))]
            s, d, back = bufs
            if n == 1:
                j = counted(t2d, wavelet, 0, s, d, pitch, es, J)
                counted(t2d, wavelet, 1, d, back, pitch, es, j)
            else:
                j = counted(dwt.transform2d_batch, wavelet, 0, s.ptr, d.ptr, pitch * H, n, pitch, W, H, J)
                counted(dwt.transform2d_batch, wavelet, 1, d.ptr, back.ptr, pitch * H, n, pitch, W, H, j)
            assert j == J
            out += [b.download(dtype).tobytes() for b in bufs]
            for b in bufs:
                b.free()
    return out, launches


def test_route_depends_only_on_the_call(dwt):
    names = [c[0] for c in CALLS]
    assert sorted(MIXED) == sorted(names)
    pairs = set(zip(MIXED, MIXED[1:]))
    for u in UNALIGNED:  # every unaligned 2-byte call directly before a 4- or 8-byte one, and directly behind one
        assert any((u, v) in pairs for v in WIDE) and any((v, u) in pairs for v in WIDE)
    alone = {}
    for name in names:
        dwt.dwt_util_finish()
        dwt.dwt_util_init()
        alone[name] = _run(dwt, name)
    for u, a in (("i16u", "i16"), ("hu", "h")):  # (the two pitches do take different routes)
        assert alone[u][1] != alone[a][1], (u, alone[u][1])
    dwt.dwt_util_finish()
    dwt.dwt_util_init()
    for order in (names, names[::-1], MIXED):
        for k, name in enumerate(order):
            got, launches = _run(dwt, name)
            assert launches == alone[name][1], ("launches", name, "after", order[:k])
            assert got == alone[name][0], ("bytes", name, "after", order[:k])
