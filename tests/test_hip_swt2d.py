"""GPU checks of the stationary wavelet transform of image batches (dwt_hip_swt2d_batch, dwt_hip_swt2d_level) against the
float32 restatement of tests/swt2d_model.py, which tests/test_swt2d.py pins to the reference's outputs.  Every comparison
is bitwise with NaN == NaN; every output buffer is filled with a canary first, and every word outside the addressed
coefficients must still hold it afterwards."""
import functools
import os
import subprocess

import numpy as np
import pytest

import swt2d_model as m2
import swt_model as sm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
CANARY = np.uint32(0xDEADBEEF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPARED = {"planes": 0, "matched": 0}
FUSED = 5            # DWT_HIP_SWT2D_FUSED_LEVELS: levels 0 .. 4 of dense device images take one launch each
TW, TH = 256, 32     # DWT_HIP_SWT2D_TILE_W / _H


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    assert (d.SWT2D_FUSED_LEVELS, d.SWT2D_TILE_W, d.SWT2D_TILE_H) == (FUSED, TW, TH)
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    d.set_option("swt2d_fused", 1)


@functools.lru_cache(maxsize=None)
def expected(wavelet, kind, batch, h, w, levels, seed):
    """-> (input (batch, h, w), LL (levels, batch, h, w), D (levels, 3, batch, h, w)); computed once, never modified"""
    x = np.stack([m2.make_input(seed + b, kind, h, w) for b in range(batch)])
    LL, D = m2.swt2d_levels(x, wavelet, levels)
    m2.check_kind(kind, LL, D)  # float_range: at most 10 % non-finite; tiny: at least half subnormal
    for a in (x, LL, D):
        a.setflags(write=False)
    return x, LL, D


def generic_launches(levels, es=4, fused=True):
    """the documented count: one launch per level on the fused route, a row pass and a column pass on the generic one"""
    return sum(1 if fused and l < FUSED and (es == 4 or l > 0) else 2 for l in range(levels))


def run_swt2d(dwt, wavelet, x, levels, device=True, pad=0, es=4, l_mode=2, off=0):
    """-> (D (levels, 3, batch, h, w), LL planes (n, batch, h, w), launches).  Rows `pad` elements longer than w on every
    side, source elements es bytes apart, 16 words between planes, 24 between images, every base `off` words past its
    allocation.  Everything outside the addressed coefficients must come back as it was."""
    batch, h, w = x.shape
    step = es // 4
    nl = max(levels, 1)
    src_img_e = h * (w + pad) * step + 24
    src = np.full(off + batch * src_img_e, F32(-7.5), F32)
    for b in range(batch):
        v = src[off + b * src_img_e:off + b * src_img_e + h * (w + pad) * step].reshape(h, (w + pad) * step)
        v[:, :w * step:step] = x[b]
    pitch_e = w + pad
    plane_e = h * pitch_e + 16
    dbs_e = 3 * nl * plane_e + 24
    out_h = np.full(off + batch * dbs_e, CANARY, np.uint32)
    out_l = np.full(off + batch * dbs_e, CANARY, np.uint32)
    src0 = src.copy()
    bufs = [Dev(dwt, a) for a in (src, out_h, out_l)] if device else None
    sp, hp, lp = [(b.ptr if device else a.ctypes.data) + 4 * off for a, b in zip((src, out_h, out_l), bufs or [None] * 3)]
    k = launches(dwt, lambda: dwt.swt2d_batch(wavelet, sp, src_img_e * 4, batch, pitch_e * step * 4, es, w, h, levels, hp, lp, l_mode,
                                              dbs_e * 4, plane_e * 4, pitch_e * 4))
    if device:
        src, out_h, out_l = bufs[0].get(src.shape), bufs[1].get(out_h.shape, np.uint32), bufs[2].get(out_l.shape, np.uint32)
        for b in bufs:
            b.free()
    assert np.array_equal(src.view(np.uint32), src0.view(np.uint32))  # src is never written

    def planes(buf, which):
        """the addressed coefficients of the planes `which` of every image; everything else must still be the canary"""
        assert (buf[:off] == CANARY).all()
        v = buf[off:].reshape(batch, dbs_e)
        assert (v[:, 3 * nl * plane_e:] == CANARY).all(), "gap between images"
        v = v[:, :3 * nl * plane_e].reshape(batch, 3 * nl, plane_e)
        assert (v[:, :, h * pitch_e:] == CANARY).all(), "gap between planes"
        body = v[:, :, :h * pitch_e].reshape(batch, 3 * nl, h, pitch_e)
        assert (body[:, :, :, w:] == CANARY).all(), "row padding"
        for p in range(3 * nl):
            if p not in which:
                assert (body[:, p] == CANARY).all(), ("plane written though not asked for", p)
        return np.stack([body[:, p, :, :w] for p in which]).view(F32) if which else np.zeros((0, batch, h, w), F32)

    D = planes(out_h, list(range(3 * levels))).reshape(levels, 3, batch, h, w)
    L = planes(out_l, list(range(levels)) if l_mode == 2 else [0] if l_mode == 1 and levels else [])
    return D, L, k


def check_planes(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    got, want = got.reshape((-1,) + got.shape[-2:]), want.reshape((-1,) + want.shape[-2:])
    for i in range(want.shape[0]):
        COMPARED["planes"] += 1
        ok = sm.same(got[i], want[i])
        COMPARED["matched"] += ok
        assert ok, (what, "plane", i)


def check_case(dwt, wavelet, h, w, levels, batch=1, device=True, pad=0, es=4, l_mode=2, kind="normal", off=0, fused=True):
    x, LL, D = expected(wavelet, kind, batch, h, w, levels, 1000 * h + w)
    gotD, gotL, k = run_swt2d(dwt, wavelet, x, levels, device, pad, es, l_mode, off)
    check_planes(gotD, D, "details")
    check_planes(gotL, LL if l_mode == 2 else LL[-1:] if l_mode == 1 else LL[:0], "LL")
    if device:
        assert k == generic_launches(levels, es, fused), k


# (size_y, size_x, levels, then keyword arguments): every size, tile edge, depth, batch, pitch, alignment, memory space,
# element stride, l_mode and input kind the kernels take a different path for
COEFF_CASES = [
    (1, 1, 3, {}),
    (1, 9, 4, {"kind": "small_ints", "l_mode": 1}),
    (7, 1, 3, {"l_mode": 0}),
    (2, 3, 6, {"kind": "tiny", "batch": 3}),
    (37, 53, 8, {"kind": "tiny"}),  # dilation beyond both sizes; the route changes mid-pyramid
    (37, 53, 8, {"l_mode": 1, "batch": 3, "pad": 3}),
    (65, 130, 3, {"pad": 1, "off": 1}),
    (130, 67, 5, {"kind": "small_ints", "l_mode": 0, "batch": 3, "pad": 16}),  # the fused limit
    (96, 120, 3, {"kind": "float_range"}),
    (96, 120, 3, {"kind": "float_range", "device": False, "l_mode": 1}),
    (40, 150, 3, {"kind": "float_range", "batch": 3, "off": 1, "pad": 3}),
    (300, 270, 6, {"l_mode": 1}),  # one level beyond the fused limit
    (300, 270, 6, {"l_mode": 2, "pad": 1}),
    (9, TW - 1, 3, {}), (9, TW, 3, {"l_mode": 0}), (9, TW + 1, 3, {"pad": 3}), (9, 2 * TW + 1, 5, {"off": 1}),
    (TH - 1, 20, 3, {}), (TH, 20, 3, {"l_mode": 1}), (TH + 1, 20, 3, {"batch": 3}), (2 * TH + 1, 20, 5, {"pad": 1}),
    (33, 40, 0, {}), (33, 40, 1, {"l_mode": 1}), (33, 40, 1, {"l_mode": 0, "off": 1}),
    (50, 77, 3, {"device": False, "batch": 3, "pad": 3}),
    (50, 77, 6, {"device": False, "l_mode": 0, "kind": "small_ints"}),
    (50, 77, 3, {"es": 8, "pad": 1}),
    (50, 77, 6, {"es": 8, "batch": 3, "l_mode": 1, "kind": "tiny"}),
    (50, 77, 2, {"es": 8, "device": False, "l_mode": 0}),
]


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
@pytest.mark.parametrize("case", COEFF_CASES, ids=lambda c: "%dx%d-%d-" % c[:3] + "-".join("%s=%s" % kv for kv in sorted(c[3].items())))
def test_coefficients_bit_identical(dwt, wavelet, case):
    h, w, levels, kw = case
    if kw.get("kind") == "float_range" and wavelet == "cdf53_s" and (h, w) == (96, 120):
        levels = 4  # (the cap on non-finite coefficients admits one more level of the shorter filters)
    check_case(dwt, wavelet, h, w, levels, **kw)


def test_all_planes_matched():
    """the share of compared planes that must match is 100 % (meaningful for a run of the whole file)"""
    assert COMPARED["planes"] == COMPARED["matched"]


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_generic_route_equals_fused(dwt, wavelet):
    """option swt2d_fused = 0: a row pass and a column pass per level through global memory, the same bits"""
    for kind, h, w, levels in (("float_range", 96, 120, 3), ("tiny", 37, 53, 6)):
        x, LL, D = expected(wavelet, kind, 2, h, w, levels, 77)
        fused = run_swt2d(dwt, wavelet, x, levels, pad=1)
        dwt.set_option("swt2d_fused", 0)
        try:
            plain = run_swt2d(dwt, wavelet, x, levels, pad=1)
        finally:
            dwt.set_option("swt2d_fused", 1)
        assert fused[2] == generic_launches(levels) and plain[2] == 2 * levels
        assert sm.same(fused[0], plain[0]) and sm.same(fused[1], plain[1])
        assert sm.same(plain[0], D) and sm.same(plain[1], LL)


def test_launch_counts(dwt):
    """a dense device image: one launch per level up to the fused limit whatever the batch; two per level beyond it and
    under swt2d_fused = 0"""
    for (h, w), levels in (((64, 64), 7), ((300, 270), 5), ((1024, 1024), 6)):
        for batch in (1, 3):
            src = Dev(dwt, np.zeros((batch, h, w), F32))
            # (dst_h and dst_l share the batch stride of 3 * levels planes)
            dh, dl = Dev(dwt, np.zeros((batch, 3 * levels, h, w), F32)), Dev(dwt, np.zeros((batch, 3 * levels, h, w), F32))
            plane = 4 * h * w

            def call(wv, l_mode):
                return launches(dwt, lambda: dwt.swt2d_batch(wv, src.ptr, plane, batch, 4 * w, 4, w, h, levels, dh.ptr, dl.ptr, l_mode,
                                                             3 * levels * plane, plane, 4 * w))

            for wv in sm.WAVELETS:
                for l_mode in (0, 1, 2):
                    assert call(wv, l_mode) == min(levels, FUSED) + 2 * max(levels - FUSED, 0), (h, w, batch, wv, l_mode)
                dwt.set_option("swt2d_fused", 0)
                try:
                    assert call(wv, 2) == 2 * levels
                finally:
                    dwt.set_option("swt2d_fused", 1)
            assert not dh.get().any() and not dl.get().any()  # zeros in, zeros out
            for d in (src, dh, dl):
                d.free()


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_level_entry(dwt, wavelet):
    """dwt_hip_swt2d_level: every level of one case, fed with the model's LL of the level before; device (dense: the fused
    kernel up to its limit; elements 8 bytes apart: the two passes) and host memory"""
    h, w, levels = 37, 53, 8
    x, LL, D = expected(wavelet, "normal", 1, h, w, levels, 55)
    for l in range(levels):
        a = x[0] if l == 0 else LL[l - 1, 0]
        want = [LL[l, 0], D[l, 0, 0], D[l, 1, 0], D[l, 2, 0]]
        for device, step in ((True, 1), (True, 2), (False, 1), (False, 2)):
            outs = [np.full((h, w * step + 3), CANARY, np.uint32) for _ in range(4)]
            bufs = [Dev(dwt, b) for b in [a] + outs] if device else None
            ptrs = [b.ptr for b in bufs] if device else [b.ctypes.data for b in [np.ascontiguousarray(a)] + outs]
            k = launches(dwt, lambda: dwt.swt2d_level(wavelet, ptrs[0], 4 * w, 4, w, h, l, *ptrs[1:], 4 * (w * step + 3), 4 * step))
            if device:
                assert k == (1 if step == 1 and l < FUSED else 2), (l, step, k)
                outs = [b.get(outs[0].shape, np.uint32) for b in bufs[1:]]
                for b in bufs:
                    b.free()
            for o, wanted in zip(outs, want):
                assert sm.same(o[:, :w * step:step].view(F32), wanted), (l, device, step)
                mask = np.ones(o.shape, bool)
                mask[:, :w * step:step] = False
                assert (o[mask] == CANARY).all()


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_one_row_image_against_row_entry(dwt, wavelet):
    """a 1-row image: the row pass is what dwt_hip_swt1d_level gives for that row, and the column pass with N = 1 sums
    every tap of the column filter over the one sample"""
    n = 300
    row = sm.make_input(31, "float_range", 1, n)[0]
    gl, gh = sm.FILTERS[wavelet]
    entry = dwt.swt_cdf97_f_ex_stride_s if wavelet == "cdf97_s" else dwt.swt_cdf53_f_ex_stride_s

    def column_of_one(v, g):
        y = np.zeros_like(v)
        with np.errstate(all="ignore"):
            for tap in g:
                y = (y + (v * tap).astype(F32)).astype(F32)
        return y

    for level in (0, 3, 6):
        bufs = [Dev(dwt, row)] + [Dev(dwt, np.zeros(n, F32)) for _ in range(6)]
        entry(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, 4, level)
        L, H = bufs[1].get(), bufs[2].get()
        dwt.swt2d_level(wavelet, bufs[0].ptr, 4 * n, 4, n, 1, level, *[b.ptr for b in bufs[3:]], 4 * n)
        LLg, HLg, LHg, HHg = [b.get() for b in bufs[3:]]
        assert sm.same(LLg, column_of_one(L, gl)) and sm.same(LHg, column_of_one(L, gh)), level
        assert sm.same(HLg, column_of_one(H, gl)) and sm.same(HHg, column_of_one(H, gh)), level
        for b in bufs:
            b.free()


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_ll_behind_the_details(dwt, wavelet):
    """dst_h and dst_l share the batch stride, so one buffer can hold every image's detail planes and its LL behind them"""
    batch, h, w, levels = 3, 21, 40, 2
    x, LL, D = expected(wavelet, "normal", batch, h, w, levels, 9)
    per = 3 * levels + 1
    src, out = Dev(dwt, x), Dev(dwt, np.full((batch, per + 1, h, w), CANARY, np.uint32))  # one spare plane an image
    plane = 4 * h * w
    dwt.swt2d_batch(wavelet, src.ptr, plane, batch, 4 * w, 4, w, h, levels, out.ptr, out.ptr + 3 * levels * plane, 1, (per + 1) * plane, plane, 4 * w)
    got = out.get()
    assert (got[:, per] == CANARY).all()
    for b in range(batch):
        assert sm.same(got[b, :3 * levels].view(F32).reshape(levels, 3, h, w), D[:, :, b]) and sm.same(got[b, 3 * levels].view(F32), LL[-1, b])
    with pytest.raises(dwt.DwtError):  # one plane too early: LL would land on HH of the last level
        dwt.swt2d_batch(wavelet, src.ptr, plane, batch, 4 * w, 4, w, h, levels, out.ptr, out.ptr + (3 * levels - 1) * plane, 1, (per + 1) * plane, plane, 4 * w)
    with pytest.raises(dwt.DwtError):  # two LL planes where one fits: the second would land on the next image
        dwt.swt2d_batch(wavelet, src.ptr, plane, batch, 4 * w, 4, w, h, levels, out.ptr, out.ptr + (3 * levels + 1) * plane, 2, (per + 1) * plane, plane, 4 * w)
    src.free()
    out.free()


def test_refusals(dwt):
    """every refused call leaves its outputs as they were"""
    w, h, levels, batch = 32, 6, 2, 2
    plane, sx = 4 * w * h, 4 * w
    x = np.zeros((batch, h, w), F32)
    hh, hl = np.full((batch, 3 * levels, h, w), CANARY, np.uint32), np.full((batch, 3 * levels, h, w), CANARY, np.uint32)
    d, dh, dl = Dev(dwt, x), Dev(dwt, hh), Dev(dwt, hl)
    dbs = 3 * levels * plane

    def call(wavelet="cdf97_s", src=d.ptr, bs=plane, batch=batch, sx=sx, sy=4, w=w, h=h, levels=levels, dst_h=dh.ptr, dst_l=dl.ptr, l_mode=2,
             dbs=dbs, ps=plane, dsx=sx):
        return lambda: dwt.swt2d_batch(wavelet, src, bs, batch, sx, sy, w, h, levels, dst_h, dst_l, l_mode, dbs, ps, dsx)

    bad = [
        call(dst_h=hh), call(src=x), call(dst_l=hl),  # host and device memory mixed
        call(sy=6, w=16), call(src=d.ptr + 2), call(dsx=sx + 2),  # device addresses and strides are multiples of 4 bytes
        call(dst_h=d.ptr), call(dst_l=d.ptr + 8, l_mode=1), call(dst_l=dh.ptr + plane, l_mode=1), call(dst_l=dh.ptr + dbs * batch - 4, l_mode=1),  # overlaps
        call(ps=plane - 4), call(dbs=dbs - 4), call(bs=plane - 4), call(dsx=sx - 4), call(sx=sx - 4), call(sy=2),
        call(batch=0), call(w=0), call(h=0), call(levels=-1), call(levels=25), call(wavelet="cdf53_i"), call(wavelet="cdf97_d"),
        call(l_mode=3), call(l_mode=1, dst_l=None),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    p4 = [Dev(dwt, np.full((h, w), CANARY, np.uint32)) for _ in range(4)]
    host_plane = np.full((h, w), CANARY, np.uint32)
    bad_level = [
        lambda: dwt.swt2d_level("cdf97_s", d.ptr, sx, 4, w, h, 24, *[b.ptr for b in p4], sx),
        lambda: dwt.swt2d_level("cdf53_i", d.ptr, sx, 4, w, h, 0, *[b.ptr for b in p4], sx),
        lambda: dwt.swt2d_level("cdf97_s", d.ptr, sx, 4, w, h, 0, p4[0].ptr, p4[1].ptr, host_plane, p4[3].ptr, sx),
        lambda: dwt.swt2d_level("cdf97_s", d.ptr, sx, 4, w, h, 0, p4[0].ptr, p4[1].ptr, p4[1].ptr + 16, p4[3].ptr, sx),
        lambda: dwt.swt2d_level("cdf97_s", d.ptr, sx, 4, w, h, 0, p4[0].ptr, p4[1].ptr, d.ptr, p4[3].ptr, sx),
        lambda: dwt.swt2d_level("cdf97_s", d.ptr, sx, 4, w, h, 0, *[b.ptr for b in p4], sx, 6),
    ]
    for i, f in enumerate(bad_level):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    assert (dh.get() == CANARY).all() and (dl.get() == CANARY).all() and not d.get().any()
    assert (hh == CANARY).all() and (hl == CANARY).all() and (host_plane == CANARY).all() and not x.any()
    assert all((b.get() == CANARY).all() for b in p4)
    for b in [d, dh, dl] + p4:
        b.free()


def test_c_example(dwt, tmp_path):
    """examples/swt2d.c: a resident batch through one call from C; one checksum per plane against the model's"""
    exe, libdir = tmp_path / "swt2d", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "swt2d.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    batch, w, h, levels = 2, 70, 48, 3
    seed, vals = 2024, []
    for _ in range(batch * h * w):  # the example's generator
        seed = (seed * 1664525 + 1013904223) & 0xFFFFFFFF
        vals.append(((seed >> 8) & 0xFFFF) / 65536.0 - 0.5)
    x = np.array(vals, np.float64).astype(F32).reshape(batch, h, w)
    LL, D = m2.swt2d_levels(x, "cdf97_s", levels)
    want = []
    for b in range(batch):
        for l in range(levels):
            for k, name in enumerate(m2.BANDS):
                want.append("image %d level %d %s %08x" % (b, l, name, int(D[l, k, b].view(np.uint32).sum(dtype=np.uint64)) & 0xFFFFFFFF))
        want.append("image %d level %d LL %08x" % (b, levels - 1, int(LL[-1, b].view(np.uint32).sum(dtype=np.uint64)) & 0xFFFFFFFF))
    want.append("%d images of %d x %d, %d levels: %d launch(es)" % (batch, w, h, levels, levels))
    assert out.stdout.splitlines() == want
