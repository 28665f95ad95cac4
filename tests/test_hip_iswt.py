"""GPU checks of the stationary transforms under the symmetric border and of their inverses (dwt_hip_swt1d_batch_ex,
dwt_hip_swt2d_batch_ex, dwt_hip_iswt1d_batch, dwt_hip_iswt2d_batch) against the float32 restatement of
tests/iswt_model.py, which tests/test_iswt.py ties to the reference.  Every comparison is bitwise with NaN == NaN
(swt_model.same); every output buffer is filled with a canary first, and every word outside the addressed samples must
still hold it afterwards.  The whole file runs on scratch that holds 0xFFFFFFFF in every word."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import iswt_model as im
import swt2d_model as m2
import swt_model as sm
from hipdev import Dev, launches
from test_iswt import BOUND_1D, BOUND_2D, ROUND_TRIP_1D, ROUND_TRIP_2D, tables

pytestmark = pytest.mark.gpu
F32 = np.float32
CANARY = np.uint32(0xDEADBEEF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = 5  # DWT_HIP_ISWT2D_FUSED_LEVELS (and DWT_HIP_SWT2D_FUSED_LEVELS): one launch per level on levels 0 .. 4
N1D_MAX = 8192  # rows up to here take one launch for every level


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)
    yield d
    d.poison_workspace(None)
    d.set_option("swt2d_fused", 1)
    d.set_option("swt_fused", 1)


@pytest.fixture(scope="module")
def st(dwt):
    from libdwt_amd import stationary

    assert stationary.ISWT2D_FUSED_LEVELS == FUSED
    return stationary


# ---- buffers -------------------------------------------------------------------------------------------------------------
class Laid:
    """A (batch, planes, rows, cols) stack in one buffer of 32-bit words: rows `pad` elements longer than cols, elements
    `step` words apart, 16 words between planes, 24 between images, the base `off` words past the allocation; everything
    that is no element holds the canary.  Strides in bytes."""

    def __init__(self, dwt, shape, pad=0, off=0, step=1, fill=None):
        self.dwt, self.shape, self.off, self.step = dwt, shape, off, step
        B, P, R, Cn = shape
        self.pitch_e = (Cn + pad) * step
        self.plane_e = R * self.pitch_e + 16
        self.batch_e = P * self.plane_e + 24
        host = np.full(off + B * self.batch_e, CANARY, np.uint32)
        if fill is not None:
            self.elements(host)[...] = np.asarray(fill, F32).view(np.uint32).reshape(shape)
        self.dev = Dev(dwt, host)
        self.ptr = self.dev.ptr + 4 * off
        self.pitch, self.plane, self.batch = 4 * self.pitch_e, 4 * self.plane_e, 4 * self.batch_e

    def elements(self, host):
        B, P, R, Cn = self.shape
        v = host[self.off:].reshape(B, self.batch_e)[:, :P * self.plane_e].reshape(B, P, self.plane_e)[:, :, :R * self.pitch_e]
        return v.reshape(B, P, R, self.pitch_e)[:, :, :, :Cn * self.step:self.step]

    def get(self, planes=None):
        """the elements as float32; every other word, and every plane not in `planes`, must still be the canary"""
        host = self.dev.get()
        el = self.elements(host).copy()
        mask = np.zeros(host.shape, bool)
        sel = self.elements(mask)
        if planes is None:
            sel[...] = True
        else:
            sel[:, list(planes)] = True
        assert (host[~mask] == CANARY).all(), "words outside the addressed elements were written"
        return el.view(F32)

    def free(self):
        self.dev.free()


# ---- expectations: computed once, never modified ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected1d(wavelet, kind, lines, n, levels, seed):
    x = sm.make_input(seed, kind, lines, n)
    L, H = im.swt_levels(x, wavelet, levels)
    y = im.iswt_levels(L[-1] if levels else x, H, wavelet)
    for a in (x, L, H, y):
        a.setflags(write=False)
    return x, L, H, y


@functools.lru_cache(maxsize=None)
def expected2d(wavelet, kind, batch, h, w, levels, seed):
    x = np.stack([m2.make_input(seed + b, kind, h, w) for b in range(batch)])
    LL, D = im.swt2d_levels(x, wavelet, levels)
    y = im.iswt2d_levels(LL[-1] if levels else x, D, wavelet)
    for a in (x, LL, D, y):
        a.setflags(write=False)
    return x, LL, D, y


# ---- rows --------------------------------------------------------------------------------------------------------------------
def run1d(dwt, st, wavelet, x, levels, L, H, y, pad=0, off=0, dst_step=1, fused=True):
    """forward under the symmetric border into laid-out planes, then the inverse straight from them: both against the model"""
    lines, n = x.shape
    nl = max(levels, 1)
    src = Laid(dwt, (1, 1, lines, n), pad, off, fill=x)
    dh, dl = Laid(dwt, (1, nl, lines, n), pad, off), Laid(dwt, (1, nl, lines, n), pad, off)
    out = Laid(dwt, (1, 1, lines, n), pad, off, dst_step)
    k = launches(dwt, lambda: st.swt1d_batch(wavelet, src.ptr, src.pitch, 4, lines, n, levels, dh.ptr, dl.ptr, 1, dh.plane, dh.pitch,
                                             border=st.BORDER_SYMMETRIC))
    one = fused and n <= N1D_MAX
    assert k == (0 if levels == 0 else 1 if one else levels), k
    gh, gl = dh.get(range(levels))[0], dl.get([0] if levels else [])[0]
    assert sm.same(gh[:levels], H), "H planes"
    if levels:
        assert sm.same(gl[0], L[-1]), "last L"
    src_l = dl if levels else src
    k = launches(dwt, lambda: st.iswt1d_batch(wavelet, st.BORDER_SYMMETRIC, dh.ptr, src_l.ptr, dh.plane, dh.pitch, lines, n, levels, out.ptr,
                                              out.pitch, 4 * dst_step))
    assert k == (0 if levels == 0 else 1 if one and dst_step == 1 else levels), k
    got = out.get()[0, 0]
    assert sm.same(got, y), "inverse"
    assert sm.same(src.get()[0, 0], x) and sm.same(dh.get(range(levels))[0][:levels], H)  # the sources are never written
    for b in (src, dh, dl, out):
        b.free()
    return got


# (N, levels, lines, kind, keyword arguments): every size at which the kernels take another path
CASES_1D = [
    (1, 3, 1, "normal", {}), (2, 3, 5, "small_ints", {}), (3, 4, 1, "float_range", {}), (7, 5, 5, "normal", {"pad": 3}),
    (257, 14, 1, "small_ints", {}),  # dilations beyond N
    (257, 10, 5, "float_range", {"off": 1}),  # a base that is 4- but not 16-byte aligned
    (1024, 3, 5, "normal", {}), (1025, 3, 1, "small_ints", {"pad": 3}),  # the thread split; spare lines of a four-line workgroup
    (4096, 3, 1, "float_range", {}), (4097, 2, 5, "normal", {"off": 1, "pad": 1}),
    (8192, 2, 1, "small_ints", {}), (8193, 2, 1, "normal", {}),  # the fused limit
    (100, 4, 5, "normal", {"dst_step": 2}), (1000, 3, 1, "float_range", {"dst_step": 3, "pad": 1}),  # strided dst elements: one launch per level
    (33, 0, 3, "normal", {"pad": 1}), (33, 1, 3, "normal", {}),
]


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
@pytest.mark.parametrize("case", CASES_1D, ids=lambda c: "%d-%d-%d-%s-" % c[:4] + "-".join("%s=%s" % kv for kv in sorted(c[4].items())))
def test_rows_forward_and_inverse(dwt, st, wavelet, case):
    n, levels, lines, kind, kw = case
    x, L, H, y = expected1d(wavelet, kind, lines, n, levels, 5000 + n)
    run1d(dwt, st, wavelet, x, levels, L, H, y, **kw)


def test_rows_kinds_are_all_held():
    assert {c[3] for c in CASES_1D} == set(sm.KINDS)


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_rows_level_route_equals_fused(dwt, st, wavelet):
    """option swt_fused = 0: one launch per level through the scratch chain, the same bits"""
    for kind, lines, n, levels in (("float_range", 5, 300, 6), ("normal", 2, 4097, 3)):
        x, L, H, y = expected1d(wavelet, kind, lines, n, levels, 61)
        a = run1d(dwt, st, wavelet, x, levels, L, H, y, pad=1)
        dwt.set_option("swt_fused", 0)
        try:
            b = run1d(dwt, st, wavelet, x, levels, L, H, y, pad=1, fused=False)
        finally:
            dwt.set_option("swt_fused", 1)
        assert sm.same(a, b)


# ---- images ------------------------------------------------------------------------------------------------------------------
def expected_launches(levels, fused=True, dense=True):
    return sum(1 if fused and l < FUSED and (dense or l > 0) else 2 for l in range(levels))


def run2d(dwt, st, wavelet, x, levels, LL, D, y, pad=0, off=0, dst_step=1, fused=True):
    batch, h, w = x.shape
    nl = max(levels, 1)
    src = Laid(dwt, (batch, 1, h, w), pad, off, fill=x[:, None])
    dh, dl = Laid(dwt, (batch, 3 * nl, h, w), pad, off), Laid(dwt, (batch, 3 * nl, h, w), pad, off)
    out = Laid(dwt, (batch, 1, h, w), pad, off, dst_step)
    k = launches(dwt, lambda: st.swt2d_batch(wavelet, src.ptr, src.batch, batch, src.pitch, 4, w, h, levels, dh.ptr, dl.ptr, 1, dh.batch,
                                             dh.plane, dh.pitch, border=st.BORDER_SYMMETRIC))
    assert k == expected_launches(levels, fused), k
    gd, gl = dh.get(range(3 * levels)), dl.get([0] if levels else [])
    if levels:
        assert sm.same(gd[:, :3 * levels].reshape(batch, levels, 3, h, w), D.transpose(2, 0, 1, 3, 4)), "detail planes"
        assert sm.same(gl[:, 0], LL[-1]), "last LL"
    if levels:
        call = lambda: st.iswt2d_batch(wavelet, st.BORDER_SYMMETRIC, dh.ptr, dl.ptr, dh.batch, dh.plane, dh.pitch, batch, w, h, levels, out.ptr,
                                       out.batch, out.pitch, 4 * dst_step)
    else:
        call = lambda: st.iswt2d_batch(wavelet, st.BORDER_SYMMETRIC, None, src.ptr, src.batch, src.plane, src.pitch, batch, w, h, 0, out.ptr,
                                       out.batch, out.pitch, 4 * dst_step)
    k = launches(dwt, call)
    assert k == expected_launches(levels, fused, dst_step == 1), k
    got = out.get()[:, 0]
    assert sm.same(got, y), "inverse"
    assert sm.same(src.get()[:, 0], x)
    for b in (src, dh, dl, out):
        b.free()
    return got


# (rows, columns, levels, batch, kind, keyword arguments)
CASES_2D = [
    (1, 1, 3, 1, "normal", {}), (1, 9, 4, 3, "small_ints", {}), (5, 3, FUSED + 2, 1, "normal", {"pad": 3}),
    (37, 300, 3, 1, "float_range", {}),  # crosses the 256-column tile
    (37, 300, FUSED + 1, 3, "normal", {"pad": 1, "off": 1}),
    (70, 41, 2, 3, "small_ints", {"pad": 3}),  # three row-lattice tiles at level 0
    (70, 41, FUSED + 2, 1, "normal", {}),  # one call switches route
    (33, 257, 4, 1, "float_range", {"off": 1}), (33, 257, 5, 3, "normal", {"dst_step": 2, "pad": 1}),  # a strided dst: level 0 alone takes the passes
    (21, 40, 0, 3, "normal", {"pad": 1}), (21, 40, 1, 1, "small_ints", {"dst_step": 3}),
]


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
@pytest.mark.parametrize("case", CASES_2D, ids=lambda c: "%dx%d-%d-%d-%s-" % c[:5] + "-".join("%s=%s" % kv for kv in sorted(c[5].items())))
def test_images_forward_and_inverse(dwt, st, wavelet, case):
    h, w, levels, batch, kind, kw = case
    x, LL, D, y = expected2d(wavelet, kind, batch, h, w, levels, 1000 * h + w)
    run2d(dwt, st, wavelet, x, levels, LL, D, y, **kw)


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_images_pass_route_equals_fused(dwt, st, wavelet):
    """option swt2d_fused = 0: a column pass and a row pass per level through global memory, the same bits"""
    for kind, batch, h, w, levels in (("float_range", 2, 96, 120, 3), ("normal", 2, 37, 53, 6)):
        x, LL, D, y = expected2d(wavelet, kind, batch, h, w, levels, 77)
        a = run2d(dwt, st, wavelet, x, levels, LL, D, y, pad=1)
        dwt.set_option("swt2d_fused", 0)
        try:
            b = run2d(dwt, st, wavelet, x, levels, LL, D, y, pad=1, fused=False)
        finally:
            dwt.set_option("swt2d_fused", 1)
        assert sm.same(a, b)


def test_images_launch_counts(dwt, st):
    """min(levels, F) + 2 * max(levels - F, 0) with F the published limit, whatever the batch; 2 * levels under swt2d_fused = 0"""
    h, w, levels = 64, 300, FUSED + 2
    for batch in (1, 3):
        dh, dl, out = [Dev(dwt, np.zeros((batch, n, h, w), F32)) for n in (3 * levels, 3 * levels, 1)]
        plane = 4 * h * w
        for wv in sm.WAVELETS:
            call = lambda: st.iswt2d_batch(wv, 1, dh.ptr, dl.ptr, 3 * levels * plane, plane, 4 * w, batch, w, h, levels, out.ptr, plane, 4 * w)
            assert launches(dwt, call) == min(levels, FUSED) + 2 * max(levels - FUSED, 0)
            dwt.set_option("swt2d_fused", 0)
            try:
                assert launches(dwt, call) == 2 * levels
            finally:
                dwt.set_option("swt2d_fused", 1)
        assert not out.get().any()  # zeros in, zeros out
        for d in (dh, dl, out):
            d.free()


# ---- operators on load -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", sm.WAVELETS)
@pytest.mark.parametrize("fused", (1, 0))
def test_rows_operators_on_load(dwt, st, wavelet, fused):
    """every code, mixed per plane: the model's operators on load, which equal (tests/test_iswt.py) the operator on the stored
    plane followed by the plain inverse -- checked here too, with the planes shaped on the host; a ZERO plane holds NaN"""
    lines, n, levels = 5, 300, 5
    x, L, H, y = expected1d(wavelet, "float_range", lines, n, levels, 88)
    ops, params = tables(levels)
    want = im.iswt_levels(L[-1], H, wavelet, ops, params)
    shaped = np.stack([im.shp.apply_op(H[l], ops[l], params[l]) for l in range(levels)])
    poisoned = H.copy()
    poisoned[ops == im.ZERO] = np.nan
    dwt.set_option("swt_fused", fused)
    try:
        outs = []
        for planes, o, p in ((poisoned, ops, params), (shaped, None, None)):
            dh, dl, out = Laid(dwt, (1, levels, lines, n), 1, 1, fill=planes), Laid(dwt, (1, 1, lines, n), 1, 1, fill=L[-1]), Laid(dwt, (1, 1, lines, n))
            st.iswt1d_batch(wavelet, 1, dh.ptr, dl.ptr, dh.plane, dh.pitch, lines, n, levels, out.ptr, out.pitch, ops=o, params=p)
            outs.append(out.get()[0, 0])
            for b in (dh, dl, out):
                b.free()
    finally:
        dwt.set_option("swt_fused", 1)
    assert sm.same(outs[0], want) and sm.same(outs[1], want)


@pytest.mark.parametrize("wavelet", sm.WAVELETS)
@pytest.mark.parametrize("fused", (1, 0))
def test_images_operators_on_load(dwt, st, wavelet, fused):
    batch, h, w, levels = 2, 37, 53, 3
    x, LL, D, y = expected2d(wavelet, "normal", batch, h, w, levels, 89)
    ops, params = tables(3 * levels, 1)
    want = im.iswt2d_levels(LL[-1], D, wavelet, ops, params)
    shaped = np.array(D)
    poisoned = np.array(D)
    for l in range(levels):
        for k in range(3):
            shaped[l, k] = im.shp.apply_op(D[l, k], ops[3 * l + k], params[3 * l + k])
            if ops[3 * l + k] == im.ZERO:
                poisoned[l, k] = np.nan
    dwt.set_option("swt2d_fused", fused)
    try:
        outs = []
        for planes, o, p in ((poisoned, ops, params), (shaped, None, None)):
            stack = planes.transpose(2, 0, 1, 3, 4).reshape(batch, 3 * levels, h, w)
            dh, out = Laid(dwt, (batch, 3 * levels, h, w), 1, 1, fill=stack), Laid(dwt, (batch, 1, h, w))
            dl = Laid(dwt, (batch, 3 * levels, h, w), 1, 1, fill=np.repeat(LL[-1][:, None], 3 * levels, 1))
            st.iswt2d_batch(wavelet, 1, dh.ptr, dl.ptr, dh.batch, dh.plane, dh.pitch, batch, w, h, levels, out.ptr, out.batch, out.pitch, ops=o, params=p)
            outs.append(out.get()[:, 0])
            for b in (dh, dl, out):
                b.free()
    finally:
        dwt.set_option("swt2d_fused", 1)
    assert sm.same(outs[0], want) and sm.same(outs[1], want)


# ---- round trip on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_round_trip_on_the_device(dwt, st, wavelet):
    """forward and inverse on the device, normal inputs, the sizes and bounds of tests/test_iswt.py"""
    for n, levels in ROUND_TRIP_1D:
        x = sm.make_input(9000 + n + levels, "normal", 2, n)
        src, dh, dl, out = Dev(dwt, x), Dev(dwt, np.zeros((levels, 2, n), F32)), Dev(dwt, np.zeros((2, n), F32)), Dev(dwt, np.zeros((2, n), F32))
        st.swt1d_batch(wavelet, src.ptr, 4 * n, 4, 2, n, levels, dh.ptr, dl.ptr, 1, 8 * n, 4 * n, border=1)
        st.iswt1d_batch(wavelet, 1, dh.ptr, dl.ptr, 8 * n, 4 * n, 2, n, levels, out.ptr, 4 * n)
        err = float(np.abs(out.get().astype(np.float64) - x).max() / np.abs(x).max())
        print("1-D %s N %d levels %d: %.2e" % (wavelet, n, levels, err))
        assert err <= BOUND_1D, (n, levels, err)
        for b in (src, dh, dl, out):
            b.free()
    for h, w, levels in ROUND_TRIP_2D:
        x = m2.make_input(9100 + h + w, "normal", h, w)
        plane = 4 * h * w
        src, dh, dl, out = Dev(dwt, x), Dev(dwt, np.zeros((3 * levels, h, w), F32)), Dev(dwt, np.zeros((h, w), F32)), Dev(dwt, np.zeros((h, w), F32))
        st.swt2d_batch(wavelet, src.ptr, plane, 1, 4 * w, 4, w, h, levels, dh.ptr, dl.ptr, 1, 3 * levels * plane, plane, 4 * w, border=1)
        st.iswt2d_batch(wavelet, 1, dh.ptr, dl.ptr, 3 * levels * plane, plane, 4 * w, 1, w, h, levels, out.ptr, plane, 4 * w)
        err = float(np.abs(out.get().astype(np.float64) - x).max() / np.abs(x).max())
        print("2-D %s %d x %d levels %d: %.2e" % (wavelet, h, w, levels, err))
        assert err <= BOUND_2D, (h, w, levels, err)
        for b in (src, dh, dl, out):
            b.free()


# ---- host memory -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", sm.WAVELETS)
def test_host_memory(dwt, st, wavelet):
    """one host-memory case per entry, padded pitches, operators on the inverse (a ZERO plane holds NaN)"""
    lines, n, levels = 3, 77, 4
    x, L, H, y = expected1d(wavelet, "small_ints", lines, n, levels, 91)
    xs = np.full((lines, n + 3), -7.5, F32)
    xs[:, :n] = x
    gh, gl = np.full((levels, lines, n + 3), CANARY, np.uint32), np.full((1, lines, n + 3), CANARY, np.uint32)
    st.swt1d_batch(wavelet, xs, 4 * (n + 3), 4, lines, n, levels, gh, gl, 1, 4 * lines * (n + 3), 4 * (n + 3), border=1)
    assert sm.same(gh[:, :, :n].view(F32), H) and sm.same(gl[0, :, :n].view(F32), L[-1])
    assert (gh[:, :, n:] == CANARY).all() and (gl[:, :, n:] == CANARY).all()
    ops, params = tables(levels, 2)
    src_h = gh.view(F32).copy()
    src_h[ops == im.ZERO] = np.nan
    out = np.full((lines, 2 * n + 1), CANARY, np.uint32)
    st.iswt1d_batch(wavelet, 1, src_h, gl, 4 * lines * (n + 3), 4 * (n + 3), lines, n, levels, out, 4 * (2 * n + 1), 8, ops=ops, params=params)
    assert sm.same(out[:, :2 * n:2].view(F32), im.iswt_levels(L[-1], H, wavelet, ops, params))
    assert (out[:, 1::2] == CANARY).all()
    batch, h, w, levels = 2, 21, 40, 3
    x, LL, D, y = expected2d(wavelet, "normal", batch, h, w, levels, 92)
    gd, gll = np.full((batch, 3 * levels, h, w + 1), CANARY, np.uint32), np.full((batch, 3 * levels, h, w + 1), CANARY, np.uint32)
    plane = 4 * h * (w + 1)
    st.swt2d_batch(wavelet, x, 4 * h * w, batch, 4 * w, 4, w, h, levels, gd, gll, 1, 3 * levels * plane, plane, 4 * (w + 1), border=1)
    assert sm.same(gd[..., :w].view(F32).reshape(batch, levels, 3, h, w), D.transpose(2, 0, 1, 3, 4)) and sm.same(gll[:, 0, :, :w].view(F32), LL[-1])
    assert (gd[..., w:] == CANARY).all() and (gll[:, 1:] == CANARY).all()
    out = np.full((batch, h, w + 2), CANARY, np.uint32)
    st.iswt2d_batch(wavelet, 1, gd, gll, 3 * levels * plane, plane, 4 * (w + 1), batch, w, h, levels, out, 4 * h * (w + 2), 4 * (w + 2))
    assert sm.same(out[..., :w].view(F32), y) and (out[..., w:] == CANARY).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(dwt, st):
    """each refused call returns an error and leaves a sentinel-filled dst as it was"""
    lines, n, levels = 3, 32, 2
    dh, dl = Dev(dwt, np.zeros((levels, lines, n), F32)), Dev(dwt, np.zeros((lines, n), F32))
    out = Dev(dwt, np.full((lines, n), CANARY, np.uint32))
    host_out = np.full((lines, n), CANARY, np.uint32)

    def rows(wavelet="cdf97_s", border=1, src_h=dh.ptr, src_l=dl.ptr, ps=4 * n * lines, sls=4 * n, lines=lines, n=n, levels=levels, dst=out.ptr,
             dls=4 * n, des=4, ops=None, params=None):
        return lambda: st.iswt1d_batch(wavelet, border, src_h, src_l, ps, sls, lines, n, levels, dst, dls, des, ops, params)

    bad = [rows(border=0), rows(border=7), rows(ops=[st.BAND_COMPRESS, st.BAND_KEEP], params=[0.7, 0]), rows(ops=[6, 0], params=[0, 0]),
           rows(dst=dh.ptr + 4 * n), rows(dst=dl.ptr), rows(src_l=out.ptr + 8),  # overlaps
           rows(levels=25), rows(levels=-1), rows(wavelet="cdf53_i"), rows(wavelet="interp53_s"),
           rows(dst=host_out), rows(src_h=np.zeros((levels, lines, n), F32)), rows(src_l=np.zeros((lines, n), F32)),  # host and device mixed
           rows(src_h=dh.ptr + 2), rows(dls=4 * n + 2), rows(des=6), rows(sls=4 * n - 4), rows(ps=4 * n)]
    for i, f in enumerate(bad):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    assert "reconstruct" in str(pytest.raises(dwt.DwtError, rows(border=0)).value)
    batch, h, w = 2, 6, 32
    plane = 4 * h * w
    d2, l2 = Dev(dwt, np.zeros((batch, 3 * levels, h, w), F32)), Dev(dwt, np.zeros((batch, 3 * levels, h, w), F32))
    out2 = Dev(dwt, np.full((batch, h, w), CANARY, np.uint32))

    def images(wavelet="cdf53_s", border=1, src_h=d2.ptr, src_l=l2.ptr, sbs=3 * levels * plane, ps=plane, ssx=4 * w, batch=batch, w=w, h=h,
               levels=levels, dst=out2.ptr, dbs=plane, dsx=4 * w, dsy=4, ops=None, params=None):
        return lambda: st.iswt2d_batch(wavelet, border, src_h, src_l, sbs, ps, ssx, batch, w, h, levels, dst, dbs, dsx, dsy, ops, params)

    bad2 = [images(border=0), images(ops=[st.BAND_COMPRESS] * 6, params=[0.7] * 6), images(dst=d2.ptr + plane), images(dst=l2.ptr),
            images(levels=25), images(wavelet="cdf97_i"), images(dst=host_out), images(src_l=np.zeros((batch, h, w), F32)),
            images(batch=0), images(w=0), images(ps=plane - 4), images(sbs=plane), images(dbs=plane - 4), images(ssx=4 * w - 4), images(dsy=6),
            images(dst=out2.ptr + 2)]
    for i, f in enumerate(bad2):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    with pytest.raises(dwt.DwtError):
        st.swt1d_batch("cdf97_s", dl.ptr, 4 * n, 4, lines, n, levels, dh.ptr, border=2)
    with pytest.raises(dwt.DwtError):
        st.swt2d_batch("cdf97_s", l2.ptr, plane, 1, 4 * w, 4, w, h, levels, d2.ptr, border=-1)
    assert (out.get() == CANARY).all() and (out2.get() == CANARY).all() and (host_out == CANARY).all()
    assert not dh.get().any() and not dl.get().any() and not d2.get().any() and not l2.get().any()
    for b in (dh, dl, out, d2, l2, out2):
        b.free()


# ---- the caller's stream -----------------------------------------------------------------------------------------------------
def test_on_a_busy_stream():
    """the four new device entries on a busy non-blocking stream, in a process of its own (tests/iswt_stream.py, on the
    harness of tests/stream_cases.py): the model's bits, queued without waiting for the stream"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "iswt_stream.py")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]


# ---- the C example -----------------------------------------------------------------------------------------------------------
def test_c_example(dwt, tmp_path):
    """examples/swt_denoise.c: a resident batch, noise of a known sigma, forward under the symmetric border, inverse with a
    SOFT table: a PSNR gain above zero and a plain round trip within the bound"""
    exe, libdir = tmp_path / "swt_denoise", os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "swt_denoise.c"),
                           "-o", str(exe), "-L", libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    vals = dict(ln.split(":") for ln in out.stdout.splitlines() if ":" in ln)
    noisy, clean, rt = float(vals["PSNR noisy (dB)"]), float(vals["PSNR denoised (dB)"]), float(vals["round trip max error / max|x|"])
    assert clean - noisy > 0, out.stdout
    assert rt <= BOUND_2D, out.stdout
