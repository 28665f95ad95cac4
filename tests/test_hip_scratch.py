"""The scratch contract (include/libdwt_hip.h): the content of every scratch buffer is unspecified on entry
to any call and no result depends on it; no sweep stores outside the LL band it was given.

Every other tests/test_hip_*.py runs with the poison mode of the package on (libdwt_amd.poison_workspace), which holds the
whole suite to the first half.  This file adds what that mode cannot see:

  - a caller-owned LL workspace of EXACTLY the documented size between guards (hipdev.GuardedWorkspace), under every 2-D
    sweep family at the edge shapes and under the knob extremes that move a store: a sweep that stores past its band hits a
    guard, one that fails to store part of it reads NaN;
  - what the bands hold after a call, against the oracle's own level-1 and level-2 LL bands -- the control that shows the
    test looks at the memory the kernels use -- and the band that the fused pair of levels 0 and 1 never writes;
  - the size rule of dwt_hip_set_workspace, the fill entry itself, and the in-place and host-pointer routes (stage_img,
    frame_a), which a caller-owned workspace does not reach, behind an explicit fill.

Inputs: floatends.finite_floats and conftest.full_range_ints (narrowed to int16 for the int16 5/3).  The expected results
are asserted free of NaN, so a NaN in a device result can only be the poison.  Expectation: the oracle's bits (interp53,
int16 5/3 and binary16 9/7: their models', as in their own GPU tests)."""
import os
import warnings

import numpy as np
import pytest

import f16_model
import floatends as F
import hipdev
import i16_model
from conftest import full_range_ints

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

PLAIN_BUILD = os.path.basename(os.environ.get("DWT_HIP_LIB", "")).startswith("libdwt_hip_plain")
KNOBS = ("cpt", "ring", "nt", "tile_pairs", "waves", "ring_inv", "fuse01", "ride_copy")
DEFAULTS = {}
# the extremes of the sweep knobs that move a store
SETTINGS = [{}, dict(cpt=8, ring=16), dict(nt=15), dict(tile_pairs=64, waves=1), dict(ring_inv=16)]
# wavelet -> (dtype, how the expectation is made)
WAVELETS = {"cdf97_s": np.float32, "cdf53_s": np.float32, "cdf53_i": np.int32, "cdf97_i": np.int32, "interp53_s": np.float32,
            "cdf97_d": np.float64, "cdf53_d": np.float64, "cdf53_i16": np.int16, "cdf97_h": np.float16}
SHAPES = F.SWEEP_SHAPES + [(132, 1028)]
SENTINEL = 7


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    DEFAULTS.update({k: d.get_option(k) for k in KNOBS})
    d.poison_workspace(hipdev.POISON)
    yield d
    d.poison_workspace(None)
    restore(d)
    d.dwt_util_set_accel(0)
    d.lib.dwt_hip_set_workspace(None, 0, None, 0)
    d.dwt_util_finish()


def bits(a):
    """the words of an array of 2-, 4- or 8-byte elements (conftest.bits takes the last two)"""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def restore(dwt):
    for k, v in DEFAULTS.items():
        dwt.set_option(k, v)


def model(oracle, wavelet, inverse, a, j):
    """(result, levels) of the dense image `a` by the CPU statement of `wavelet`; `a` is left as it is"""
    if wavelet in ("cdf53_i", "cdf97_i"):
        b = a.copy()
        return b, (oracle.inv if inverse else oracle.fwd)("%s_2%s_i" % (wavelet[:5], "i" if inverse else "f"), b, j)
    if wavelet in ("cdf53_i16", "cdf97_h"):
        m, b = (i16_model if wavelet == "cdf53_i16" else f16_model), a.copy()
        jo = (m.inv2d if inverse else m.fwd2d)(b, j_max=j)
        return b, (j if inverse else jo)
    with (F.reflected_ends(oracle) if PLAIN_BUILD else warnings.catch_warnings()):
        return F.transform(oracle, "interp53_2d" if wavelet == "interp53_s" else wavelet, inverse, a, j)


def make_input(wavelet, shape, seed):
    dt = WAVELETS[wavelet]
    rng = np.random.default_rng(seed)
    if dt == np.int32:
        return full_range_ints(rng, shape)
    if dt == np.int16:
        return full_range_ints(rng, shape).astype(np.int16)  # (the low halves: the whole int16 range, the specials' low bits)
    return F.finite_floats(rng, shape, dt)


def clean(a):
    return True if np.issubdtype(a.dtype, np.integer) else not np.isnan(a).any()


class Batch:
    """`nb` images of (h, w) in device memory, rows `pitch` elements apart (2-byte elements: an even count, so that every
    base, pitch and batch stride is a multiple of 4 bytes and the fused sweeps run), the padding a sentinel that must stay."""

    def __init__(self, dwt, dt, nb, shape):
        self.dwt, self.dt, self.nb, (self.h, self.w) = dwt, np.dtype(dt), nb, shape
        self.pitch = self.w + (self.w & 1 if self.dt.itemsize == 2 else 0)
        self.host = np.full((nb, self.h, self.pitch), SENTINEL, dt)
        self.dev = hipdev.Dev(dwt, self.host)

    def put(self, imgs):
        self.host[:] = SENTINEL
        if imgs is not None:
            self.host[:, :, :self.w] = imgs
        assert self.dwt.lib.dwt_hip_memcpy_h2d(self.dev.ptr, self.host.ctypes.data, self.host.nbytes) == 0
        return self

    def get(self):
        got = self.dev.get()
        assert (bits(got[:, :, self.w:]) == bits(np.full(1, SENTINEL, self.dt))[0]).all(), "padding written"
        return np.ascontiguousarray(got[:, :, :self.w])

    def free(self):
        self.dev.free()


def t2d_batch(dwt, wavelet, inverse, src, dst, j):
    es = src.dt.itemsize
    return dwt.transform2d_batch(wavelet, inverse, src.dev.ptr, dst.dev.ptr, src.pitch * src.h * es, src.nb, src.pitch * es, src.w, src.h, j)


# ---- exact, guarded bands under every 2-D sweep family ------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("wavelet", list(WAVELETS))
def test_exact_guarded_bands_under_every_sweep_family(dwt, oracle, wavelet, shape):
    """A batch of 3 at full depth through dwt_hip_transform2d_batch, forward and inverse, the LL bands the caller's, of exactly
    the documented size, poisoned, between guards: under the default options and under each extreme of SETTINGS -- on
    (132, 1028) also 3 levels under fuse01 = 2 -- the oracle's bits, intact guards, an unmodified source."""
    nb, (h, w), dt = 3, shape, WAVELETS[wavelet]
    imgs = np.stack([make_input(wavelet, shape, 1000 * h + w + b) for b in range(nb)])
    runs = [(-1, s) for s in SETTINGS] + ([(3, dict(fuse01=2))] if shape == (132, 1028) else [])
    want = {}
    for j in sorted({j for j, _ in runs}):
        f = [model(oracle, wavelet, 0, imgs[b], j) for b in range(nb)]
        jo = f[0][1]
        wf = np.stack([x[0] for x in f])
        wi = np.stack([model(oracle, wavelet, 1, wf[b], jo)[0] for b in range(nb)])
        assert clean(wf) and clean(wi), "the expectation itself holds a NaN"
        want[j] = (jo, wf, wi)
    src, dst = Batch(dwt, dt, nb, shape), Batch(dwt, dt, nb, shape)
    ws = hipdev.GuardedWorkspace(dwt, wavelet, nb, w, h)
    try:
        for j, opts in runs:
            jo, wf, wi = want[j]
            for k, v in opts.items():
                dwt.set_option(k, v)
            for inverse, inp, exp in ((0, imgs, wf), (1, wf, wi)):
                src.put(inp)
                dst.put(None)
                ws.arm()
                assert t2d_batch(dwt, wavelet, inverse, src, dst, j if not inverse else jo) == jo, (opts, inverse)
                got = dst.get()
                ws.check()
                assert np.array_equal(bits(got), bits(exp)), (opts, "inverse" if inverse else "forward", int((bits(got) != bits(exp)).sum()),
                                                              "NaN in the result: %d" % (0 if dt in (np.int32, np.int16) else int(np.isnan(got).sum())))
                assert np.array_equal(bits(src.get()), bits(inp)), (opts, inverse, "source modified")
            restore(dwt)
    finally:
        restore(dwt)
        ws.close()
        src.free()
        dst.free()


# ---- what the scratch holds afterwards -----------------------------------------------------------------------------------
def ll_of(oracle, img, levels):
    """the LL band after `levels` levels of the float 9/7, by the oracle"""
    out, jo = model(oracle, "cdf97_s", 0, img, levels)
    assert jo == levels
    h, w = img.shape
    return out[:(h + (1 << levels) - 1) >> levels, :(w + (1 << levels) - 1) >> levels]


def band_image(words, rows, width):
    """(the rows x pitch image at the start of a band, the words behind it)"""
    pitch = (width + 3) // 4 * 4
    return words[:rows * pitch].reshape(rows, pitch), words[rows * pitch:]


def forward_s2(dwt, img, J):
    h, w = img.shape
    src, dst = dwt.DeviceImage(h, w).upload(img), dwt.DeviceImage(h, w).upload(np.full_like(img, SENTINEL))
    try:
        assert dwt.dwt_cdf97_2f_s2(src.ptr, dst.ptr, dst.stride_x, 4, w, h, w, h, J) == J
        return dst.download(np.float32)
    finally:
        src.free()
        dst.free()


def test_the_bands_hold_the_oracles_ll_bands(dwt, oracle):
    """The control: after the 3-level out-of-place float 9/7 forward of one (131, 1030) image, level by level (fuse01 = 0),
    band 0 holds the oracle's level-1 LL band (66 rows of 515 at pitch 516) and band 1 its level-2 band (33 rows of 258 at
    pitch 260), bit for bit; every word behind those rows still holds the poison.  (The pad columns inside the pitch belong
    to the rows' 16-byte stores: their content is unspecified.)"""
    h, w, J = 131, 1030, 3
    img = make_input("cdf97_s", (h, w), 131)
    want, _ = model(oracle, "cdf97_s", 0, img, J)
    ws = hipdev.GuardedWorkspace(dwt, "cdf97_s", 1, w, h)
    try:
        dwt.set_option("fuse01", 0)
        ws.arm()
        got = forward_s2(dwt, img, J)
        bands = ws.check()
        assert np.array_equal(bits(got), bits(want))
        for k, (rows, width) in enumerate(((66, 515), (33, 258))):
            ll = ll_of(oracle, img, k + 1)
            assert ll.shape == (rows, width) and not np.isnan(ll).any()
            image, rest = band_image(bands[k], rows, width)
            assert np.array_equal(image[:, :width], bits(ll)), "band %d is not the level-%d LL band" % (k, k + 1)
            assert len(rest) == 16 and (rest == hipdev.POISON).all(), "band %d: words behind its rows written" % k
    finally:
        restore(dwt)
        ws.close()


def test_the_fused_pair_never_writes_band_0(dwt, oracle):
    """Under fuse01 = 2 on (132, 1028) with 3 levels the fused launch of levels 0 and 1 never writes level 0's LL band (its
    own stated property): every word of band 0 still holds the poison, band 1 holds the oracle's level-2 band, and the call
    took 2 launches."""
    h, w, J = 132, 1028, 3
    img = make_input("cdf97_s", (h, w), 132)
    want, _ = model(oracle, "cdf97_s", 0, img, J)
    ws = hipdev.GuardedWorkspace(dwt, "cdf97_s", 1, w, h)
    try:
        dwt.set_option("fuse01", 2)
        ws.arm()
        n = hipdev.launches(dwt, lambda: np.testing.assert_array_equal(bits(forward_s2(dwt, img, J)), bits(want)))
        bands = ws.check()
        assert n == 2, "the fused pair did not run"
        assert (bands[0] == hipdev.POISON).all(), "%d words of band 0 written" % int((bands[0] != hipdev.POISON).sum())
        image, rest = band_image(bands[1], 33, 257)
        assert np.array_equal(image[:, :257], bits(ll_of(oracle, img, 2))) and (rest == hipdev.POISON).all()
    finally:
        restore(dwt)
        ws.close()


def test_the_guards_see_a_stray_word_next_to_a_band(dwt):
    """The control of the guards: one word stored right behind the last byte of a band of the documented size, or right in
    front of its first, fails check() -- the guards start where the band ends, with no slack of their own."""
    ws = hipdev.GuardedWorkspace(dwt, "cdf97_s", 3, 259, 67)
    stray = np.array([0], np.uint32)
    try:
        for k in range(2):
            for where in (hipdev.GUARD + ws.bytes[k], hipdev.GUARD - 4):
                ws.arm()
                ws.check()
                assert dwt.lib.dwt_hip_memcpy_h2d(ws.bufs[k].ptr + where, stray.ctypes.data, 4) == 0
                with pytest.raises(AssertionError, match="band %d: 1 words written" % k):
                    ws.check()
    finally:
        ws.close()


# ---- the size rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [(1, 0), (0, 1)], ids=["band0", "band1"])
def test_one_byte_less_is_refused_and_nothing_is_written(dwt, short):
    """Bands of exactly the documented size are accepted (every test above); one byte less in either is refused with the
    "too small" error before anything is written: dst keeps its canary, the bands their poison."""
    nb, shape = 3, (67, 259)
    src, dst = Batch(dwt, np.float32, nb, shape).put(np.stack([make_input("cdf97_s", shape, b) for b in range(nb)])), Batch(dwt, np.float32, nb, shape).put(None)
    ws = hipdev.GuardedWorkspace(dwt, "cdf97_s", nb, shape[1], shape[0], short=short)
    try:
        with pytest.raises(dwt.DwtError, match="too small: band %d needs %d bytes" % (short[1], ws.bytes[short[1]])):
            t2d_batch(dwt, "cdf97_s", 0, src, dst, -1)
        assert (bits(dst.dev.get()) == bits(np.full(1, SENTINEL, np.float32))[0]).all(), "dst written by a refused call"
        assert all((b == hipdev.POISON).all() for b in ws.check())
    finally:
        ws.close()
        src.free()
        dst.free()


def test_interleaved_entry_under_a_callers_workspace_is_refused(dwt):
    h, w = 64, 80
    img = make_input("cdf97_s", (h, w), 5)
    d = dwt.DeviceImage(h, w).upload(img)
    ws = hipdev.GuardedWorkspace(dwt, "cdf97_s", 1, w, h)
    try:
        with pytest.raises(dwt.DwtError, match="hand it back first"):
            dwt.dwt_cdf97_2f_inplace_s(d.ptr, w * 4, 4, w, h, w, h, -1)
        assert np.array_equal(bits(d.download(np.float32)), bits(img))
        ws.check()
    finally:
        ws.close()
        d.free()


# ---- the fill entry itself -------------------------------------------------------------------------------------------------
def test_fill_reaches_every_word_of_a_callers_workspace(dwt):
    """dwt_hip_fill_workspace(w) leaves every word of both caller-owned bands equal to w, for two different words, touches
    no guard, and counts neither as a launch nor as an allocation."""
    ws = hipdev.GuardedWorkspace(dwt, "cdf97_s", 3, 259, 67)
    try:
        for word in (0x11223344, 0x80000001):
            ws.arm()
            n0, a0 = dwt.get_option("stat_launches"), dwt.get_option("stat_allocs")
            dwt.fill_workspace(word)
            assert (dwt.get_option("stat_launches"), dwt.get_option("stat_allocs")) == (n0, a0)
            for k, b in enumerate(ws.check()):
                assert (b == word).all(), (k, hex(word), int((b != word).sum()))
    finally:
        ws.close()


def test_the_poison_mode_fills_in_front_of_a_call(dwt, oracle):
    """What every GPU module's fixture relies on: while poison_workspace is on, a call made through the package is preceded by
    the fill.  A one-level forward never touches the LL bands (its LL goes to its final place), so what they hold after it
    is what they held before it: the mode's word while the switch is on, the armed word while it is off."""
    h, w = 67, 259
    img = make_input("cdf97_s", (h, w), 67)
    want, _ = model(oracle, "cdf97_s", 0, img, 1)
    armed = 0x12345678
    ws = hipdev.GuardedWorkspace(dwt, "cdf97_s", 1, w, h, poison=armed)
    try:
        for mode, held in ((hipdev.POISON, hipdev.POISON), (None, armed), (0x0BADF00D, 0x0BADF00D)):
            dwt.poison_workspace(mode)
            ws.arm()
            assert np.array_equal(bits(forward_s2(dwt, img, 1)), bits(want))
            for k, b in enumerate(ws.check()):
                assert (b == held).all(), (mode, k, hex(int(b[0])))
    finally:
        dwt.poison_workspace(hipdev.POISON)
        ws.close()


def test_fill_gives_trailing_bytes_the_words_low_bytes(dwt):
    """Bands told one byte short of a multiple of 4: the last 3 bytes get the word's low bytes, the byte behind them stays."""
    ws = hipdev.GuardedWorkspace(dwt, "cdf97_s", 3, 259, 67, short=(1, 1))
    try:
        ws.arm()
        dwt.fill_workspace(0x11223344)
        for b in ws.check():
            assert (b[:-1] == 0x11223344).all() and b[-1] == 0xFF223344, hex(int(b[-1]))
    finally:
        ws.close()


def test_rows_warnings_after_a_fill_answers_as_before_any_call(dwt):
    """The warning counters of a conditioning call lie in scratch: after a fill the query fails as before any such call."""
    rows = hipdev.Dev(dwt, make_input("cdf97_s", (4, 64), 9))
    try:
        dwt.rows_condition(7, rows.ptr, 64 * 4, 4, 4, 64, 20, -1.0, 2.5)
        assert len(dwt.rows_warnings()) == 2
        dwt.fill_workspace(hipdev.POISON)
        with pytest.raises(dwt.DwtError, match="precedes on this thread"):
            dwt.rows_warnings()
        dwt.rows_condition(7, rows.ptr, 64 * 4, 4, 4, 64, 20, -1.0, 2.5)
        assert len(dwt.rows_warnings()) == 2
    finally:
        rows.free()


# ---- the routes a caller-owned workspace does not reach ---------------------------------------------------------------------
@pytest.mark.parametrize("route", ["device ride_copy 1", "device ride_copy 0", "host accel 0", "host accel 1"])
def test_in_place_and_staged_routes_behind_a_fill(dwt, oracle, route):
    """dwt_cdf97_2f_s / _2i_s in place on a (771, 517) image at pitch 520, at full depth: on the device with the staged
    subbands' copy riding along and as a launch of its own (stage_img), and through the host-pointer entry on the fused
    sweeps and on the line passes (frame_a, frame_b).  Each call behind an explicit fill; the oracle's bits, the padding kept."""
    h, w, pe = 771, 517, 520
    buf = F.finite_floats(np.random.default_rng(771), (h, pe))
    want = buf.copy()
    with (oracle.reflected_ends() if PLAIN_BUILD else warnings.catch_warnings()):
        J = oracle.fwd("cdf97_2f_s", want[:, :w], -1)
        back = want.copy()
        oracle.inv("cdf97_2i_s", back[:, :w], J)
    assert not np.isnan(want).any() and not np.isnan(back).any()
    kind, opt, val = route.split()
    try:
        if kind == "device":
            dwt.set_option(opt, int(val))
            d = dwt.DeviceImage(h, w, pitch_bytes=pe * 4).upload(buf)
            try:
                dwt.fill_workspace(hipdev.POISON)
                assert dwt.dwt_cdf97_2f_s(d.ptr, pe * 4, 4, w, h, w, h, -1) == J
                assert np.array_equal(bits(d.download(np.float32)), bits(want)), "forward"
                dwt.fill_workspace(hipdev.POISON)
                dwt.dwt_cdf97_2i_s(d.ptr, pe * 4, 4, w, h, w, h, J)
                assert np.array_equal(bits(d.download(np.float32)), bits(back)), "inverse"
            finally:
                d.free()
        else:
            dwt.dwt_util_set_accel(int(val))
            got = buf.copy()
            dwt.fill_workspace(hipdev.POISON)
            assert dwt.dwt_cdf97_2f_s(got, pe * 4, 4, w, h, w, h, -1) == J
            assert np.array_equal(bits(got), bits(want)), "forward"
            dwt.fill_workspace(hipdev.POISON)
            dwt.dwt_cdf97_2i_s(got, pe * 4, 4, w, h, w, h, J)
            assert np.array_equal(bits(got), bits(back)), "inverse"
    finally:
        dwt.dwt_util_set_accel(0)
        restore(dwt)
