"""CPU checks of the pixel front end's arithmetic as tests/pixels_model.py states it (include/libdwt_hip.h):
which depths the RCT and the ICT restore exactly, through which plane types; rounding and clamping of the inverse; the
model composed with the float 9/7 oracle; the header and the built library.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pixels_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENTRIES = ("dwt_hip_pixels_to_planes_batch", "dwt_hip_planes_to_pixels_batch", "dwt_hip_picture_forward_batch",
           "dwt_hip_picture_inverse_batch")


@pytest.fixture(scope="module")
def all_rgb8():
    """every one of the 2^24 8-bit triples, computed once and left unchanged"""
    a = np.arange(1 << 24, dtype=np.int64)
    p = np.stack([a >> 16, (a >> 8) & 255, a & 255], -1).astype(np.uint8)
    p.setflags(write=False)
    return p


def triples(depth, n, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, 1 << depth, (n, 3)), pm.corners(depth)]).astype(np.uint8 if depth <= 8 else np.uint16)


def ict_trip(pix, fmt, depth, plane):
    """(pixels restored exactly, the largest error before rounding, the fraction of samples that changed)"""
    off = 1 << (depth - 1)
    planes = pm.to_planes(pix, pm.RGB, off, 1.0, pm.ICT, plane)
    back = np.stack(pm.ict_inverse(*[planes[c].astype(F) for c in range(3)]), -1).astype(np.float64) + off
    got = pm.to_pixels(planes, fmt, pm.RGB, depth, off, 1.0, pm.ICT)
    return np.array_equal(got, pix), float(np.abs(back - pix).max()), float((got != pix).mean())


def test_rct_restores_every_8_bit_triple(all_rgb8):
    for order in (pm.RGB, pm.BGR):
        planes = pm.to_planes(all_rgb8, order, 128, 1.0, pm.RCT, pm.I16)
        assert planes.dtype == np.int16
        assert np.array_equal(pm.to_pixels(planes, pm.U8, order, 8, 128, 1.0, pm.RCT), all_rgb8)
    # components in the header's order whatever the pixel's: Y, U = B - G, V = R - G
    p = np.array([[200, 100, 50]], np.uint8)
    assert pm.to_planes(p, pm.RGB, 128, 1.0, pm.RCT, pm.I32)[:, 0].tolist() == [(72 - 2 * 28 - 78) >> 2, -78 - -28, 72 - -28]
    assert pm.to_planes(p[:, ::-1], pm.BGR, 128, 1.0, pm.RCT, pm.I32)[:, 0].tolist() == [(72 - 2 * 28 - 78) >> 2, -78 - -28, 72 - -28]


@pytest.mark.parametrize("depth", [12, 15])
def test_rct_through_int16_is_exact_up_to_depth_15(depth):
    pix = triples(depth, 1 << 20, depth)
    planes = pm.to_planes(pix, pm.RGB, 1 << (depth - 1), 1.0, pm.RCT, pm.I16)
    assert np.array_equal(pm.to_pixels(planes, pm.U16, pm.RGB, depth, 1 << (depth - 1), 1.0, pm.RCT), pix)


def test_rct_through_int16_at_depth_16_is_not_exact():
    """U and V need 17 bits: why the entries refuse the combination.  Through int32 planes it is exact."""
    pix = triples(16, 1 << 20, 16)
    p16 = pm.to_planes(pix, pm.RGB, 32768, 1.0, pm.RCT, pm.I16)
    assert not np.array_equal(pm.to_pixels(p16, pm.U16, pm.RGB, 16, 32768, 1.0, pm.RCT), pix)
    p32 = pm.to_planes(pix, pm.RGB, 32768, 1.0, pm.RCT, pm.I32)
    assert np.array_equal(pm.to_pixels(p32, pm.U16, pm.RGB, 16, 32768, 1.0, pm.RCT), pix)
    assert not pm.legal(pm.U16, 3, 16, pm.RCT, pm.I16) and pm.legal(pm.U16, 3, 16, pm.RCT, pm.I32) and pm.legal(pm.U16, 3, 15, pm.RCT, pm.I16)


def test_ict_binary32_restores_every_8_bit_triple(all_rgb8):
    exact, err, _ = ict_trip(all_rgb8, pm.U8, 8, pm.S)
    print("ICT binary32 depth 8: largest error before rounding %.5f" % err)
    assert exact and 0.0041 < err < 0.0042  # 0.00415


@pytest.mark.parametrize("depth, lo, hi", [(10, 0.0165, 0.0167), (12, 0.066, 0.0665)])
def test_ict_binary32_is_exact_at_depths_10_and_12(depth, lo, hi):
    exact, err, _ = ict_trip(triples(depth, 1 << 24, depth), pm.U16, depth, pm.S)
    print("ICT binary32 depth %d: largest error before rounding %.5f" % (depth, err))
    assert exact and lo < err < hi  # 0.0166, 0.0663


def test_ict_binary32_is_not_exact_at_depth_16():
    exact, err, changed = ict_trip(triples(16, 1 << 24, 16), pm.U16, 16, pm.S)
    print("ICT binary32 depth 16: largest error %.3f, %.1f %% of the samples change" % (err, 100 * changed))
    assert not exact and 1.0 < err < 1.1 and 0.12 < changed < 0.14  # 1.06, about 13 %


def test_ict_through_binary16_planes(all_rgb8):
    """exact pixels at depth 8 (error 0.088) and 10 (0.352), not at 12 (1.42)"""
    exact, err, _ = ict_trip(all_rgb8, pm.U8, 8, pm.H)
    assert exact and 0.087 < err < 0.089
    exact, err, _ = ict_trip(triples(10, 1 << 22, 10), pm.U16, 10, pm.H)
    assert exact and 0.34 < err < 0.36
    exact, err, changed = ict_trip(triples(12, 1 << 22, 12), pm.U16, 12, pm.H)
    assert not exact and 1.3 < err < 1.5 and changed > 0.01


@pytest.mark.parametrize("depth, fmt", [(8, pm.U8), (12, pm.U16), (16, pm.U16)])
def test_rounding_and_clamping_of_float_planes(depth, fmt):
    top = float(1 << depth)
    m = (1 << depth) - 1
    x = np.array([0.5, 1.5, 2.5, top - 1.5, top - 0.5, np.nan, np.inf, -np.inf, -0.0, -1.0, top, -0.5, top - 1.0], F)
    # ties to even: top - 1.5 -> top - 2 (even), top - 0.5 -> top (even), which then clamps
    want = [0, 2, 2, m - 1, m, 0, m, 0, 0, 0, m, 0, m]
    assert pm.float_pixel(x, 0, depth).tolist() == want
    planes = x.reshape(1, -1)
    assert pm.to_pixels(planes, fmt, pm.RGB, depth, 0, 1.0, pm.NONE)[:, 0].tolist() == want
    # NaN gives 0 whatever the offset; the offset is added after the rounding, exactly
    assert pm.float_pixel(np.array([np.nan, 0.5, -0.5, 1.5], F), 3, depth).tolist() == [0, 3, 3, 5]
    # binary16 planes widen exactly
    h = np.array([0.5, 1.5, np.nan, np.inf, -np.inf, -0.0, 65504.0], np.float16).reshape(1, -1)
    assert pm.to_pixels(h, fmt, pm.RGB, depth, 0, 1.0, pm.NONE)[:, 0].tolist() == [0, 2, 0, m, 0, 0, min(m, 65504)]


def test_int_path_wraps_and_clamps():
    big = np.iinfo(np.int32)
    s = np.array([big.max, big.max - 5, big.min, -1, 0, 255, 256, 70000], np.int32).reshape(1, -1)
    # + 128 wraps at INT_MAX: the two largest samples come out negative and clamp to 0
    assert pm.to_pixels(s, pm.U8, pm.RGB, 8, 128, 1.0, pm.NONE)[:, 0].tolist() == [0, 0, 0, 127, 128, 255, 255, 255]
    assert pm.to_pixels(s, pm.U16, pm.RGB, 16, 0, 1.0, pm.NONE)[:, 0].tolist() == [65535, 65535, 0, 0, 0, 255, 256, 65535]
    # int16 planes widen with their sign; the forward truncates to the plane's width
    assert pm.to_pixels(np.array([[-32768, 32767]], np.int16), pm.U16, pm.RGB, 16, 32768, 1.0, pm.NONE)[:, 0].tolist() == [0, 65535]
    assert pm.to_planes(np.array([[0], [65535]], np.uint16), pm.RGB, 32768, 1.0, pm.NONE, pm.I16)[0].tolist() == [-32768, 32767]
    assert pm.to_planes(np.array([[65535]], np.uint16), pm.RGB, 0, 1.0, pm.NONE, pm.I16)[0].tolist() == [-1]
    # the RCT's sums wrap in 32 bits (an offset far outside the pixel range)
    y = pm.to_planes(np.array([[0, 0, 0]], np.uint8), pm.RGB, -(1 << 30), 1.0, pm.RCT, pm.I32)
    assert y[:, 0].tolist() == [0, 0, 0]  # 4 * 2^30 wraps to 0


def test_fourth_channel_never_takes_the_component_transform():
    rng = np.random.default_rng(4)
    pix = rng.integers(0, 256, (50, 4)).astype(np.uint8)
    for colour, plane in ((pm.RCT, pm.I16), (pm.ICT, pm.S)):
        planes = pm.to_planes(pix, pm.BGR, 128, 1.0, colour, plane)
        assert np.array_equal(planes[3], pm.to_planes(pix[:, 3:], pm.RGB, 128, 1.0, pm.NONE, plane)[0])
        assert np.array_equal(pm.to_pixels(planes, pm.U8, pm.BGR, 8, 128, 1.0, colour), pix)


def test_scale_is_one_rounding():
    pix = np.arange(256, dtype=np.uint8).reshape(-1, 1)
    planes = pm.to_planes(pix, pm.RGB, 128, 1.0 / 256, pm.NONE, pm.S)
    assert np.array_equal(planes[0], ((np.arange(256) - 128) / 256.0).astype(F))
    assert np.array_equal(pm.to_pixels(planes, pm.U8, pm.RGB, 8, 128, 256.0, pm.NONE), pix)


def test_pipeline_ict_and_float_97_on_the_model():
    """a 5-level CDF97_S round trip of a 64 x 48 ICT picture returns the 8-bit pixels exactly (the model and the oracle)"""
    import f16_model

    orc = f16_model.oracle()
    rng = np.random.default_rng(97)
    pix = rng.integers(0, 256, (48, 64, 3)).astype(np.uint8)
    planes = pm.to_planes(pix, pm.RGB, 128, 1.0, pm.ICT, pm.S)
    for c in range(3):
        a = planes[c].copy()
        assert orc.fwd("cdf97_2f_s", a, 5) == 5
        assert not np.array_equal(a, planes[c])
        orc.inv("cdf97_2i_s", a, 5)
        planes[c] = a
    assert np.array_equal(pm.to_pixels(planes, pm.U8, pm.RGB, 8, 128, 1.0, pm.ICT), pix)


def test_header_declares_and_library_exports_the_entries():
    text = open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    import libdwt_amd
    from libdwt_amd import pixels

    for name in ENTRIES + ("dwt_hip_pixels_route",):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(libdwt_amd.lib, name), name
    # the constant tables of the Python mirror are the header's
    for py, c_name in ((pixels.U8, "DWT_HIP_PIX_U8"), (pixels.U16, "DWT_HIP_PIX_U16"), (pixels.BGR, "DWT_HIP_ORDER_BGR"),
                       (pixels.RCT, "DWT_HIP_COLOUR_RCT"), (pixels.ICT, "DWT_HIP_COLOUR_ICT"), (pixels.I16, "DWT_HIP_PLANE_I16"),
                       (pixels.I32, "DWT_HIP_PLANE_I32"), (pixels.H, "DWT_HIP_PLANE_H"), (pixels.S, "DWT_HIP_PLANE_S")):
        assert re.search(r"\b%s\s*=\s*%d\b" % (c_name, py), text), c_name
    for py, c_name in ((pixels.PIXELS_PER_LANE, "DWT_HIP_PIXELS_PER_LANE"), (pixels.GRID_ROWS, "DWT_HIP_PIXELS_GRID_ROWS"),
                       (pixels.GRID_BATCH, "DWT_HIP_PIXELS_GRID_BATCH")):
        assert re.search(r"#define\s+%s\s+%d\b" % (c_name, py), text), c_name
    assert (pm.U8, pm.U16, pm.RGB, pm.BGR, pm.NONE, pm.RCT, pm.ICT, pm.I16, pm.I32, pm.H, pm.S) == (
        pixels.U8, pixels.U16, pixels.RGB, pixels.BGR, pixels.NONE, pixels.RCT, pixels.ICT, pixels.I16, pixels.I32, pixels.H, pixels.S)
    # the package namespace is unchanged: the entries live in the submodule only
    assert not [n for n in dir(libdwt_amd) if "pixel" in n and callable(getattr(libdwt_amd, n))]


def test_refusals_need_no_device():
    """what the header refuses is refused before the device is touched"""
    import libdwt_amd as dwt
    from libdwt_amd import pixels

    pix = np.full(3 * 8 * 8, 7, np.uint8)
    planes = np.full(3 * 8 * 8, -9, np.int32)

    def refused(fmt=pixels.U8, channels=3, depth=8, scale=1.0, colour=pixels.NONE, plane=pixels.I32, planes_=None):
        with pytest.raises(dwt.DwtError) as e:
            pixels.pixels_to_planes_batch(fmt, pix, channels * 64, channels * 8, channels, 1, 1, channels, pixels.RGB, depth, 128, scale,
                                          colour, plane, planes if planes_ is None else planes_, 8 * 8 * 4, 8 * 4, 8, 8)
        assert len(str(e.value)) > 30
        assert (planes == -9).all() and (pix == 7).all()

    refused(colour=pixels.RCT, plane=pixels.S)
    refused(colour=pixels.RCT, plane=pixels.H)
    refused(colour=pixels.ICT, plane=pixels.I32)
    refused(colour=pixels.ICT, plane=pixels.I16)
    refused(scale=0.5)
    refused(colour=pixels.RCT, channels=1)
    refused(depth=9)
    refused(depth=0)
    refused(fmt=pixels.U16, depth=17, plane=pixels.I32)
    refused(fmt=pixels.U16, depth=16, colour=pixels.RCT, plane=pixels.I16)
    refused(channels=2)
    refused(channels=5)
    refused(planes_=pix[16:].view(np.uint8))  # the planes inside the pixels
    for wavelet in (dwt.CDF97_D, dwt.CDF53_D):
        with pytest.raises(dwt.DwtError):
            pixels.picture_forward_batch(wavelet, pixels.U8, pix, 192, 24, 3, 1, 1, 3, pixels.RGB, 8, 128, 1.0, pixels.NONE, planes, 256, 32, 8, 8)
    # 21846 * 3 planes of 1 x 1: past the batched transform's 65535 (buffers as large as the call describes)
    many_pix, many_planes = np.full(21846 * 3, 7, np.uint8), np.full(21846 * 3, -9, np.int32)
    with pytest.raises(dwt.DwtError) as e:
        pixels.picture_forward_batch(dwt.CDF53_I, pixels.U8, many_pix, 3, 3, 3, 1, 21846, 3, pixels.RGB, 8, 128, 1.0, pixels.NONE, many_planes, 4, 4,
                                     1, 1)
    assert "65535" in str(e.value)
    # a row pitch the batched transform's int cannot hold, refused before any byte is addressed (the pixels in front of the
    # planes in one buffer, so that the region the pitch describes cannot run into them)
    both = np.full(1024, 7, np.uint8)
    with pytest.raises(dwt.DwtError) as e:
        pixels.picture_forward_batch(dwt.CDF53_I, pixels.U8, both[:16], 16, 8, 1, 1, 1, 1, pixels.RGB, 8, 128, 1.0, pixels.NONE, both[256:], 1 << 33,
                                     1 << 31, 8, 2)
    assert "2 GiB" in str(e.value) and (both == 7).all()
    assert (planes == -9).all() and (many_planes == -9).all() and (many_pix == 7).all()
