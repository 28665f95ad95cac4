"""The pixel front end (include/libdwt_hip.h) restated in numpy: unsigned pixels <-> wavelet planes with the
DC level shift and the RCT / ICT of ITU-T T.800 Annex G.

Arrays are logical, not laid out: pixels (..., C) unsigned with the channels last in the pixel's own order, planes
(C, ...) with the components first (Y, Cb / U, Cr / V, then a fourth channel that never takes the component transform).
Integer paths run in np.int32, whose array arithmetic wraps; float paths in np.float32 with every product and every sum
an operation of its own, so each is rounded once; the pixel is np.rint (ties to even) of the binary32 value, the offset
is added exactly (float64 holds every sum that matters), NaN gives 0."""
import numpy as np

U8, U16 = 0, 1
RGB, BGR = 0, 1
NONE, RCT, ICT = 0, 1, 2
I16, I32, H, S = 0, 1, 2, 3
PIXEL_DTYPE = {U8: np.uint8, U16: np.uint16}
PLANE_DTYPE = {I16: np.int16, I32: np.int32, H: np.float16, S: np.float32}
F = np.float32


def is_float(plane):
    return plane in (H, S)


def legal(fmt, channels, depth, colour, plane, scale=1.0):
    """the combinations the entries take (the header's list of errors, without the memory ones)"""
    if channels not in (1, 3, 4) or not 1 <= depth <= (8 if fmt == U8 else 16):
        return False
    if colour == RCT and is_float(plane) or colour == ICT and not is_float(plane):
        return False
    if not is_float(plane) and scale != 1.0:
        return False
    if colour != NONE and channels < 3:
        return False
    return not (colour == RCT and plane == I16 and depth == 16)


def _rgb(chans, order):
    """the first three channels as (R, G, B)"""
    return (chans[2], chans[1], chans[0]) if order == BGR else (chans[0], chans[1], chans[2])


def rct_forward(R, G, B):
    """int32 arrays, wrapping; >> is arithmetic"""
    return (R + (G + G) + B) >> 2, B - G, R - G


def rct_inverse(Y, U, V):
    G = Y - ((U + V) >> 2)
    return V + G, G, U + G


def ict_forward(R, G, B):
    """float32 arrays: every product and sum rounded on its own, in the header's order"""
    Y = (F(0.299) * R + F(0.587) * G) + F(0.114) * B
    Cb = (F(-0.16875) * R + F(-0.33126) * G) + F(0.5) * B
    Cr = (F(0.5) * R + F(-0.41869) * G) + F(-0.08131) * B
    return Y, Cb, Cr


def ict_inverse(Y, Cb, Cr):
    R = Y + F(1.402) * Cr
    G = (Y + F(-0.34413) * Cb) + F(-0.71414) * Cr
    B = Y + F(1.772) * Cb
    return R, G, B


def to_planes(pix, order, offset, scale, colour, plane):
    """pix (..., C) unsigned -> planes (C, ...) of PLANE_DTYPE[plane]"""
    pix = np.asarray(pix)
    C = pix.shape[-1]
    with np.errstate(over="ignore", invalid="ignore"):
        v = [pix[..., c].astype(np.int64).astype(np.int32) - np.int32(offset) for c in range(C)]
        if not is_float(plane):
            assert scale == 1.0
            if colour == RCT:
                v[:3] = rct_forward(*_rgb(v, order))
            return np.stack([c.astype(PLANE_DTYPE[plane]) for c in v])
        f = [c.astype(F) * F(scale) for c in v]
        if colour == ICT:
            f[:3] = ict_forward(*_rgb(f, order))
        return np.stack([c.astype(PLANE_DTYPE[plane]) for c in f])


def float_pixel(x, offset, depth):
    """binary32 samples -> pixel values (int64): rint, + offset, clamp; NaN gives 0"""
    with np.errstate(invalid="ignore"):
        r = np.rint(np.asarray(x, F))
        t = np.clip(r.astype(np.float64) + float(offset), 0.0, float((1 << depth) - 1))
    return np.where(np.isnan(r), 0.0, t).astype(np.int64)


def int_pixel(s, offset, depth):
    """int32 samples -> pixel values: + offset (wrapping), clamp"""
    with np.errstate(over="ignore"):
        return np.clip(np.asarray(s, np.int32) + np.int32(offset), 0, (1 << depth) - 1).astype(np.int64)


def to_pixels(planes, fmt, order, depth, offset, scale, colour):
    """planes (C, ...) -> pix (..., C) of PIXEL_DTYPE[fmt]; the plane type is the array's dtype"""
    planes = np.asarray(planes)
    C = planes.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        if np.issubdtype(planes.dtype, np.integer):
            assert scale == 1.0
            s = [planes[c].astype(np.int32) for c in range(C)]
            if colour == RCT:
                s[:3] = _rgb(rct_inverse(*s[:3]), order)  # (R, G, B) -> the pixel's order: the swap is its own inverse
            out = [int_pixel(c, offset, depth) for c in s]
        else:
            s = [planes[c].astype(F) for c in range(C)]
            if colour == ICT:
                s[:3] = _rgb(ict_inverse(*s[:3]), order)
            out = [float_pixel(c * F(scale), offset, depth) for c in s]
    return np.stack(out, axis=-1).astype(PIXEL_DTYPE[fmt])


def corners(depth):
    m = (1 << depth) - 1
    return np.array([[r, g, b] for r in (0, m) for g in (0, m) for b in (0, m)], np.int64)
