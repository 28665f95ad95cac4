"""User-defined lifting wavelets (include/libdwt_hip.h): multi-level Mallat transforms of image batches by a
lifting scheme described in a small table -- Haar, Daubechies D4, the S transform, a filter of one's own --, binary32 or
reversible int32.  A submodule of its own: import it as ``from libdwt_amd import lifting``.

    d4 = lifting.builtin("D4")
    J = lifting.lifting2d_batch(d4, False, src, dst, 4 * W * H, B, 4 * W, 4, W, H)      # forward, all levels
    lifting.lifting2d_batch(d4, True, dst, dst, 4 * W * H, B, 4 * W, 4, W, H, J)         # inverse, in place

    mine = lifting.scheme(lifting.F32, [lifting.step(1, [(-0.5, -1, 1)]), lifting.step(0, [(0.25, -1, 1)])],
                          fwd_scale=(2 ** .5, .5 ** .5), inv_scale=(.5 ** .5, 2 ** .5))

Pointers are numpy arrays, torch tensors or integer addresses, src and dst both host or both device memory.  The planes are
plain Mallat planes: bands_apply_batch, the quantizer, the sparse streams and the feature statistics take them.

Line batches: lifting1d_batch leaves the 1-D Mallat layout of transform1d_batch, every level of lines of up
to 8192 samples in one launch; norms and quant_steps give a float scheme's synthesis norms and the quantizer's step table.

    J = lifting.lifting1d_batch(d4, False, rows, rows, 4 * N, 4, n_rows, N)               # forward, all levels, in place
    steps = lifting.quant_steps(d4, J, 1 / 256)
"""
import ctypes as C

from . import DwtError, _addr, _check, lib

_I, _P, _S = C.c_int, C.c_void_p, C.c_size_t

F32, I32 = 0, 1  # sample types (DWT_HIP_LIFT_F32, _I32)
CDF97, CDF53, INTERP53, CDF53_INT, CDF97_INT, HAAR, HAAR_INT, D4 = range(8)  # built-in schemes (DWT_HIP_LIFT_*)
BUILTIN_IDS = {"CDF97": CDF97, "CDF53": CDF53, "INTERP53": INTERP53, "CDF53_INT": CDF53_INT, "CDF97_INT": CDF97_INT, "HAAR": HAAR,
               "HAAR_INT": HAAR_INT, "D4": D4}
STEPS, FUSED = 0, 1  # routes (DWT_HIP_LIFT_STEPS, _FUSED)
MAX_STEPS, MAX_TERMS, MAX_OFFSET, FUSED_REACH, MAX_BATCH = 8, 4, 7, 8, 65535


class Term(C.Structure):
    _fields_ = [("coef", C.c_float), ("num", _I), ("off_a", _I), ("off_b", _I)]


class Step(C.Structure):
    _fields_ = [("parity", _I), ("n_terms", _I), ("sign", _I), ("add", _I), ("shift", _I), ("reserved", _I * 3), ("terms", Term * MAX_TERMS)]


class Scheme(C.Structure):
    """struct dwt_hip_lifting"""
    _fields_ = [("type", _I), ("n_steps", _I), ("inverse_cols_first", _I), ("reserved", _I), ("fwd_scale", C.c_float * 2),
                ("inv_scale", C.c_float * 2), ("steps", Step * MAX_STEPS)]

    def table(self):
        """the scheme as plain values, floats as their bits"""
        bits = lambda v: C.c_uint32.from_buffer_copy(C.c_float(v)).value
        return (self.type, self.inverse_cols_first, tuple(bits(v) for v in self.fwd_scale), tuple(bits(v) for v in self.inv_scale),
                tuple((st.parity, st.sign, st.add, st.shift, tuple((bits(t.coef), t.num, t.off_a, t.off_b) for t in st.terms[:max(st.n_terms, 0)]))
                      for st in self.steps[:max(self.n_steps, 0)]))


assert C.sizeof(Scheme) == 800

lib.dwt_hip_lifting_check.argtypes = [C.POINTER(Scheme), C.POINTER(_I)]
lib.dwt_hip_lifting_builtin.argtypes = [_I, C.POINTER(Scheme)]
lib.dwt_hip_lifting2d_batch.argtypes = [C.POINTER(Scheme), _I, _P, _P, _S, _I, _I, _I, _I, _I, C.POINTER(_I)]
lib.dwt_hip_lifting_route.argtypes = [C.POINTER(Scheme)]
lib.dwt_hip_lifting1d_batch.argtypes = [C.POINTER(Scheme), _I, _P, _P, _S, _I, _I, _I, C.POINTER(_I)]
lib.dwt_hip_lifting1d_route.argtypes = [C.POINTER(Scheme), _I]
lib.dwt_hip_lifting_norms.argtypes = [C.POINTER(Scheme), _I, C.POINTER(C.c_double), C.POINTER(C.c_double)]
lib.dwt_hip_lifting_quant_steps.argtypes = [C.POINTER(Scheme), _I, C.c_float, C.POINTER(C.c_float)]
for _n in ("dwt_hip_lifting_check", "dwt_hip_lifting_builtin", "dwt_hip_lifting2d_batch", "dwt_hip_lifting_route", "dwt_hip_lifting1d_batch",
           "dwt_hip_lifting1d_route", "dwt_hip_lifting_norms", "dwt_hip_lifting_quant_steps"):
    getattr(lib, _n).restype = _I
MAX_LINE_FUSED, QUANT_MAX_LEVELS = 8192, 16  # the longest line of the one-launch route; DWT_HIP_QUANT_MAX_LEVELS


def step(parity, terms, sign=1, add=0, shift=0):
    """one lifting step: terms [(coefficient, off_a, off_b)], the coefficient a float (float schemes) or an int (int schemes,
    with sign, add, shift: x += sign * ((sum + add) >> shift))"""
    return (parity, list(terms), sign, add, shift)


def scheme(sample_type, steps, fwd_scale=(1.0, 1.0), inv_scale=(1.0, 1.0), inverse_cols_first=None):
    """a Scheme from steps made by step().  inverse_cols_first: None stands for 1 with int samples and 0 with float ones.
    Nothing is checked here: check() or the transform does that."""
    s = Scheme()
    s.type, s.n_steps = sample_type, len(steps)
    s.inverse_cols_first = int(sample_type == I32) if inverse_cols_first is None else int(inverse_cols_first)
    s.fwd_scale[:] = [float(v) for v in fwd_scale]
    s.inv_scale[:] = [float(v) for v in inv_scale]
    for st, (parity, terms, sign, add, shift) in zip(s.steps, steps[:MAX_STEPS]):
        st.parity, st.n_terms, st.sign, st.add, st.shift = parity, len(terms), sign, add, shift
        for t, (c, off_a, off_b) in zip(st.terms, terms[:MAX_TERMS]):
            if sample_type == I32:
                t.num = int(c)
            else:
                t.coef = float(c)
            t.off_a, t.off_b = off_a, off_b
    return s


def builtin(name):
    """dwt_hip_lifting_builtin: the scheme of "CDF97", "CDF53", "INTERP53", "CDF53_INT", "CDF97_INT", "HAAR", "HAAR_INT", "D4"
    (or of its id)"""
    s = Scheme()
    _check(lib.dwt_hip_lifting_builtin(BUILTIN_IDS.get(name, name) if isinstance(name, str) else name, C.byref(s)), "dwt_hip_lifting_builtin")
    return s


def check(s):
    """dwt_hip_lifting_check -> the scheme's reach; DwtError with the reason for a malformed scheme"""
    reach = _I(0)
    _check(lib.dwt_hip_lifting_check(C.byref(s), C.byref(reach)), "dwt_hip_lifting_check")
    return reach.value


def lifting2d_batch(s, inverse, src, dst, batch_stride, batch, stride_x, stride_y, size_x, size_y, j=-1):
    """dwt_hip_lifting2d_batch -> the level count the call used (dwt_hip_band_levels(size_x, size_y, j))"""
    jj = _I(j)
    _check(lib.dwt_hip_lifting2d_batch(C.byref(s), int(bool(inverse)), _addr(src), _addr(dst), batch_stride, batch, stride_x, stride_y,
                                       size_x, size_y, C.byref(jj)), "dwt_hip_lifting2d_batch")
    return jj.value


def route(s):
    """dwt_hip_lifting_route: FUSED or STEPS for a call with this scheme under the current options"""
    r = lib.dwt_hip_lifting_route(C.byref(s))
    if r < 0:
        raise DwtError("dwt_hip_lifting_route: " + lib.dwt_hip_last_error().decode(errors="replace"))
    return r


def lifting1d_batch(s, inverse, src, dst, line_stride, elem_stride, n_lines, size, j=-1):
    """dwt_hip_lifting1d_batch: n_lines lines of `size` samples -> the 1-D Mallat layout of transform1d_batch.
    Returns the level count: the one the forward call used; the inverse only reads j and returns it as given."""
    jj = _I(j)
    _check(lib.dwt_hip_lifting1d_batch(C.byref(s), int(bool(inverse)), _addr(src), _addr(dst), line_stride, elem_stride, n_lines, size,
                                       C.byref(jj)), "dwt_hip_lifting1d_batch")
    return jj.value


def route1d(s, size):
    """dwt_hip_lifting1d_route: FUSED where lines of `size` samples run every level in one launch under the current options,
    STEPS where not"""
    r = lib.dwt_hip_lifting1d_route(C.byref(s), size)
    if r < 0:
        raise DwtError("dwt_hip_lifting1d_route: " + lib.dwt_hip_last_error().decode(errors="replace"))
    return r


def norms(s, levels):
    """dwt_hip_lifting_norms -> (norm_l, norm_h): two lists of `levels` floats, the L2 norms of the float scheme's synthesis
    functions of levels 1 .. levels (host arithmetic)"""
    nl, nh = (C.c_double * max(levels, 1))(), (C.c_double * max(levels, 1))()
    _check(lib.dwt_hip_lifting_norms(C.byref(s), levels, nl, nh), "dwt_hip_lifting_norms")
    return list(nl[:max(levels, 0)]), list(nh[:max(levels, 0)])


def quant_steps(s, levels, base_step):
    """dwt_hip_lifting_quant_steps -> the 3*levels + 1 steps of a float scheme as a ctypes float array, in the layout of
    quant.quant_steps: what quantize_batch takes for planes made with this scheme"""
    steps = (C.c_float * (3 * max(levels, 0) + 1))()
    _check(lib.dwt_hip_lifting_quant_steps(C.byref(s), levels, base_step, steps), "dwt_hip_lifting_quant_steps")
    return steps
