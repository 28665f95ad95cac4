"""libdwt_amd -- Python mirror of libdwt's 2-D DWT entry points over the MI355X backend.

The product is the C-ABI shared library ``libdwt_amd/libdwt_hip.so`` (C host code +
hand-written gfx950 HIP kernels; headers in ``include/``).  This module is only a
ctypes binding with the reference's function names and argument order
(``src/libdwt.h:562-573`` etc.), so tests read like programs written against libdwt:

    import libdwt_amd as dwt
    dwt.dwt_util_init()
    j = dwt.dwt_cdf97_2f_s(img, stride_x, 4, w, h, w, h, -1, 0, 0)   # returns levels done
    dwt.dwt_cdf97_2i_s(img, stride_x, 4, w, h, w, h, j, 0, 0)

``img`` may be a numpy array (host memory: staged through HBM), a torch tensor
(host or device), or a raw address (``int``) -- e.g. from ``dwt_hip_malloc``.

There is no CPU fallback anywhere: if the library is missing, importing this module
raises; if no gfx950 device is usable, every transform raises ``DwtError``.

When PyTorch is used in the same process (device tensors, streams, HIP graphs), import
``torch`` BEFORE this module: the library then binds to the HIP runtime torch ships
instead of loading a second one, and tensors' ``data_ptr()`` are valid for it.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DWT_HIP_LIB") or os.path.join(_HERE, "libdwt_hip.so")  # (DWT_HIP_LIB: another build of the library, for A/B scripts)

CDF97_S, CDF53_I, CDF53_S, CDF97_D, CDF53_D, CDF97_I = 0, 1, 2, 3, 4, 5
INTERP53_S = 6  # interpolating 5/3 float: the CDF 5/3 predict step alone (DWT_HIP_INTERP53_S)
CDF53_I16 = 8  # reversible int16 CDF 5/3 in JPEG 2000 order, 2-byte elements (DWT_HIP_CDF53_I16)
CDF97_H = 9  # float CDF 9/7 on IEEE binary16 storage, 2-byte elements (DWT_HIP_CDF97_H)


class DwtError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C libdwt_amd/csrc` (hipcc, gfx950). libdwt_amd has no CPU fallback."
    )

_cdll = C.CDLL(LIB_PATH)

# ---- the scratch contract: fill and poison mode (include/libdwt_hip.h) ---------------------------------
# Entries that are NEVER preceded by a fill while poison_workspace is on.  A deny list, not an allow list: an entry added
# later and forgotten here is poisoned like every transform, and fails loudly if it keeps state in scratch.
NEVER_PREFILLED = frozenset((
    "dwt_hip_fill_workspace",  # the fill itself
    # lifecycle, device, stream and workspace setters, options
    "dwt_hip_init", "dwt_hip_finish", "dwt_hip_sync", "dwt_hip_set_device", "dwt_hip_get_device", "dwt_hip_device_count",
    "dwt_hip_device_name", "dwt_hip_set_stream", "dwt_hip_set_workspace", "dwt_hip_set_option", "dwt_hip_get_option",
    "dwt_util_init", "dwt_util_finish", "dwt_util_set_accel", "dwt_util_get_accel",
    # allocation and copies
    "dwt_hip_malloc", "dwt_hip_free", "dwt_hip_malloc_host", "dwt_hip_free_host", "dwt_hip_alloc_batch", "dwt_hip_alloc_volumes",
    "dwt_hip_grant_access", "dwt_hip_memcpy_h2d", "dwt_hip_memcpy_d2h",
    # the bank objects
    "dwt_hip_timefreq_bank_create", "dwt_hip_timefreq_bank_from_kernels", "dwt_hip_timefreq_bank_free", "dwt_hip_timefreq_bank_bins",
    "dwt_hip_timefreq_bank_taps", "dwt_hip_timefreq_bank_query",
    # queries of a previous call or of a pointer: a fill in front of them would change the answer or is pointless
    "dwt_hip_last_error", "dwt_hip_is_device_pointer", "dwt_hip_rows_warnings", "dwt_hip_features_raw_sums", "dwt_hip_placement_report",
    "dwt_hip_alloc_batch_note", "dwt_hip_alloc_batch_report", "dwt_hip_prof_enable", "dwt_hip_prof_read", "dwt_hip_prof_read_levels",
    # host arithmetic on a lifting scheme, and the route query: no device work, no scratch
    "dwt_hip_lifting_norms", "dwt_hip_lifting_quant_steps", "dwt_hip_lifting1d_route",
))
_poison = None  # the word, or None: off


class _Prefilled:
    """A library function behind a fill of the calling thread's scratch.  Attributes (argtypes, restype) are the function's."""

    def __init__(self, fn):
        object.__setattr__(self, "_fn", fn)

    def __call__(self, *args):
        if _poison is not None and _cdll.dwt_hip_fill_workspace(_poison):
            raise DwtError("dwt_hip_fill_workspace: " + _cdll.dwt_hip_last_error().decode(errors="replace"))
        return self._fn(*args)

    def __getattr__(self, name):
        return getattr(self._fn, name)

    def __setattr__(self, name, value):
        setattr(self._fn, name, value)


class _Lib:
    """A thin proxy over the CDLL: the same function objects, or -- while poison_workspace is on -- every function that is
    not in NEVER_PREFILLED behind a fill.  It sees only the calls made from Python, that is top-level calls: a fill inside
    the library would destroy the scratch of an entry that calls another entry (the picture entries, the 3-D host entries)."""

    def __getattr__(self, name):
        fn = getattr(_cdll, name)
        if _poison is None or name in NEVER_PREFILLED or name.startswith("_"):
            return fn
        return _Prefilled(fn)

    def __setattr__(self, name, value):
        setattr(_cdll, name, value)


lib = _Lib()

_I, _P, _S = C.c_int, C.c_void_p, C.c_size_t
_FWD = [_P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _I]
_INV = [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I]
_FWD2 = [_P, _P] + _FWD[1:]
_INV2 = [_P, _P] + _INV[1:]

# libdwt entry points (void functions: they log + abort() on failure, like the
# reference).  The Python wrappers below go through dwt_hip_transform2d instead so
# that a failure surfaces as an exception rather than killing the interpreter.
for _n, _sig in (("dwt_cdf97_2f_s", _FWD), ("dwt_cdf97_2i_s", _INV), ("dwt_cdf97_2f_s2", _FWD2),
                 ("dwt_cdf97_2i_s2", _INV2), ("dwt_cdf53_2f_i", _FWD), ("dwt_cdf53_2i_i", _INV),
                 ("dwt_cdf53_2f_s", _FWD), ("dwt_cdf53_2i_s", _INV), ("dwt_cdf97_2f_d", _FWD), ("dwt_cdf97_2i_d", _INV),
                 ("dwt_cdf53_2f_d", _FWD), ("dwt_cdf53_2i_d", _INV), ("dwt_cdf97_2f_i", _FWD), ("dwt_cdf97_2i_i", _INV),
                 ("dwt_interp53_2f_s", _FWD), ("dwt_interp53_2i_s", _INV), ("dwt_cdf53_2f_i16", _FWD), ("dwt_cdf53_2i_i16", _INV),
                 ("dwt_cdf97_2f_h", _FWD), ("dwt_cdf97_2i_h", _INV)):
    getattr(lib, _n).argtypes = _sig
    getattr(lib, _n).restype = None

lib.dwt_hip_init.restype = _I
lib.dwt_hip_device_count.restype = _I
lib.dwt_hip_set_device.argtypes = [_I]
lib.dwt_hip_set_device.restype = _I
lib.dwt_hip_get_device.restype = _I
lib.dwt_hip_device_name.restype = C.c_char_p
lib.dwt_hip_last_error.restype = C.c_char_p
lib.dwt_hip_set_stream.argtypes = [_P]
lib.dwt_hip_set_workspace.argtypes = [_P, C.c_size_t, _P, C.c_size_t]
lib.dwt_hip_set_workspace.restype = _I
lib.dwt_hip_fill_workspace.argtypes = [C.c_uint]
lib.dwt_hip_fill_workspace.restype = _I
lib.dwt_hip_transform2d_batch_sharded.argtypes = [_I, _I, _P, _P, C.c_size_t, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), _I]
lib.dwt_hip_transform2d_batch_sharded.restype = _I
_PP = C.POINTER(_P)
lib.dwt_hip_transform2d_batch_multi.argtypes = [_I, _I, _PP, _PP, C.POINTER(_I), C.POINTER(_I), _I, C.c_size_t, _I, _I, _I, C.POINTER(_I)]
lib.dwt_hip_transform2d_batch_multi.restype = _I
lib.dwt_hip_tune_batch_multi.argtypes = [_I, _I, _PP, _PP, C.POINTER(_I), C.POINTER(_I), _I, C.c_size_t, _I, _I, _I, _I]
lib.dwt_hip_tune_batch_multi.restype = _I
lib.dwt_hip_shard_bounds.argtypes = [_I, _I, _I, C.POINTER(_I), C.POINTER(_I)]
lib.dwt_hip_shard_bounds.restype = None
lib.dwt_hip_tune.argtypes = [_I, _I, _P, _P, C.c_size_t, _I, _I, _I, _I, _I]
lib.dwt_hip_tune.restype = _I
lib.dwt_hip_grant_access.argtypes = [_P, C.POINTER(_I), _I]
lib.dwt_hip_grant_access.restype = _I
lib.dwt_hip_alloc_batch_note.restype = C.c_char_p
lib.dwt_hip_alloc_batch.argtypes = [_I, _I, _I, _I, _I, C.POINTER(_P), C.POINTER(_P)]
lib.dwt_hip_alloc_batch.restype = _I
lib.dwt_hip_placement_report.argtypes = [C.POINTER(C.c_double), _I]
lib.dwt_hip_placement_report.restype = _I
lib.dwt_hip_alloc_volumes.argtypes = [_I, _I, _I, _I, C.POINTER(_P), C.POINTER(_P)]
lib.dwt_hip_alloc_volumes.restype = _I
lib.dwt_hip_alloc_batch_report.argtypes = [C.POINTER(_I)] * 5 + [C.POINTER(C.c_double)] * 2
lib.dwt_hip_set_option.argtypes = [C.c_char_p, _I]
lib.dwt_hip_set_option.restype = _I
lib.dwt_hip_get_option.argtypes = [C.c_char_p]
lib.dwt_hip_get_option.restype = _I
lib.dwt_hip_transform2d.argtypes = [_I, _I, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _I]
lib.dwt_hip_transform2d.restype = _I
lib.dwt_hip_transform2d_batch.argtypes = [_I, _I, _P, _P, _S, _I, _I, _I, _I, C.POINTER(_I)]
lib.dwt_hip_transform1d.argtypes = [_I, _I, _P, _P, _I, _I, _I, C.POINTER(_I), _I]
lib.dwt_hip_transform1d.restype = _I
lib.dwt_hip_transform1d_batch.argtypes = [_I, _I, _P, _P, _S, _I, _I, _I, _I, C.POINTER(_I), _I]
lib.dwt_hip_transform1d_batch.restype = _I
lib.dwt_hip_transform2d_batch.restype = _I
lib.dwt_hip_transform2d_interleaved.argtypes = [_I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I]
lib.dwt_hip_transform2d_interleaved.restype = _I
lib.dwt_hip_transform3d.argtypes = [_I, _P, _S, _S, _I, _I, _I, _I]
lib.dwt_hip_transform3d.restype = _I
lib.dwt_hip_transform3d_op.argtypes = [_P, _P, _S, _S, _I, _I, _I, _I]
lib.dwt_hip_transform3d_op.restype = _I
lib.dwt_hip_volume_fwd_op.argtypes = [_P, _S, _S, _P, _S, _S, _I, _I, _I, _I]
lib.dwt_hip_volume_fwd_op.restype = _I
lib.dwt_hip_volume_ip.argtypes = [_I, _P, _S, _S, _I, _I, _I]
lib.dwt_hip_volume_ip.restype = _I
lib.dwt_hip_malloc.argtypes = [_S]
lib.dwt_hip_malloc.restype = _P
lib.dwt_hip_free.argtypes = [_P]
lib.dwt_hip_memcpy_h2d.argtypes = [_P, _P, _S]
lib.dwt_hip_memcpy_h2d.restype = _I
lib.dwt_hip_memcpy_d2h.argtypes = [_P, _P, _S]
lib.dwt_hip_memcpy_d2h.restype = _I
lib.dwt_hip_is_device_pointer.argtypes = [_P]
lib.dwt_hip_is_device_pointer.restype = _I
lib.dwt_hip_prof_enable.argtypes = [_I]
lib.dwt_hip_prof_read.argtypes = [C.POINTER(C.c_double), C.POINTER(_I)]
lib.dwt_hip_prof_read.restype = _I
lib.dwt_hip_prof_read_levels.argtypes = [C.POINTER(C.c_double), C.POINTER(_I), _I]
lib.dwt_hip_prof_read_levels.restype = _I
lib.dwt_util_get_opt_stride.argtypes = [_I]
lib.dwt_util_get_opt_stride.restype = _I
lib.dwt_util_get_stride.argtypes = [_I, _I]
lib.dwt_util_get_stride.restype = _I
lib.dwt_util_set_accel.argtypes = [_I]
lib.dwt_util_get_accel.restype = _I
for _n in ("dwt_util_test_image_fill_s", "dwt_util_test_image_fill_i"):
    getattr(lib, _n).argtypes = [_P, _I, _I, _I, _I, _I]
    getattr(lib, _n).restype = None
for _n in ("dwt_util_compare_s", "dwt_util_compare_i"):
    getattr(lib, _n).argtypes = [_P, _P, _I, _I, _I, _I]
    getattr(lib, _n).restype = _I
for _n in ("dwt_util_conv_show_s", "dwt_util_conv_show_i", "dwt_util_copy_s", "dwt_util_copy_i"):
    getattr(lib, _n).argtypes = [_P, _P, _I, _I, _I, _I]
    getattr(lib, _n).restype = None
lib.dwt_util_save_to_pgm_s.argtypes = [C.c_char_p, C.c_float, _P, _I, _I, _I, _I]
lib.dwt_util_save_to_pgm_s.restype = _I
lib.dwt_util_save_to_pgm_i.argtypes = [C.c_char_p, _I, _P, _I, _I, _I, _I]
lib.dwt_util_save_to_pgm_i.restype = _I
lib.dwt_util_version.restype = C.c_char_p


def _addr(obj):
    """Address of a numpy array / torch tensor / ctypes buffer / int."""
    if obj is None:
        raise DwtError("null image")
    if isinstance(obj, int):
        return obj
    if hasattr(obj, "data_ptr"):  # torch tensor (host or device)
        return obj.data_ptr()
    if hasattr(obj, "ctypes"):  # numpy
        return obj.ctypes.data
    return C.cast(obj, C.c_void_p).value


def last_error():
    return lib.dwt_hip_last_error().decode(errors="replace")


def _check(rc, what):
    if rc:
        raise DwtError(f"{what}: {last_error()}")


# ---- lifecycle -----------------------------------------------------------------------
def dwt_util_init():
    _check(lib.dwt_hip_init(), "dwt_util_init")


def dwt_util_finish():
    lib.dwt_hip_finish()


def dwt_util_set_accel(accel_type):
    lib.dwt_util_set_accel(accel_type)


def dwt_util_get_accel():
    return lib.dwt_util_get_accel()


def device_count():
    return lib.dwt_hip_device_count()


def set_device(device):
    """Bind the calling thread's context to `device` (one host thread per GPU drives several GPUs)."""
    _check(lib.dwt_hip_set_device(int(device)), "dwt_hip_set_device")


def get_device():
    return lib.dwt_hip_get_device()


def device_name():
    return lib.dwt_hip_device_name().decode()


def set_stream(stream_handle):
    """Run subsequent transforms on this hipStream_t (int handle; 0 = default)."""
    lib.dwt_hip_set_stream(stream_handle)


def use_torch_stream():
    import torch

    lib.dwt_hip_set_stream(torch.cuda.current_stream().cuda_stream)


def sync():
    lib.dwt_hip_sync()


def fill_workspace(word):
    """dwt_hip_fill_workspace: `word` into every 32-bit word of every scratch buffer of this thread's context (a
    caller-owned workspace included), on the context's stream, without a synchronise.  No result depends on it."""
    _check(lib.dwt_hip_fill_workspace(int(word) & 0xFFFFFFFF), "dwt_hip_fill_workspace")


def poison_workspace(word):
    """The poison mode of the tests: while `word` is not None, every call made through `lib` -- except the entries of
    NEVER_PREFILLED -- is preceded by fill_workspace(word) on the calling thread.  None turns it off.  Returns the
    previous setting."""
    global _poison
    before, _poison = _poison, (None if word is None else int(word) & 0xFFFFFFFF)
    return before


def set_option(name, value):
    _check(lib.dwt_hip_set_option(name.encode(), int(value)), "dwt_hip_set_option")


def get_option(name):
    return lib.dwt_hip_get_option(name.encode())


# ---- the reference's 2-D entry points --------------------------------------------------
def _fwd(wavelet, src, dst, stride_x, stride_y, sox, soy, six, siy, j_max, decompose_one, zero_padding, who):
    j = _I(j_max)
    rc = lib.dwt_hip_transform2d(wavelet, 0, _addr(src), _addr(dst), stride_x, stride_y, sox, soy, six, siy,
                                 C.byref(j), decompose_one, zero_padding)
    _check(rc, who)
    return j.value


def _inv(wavelet, src, dst, stride_x, stride_y, sox, soy, six, siy, j_max, decompose_one, zero_padding, who):
    j = _I(j_max)
    rc = lib.dwt_hip_transform2d(wavelet, 1, _addr(src), _addr(dst), stride_x, stride_y, sox, soy, six, siy,
                                 C.byref(j), decompose_one, zero_padding)
    _check(rc, who)


def dwt_cdf97_2f_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:12776.  Returns the level count the C function stores in *j_max_ptr."""
    return _fwd(CDF97_S, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_cdf97_2f_s")


def dwt_cdf97_2i_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:17040"""
    _inv(CDF97_S, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_cdf97_2i_s")


def dwt_cdf97_2f_s2(src, dst, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                    j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:12619"""
    return _fwd(CDF97_S, src, dst, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_cdf97_2f_s2")


def dwt_cdf97_2i_s2(src, dst, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                    j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:17985"""
    _inv(CDF97_S, src, dst, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_cdf97_2i_s2")


def dwt_cdf53_2f_i(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:16304"""
    return _fwd(CDF53_I, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_cdf53_2f_i")


def dwt_cdf53_2i_i(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:18142"""
    _inv(CDF53_I, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_cdf53_2i_i")


def dwt_cdf53_2f_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:16470"""
    return _fwd(CDF53_S, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_cdf53_2f_s")


def dwt_cdf53_2i_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:18296"""
    _inv(CDF53_S, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_cdf53_2i_s")


def dwt_cdf97_2f_d(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:12451 (double precision; stride_y = 8)"""
    return _fwd(CDF97_D, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_cdf97_2f_d")


def dwt_cdf97_2i_d(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:16884"""
    _inv(CDF97_D, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_cdf97_2i_d")


def dwt_cdf53_2f_d(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:12535"""
    return _fwd(CDF53_D, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_cdf53_2f_d")


def dwt_cdf53_2i_d(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:16962"""
    _inv(CDF53_D, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_cdf53_2i_d")


def dwt_cdf97_2f_i(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:16387 (fixed-point int32 CDF 9/7)"""
    return _fwd(CDF97_I, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_cdf97_2f_i")


def dwt_cdf97_2i_i(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:18219"""
    _inv(CDF97_I, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_cdf97_2i_i")


def dwt_interp53_2f_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                      j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:16801 (interpolating 5/3: CDF 5/3 without the update step)"""
    return _fwd(INTERP53_S, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_interp53_2f_s")


def dwt_interp53_2i_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                      j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:18457"""
    _inv(INTERP53_S, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_interp53_2i_s")


def dwt_cdf53_2f_i16(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                     j_max=-1, decompose_one=0, zero_padding=0):
    """Reversible int16 CDF 5/3 in JPEG 2000 order (columns before rows; int16 samples, stride_y >= 2).  An extension: the
    reference has the transform as a core only (examples/cores/cores.c)."""
    return _fwd(CDF53_I16, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_cdf53_2f_i16")


def dwt_cdf53_2i_i16(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                     j_max=-1, decompose_one=0, zero_padding=0):
    """The inverse of dwt_cdf53_2f_i16: rows before columns; restores every int16 image bit for bit."""
    _inv(CDF53_I16, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_cdf53_2i_i16")


def dwt_cdf97_2f_h(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """Float CDF 9/7 on IEEE binary16 storage (float16 samples, stride_y >= 2): every level is one level of dwt_cdf97_2f_s
    in binary32, rounded to binary16 once.  No overflow protection: max|x| * 2^levels must stay below 65504."""
    return _fwd(CDF97_H, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                j_max, decompose_one, zero_padding, "dwt_cdf97_2f_h")


def dwt_cdf97_2i_h(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                   j_max=-1, decompose_one=0, zero_padding=0):
    """The inverse of dwt_cdf97_2f_h, level by level: one level of dwt_cdf97_2i_s in binary32, rounded to binary16 once.
    Not exact: a 5-level round trip of 8-bit data returns within one grey level (0.625 measured on 8192 x 8192)."""
    _inv(CDF97_H, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
         j_max, decompose_one, zero_padding, "dwt_cdf97_2i_h")


FORWARD = {"cdf97_s": dwt_cdf97_2f_s, "cdf53_i": dwt_cdf53_2f_i, "cdf53_s": dwt_cdf53_2f_s,
           "cdf97_d": dwt_cdf97_2f_d, "cdf53_d": dwt_cdf53_2f_d, "cdf97_i": dwt_cdf97_2f_i,
           "interp53_s": dwt_interp53_2f_s, "cdf53_i16": dwt_cdf53_2f_i16, "cdf97_h": dwt_cdf97_2f_h}
INVERSE = {"cdf97_s": dwt_cdf97_2i_s, "cdf53_i": dwt_cdf53_2i_i, "cdf53_s": dwt_cdf53_2i_s,
           "cdf97_d": dwt_cdf97_2i_d, "cdf53_d": dwt_cdf53_2i_d, "cdf97_i": dwt_cdf97_2i_i,
           "interp53_s": dwt_interp53_2i_s, "cdf53_i16": dwt_cdf53_2i_i16, "cdf97_h": dwt_cdf97_2i_h}
WAVELET_ID = {"cdf97_s": CDF97_S, "cdf53_i": CDF53_I, "cdf53_s": CDF53_S, "cdf97_d": CDF97_D, "cdf53_d": CDF53_D,
              "cdf97_i": CDF97_I, "interp53_s": INTERP53_S, "cdf53_i16": CDF53_I16,
              "cdf97_h": CDF97_H}


# ---- interleaved (in-place lifting) layout ------------------------------------------------
def transform2d_interleaved(wavelet, inverse, flavour, src, dst, stride_x, stride_y, size_o_big_x, size_o_big_y,
                            size_i_big_x=None, size_i_big_y=None, j_max=-1, decompose_one=0):
    """dwt_hip_transform2d_interleaved: host or device pointers, in place (src is dst) or out of place.
    flavour 0 = libdwt.h *_inplace_s entries, 1 = dwt-simple.h fdwt2_* (forward only).  Returns j."""
    j = _I(j_max)
    six = size_o_big_x if size_i_big_x is None else size_i_big_x
    siy = size_o_big_y if size_i_big_y is None else size_i_big_y
    rc = lib.dwt_hip_transform2d_interleaved(WAVELET_ID.get(wavelet, wavelet), int(inverse), flavour, _addr(src), _addr(dst),
                                             stride_x, stride_y, size_o_big_x, size_o_big_y, six, siy, C.byref(j), decompose_one)
    _check(rc, "dwt_hip_transform2d_interleaved")
    return j.value


def dwt_cdf97_2f_inplace_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                           j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:12926.  Returns the level count."""
    return transform2d_interleaved(CDF97_S, 0, 0, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y,
                                   size_i_big_x, size_i_big_y, j_max, decompose_one)


def dwt_cdf97_2i_inplace_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                           j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:17474"""
    transform2d_interleaved(CDF97_S, 1, 0, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y,
                            size_i_big_x, size_i_big_y, j_max, decompose_one)


def dwt_cdf53_2f_inplace_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                           j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:16553.  Returns the level count."""
    return transform2d_interleaved(CDF53_S, 0, 0, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y,
                                   size_i_big_x, size_i_big_y, j_max, decompose_one)


def dwt_cdf53_2i_inplace_s(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                           j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:17886"""
    transform2d_interleaved(CDF53_S, 1, 0, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y,
                            size_i_big_x, size_i_big_y, j_max, decompose_one)


def dwt_cdf97_2f_inplace_i(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                           j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:17424 (fixed-point int 9/7, interleaved).  Returns the level count."""
    return transform2d_interleaved(CDF97_I, 0, 0, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y,
                                   size_i_big_x, size_i_big_y, j_max, decompose_one)


def dwt_cdf97_2i_inplace_i(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y,
                           j_max=-1, decompose_one=0, zero_padding=0):
    """src/libdwt.c:17308"""
    transform2d_interleaved(CDF97_I, 1, 0, ptr, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y,
                            size_i_big_x, size_i_big_y, j_max, decompose_one)


def _newapi(wavelet):
    def f(ptr, size_x, size_y, stride_x, stride_y, j_max=-1, decompose_one=0):
        return transform2d_interleaved(wavelet, 0, 1, ptr, ptr, stride_x, stride_y, size_x, size_y, size_x, size_y,
                                       j_max, decompose_one)
    return f


# src/dwt-simple.c:2224 / :1615 / :3034 and :2356 / :1927 / :3166 (argument order of dwt-simple.h)
fdwt2_cdf97_horizontal_s = fdwt2_cdf97_vertical_s = fdwt2_cdf97_diagonal_s = _newapi(CDF97_S)
fdwt2_cdf53_horizontal_s = fdwt2_cdf53_vertical_s = fdwt2_cdf53_diagonal_s = _newapi(CDF53_S)


# ---- the reference's 1-D entry points (float, Mallat layout) ---------------------------
def _line(wavelet, inverse, ptr, stride, size_o, size_i, j_max, zero_padding, who):
    j = _I(j_max)
    p = _addr(ptr)
    _check(lib.dwt_hip_transform1d(wavelet, int(inverse), p, p, stride, size_o, size_i, C.byref(j), zero_padding), who)
    return j.value


def dwt_cdf97_1f_s(ptr, stride, size_o, size_i, j_max=-1, zero_padding=0):
    """src/libdwt.c:16025.  Returns the level count the C function stores in *j_max_ptr."""
    return _line(CDF97_S, 0, ptr, stride, size_o, size_i, j_max, zero_padding, "dwt_cdf97_1f_s")


def dwt_cdf53_1f_s(ptr, stride, size_o, size_i, j_max=-1, zero_padding=0):
    """src/libdwt.c:16097"""
    return _line(CDF53_S, 0, ptr, stride, size_o, size_i, j_max, zero_padding, "dwt_cdf53_1f_s")


def dwt_cdf97_1i_s(ptr, stride, size_o, size_i, j_max=-1, zero_padding=0):
    """src/libdwt.c:15766.  Returns j_max as passed (the C function takes it by value)."""
    return _line(CDF97_S, 1, ptr, stride, size_o, size_i, j_max, zero_padding, "dwt_cdf97_1i_s")


def dwt_cdf53_1i_s(ptr, stride, size_o, size_i, j_max=-1, zero_padding=0):
    """src/libdwt.c:15835"""
    return _line(CDF53_S, 1, ptr, stride, size_o, size_i, j_max, zero_padding, "dwt_cdf53_1i_s")


def dwt_interp53_1f_s(ptr, stride, size_o, size_i, j_max=-1, zero_padding=0):
    """src/libdwt.c:16166"""
    return _line(INTERP53_S, 0, ptr, stride, size_o, size_i, j_max, zero_padding, "dwt_interp53_1f_s")


def dwt_interp53_1i_s(ptr, stride, size_o, size_i, j_max=-1, zero_padding=0):
    """src/libdwt.c:15900"""
    return _line(INTERP53_S, 1, ptr, stride, size_o, size_i, j_max, zero_padding, "dwt_interp53_1i_s")


def _series(wavelet, who):
    def f(ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max=-1, zero_padding=0):
        """The forward 1-D transform of rows 0 .. size_i_big_y-1 (size_o_big_y unused), as one batch.  Returns
        *j_max_ptr as the C function leaves it (unchanged when there are no rows)."""
        if size_i_big_y <= 0:
            return j_max
        j = _I(j_max)
        p = _addr(ptr)
        _check(lib.dwt_hip_transform1d_batch(wavelet, 0, p, p, stride_x, stride_y, size_i_big_y, size_o_big_x,
                                             size_i_big_x, C.byref(j), zero_padding), who)
        return j.value
    f.__name__ = who
    return f


dwt_cdf97_2f1_s = _series(CDF97_S, "dwt_cdf97_2f1_s")  # src/libdwt.c:15965
dwt_cdf53_2f1_s = _series(CDF53_S, "dwt_cdf53_2f1_s")  # src/libdwt.c:15995


def transform1d_batch(wavelet, inverse, src, dst, line_stride, n_lines, size, j_max=-1, elem_stride=4):
    """Dense-frame 1-D transform of `n_lines` lines of `size` float samples (`line_stride` / `elem_stride` in bytes);
    numpy arrays, torch tensors (host or device) or raw pointers.  Returns the level count (forward: clamped)."""
    j = _I(j_max)
    _check(lib.dwt_hip_transform1d_batch(WAVELET_ID.get(wavelet, wavelet), int(inverse), _addr(src), _addr(dst),
                                         line_stride, elem_stride, n_lines, size, size, C.byref(j), 0),
           "dwt_hip_transform1d_batch")
    return j.value


# ---- edge-avoiding 5/3 and 9/7 (EAW) entry points -------------------------------------
EAW_MALLAT, EAW_INTERLEAVED = 0, 1
EAW53, EAW97 = "eaw53", "eaw97"  # the wavelet argument of _eaw_call / _eaw_forward / _eaw_inverse
lib.dwt_hip_eaw97_2d.argtypes = [_I, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _I, _P, C.c_float]
lib.dwt_hip_eaw97_2d.restype = _I
lib.dwt_hip_eaw97_2d_batch.argtypes = [_I, _P, _S, _I, _I, _I, _I, C.POINTER(_I), _I, _P, _S, C.c_float]
lib.dwt_hip_eaw97_2d_batch.restype = _I
lib.dwt_hip_eaw53_2d.argtypes = [_I, _I, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _I, _P, C.c_float]
lib.dwt_hip_eaw53_2d.restype = _I
lib.dwt_hip_eaw53_2d_batch.argtypes = [_I, _P, _S, _I, _I, _I, _I, C.POINTER(_I), _I, _P, _S, C.c_float]
lib.dwt_hip_eaw53_2d_batch.restype = _I
lib.dwt_hip_eaw53_weights_layout.argtypes = [_I, _I, _I, _I, _I, _I, C.POINTER(C.c_long), C.POINTER(C.c_long)]
lib.dwt_hip_eaw53_weights_layout.restype = C.c_long
lib.dwt_eaw53_2f_dummy_s.argtypes = [_P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I]
lib.dwt_eaw53_2f_dummy_s.restype = None


def eaw53_weights_layout(layout, size_o_x, size_o_y, size_i_x, size_i_y, j):
    """dwt_hip_eaw53_weights_layout: (floats of the weight buffer, [(offset, shape) of wH[k]], [(offset, shape) of
    wV[k]]).  wV[k] has shape (columns, samples per column): the C array is column-major."""
    oh, ov = (C.c_long * 33)(), (C.c_long * 33)()
    total = lib.dwt_hip_eaw53_weights_layout(layout, size_o_x, size_o_y, size_i_x, size_i_y, j, oh, ov)
    if total < 0:
        raise DwtError("dwt_hip_eaw53_weights_layout: bad arguments")

    def cd(a, k):
        return (a + (1 << k) - 1) >> k
    hs, vs = [], []
    for k in range(j):
        if layout == EAW_MALLAT:
            hs.append((oh[k], (cd(size_o_y, k), cd(size_i_x, k))))
            vs.append((ov[k], (cd(size_o_x, k), cd(size_i_y, k))))
        else:
            hs.append((oh[k], (cd(size_i_y, k), cd(size_i_x, k))))
            vs.append((ov[k], (cd(size_i_x, k), cd(size_i_y, k))))
    return total, hs, vs


def dwt_eaw53_2f_dummy_s(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max=-1, decompose_one=0):
    """src/libdwt.c:16759: the level count the forward would take."""
    j = _I(j_max)
    lib.dwt_eaw53_2f_dummy_s(None, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, C.byref(j), decompose_one)
    return j.value


def _eaw_levels(inverse, size_o_x, size_o_y, j_max, decompose_one):
    n = max(size_o_x, size_o_y) if decompose_one else min(size_o_x, size_o_y)
    lim = 0 if n else 32  # src/inline.h:443: 32 for an empty frame
    while lim < 31 and (1 << lim) < n:
        lim += 1
    if not inverse:
        return lim if (j_max < 0 or j_max > lim) else j_max
    return j_max if 0 <= j_max < lim else lim


def _eaw_call(inverse, layout, ptr, stride_x, stride_y, sox, soy, six, siy, j_max, decompose_one, zero_padding, wbuf, alpha, who,
              wavelet=EAW53):
    j = _I(j_max)
    if wavelet == EAW97:  # Mallat only
        _check(lib.dwt_hip_eaw97_2d(int(inverse), _addr(ptr), stride_x, stride_y, sox, soy, six, siy, C.byref(j),
                                    decompose_one, zero_padding, wbuf, float(alpha)), who)
    else:
        _check(lib.dwt_hip_eaw53_2d(int(inverse), layout, _addr(ptr), stride_x, stride_y, sox, soy, six, siy, C.byref(j),
                                    decompose_one, zero_padding, wbuf, float(alpha)), who)
    return j.value


def _eaw_forward(layout, ptr, stride_x, stride_y, sox, soy, six, siy, j_max, decompose_one, zero_padding, alpha, who,
                 wavelet=EAW53):
    import numpy as np

    J = _eaw_levels(False, sox, soy, j_max, decompose_one)
    total, hs, vs = eaw53_weights_layout(layout, sox, soy, six, siy, J)
    w = np.zeros(max(total, 1), dtype=np.float32)
    p = _addr(ptr)
    if lib.dwt_hip_is_device_pointer(p):
        d = lib.dwt_hip_malloc(w.nbytes)
        if not d:
            raise DwtError("dwt_hip_malloc: " + last_error())
        try:
            _check(lib.dwt_hip_memcpy_h2d(d, w.ctypes.data, w.nbytes), who)
            j = _eaw_call(0, layout, p, stride_x, stride_y, sox, soy, six, siy, j_max, decompose_one, zero_padding, d, alpha, who,
                          wavelet)
            _check(lib.dwt_hip_memcpy_d2h(w.ctypes.data, d, w.nbytes), who)
        finally:
            lib.dwt_hip_free(d)
    else:
        j = _eaw_call(0, layout, p, stride_x, stride_y, sox, soy, six, siy, j_max, decompose_one, zero_padding, w.ctypes.data,
                      alpha, who, wavelet)
    wH = [w[o:o + a * b].reshape(a, b).copy() for o, (a, b) in hs]
    wV = [w[o:o + a * b].reshape(a, b).copy() for o, (a, b) in vs]
    return j, wH, wV


def _eaw_inverse(layout, ptr, stride_x, stride_y, sox, soy, six, siy, j_max, decompose_one, zero_padding, wH, wV, who,
                 wavelet=EAW53):
    import numpy as np

    J = _eaw_levels(True, sox, soy, j_max, decompose_one)
    total, hs, vs = eaw53_weights_layout(layout, sox, soy, six, siy, J)
    w = np.zeros(max(total, 1), dtype=np.float32)
    for k in range(J):
        for (o, (a, b)), arr in ((hs[k], wH[k]), (vs[k], wV[k])):
            w[o:o + a * b] = np.asarray(arr, dtype=np.float32).reshape(-1)[:a * b]
    p = _addr(ptr)
    if lib.dwt_hip_is_device_pointer(p):
        d = lib.dwt_hip_malloc(w.nbytes)
        if not d:
            raise DwtError("dwt_hip_malloc: " + last_error())
        try:
            _check(lib.dwt_hip_memcpy_h2d(d, w.ctypes.data, w.nbytes), who)
            _eaw_call(1, layout, p, stride_x, stride_y, sox, soy, six, siy, j_max, decompose_one, zero_padding, d, 1.0, who, wavelet)
        finally:
            lib.dwt_hip_free(d)
    else:
        _eaw_call(1, layout, p, stride_x, stride_y, sox, soy, six, siy, j_max, decompose_one, zero_padding, w.ctypes.data, 1.0, who,
                  wavelet)
    return j_max


def dwt_eaw53_2f_s(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max=-1, decompose_one=0,
                   zero_padding=0, alpha=1.0):
    """src/libdwt.c:16663.  Returns (levels done, wH, wV): wH[k] a (size_o_src_y, size_i_src_x) array, wV[k] a
    (size_o_src_x, size_i_src_y) array (wV[k][x, y], the C array's column-major order)."""
    return _eaw_forward(EAW_MALLAT, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, decompose_one,
                        zero_padding, alpha, "dwt_eaw53_2f_s")


def dwt_eaw53_2i_s(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, decompose_one, zero_padding, wH, wV):
    """src/libdwt.c:18373, with the forward's weight arrays."""
    return _eaw_inverse(EAW_MALLAT, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, decompose_one,
                        zero_padding, wH, wV, "dwt_eaw53_2i_s")


def dwt_eaw53_2f_inplace_s(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max=-1, decompose_one=0,
                           zero_padding=0, alpha=1.0):
    """src/libdwt.c:16602 (interleaved layout).  wH[k], wV[k] as for dwt_eaw53_2f_s over the inner frame."""
    return _eaw_forward(EAW_INTERLEAVED, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max,
                        decompose_one, zero_padding, alpha, "dwt_eaw53_2f_inplace_s")


def dwt_eaw53_2i_inplace_s(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, decompose_one, zero_padding,
                           wH, wV):
    """src/libdwt.c:17932"""
    return _eaw_inverse(EAW_INTERLEAVED, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, decompose_one,
                        zero_padding, wH, wV, "dwt_eaw53_2i_inplace_s")


def dwt_eaw97_2f_s(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max=-1, decompose_one=0,
                   zero_padding=0, alpha=1.0):
    """src/eaw-experimental.c:300 (edge-avoiding CDF 9/7, Mallat layout).  Returns (levels done, wH, wV), shaped as
    dwt_eaw53_2f_s's."""
    return _eaw_forward(EAW_MALLAT, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, decompose_one,
                        zero_padding, alpha, "dwt_eaw97_2f_s", EAW97)


def dwt_eaw97_2i_s(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, decompose_one, zero_padding, wH, wV):
    """src/eaw-experimental.c:398, with the forward's weight arrays."""
    return _eaw_inverse(EAW_MALLAT, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, decompose_one,
                        zero_padding, wH, wV, "dwt_eaw97_2i_s", EAW97)


def eaw53_2d_batch(inverse, ptr, batch_stride, batch, stride_x, size_x, size_y, weights, weights_stride, j_max=-1,
                   decompose_one=0, alpha=1.0):
    """EAW 5/3 of `batch` dense float images (Mallat layout, in place) `batch_stride` bytes apart, image b's weights
    (one buffer laid out as eaw53_weights_layout says) at `weights` + b * weights_stride floats.  numpy arrays, torch
    tensors or raw pointers: device memory runs one launch per level for the whole batch, host memory image by image.
    Returns the level count (forward: clamped)."""
    return _eaw_batch(EAW53, inverse, ptr, batch_stride, batch, stride_x, size_x, size_y, weights, weights_stride, j_max,
                      decompose_one, alpha)


def eaw97_2d_batch(inverse, ptr, batch_stride, batch, stride_x, size_x, size_y, weights, weights_stride, j_max=-1,
                   decompose_one=0, alpha=1.0):
    """EAW 9/7 of a batch: eaw53_2d_batch's arguments, layout (eaw53_weights_layout(EAW_MALLAT, ...)) and return."""
    return _eaw_batch(EAW97, inverse, ptr, batch_stride, batch, stride_x, size_x, size_y, weights, weights_stride, j_max,
                      decompose_one, alpha)


def _eaw_batch(wavelet, inverse, ptr, batch_stride, batch, stride_x, size_x, size_y, weights, weights_stride, j_max, decompose_one,
               alpha):
    p, w = _addr(ptr), _addr(weights)
    j = _I(j_max)
    if lib.dwt_hip_is_device_pointer(p):
        fn = lib.dwt_hip_eaw97_2d_batch if wavelet == EAW97 else lib.dwt_hip_eaw53_2d_batch
        _check(fn(int(inverse), p, batch_stride, batch, stride_x, size_x, size_y, C.byref(j), decompose_one, w, weights_stride,
                  float(alpha)), "dwt_hip_%s_2d_batch" % wavelet)
        return j.value
    for b in range(batch):
        j = _I(j_max)
        j.value = _eaw_call(inverse, EAW_MALLAT, p + b * batch_stride, stride_x, 4, size_x, size_y, size_x, size_y, j_max,
                            decompose_one, 0, w + 4 * b * weights_stride, alpha, "dwt_hip_%s_2d" % wavelet, wavelet)
    return _eaw_levels(bool(inverse), size_x, size_y, j_max, decompose_one) if batch == 0 else j.value


# ---- per-subband feature statistics (include/libdwt_hip.h) ---------------------------------------------
FEATURE_NAMES = ("wps", "maxidx", "mean", "med", "var", "stdev", "skew", "kurt", "maxnorm", "lpnorm", "norm")
FEATURE = {name: 1 << i for i, name in enumerate(FEATURE_NAMES)}  # name -> bit of a feature mask (enum dwt_hip_feature)
_F = C.c_float
lib.dwt_hip_count_subbands.argtypes = [_I] * 5
lib.dwt_hip_count_subbands.restype = _I
lib.dwt_hip_features2d.argtypes = [C.c_uint, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P]
lib.dwt_hip_features2d.restype = _I
lib.dwt_hip_features2d_hostfv.argtypes = [C.c_uint, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P]
lib.dwt_hip_features2d_hostfv.restype = _I
lib.dwt_hip_features_raw_sums.argtypes = [_I, _P, C.c_long]
lib.dwt_hip_features_raw_sums.restype = C.c_long
lib.dwt_hip_features2d_batch.argtypes = [C.c_uint, _P, _S, _I, _I, _I, _I, _I, _F, _P, _S]
lib.dwt_hip_features2d_batch.restype = _I
lib.dwt_hip_features1d_batch.argtypes = [C.c_uint, _P, _S, _S, _I, _I, _I, _F, _P, _S]
lib.dwt_hip_features1d_batch.restype = _I
lib.dwt_hip_band_feature.argtypes = [_I, _P, _I, _I, _I, _I, _I, _F, C.POINTER(_F)]
lib.dwt_hip_band_feature.restype = _I
lib.dwt_hip_band_moment.argtypes = [_P, _I, _I, _I, _I, _I, _I, _F, C.POINTER(_F)]
lib.dwt_hip_band_moment.restype = _I
lib.dwt_hip_abs.argtypes = [_P, _I, _I, _I, _I]
lib.dwt_hip_abs.restype = _I


def feature_mask(features):
    """A feature mask from a mask, a name or an iterable of names of FEATURE."""
    if isinstance(features, int):
        return features
    if isinstance(features, str):
        features = (features,)
    return sum({FEATURE[f] for f in features})


def count_subbands(size_o_x, size_o_y, size_i_x, size_i_y, j_max):
    """dwt_util_count_subbands_s: the non-empty detail bands of levels 1 .. j_max-1."""
    n = lib.dwt_hip_count_subbands(size_o_x, size_o_y, size_i_x, size_i_y, j_max)
    if n < 0:
        raise DwtError("dwt_hip_count_subbands: bad sizes")
    return n


def features2d(features, ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, fv, p=2.0):
    """dwt_hip_features2d: `fv` (in the memory space of `ptr`) receives one block of count_subbands floats per
    feature of the mask, in FEATURE_NAMES order."""
    _check(lib.dwt_hip_features2d(feature_mask(features), _addr(ptr), stride_x, stride_y, size_o_x, size_o_y, size_i_x,
                                  size_i_y, j_max, float(p), _addr(fv)), "dwt_hip_features2d")


def features_raw_sums(plane, n):
    """dwt_hip_features_raw_sums: the raw double sums (plane 0 .. 5) behind this thread's last feature call."""
    import numpy as np

    out = np.zeros(n, dtype=np.float64)
    m = lib.dwt_hip_features_raw_sums(plane, out.ctypes.data, n)
    if m < 0:
        raise DwtError("dwt_hip_features_raw_sums: plane %d was not part of the last call" % plane)
    return out[:m]


def features2d_batch(features, ptr, batch_stride, batch, stride_x, size_x, size_y, j_max, fv, fv_stride, p=2.0):
    """dwt_hip_features2d_batch: image b's vector at fv + b * fv_stride floats."""
    _check(lib.dwt_hip_features2d_batch(feature_mask(features), _addr(ptr), batch_stride, batch, stride_x, size_x, size_y,
                                        j_max, float(p), _addr(fv), fv_stride), "dwt_hip_features2d_batch")


def features1d_batch(features, ptr, line_stride, elem_stride, n_lines, size, j_max, fv, fv_stride, p=2.0):
    """dwt_hip_features1d_batch: every row a frame with size_y = 1; rows of up to 8192 samples take one launch."""
    _check(lib.dwt_hip_features1d_batch(feature_mask(features), _addr(ptr), line_stride, elem_stride, n_lines, size,
                                        j_max, float(p), _addr(fv), fv_stride), "dwt_hip_features1d_batch")


def dwt_util_count_subbands_s(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max):
    return count_subbands(size_o_x, size_o_y, size_i_x, size_i_y, j_max)


def _vector_entry(name):
    fn = getattr(lib, "dwt_util_%s_s" % name)
    fn.argtypes = [_P, _I, _I, _I, _I, _I, _I, _I, _P] + ([_F] if name == "lpnorm" else [])
    fn.restype = None

    def entry(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, fv=None, *p):
        """libdwt's prototype; `fv` is a host float32 array (made and returned when None)."""
        import numpy as np

        if fv is None:
            fv = np.zeros(count_subbands(size_o_x, size_o_y, size_i_x, size_i_y, j_max), dtype=np.float32)
        if not lib.dwt_hip_is_device_pointer(_addr(ptr)) and lib.dwt_hip_init():
            raise DwtError(lib.dwt_hip_last_error().decode())  # (the C entry would abort)
        getattr(lib, "dwt_util_%s_s" % name)(_addr(ptr), stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, fv.ctypes.data,
                                             *[float(q) for q in p])
        return fv

    entry.__name__ = "dwt_util_%s_s" % name
    return entry


for _n in FEATURE_NAMES:
    globals()["dwt_util_%s_s" % _n] = _vector_entry(_n)


def _band_entry(name, extra):
    fn = getattr(lib, "dwt_util_band_%s_s" % name)
    fn.argtypes = [_P, _I, _I, _I, _I] + extra
    fn.restype = _F

    def entry(ptr, stride_x, stride_y, size_x, size_y, *more):
        if lib.dwt_hip_init():
            raise DwtError(lib.dwt_hip_last_error().decode())
        return getattr(lib, "dwt_util_band_%s_s" % name)(_addr(ptr), stride_x, stride_y, size_x, size_y, *more)

    entry.__name__ = "dwt_util_band_%s_s" % name
    return entry


for _n in FEATURE_NAMES + ("moment", "cmoment", "smoment"):
    globals()["dwt_util_band_%s_s" % _n] = _band_entry(
        _n, {"wps": [_I], "lpnorm": [_F], "moment": [_I, _F], "cmoment": [_I], "smoment": [_I]}.get(_n, []))

lib.dwt_util_abs_s.argtypes = [_P, _I, _I, _I, _I]
lib.dwt_util_abs_s.restype = None
lib.dwt_util_subband_const_s.argtypes = [_P, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_P), C.POINTER(_I), C.POINTER(_I)]
lib.dwt_util_subband_const_s.restype = None


def dwt_hip_abs(ptr, stride_x, stride_y, size_x, size_y):
    """|x| in place, host or device memory."""
    _check(lib.dwt_hip_abs(_addr(ptr), stride_x, stride_y, size_x, size_y), "dwt_hip_abs")


def dwt_util_abs_s(ptr, stride_x, stride_y, size_x, size_y):
    if lib.dwt_hip_init():
        raise DwtError(lib.dwt_hip_last_error().decode())
    lib.dwt_util_abs_s(_addr(ptr), stride_x, stride_y, size_x, size_y)


def dwt_util_subband_const_s(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, band):
    """(address, size_x, size_y) of a subband."""
    q, sx, sy = _P(), _I(), _I()
    lib.dwt_util_subband_const_s(_addr(ptr), stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, band,
                                 C.byref(q), C.byref(sx), C.byref(sy))
    return q.value, sx.value, sy.value


# ---- conditioning of row batches (include/libdwt_hip.h, include/libdwt.h) ------------------------------
ROWS_OP = {"med_shift": 1, "center": 2, "scale": 4}  # name -> bit of an operation mask (enum dwt_hip_rows_op)
lib.dwt_hip_rows_condition.argtypes = [C.c_uint, _P, _S, _S, _I, _I, _I, _F, _F, _P]
lib.dwt_hip_rows_condition.restype = _I
lib.dwt_hip_rows_center_index.argtypes = [_P, _S, _S, _I, _I, _P]
lib.dwt_hip_rows_center_index.restype = _I
lib.dwt_hip_rows_warnings.argtypes = [C.POINTER(_I), C.POINTER(_I)]
lib.dwt_hip_rows_warnings.restype = _I
lib.dwt_hip_rows_min_max.argtypes = [_P, _S, _S, _I, _I, _P, _P]
lib.dwt_hip_rows_min_max.restype = _I
lib.dwt_hip_rows_displace.argtypes = [_P, _S, _S, _I, _I, _P, _I, _I]
lib.dwt_hip_rows_displace.restype = _I
lib.dwt_hip_shift.argtypes = [_P, _I, _I, _I, _I, _F]
lib.dwt_hip_shift.restype = _I
lib.dwt_hip_scale.argtypes = [_P, _I, _I, _I, _I, _F]
lib.dwt_hip_scale.restype = _I
for _n in ("dwt_util_viewport", "dwt_util_crop21"):
    getattr(lib, _n).argtypes = [_P, _I, _I, _I, _I, _I] + ([_I] if _n == "dwt_util_viewport" else [])
    getattr(lib, _n).restype = _P


def rows_op_mask(ops):
    """An operation mask from a mask, a name or an iterable of names of ROWS_OP."""
    if isinstance(ops, int):
        return ops
    if isinstance(ops, str):
        ops = (ops,)
    return sum({ROWS_OP[o] for o in ops})


def rows_condition(ops, ptr, line_stride, elem_stride, n_lines, size, max_iters=20, lo=0.0, hi=1.0, info=None):
    """dwt_hip_rows_condition: median shift, centring and range scaling of n_lines rows in place, in this order; `info`
    (host or device, 4 int32 per row) receives net offset, moves made, last centre found, 1 if the scale skipped the row.
    Dense device rows of up to 8192 samples take one launch up to the batch size from which one kernel per operation is
    faster (option "cond_fused": 1 / 0 force either route, -1 the choice)."""
    _check(lib.dwt_hip_rows_condition(rows_op_mask(ops), _addr(ptr), line_stride, elem_stride, n_lines, size, max_iters, float(lo),
                                      float(hi), None if info is None else _addr(info)), "dwt_hip_rows_condition")


def rows_center_index(ptr, line_stride, elem_stride, n_lines, size, center=None):
    """dwt_hip_rows_center_index: dwt_util_get_center1_s of every row -> `center` (int32, host or device; a host array is
    made and returned when None)."""
    import numpy as np

    if center is None:
        center = np.zeros(n_lines, dtype=np.int32)
    _check(lib.dwt_hip_rows_center_index(_addr(ptr), line_stride, elem_stride, n_lines, size, _addr(center)), "dwt_hip_rows_center_index")
    return center


def rows_warnings():
    """dwt_hip_rows_warnings -> (zero norms, missing crossing indexes) among the centre evaluations of this thread's last
    rows_condition / rows_center_index call: what the reference would have warned about."""
    a, b = _I(), _I()
    _check(lib.dwt_hip_rows_warnings(C.byref(a), C.byref(b)), "dwt_hip_rows_warnings")
    return a.value, b.value


def rows_min_max(ptr, line_stride, elem_stride, n_lines, size, mn=None, mx=None):
    """dwt_hip_rows_min_max -> (min, max), float32 per row (host arrays are made when None)."""
    import numpy as np

    mn = np.zeros(n_lines, dtype=np.float32) if mn is None else mn
    mx = np.zeros(n_lines, dtype=np.float32) if mx is None else mx
    _check(lib.dwt_hip_rows_min_max(_addr(ptr), line_stride, elem_stride, n_lines, size, _addr(mn), _addr(mx)), "dwt_hip_rows_min_max")
    return mn, mx


def rows_displace(ptr, line_stride, elem_stride, n_lines, size, displ, zero_fill=True):
    """dwt_hip_rows_displace: row[x] = row[x + d] in place; `displ` is one int for every row or an int32 array (host or
    device) with one per row; zeros (zero_fill) or the border sample move in."""
    import numbers

    per_row = not isinstance(displ, numbers.Integral)  # (numpy integer scalars are Integral too)
    _check(lib.dwt_hip_rows_displace(_addr(ptr), line_stride, elem_stride, n_lines, size, _addr(displ) if per_row else None,
                                     0 if per_row else int(displ), 1 if zero_fill else 0), "dwt_hip_rows_displace")


def _row_stride(stride_x, size_y):
    return stride_x if size_y > 1 else 0


def dwt_util_shift21_med_s(ptr, size_x, size_y, stride_x, stride_y):
    """libdwt's prototype (sizes before strides, as every entry of this block); host or device memory."""
    rows_condition(1, ptr, _row_stride(stride_x, size_y), stride_y, size_y, size_x, 0)


def dwt_util_center21_s(ptr, size_x, size_y, stride_x, stride_y, max_iters):
    if max_iters > 0:
        rows_condition(2, ptr, _row_stride(stride_x, size_y), stride_y, size_y, size_x, max_iters)
    return 0


def dwt_util_center1_s(ptr, size_x, stride_y, max_iters):
    return dwt_util_center21_s(ptr, size_x, 1, 0, stride_y, max_iters)


def dwt_util_get_center1_s(ptr, size_x, stride_y):
    return int(rows_center_index(ptr, 0, stride_y, 1, size_x)[0])


def dwt_util_displace1_s(ptr, size_x, stride_y, displ_x):
    if displ_x:
        rows_displace(ptr, 0, stride_y, 1, size_x, int(displ_x), zero_fill=False)
    return 0


def dwt_util_displace1_zero_s(ptr, size_x, stride_y, displ_x):
    if displ_x:
        rows_displace(ptr, 0, stride_y, 1, size_x, int(displ_x), zero_fill=True)
    return 0


def dwt_util_scale21_s(ptr, size_x, size_y, stride_x, stride_y, lo, hi):
    rows_condition(4, ptr, _row_stride(stride_x, size_y), stride_y, size_y, size_x, 0, lo, hi)
    return 0


def dwt_util_shift_s(ptr, size_x, size_y, stride_x, stride_y, a):
    _check(lib.dwt_hip_shift(_addr(ptr), stride_x, stride_y, size_x, size_y, float(a)), "dwt_hip_shift")
    return 0


def dwt_util_scale_s(ptr, size_x, size_y, stride_x, stride_y, a):
    _check(lib.dwt_hip_scale(_addr(ptr), stride_x, stride_y, size_x, size_y, float(a)), "dwt_hip_scale")
    return 0


def dwt_util_find_min_max_s(ptr, size_x, size_y, stride_x, stride_y):
    """-> (min, max) over the size_x x size_y elements"""
    mn, mx = rows_min_max(ptr, _row_stride(stride_x, size_y), stride_y, size_y, size_x)
    return float(mn.min()), float(mx.max())


def dwt_util_viewport(ptr, size_x, size_y, stride_x, stride_y, offset_x, offset_y):
    """the address of element (offset_y, offset_x): pointer arithmetic only"""
    return lib.dwt_util_viewport(_addr(ptr), size_x, size_y, stride_x, stride_y, offset_x, offset_y)


def dwt_util_crop21(ptr, size_x, size_y, stride_x, stride_y, len_x):
    """the address of the first of the len_x columns about column size_x / 2: pointer arithmetic only"""
    return lib.dwt_util_crop21(_addr(ptr), size_x, size_y, stride_x, stride_y, len_x)


# ---- per-band coefficient operators, log / exp maps, universal threshold (include/libdwt_hip.h) ----------
BAND_OP = {"keep": 0, "zero": 1, "scale": 2, "hard": 3, "soft": 4, "compress": 5}  # name -> enum dwt_hip_band_op
MAP_OP = {"log": 0, "exp": 1}  # name -> enum dwt_hip_map_op
lib.dwt_hip_band_slots.argtypes = [_I]
lib.dwt_hip_band_slots.restype = _I
lib.dwt_hip_band_levels.argtypes = [_I, _I, _I]
lib.dwt_hip_band_levels.restype = _I
lib.dwt_hip_band_geometry.argtypes = [_I, _I, _I, _I, _I, _P]
lib.dwt_hip_band_geometry.restype = _I
lib.dwt_hip_bands_apply.argtypes = [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P]
lib.dwt_hip_bands_apply.restype = _I
lib.dwt_hip_bands_apply_batch.argtypes = [_P, _S, _I, _I, _I, _I, _I, _P, _P, _S]
lib.dwt_hip_bands_apply_batch.restype = _I
lib.dwt_hip_map.argtypes = [_I, _P, _I, _I, _I, _I, _F]
lib.dwt_hip_map.restype = _I
lib.dwt_hip_map_batch.argtypes = [_I, _P, _S, _I, _I, _I, _I, _F]
lib.dwt_hip_map_batch.restype = _I
lib.dwt_hip_universal_threshold_batch.argtypes = [_P, _S, _I, _I, _I, _I, _P]
lib.dwt_hip_universal_threshold_batch.restype = _I


def band_slots(j_max):
    """dwt_hip_band_slots: 3 * j_max + 1, the entries of a table for j_max levels."""
    n = lib.dwt_hip_band_slots(j_max)
    if n < 0:
        raise DwtError("dwt_hip_band_slots: bad level count %d" % j_max)
    return n


def band_levels(size_o_x, size_o_y, j_max=-1):
    """dwt_hip_band_levels: the level count the band entries use for these sizes and this j_max."""
    n = lib.dwt_hip_band_levels(size_o_x, size_o_y, j_max)
    if n < 0:
        raise DwtError("dwt_hip_band_levels: bad sizes")
    return n


def band_geometry(size_o_x, size_o_y, size_i_x, size_i_y, j_max=-1):
    """dwt_hip_band_geometry -> int32 array (slots, 4) of x, y, size_x, size_y."""
    import numpy as np

    out = np.zeros((94, 4), dtype=np.int32)
    n = lib.dwt_hip_band_geometry(size_o_x, size_o_y, size_i_x, size_i_y, j_max, out.ctypes.data)
    if n < 0:
        raise DwtError("dwt_hip_band_geometry: bad sizes")
    return out[:n]


def _band_table(ops, params):
    """(int32 array, float32 array) of a table given as numbers or names of BAND_OP; the arrays are what the C entry reads"""
    import numpy as np

    if ops is None or params is None:
        return None, None
    if not isinstance(ops, np.ndarray):
        ops = [[BAND_OP[o] if isinstance(o, str) else int(o) for o in row] if isinstance(row, (list, tuple)) else
               (BAND_OP[row] if isinstance(row, str) else int(row)) for row in ops]
    return np.ascontiguousarray(ops, dtype=np.int32), np.ascontiguousarray(params, dtype=np.float32)


def bands_apply(ptr, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, ops, params):
    """dwt_hip_bands_apply: one operator and one parameter per slot of a Mallat frame (host or device), in place, in one
    launch.  `ops` holds numbers or names of BAND_OP, band_slots(band_levels(size_o_x, size_o_y, j_max)) of them."""
    o, p = _band_table(ops, params)
    _check(lib.dwt_hip_bands_apply(_addr(ptr), stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max,
                                   None if o is None else o.ctypes.data, None if p is None else p.ctypes.data), "dwt_hip_bands_apply")


def bands_apply_batch(ptr, batch_stride, batch, stride_x, size_x, size_y, j_max, ops, params, table_stride=0):
    """dwt_hip_bands_apply_batch: table_stride 0 -- one table for every frame; otherwise frame b's table at entry
    b * table_stride of `ops` / `params` (per-image thresholds), still one launch."""
    o, p = _band_table(ops, params)
    _check(lib.dwt_hip_bands_apply_batch(_addr(ptr), batch_stride, batch, stride_x, size_x, size_y, j_max,
                                         None if o is None else o.ctypes.data, None if p is None else p.ctypes.data, table_stride),
           "dwt_hip_bands_apply_batch")


def map_log(ptr, stride_x, stride_y, size_x, size_y, a):
    """dwt_hip_map(LOG): c = log(c + a) in place (the hdr flow's logf(*c + eps))."""
    _check(lib.dwt_hip_map(0, _addr(ptr), stride_x, stride_y, size_x, size_y, float(a)), "dwt_hip_map")


def map_exp(ptr, stride_x, stride_y, size_x, size_y, a):
    """dwt_hip_map(EXP): c = exp(c) - a in place."""
    _check(lib.dwt_hip_map(1, _addr(ptr), stride_x, stride_y, size_x, size_y, float(a)), "dwt_hip_map")


def map_log_batch(ptr, batch_stride, batch, stride_x, size_x, size_y, a):
    _check(lib.dwt_hip_map_batch(0, _addr(ptr), batch_stride, batch, stride_x, size_x, size_y, float(a)), "dwt_hip_map_batch")


def map_exp_batch(ptr, batch_stride, batch, stride_x, size_x, size_y, a):
    _check(lib.dwt_hip_map_batch(1, _addr(ptr), batch_stride, batch, stride_x, size_x, size_y, float(a)), "dwt_hip_map_batch")


def universal_threshold_batch(ptr, batch_stride, batch, stride_x, size_x, size_y, lam=None):
    """dwt_hip_universal_threshold_batch -> float32 host array, one threshold per frame, from the median magnitude of
    the Mallat HH(1) band; the frames are only read."""
    import numpy as np

    if lam is None:
        lam = np.zeros(batch, dtype=np.float32)
    _check(lib.dwt_hip_universal_threshold_batch(_addr(ptr), batch_stride, batch, stride_x, size_x, size_y, lam.ctypes.data),
           "dwt_hip_universal_threshold_batch")
    return lam


# ---- N-term approximation: keep the N largest magnitudes (include/libdwt_hip.h) -------------------------
NTERM_FRAME, NTERM_DETAILS = 0, 1  # enum dwt_hip_nterm_scope
lib.dwt_hip_keep_largest_batch.argtypes = [_P, _S, _I, _I, _S, _I, _I, _I, _I, _I, _P, _P, _P]
lib.dwt_hip_keep_largest_batch.restype = _I
lib.dwt_hip_keep_largest.argtypes = [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P]
lib.dwt_hip_keep_largest.restype = _I
lib.dwt_hip_magnitude_batch.argtypes = [_P, _S, _I, _I, _S, _I, _I, _I, _P, _S, _I]
lib.dwt_hip_magnitude_batch.restype = _I


def keep_largest_batch(ptr, batch_stride, batch, channels, channel_stride, stride_x, size_x, size_y, keep, j_max=-1,
                       scope=NTERM_FRAME):
    """dwt_hip_keep_largest_batch: in every group of `channels` frames (host or device) the positions of the keep[g]
    largest magnitudes stay, every other position in scope gets +0 in every channel.  `keep` is one number for every
    group or a sequence of `batch` numbers.  -> (thr, kept): float32 and int32 host arrays, one entry per group."""
    import numpy as np

    n = max(batch, 0)
    k = np.full(n, keep, dtype=np.int32) if np.isscalar(keep) else np.ascontiguousarray(keep, dtype=np.int32)
    if k.size < n:
        raise DwtError("dwt_hip_keep_largest_batch: %d keep counts for %d groups" % (k.size, batch))
    thr, kept = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
    _check(lib.dwt_hip_keep_largest_batch(_addr(ptr), batch_stride, batch, channels, channel_stride, stride_x, size_x, size_y,
                                          j_max, scope, k.ctypes.data, thr.ctypes.data, kept.ctypes.data),
           "dwt_hip_keep_largest_batch")
    return thr, kept


def keep_largest(ptr, stride_x, stride_y, size_x, size_y, keep, j_max=-1, scope=NTERM_FRAME):
    """dwt_hip_keep_largest: one frame of one channel with any element stride -> (thr, kept)."""
    thr, kept = C.c_float(0), C.c_int(0)
    _check(lib.dwt_hip_keep_largest(_addr(ptr), stride_x, stride_y, size_x, size_y, j_max, scope, keep, C.addressof(thr),
                                    C.addressof(kept)), "dwt_hip_keep_largest")
    return thr.value, kept.value


def magnitude_batch(ptr, batch_stride, batch, channels, channel_stride, stride_x, size_x, size_y, map_ptr, map_batch_stride,
                    map_stride_x):
    """dwt_hip_magnitude_batch: the magnitude map of every group -> map_ptr (where the frames lie: host or device), one
    launch; the frames are only read."""
    _check(lib.dwt_hip_magnitude_batch(_addr(ptr), batch_stride, batch, channels, channel_stride, stride_x, size_x, size_y,
                                       _addr(map_ptr), map_batch_stride, map_stride_x), "dwt_hip_magnitude_batch")


# ---- stationary wavelet transform of rows (include/libdwt_hip.h, include/swt.h) -------------------------
SWT_MAX_LEVELS = 24
lib.dwt_hip_swt1d_batch.argtypes = [_I, _P, _S, _S, _I, _I, _I, _P, _P, _I, _S, _S]
lib.dwt_hip_swt1d_batch.restype = _I
lib.dwt_hip_swt1d_level.argtypes = [_I, _P, _P, _P, _I, _I, _I]
lib.dwt_hip_swt1d_level.restype = _I
lib.dwt_hip_swt_features1d_batch.argtypes = [_I, C.c_uint, _P, _S, _S, _I, _I, _I, _I, _F, _P, _I]
lib.dwt_hip_swt_features1d_batch.restype = _I


def _swt_wavelet(wavelet):
    w = WAVELET_ID.get(wavelet, wavelet) if isinstance(wavelet, str) else wavelet
    if w not in (CDF97_S, CDF53_S):
        raise DwtError("the SWT takes cdf97_s or cdf53_s (got %r)" % (wavelet,))
    return w


def _swt_sizes(n_lines, size, levels, who):
    if n_lines < 0 or size < 0 or levels < 0 or levels > SWT_MAX_LEVELS:
        raise DwtError("%s: bad arguments (%d lines of %d samples, %d levels of at most %d)"
                       % (who, n_lines, size, levels, SWT_MAX_LEVELS))


def swt1d_batch(wavelet, src, line_stride, elem_stride, n_lines, size, levels, dst_h, dst_l=None, l_mode=0, plane_stride=0,
                dst_line_stride=0):
    """dwt_hip_swt1d_batch: every level of the stationary transform of n_lines rows.  H of level l of row y at
    dst_h + l*plane_stride + y*dst_line_stride bytes; l_mode 0: no L, 1: the last level's at dst_l, 2: every level's
    laid out like H.  Rows of up to 8192 dense samples take one launch."""
    w = _swt_wavelet(wavelet)
    _swt_sizes(n_lines, size, levels, "swt1d_batch")
    if l_mode not in (0, 1, 2):
        raise DwtError("swt1d_batch: l_mode %r" % (l_mode,))
    if l_mode and dst_l is None:
        raise DwtError("swt1d_batch: l_mode %d needs dst_l" % l_mode)
    _check(lib.dwt_hip_swt1d_batch(w, _addr(src), line_stride, elem_stride, n_lines, size, levels, _addr(dst_h),
                                   0 if dst_l is None else _addr(dst_l), l_mode, plane_stride, dst_line_stride),
           "dwt_hip_swt1d_batch")


def swt_features1d_batch(wavelet, features, src, line_stride, elem_stride, n_lines, size, levels, fv, fv_line_stride, band=0,
                         p=2.0):
    """dwt_hip_swt_features1d_batch: feature k of the mask of level l of row y at fv[y*fv_line_stride + k*levels + l];
    band 0: the H planes, 1: the L planes.  No coefficient is stored for rows of up to 8192 dense samples."""
    w = _swt_wavelet(wavelet)
    _swt_sizes(n_lines, size, levels, "swt_features1d_batch")
    if band not in (0, 1):
        raise DwtError("swt_features1d_batch: band %r" % (band,))
    _check(lib.dwt_hip_swt_features1d_batch(w, feature_mask(features), _addr(src), line_stride, elem_stride, n_lines, size,
                                            levels, band, float(p), _addr(fv), fv_line_stride),
           "dwt_hip_swt_features1d_batch")


def _swt_entry(name, wavelet):
    def entry(src, dst_l, dst_h, size, stride, level):
        """libdwt's prototype (include/swt.h, an inline wrapper over dwt_hip_swt1d_level as this is): one level at
        dilation 1 << level of one line, host or device memory."""
        if size < 0 or stride < 4 or level < 0 or level >= SWT_MAX_LEVELS:
            raise DwtError("%s: bad arguments (%d samples, stride %d, level %d)" % (name, size, stride, level))
        _check(lib.dwt_hip_swt1d_level(wavelet, _addr(src), _addr(dst_l), _addr(dst_h), size, stride, level), name)

    entry.__name__ = name
    return entry


swt_cdf97_f_ex_stride_s = _swt_entry("swt_cdf97_f_ex_stride_s", CDF97_S)
swt_cdf53_f_ex_stride_s = _swt_entry("swt_cdf53_f_ex_stride_s", CDF53_S)


# ---- stationary wavelet transform of image batches (include/libdwt_hip.h) ------------------------------
SWT2D_FUSED_LEVELS = 5  # DWT_HIP_SWT2D_FUSED_LEVELS: dense device images take one launch per level on levels 0 .. 4
SWT2D_TILE_W, SWT2D_TILE_H = 256, 32  # DWT_HIP_SWT2D_TILE_W / _H: the fused kernel's tile (columns, rows of the row lattice)
lib.dwt_hip_swt2d_batch.argtypes = [_I, _P, _S, _I, _I, _I, _I, _I, _I, _P, _P, _I, _S, _S, _I]
lib.dwt_hip_swt2d_batch.restype = _I
lib.dwt_hip_swt2d_level.argtypes = [_I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I]
lib.dwt_hip_swt2d_level.restype = _I


def swt2d_batch(wavelet, src, batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, dst_h, dst_l=None, l_mode=0,
                dst_batch_stride=0, plane_stride=0, dst_stride_x=0):
    """dwt_hip_swt2d_batch: every level of the stationary transform of a batch of images, rows then columns.  Detail band
    k (HL = 1, LH = 2, HH = 3) of level l of image b at dst_h + b*dst_batch_stride + (3*l + k-1)*plane_stride +
    y*dst_stride_x + 4*x bytes; l_mode 0: no LL, 1: the last level's at plane 0 of dst_l, 2: level l's at plane l.  Dense
    device images take one launch per level on levels 0 .. SWT2D_FUSED_LEVELS-1, two otherwise."""
    w = _swt_wavelet(wavelet)
    if batch < 1 or size_x < 1 or size_y < 1 or levels < 0 or levels > SWT_MAX_LEVELS:
        raise DwtError("swt2d_batch: bad arguments (%d images of %d x %d samples, %d levels of at most %d)"
                       % (batch, size_x, size_y, levels, SWT_MAX_LEVELS))
    if l_mode not in (0, 1, 2):
        raise DwtError("swt2d_batch: l_mode %r" % (l_mode,))
    if l_mode and dst_l is None:
        raise DwtError("swt2d_batch: l_mode %d needs dst_l" % l_mode)
    if min(batch_stride, stride_x, stride_y, dst_batch_stride, plane_stride, dst_stride_x) < 0:
        raise DwtError("swt2d_batch: negative stride")
    _check(lib.dwt_hip_swt2d_batch(w, _addr(src), batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, _addr(dst_h),
                                   0 if dst_l is None else _addr(dst_l), l_mode, dst_batch_stride, plane_stride, dst_stride_x),
           "dwt_hip_swt2d_batch")


def swt2d_level(wavelet, src, stride_x, stride_y, size_x, size_y, level, dst_ll, dst_hl, dst_lh, dst_hh, dst_stride_x,
                dst_stride_y=4):
    """dwt_hip_swt2d_level: one level at dilation 1 << level of one image into four planes whose rows are dst_stride_x and
    elements dst_stride_y bytes apart; host or device memory."""
    w = _swt_wavelet(wavelet)
    if size_x < 1 or size_y < 1 or level < 0 or level >= SWT_MAX_LEVELS:
        raise DwtError("swt2d_level: bad arguments (%d x %d samples, level %d)" % (size_x, size_y, level))
    _check(lib.dwt_hip_swt2d_level(w, _addr(src), stride_x, stride_y, size_x, size_y, level, _addr(dst_ll), _addr(dst_hl),
                                   _addr(dst_lh), _addr(dst_hh), dst_stride_x, dst_stride_y), "dwt_hip_swt2d_level")


# ---- time-frequency planes (include/libdwt_hip.h, include/gabor.h) -------------------------------------
TIMEFREQ_KINDS = {"ft": 0, "wt": 1, "st": 2}
TIMEFREQ_OUT = {"complex": 0, "abs": 1, "arg": 2}
lib.dwt_hip_timefreq_bank_create.argtypes = [_I, _I, _F, _F]
lib.dwt_hip_timefreq_bank_create.restype = _P
lib.dwt_hip_timefreq_bank_from_kernels.argtypes = [_I, _P, _P, _P]
lib.dwt_hip_timefreq_bank_from_kernels.restype = _P
lib.dwt_hip_timefreq_bank_free.argtypes = [_P]
lib.dwt_hip_timefreq_bank_free.restype = None
lib.dwt_hip_timefreq_bank_bins.argtypes = [_P]
lib.dwt_hip_timefreq_bank_bins.restype = _I
lib.dwt_hip_timefreq_bank_taps.argtypes = [_P]
lib.dwt_hip_timefreq_bank_taps.restype = C.c_long
lib.dwt_hip_timefreq_bank_query.argtypes = [_P, _P, _P, _P]
lib.dwt_hip_timefreq_bank_query.restype = _I
lib.dwt_hip_timefreq_batch.argtypes = [_P, _P, _S, _S, _I, _I, _I, _P, _S, _S]
lib.dwt_hip_timefreq_batch.restype = _I
lib.dwt_hip_timefreq_batch_strided.argtypes = [_P, _P, _S, _S, _I, _I, _I, _P, _S, _S, _S]
lib.dwt_hip_timefreq_batch_strided.restype = _I
lib.dwt_hip_gabor_transform.argtypes = [_I, _I, _P, _I, _I, _P, _I, _I, _I, _F, _F]
lib.dwt_hip_gabor_transform.restype = _I
lib.dwt_hip_timefreq_line.argtypes = [_I, _P, _I, _P, _I, _I, _P, _I, _I, _I]
lib.dwt_hip_timefreq_line.restype = _I
lib.dwt_hip_cdot1.argtypes = [_P, _I, _I, _I, _P, _I, _I, _I, _P]
lib.dwt_hip_cdot1.restype = _I
lib.dwt_hip_phase_derivative.argtypes = [_P, _P, _I, _I, _I, _I, _I, _S, _F]
lib.dwt_hip_phase_derivative.restype = _I
lib.dwt_hip_detect_ridges.argtypes = [_I, _P, _P, _I, _I, _I, _I, _I, _S, _F]
lib.dwt_hip_detect_ridges.restype = _I
lib.dwt_hip_gaussian_size.argtypes = [_F, _F]
lib.dwt_hip_gaussian_size.restype = _I


class TimefreqBank:
    """A bank of complex kernels (dwt_hip_timefreq_bank): `sizes`, `centers` and `taps` (one complex64 array per bin) read
    back from the library.  Freed by free() or with the object."""

    def __init__(self, handle):
        self.handle = handle
        if not handle:
            raise DwtError(lib.dwt_hip_last_error().decode())
        self.bins = lib.dwt_hip_timefreq_bank_bins(handle)

    def query(self):
        import numpy as np

        sizes, centers = np.zeros(self.bins, np.int32), np.zeros(self.bins, np.int32)
        taps = np.zeros(2 * lib.dwt_hip_timefreq_bank_taps(self.handle), np.float32)
        _check(lib.dwt_hip_timefreq_bank_query(self.handle, sizes.ctypes.data, centers.ctypes.data, taps.ctypes.data), "dwt_hip_timefreq_bank_query")
        return sizes, centers, np.split(taps.view(np.complex64), np.cumsum(sizes)[:-1])

    def free(self):
        if self.handle:
            lib.dwt_hip_timefreq_bank_free(self.handle)
            self.handle = None

    def __del__(self):
        self.free()


def timefreq_bank(kind=None, bins=0, sigma=0.0, freq=0.0, kernels=None, centers=None):
    """A bank of one transform -- kind "ft" (reads sigma), "wt" (sigma, freq) or "st" with `bins` bins, generated as the
    reference generates its kernels -- or of the caller's `kernels` (complex64 arrays) with their `centers`."""
    if kernels is not None:
        import numpy as np

        sizes = np.array([len(k) for k in kernels], np.int32)
        cs = np.array(centers, np.int32)
        if len(kernels) < 1 or len(cs) != len(kernels):
            raise DwtError("timefreq_bank: one centre per kernel, at least one kernel")
        taps = np.ascontiguousarray(np.concatenate([np.asarray(k, np.complex64) for k in kernels])).view(np.float32)
        return TimefreqBank(lib.dwt_hip_timefreq_bank_from_kernels(len(kernels), sizes.ctypes.data, cs.ctypes.data, taps.ctypes.data))
    k = TIMEFREQ_KINDS.get(kind, kind) if isinstance(kind, str) else kind
    if k not in (0, 1, 2):
        raise DwtError("timefreq_bank: kind %r (ft, wt or st)" % (kind,))
    return TimefreqBank(lib.dwt_hip_timefreq_bank_create(k, bins, float(sigma), float(freq)))


def timefreq_batch(bank, src, line_stride, elem_stride, n_lines, size, out_kind, dst, plane_stride, row_stride, dst_elem_stride=None):
    """dwt_hip_timefreq_batch: every line against every kernel of the bank; out_kind "complex", "abs" or "arg".  Output
    (line, row, t) at dst + line*plane_stride + row*row_stride + t*dst_elem_stride bytes (dense by default), bin y in
    row bins-1-y.  One launch for device memory."""
    o = TIMEFREQ_OUT.get(out_kind, out_kind) if isinstance(out_kind, str) else out_kind
    if o not in (0, 1, 2):
        raise DwtError("timefreq_batch: out_kind %r (complex, abs or arg)" % (out_kind,))
    if not isinstance(bank, TimefreqBank) or not bank.handle:
        raise DwtError("timefreq_batch: the bank is freed or no TimefreqBank")
    if dst_elem_stride is None:
        _check(lib.dwt_hip_timefreq_batch(bank.handle, _addr(src), line_stride, elem_stride, n_lines, size, o, _addr(dst), plane_stride,
                                          row_stride), "dwt_hip_timefreq_batch")
    else:
        _check(lib.dwt_hip_timefreq_batch_strided(bank.handle, _addr(src), line_stride, elem_stride, n_lines, size, o, _addr(dst),
                                                  plane_stride, row_stride, dst_elem_stride), "dwt_hip_timefreq_batch_strided")


def _gabor_entry(name, kind, arg):
    def entry(sig, sig_stride, sig_size, plane, stride_x, stride_y, bins, sigma=0.0, freq=0.0):
        """libdwt's prototype (include/gabor.h): one plane of one signal, host or device memory."""
        if min(sig_stride, stride_x, stride_y) < 0:
            raise DwtError("%s: negative stride" % name)
        _check(lib.dwt_hip_gabor_transform(kind, arg, _addr(sig), sig_stride, sig_size, _addr(plane), stride_x, stride_y, bins, float(sigma),
                                           float(freq)), name)

    entry.__name__ = name
    return entry


gabor_ft_s, gabor_ft_arg_s = _gabor_entry("gabor_ft_s", 0, 0), _gabor_entry("gabor_ft_arg_s", 0, 1)
gabor_wt_s, gabor_wt_arg_s = _gabor_entry("gabor_wt_s", 1, 0), _gabor_entry("gabor_wt_arg_s", 1, 1)
gabor_st_s, gabor_st_arg_s = _gabor_entry("gabor_st_s", 2, 0), _gabor_entry("gabor_st_arg_s", 2, 1)


def phase_derivative(angle, derivative, stride_x, stride_y, size_x, size_y, limit, n_planes=1, plane_stride=0):
    """dwt_hip_phase_derivative (phase_derivative_s over n_planes planes)."""
    _check(lib.dwt_hip_phase_derivative(_addr(angle), _addr(derivative), stride_x, stride_y, size_x, size_y, n_planes, plane_stride,
                                        float(limit)), "dwt_hip_phase_derivative")


def detect_ridges(kind, src, ridges, stride_x, stride_y, size_x, size_y, threshold, n_planes=1, plane_stride=0):
    """dwt_hip_detect_ridges (detect_ridges1_s / 2_s / 3_s by kind, over n_planes planes)."""
    _check(lib.dwt_hip_detect_ridges(kind, _addr(src), _addr(ridges), stride_x, stride_y, size_x, size_y, n_planes, plane_stride,
                                     float(threshold)), "dwt_hip_detect_ridges")


# ---- batches resident in HBM -----------------------------------------------------------
def transform2d_batch(wavelet, inverse, src, dst, batch_stride, batch, stride_x, size_x, size_y, j_max=-1):
    j = _I(j_max)
    rc = lib.dwt_hip_transform2d_batch(WAVELET_ID.get(wavelet, wavelet), int(inverse), _addr(src), _addr(dst),
                                       batch_stride, batch, stride_x, size_x, size_y, C.byref(j))
    _check(rc, "dwt_hip_transform2d_batch")
    return j.value


def transform2d_batch_sharded(wavelet, inverse, src, dst, batch_stride, batch, stride_x, size_x, size_y, j_max, devices):
    """dwt_hip_transform2d_batch_sharded: the batch split over `devices` (one process, one host thread per slot)."""
    j = _I(j_max)
    dv = (_I * len(devices))(*devices)
    rc = lib.dwt_hip_transform2d_batch_sharded(WAVELET_ID.get(wavelet, wavelet), int(inverse), _addr(src), _addr(dst),
                                               batch_stride, batch, stride_x, size_x, size_y, C.byref(j), dv, len(devices))
    _check(rc, "dwt_hip_transform2d_batch_sharded")
    return j.value


def shard_bounds(batch, n_slots, slot):
    """dwt_hip_shard_bounds: (first image, number of images) of `slot` when image b belongs to slot b*n_slots//batch."""
    a, n = _I(), _I()
    lib.dwt_hip_shard_bounds(batch, n_slots, slot, C.byref(a), C.byref(n))
    return a.value, n.value


def _multi_args(srcs, dsts, counts, devices):
    n = len(srcs)
    assert len(dsts) == n and len(counts) == n and len(devices) == n
    # (`None if p is None`: truth-testing a tensor or array with several elements raises, and a one-element zero
    # tensor must not turn into NULL)
    ptrs = lambda ps: (_P * n)(*[None if p is None else _addr(p) for p in ps])  # noqa: E731
    return ptrs(srcs), ptrs(dsts), (_I * n)(*counts), (_I * n)(*devices), n


def transform2d_batch_multi(wavelet, inverse, srcs, dsts, counts, devices, batch_stride, stride_x, size_x, size_y, j_max=-1):
    """dwt_hip_transform2d_batch_multi: shard k (counts[k] images at srcs[k] / dsts[k]) is RESIDENT on devices[k];
    all shards are transformed at once, nothing crosses xGMI."""
    j = _I(j_max)
    s_, d_, c_, v_, n = _multi_args(srcs, dsts, counts, devices)
    rc = lib.dwt_hip_transform2d_batch_multi(WAVELET_ID.get(wavelet, wavelet), int(inverse), s_, d_, c_, v_, n, batch_stride, stride_x,
                                             size_x, size_y, C.byref(j))
    _check(rc, "dwt_hip_transform2d_batch_multi")
    return j.value


def tune_batch_multi(wavelet, inverse, srcs, dsts, counts, devices, batch_stride, stride_x, size_x, size_y, levels=-1):
    """dwt_hip_tune_batch_multi: dwt_hip_tune in every slot of a resident sharded batch."""
    s_, d_, c_, v_, n = _multi_args(srcs, dsts, counts, devices)
    _check(lib.dwt_hip_tune_batch_multi(WAVELET_ID.get(wavelet, wavelet), int(inverse), s_, d_, c_, v_, n, batch_stride, stride_x,
                                        size_x, size_y, levels), "dwt_hip_tune_batch_multi")


def tune(wavelet, inverse, src, dst, batch_stride, batch, stride_x, size_x, size_y, levels=-1):
    """dwt_hip_tune: the explicit measurement (scratch placement, tile heights) on the caller's own device buffers;
    `dst` receives the transform of `src`.  The calling thread's context keeps the results."""
    _check(lib.dwt_hip_tune(WAVELET_ID.get(wavelet, wavelet), int(inverse), _addr(src), _addr(dst), batch_stride, batch, stride_x,
                            size_x, size_y, levels), "dwt_hip_tune")


def grant_access(ptr, devices):
    dv = (_I * len(devices))(*devices)
    _check(lib.dwt_hip_grant_access(_addr(ptr), dv, len(devices)), "dwt_hip_grant_access")


def alloc_batch_note():
    """'' when the last alloc_batch / alloc_volumes of this thread ran its search, else why it allocated plainly."""
    return lib.dwt_hip_alloc_batch_note().decode()


def transform3d(inverse, vol, stride_y, stride_z, size_x, size_y, size_z, levels=1):
    _check(lib.dwt_hip_transform3d(int(inverse), _addr(vol), stride_y, stride_z, size_x, size_y, size_z, levels),
           "dwt_hip_transform3d")


def transform3d_op(src, dst, stride_y, stride_z, size_x, size_y, size_z, levels=1):
    """Forward 3-D transform out of place (cdf97_3f_op_sep_horizontal_s, src/volume-dwt.c:727)."""
    _check(lib.dwt_hip_transform3d_op(_addr(src), _addr(dst), stride_y, stride_z, size_x, size_y, size_z, levels),
           "dwt_hip_transform3d_op")


# ---- struct volume_t (include/volume.h, include/volume-dwt.h) ---------------------------
class volume_t(C.Structure):
    """The reference's 3-D container (src/volume.h:14-24): sizes, byte strides, data pointer."""
    _fields_ = [("size_x", _I), ("size_y", _I), ("size_z", _I), ("stride_x", _S), ("stride_y", _S), ("stride_z", _S),
                ("data", _P)]


def volume_of(arr_or_ptr, shape_zyx=None, strides_zyx=None):
    """A volume_t over a (z, y, x) float32 numpy array / torch tensor, or over a raw pointer with
    explicit shape and byte strides.  The caller keeps the memory alive."""
    if shape_zyx is None:
        shape_zyx = tuple(arr_or_ptr.shape)
        if hasattr(arr_or_ptr, "data_ptr"):
            strides_zyx = tuple(s * arr_or_ptr.element_size() for s in arr_or_ptr.stride())
        else:
            strides_zyx = tuple(arr_or_ptr.strides)
    nz, ny, nx = shape_zyx
    sz, sy, sx = strides_zyx
    return volume_t(nx, ny, nz, sx, sy, sz, _addr(arr_or_ptr))


_VP = C.POINTER(volume_t)
for _n in ("volume_alloc_realiably", "volume_alloc_realiably_locked", "volume_alloc_device"):
    getattr(lib, _n).argtypes = [_S, _I, _I, _I, _I]
    getattr(lib, _n).restype = _VP
for _n in ("volume_free", "volume_fill_s", "volume_invalidate_cache", "cdf97_3f_ip_sep_horizontal_s", "cdf97_3i_ip_sep_horizontal_s"):
    getattr(lib, _n).argtypes = [_VP]
    getattr(lib, _n).restype = None
for _n in ("volume_copy_s", "volume_compare_s"):
    getattr(lib, _n).argtypes = [_VP, _VP]
    getattr(lib, _n).restype = _I
VOLUME_OP_SCHEDULES = ("sep_horizontal", "sep_vertical", "slices_vert4x4", "baseline_vert2x2x2", "HORIZ_vert2x2x2",
                       "cube_vert4x4x2", "HORIZ_vert4x4x2", "HORIZ_vert4x4x4", "baseline_diag2x2x2", "HORIZ_diag2x2x2")
for _n in VOLUME_OP_SCHEDULES:
    getattr(lib, "cdf97_3f_op_%s_s" % _n).argtypes = [_VP, _VP]
    getattr(lib, "cdf97_3f_op_%s_s" % _n).restype = None
lib.cdf97_3f_op_wrapper_s.argtypes = [_VP, _VP, _I]
lib.cdf97_3f_op_wrapper_s.restype = None
lib.volume_save_to_pgm_s.argtypes = [_VP, C.c_char_p]
lib.volume_save_to_pgm_s.restype = None
lib.volume_perftest_fwd97op_s.argtypes = [_I, _I, _I, _I, C.POINTER(C.c_double), C.POINTER(C.c_ulong)]
lib.volume_perftest_fwd97op_s.restype = _I
lib.volume_perftest_fwd97op_device_s.argtypes = [_I, _I, _I, _I, C.POINTER(C.c_double)]
lib.volume_perftest_fwd97op_device_s.restype = _I
lib.volume_measure_fwd97op_s.argtypes = [_I, _I, _I, _I, _I, _I]
lib.volume_measure_fwd97op_s.restype = _I


def cdf97_3f_ip_sep_horizontal_s(volume):
    """src/volume-dwt.c:677: forward, in place (a volume_t; host or device data)."""
    lib.cdf97_3f_ip_sep_horizontal_s(C.byref(volume))


def cdf97_3i_ip_sep_horizontal_s(volume):
    """src/volume-dwt.c:1115: inverse, in place."""
    lib.cdf97_3i_ip_sep_horizontal_s(C.byref(volume))


def cdf97_3f_op_sep_horizontal_s(volume_src, volume_dst):
    """src/volume-dwt.c:727: forward, out of place."""
    lib.cdf97_3f_op_sep_horizontal_s(C.byref(volume_src), C.byref(volume_dst))


def cdf97_3f_op_wrapper_s(volume_src, volume_dst, approach):
    """src/volume-dwt.c:2787: the schedule dispatcher (enum volume_approach 0..12)."""
    lib.cdf97_3f_op_wrapper_s(C.byref(volume_src), C.byref(volume_dst), int(approach))


def volume_perftest_fwd97op_s(size, opt_stride, approach, N, device=False):
    """src/volume-dwt.c:2810: (errors, seconds per voxel); device=True keeps both volumes in HBM."""
    secs = C.c_double()
    if device:
        err = lib.volume_perftest_fwd97op_device_s(size, opt_stride, int(approach), N, C.byref(secs))
    else:
        faults = C.c_ulong()
        err = lib.volume_perftest_fwd97op_s(size, opt_stride, int(approach), N, C.byref(secs), C.byref(faults))
    return err, secs.value


# ---- device memory without torch -------------------------------------------------------
class DeviceImage:
    """A dense device-resident image (hipMalloc) addressed like libdwt images."""

    def __init__(self, height, width, itemsize=4, pitch_bytes=None):
        self.h, self.w = height, width
        self.stride_x = pitch_bytes or width * itemsize
        self.stride_y = itemsize
        self.nbytes = self.stride_x * height
        self.ptr = lib.dwt_hip_malloc(max(self.nbytes, 16))
        if not self.ptr:
            raise DwtError("dwt_hip_malloc: " + last_error())

    def upload(self, arr):
        import numpy as np

        a = np.ascontiguousarray(arr)
        assert a.nbytes == self.nbytes, (a.nbytes, self.nbytes)
        _check(lib.dwt_hip_memcpy_h2d(self.ptr, a.ctypes.data, self.nbytes), "h2d")
        return self

    def download(self, dtype):
        import numpy as np

        out = np.empty((self.h, self.stride_x // np.dtype(dtype).itemsize), dtype=dtype)
        _check(lib.dwt_hip_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes), "d2h")
        return out

    def free(self):
        if self.ptr:
            lib.dwt_hip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- kernel timing ----------------------------------------------------------------------
def prof_enable(on=True):
    """True/1: time the level-0 kernel; 2: time every level's kernel."""
    lib.dwt_hip_prof_enable(int(on))


def prof_read_levels(n=8):
    ms = (C.c_double * n)()
    cnt = (_I * n)()
    _check(lib.dwt_hip_prof_read_levels(ms, cnt, n), "dwt_hip_prof_read_levels")
    return [(ms[i] / cnt[i] if cnt[i] else 0.0) for i in range(n)], list(cnt)


def prof_read():
    """(summed ms of the level-0 sweep kernel launches, number of launches) since last read."""
    ms, n = C.c_double(0), _I(0)
    _check(lib.dwt_hip_prof_read(C.byref(ms), C.byref(n)), "dwt_hip_prof_read")
    return ms.value, n.value


def placement_report():
    """Milliseconds the last placement search measured per candidate (empty: no search ran) and the index kept."""
    ms = (C.c_double * 8)()
    n = lib.dwt_hip_placement_report(ms, 8)
    return [round(ms[i], 4) for i in range(n)], lib.dwt_hip_get_option(b"place_last_best")


def alloc_batch_report():
    """What the last dwt_hip_alloc_batch of this thread measured (chunks == 0: plain allocations)."""
    v = [_I() for _ in range(5)]
    ms = (C.c_double * 5)()
    sec = C.c_double()
    lib.dwt_hip_alloc_batch_report(*[C.byref(x) for x in v], ms, C.byref(sec))
    return {"arena_GiB": v[0].value, "dst_positions_tried": v[1].value, "scratch_positions_tried": v[2].value,
            "dst_at_GiB": v[3].value, "scratch_at_GiB": v[4].value,
            "dst_one_level_ms_best_worst": [round(ms[0], 4), round(ms[1], 4)],
            "whole_call_ms_best_worst": [round(ms[2], 4), round(ms[3], 4)], "kept_arrangement_ms": round(ms[4], 4), "seconds": round(sec.value, 2)}


def alloc_batch(wavelet, n_images, size_x, size_y, levels=-1):
    """dwt_hip_alloc_batch: (src, dst) device pointers of a resident batch, placed; free with lib.dwt_hip_free."""
    s_, d_ = _P(), _P()
    _check(lib.dwt_hip_alloc_batch(WAVELET_ID.get(wavelet, wavelet), n_images, size_x, size_y, levels, C.byref(s_), C.byref(d_)), "dwt_hip_alloc_batch")
    return s_.value, d_.value


def alloc_volumes(size_x, size_y, size_z, levels):
    """dwt_hip_alloc_volumes: (src, dst) dense device volumes of an out-of-place 3-D call, placed; free with lib.dwt_hip_free."""
    s_, d_ = _P(), _P()
    _check(lib.dwt_hip_alloc_volumes(size_x, size_y, size_z, levels, C.byref(s_), C.byref(d_)), "dwt_hip_alloc_volumes")
    return s_.value, d_.value
