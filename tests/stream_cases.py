"""Every device entry on the caller's stream, on a BUSY stream (tests/test_hip_streams.py starts this module).

include/libdwt_hip.h promises that calls on device pointers are ordered on the stream given to dwt_hip_set_stream and
asynchronous, that every host thread has its own context, and that a change of stream is ordered behind what the context
queued on the old one.  On the default stream, with a synchronise between calls, a launch on the wrong stream, a host
value read back too early or scratch handed over too early are all invisible.  Here every entry runs on a non-blocking
stream that is busy: a bounded delay sits in front of the copy that brings the true input, so work that ran early or on
another stream reads a different image, and work that is not joined back to the stream is missed by the copy-out that
follows the call without a host synchronise.

This is a plain module (no conftest, no fixtures).  It needs no GPU to be imported: TABLE, EXCLUDED and the case lists are
what the CPU test of tests/test_hip_streams.py reads.  `python tests/stream_cases.py <family>` is the GPU run, in a process
of its own because torch must be imported before the library (one HIP runtime: libdwt_amd/__init__.py).

Expected values come from the CPU side only -- oraclelib and the tests/*_model.py models, called as each family's GPU test
calls them -- and every comparison is that family's own (named at each case list); no tolerance is introduced here."""
import os
import sys
import threading
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F32 = np.float32
D_FLOOR_MS = 50.0  # only so that a wrong-stream kernel -- microseconds at these sizes -- has finished long before the input arrives

# ---- the table of kinds ------------------------------------------------------------------------------------------------
# Every public callable of libdwt_amd that takes a device pointer and launches work has a row here ("name" or
# "name[variant]") or stands in EXCLUDED with its reason.  "async": the call returns while the stream is still busy.
# "sync(reason)": a hipStreamSynchronize(g.stream) -- or a copy that waits for the stream -- lies on the entry's path; the
# reason names the value that goes to the host.  Built from the code, call path by call path.
ASYNC = "async"


def SYNC(reason):
    return "sync(%s)" % reason


_W2D = ("cdf97_2%s_s", "cdf53_2%s_i", "cdf53_2%s_s", "cdf97_2%s_d", "cdf53_2%s_d", "cdf97_2%s_i", "interp53_2%s_s", "cdf53_2%s_i16",
        "cdf97_2%s_h")
_WEIGHTS = SYNC("the wrapper brings the weight arrays to the host: dwt_hip_memcpy_h2d / _d2h")
_RECORDS = SYNC("the per-band records are read back and finished on the host")
TABLE = {}
for _w in _W2D:
    TABLE["dwt_" + _w % "f"] = TABLE["dwt_" + _w % "i"] = ASYNC
TABLE.update({
    "dwt_cdf97_2f_s2": ASYNC, "dwt_cdf97_2i_s2": ASYNC,
    "dwt_cdf97_2f_inplace_s": ASYNC, "dwt_cdf97_2i_inplace_s": ASYNC, "dwt_cdf53_2f_inplace_s": ASYNC,
    "dwt_cdf53_2i_inplace_s": ASYNC, "dwt_cdf97_2f_inplace_i": ASYNC, "dwt_cdf97_2i_inplace_i": ASYNC,
    "transform2d_batch": ASYNC,
    "transform1d_batch": ASYNC,
    "dwt_eaw53_2f_s": _WEIGHTS, "dwt_eaw53_2i_s": _WEIGHTS, "dwt_eaw53_2f_inplace_s": _WEIGHTS, "dwt_eaw53_2i_inplace_s": _WEIGHTS,
    "dwt_eaw97_2f_s": _WEIGHTS, "dwt_eaw97_2i_s": _WEIGHTS,
    "eaw53_2d_batch": ASYNC, "eaw97_2d_batch": ASYNC,
    "features2d": _RECORDS, "features2d_batch": _RECORDS, "features1d_batch": _RECORDS,
    "bands_apply": ASYNC, "bands_apply_batch": ASYNC, "bands_apply_batch[per-image tables]": ASYNC,  # (the tables' upload from pageable memory is staged by the runtime: no wait)
    "map_log": ASYNC, "map_exp": ASYNC,
    "universal_threshold_batch": SYNC("the medians are read back; the thresholds are finished on the host"),
    "keep_largest_batch": SYNC("thr and kept are read back"),
    "keep_largest_batch[no records]": ASYNC,  # (thr == NULL && kept == NULL: "does not wait for the device")
    "magnitude_batch": ASYNC,
    "rows_condition": ASYNC,
    "rows_condition[per operation]": SYNC("`moved` is read back after every centring iteration"),
    "rows_center_index": SYNC("the centres go to a host array"), "rows_center_index[device result]": ASYNC,
    "rows_min_max": SYNC("min and max go to host arrays"), "rows_min_max[device result]": ASYNC,
    "dwt_hip_abs": ASYNC, "dwt_util_shift_s": ASYNC, "dwt_util_scale_s": ASYNC,
    "rows_displace": ASYNC, "rows_displace[host array]": SYNC("the host array of moves is uploaded and waited for"),
    "swt1d_batch": ASYNC, "swt_features1d_batch": _RECORDS, "swt2d_batch": ASYNC, "swt2d_level": ASYNC,
    "timefreq_batch": ASYNC, "phase_derivative": ASYNC, "detect_ridges": ASYNC,
    "transform3d": ASYNC, "transform3d_op": ASYNC,
    "fill_workspace": ASYNC,  # (memsets on the context's stream: DESIGN.md s27)
})

_MIRROR = "a one-line mirror of %s, which is in the table"
_NO_WORK = "launches nothing: host arithmetic, a query or a setting"
_HOST_ONLY = "host memory only, or a host result by definition (synchronous like every host-pointer call)"
EXCLUDED = {
    "DeviceImage": "a class: hipMalloc, and blocking copies through dwt_hip_memcpy_h2d / _d2h", "DwtError": "a class: the exception type",
    "TimefreqBank": "a class: host tables of a bank", "volume_t": "a ctypes structure",
    "alloc_batch": "placement search: synchronous by contract, measures on its own buffers", "alloc_batch_note": _NO_WORK,
    "alloc_batch_report": _NO_WORK, "alloc_volumes": "placement search: synchronous by contract", "placement_report": _NO_WORK,
    "tune": "dwt_hip_tune is synchronous by contract (it times the call)", "tune_batch_multi": "multi-device: own streams and workers (test_hip_multi.py)",
    "transform2d_batch_multi": "multi-device: own streams and workers (test_hip_multi.py)",
    "transform2d_batch_sharded": "multi-device: own streams and workers (test_hip_multi.py)", "shard_bounds": _NO_WORK,
    "grant_access": _NO_WORK,
    "band_geometry": _NO_WORK, "band_levels": _NO_WORK, "band_slots": _NO_WORK, "count_subbands": _NO_WORK,
    "dwt_util_count_subbands_s": _NO_WORK, "eaw53_weights_layout": _NO_WORK, "dwt_eaw53_2f_dummy_s": _NO_WORK, "feature_mask": _NO_WORK,
    "rows_op_mask": _NO_WORK, "device_count": _NO_WORK, "device_name": _NO_WORK, "get_device": _NO_WORK, "set_device": _NO_WORK,
    "get_option": _NO_WORK, "set_option": _NO_WORK, "last_error": _NO_WORK, "set_stream": _NO_WORK, "use_torch_stream": _NO_WORK,
    "poison_workspace": "a switch of the Python package, no device work of its own: it puts fill_workspace, which is in the table, in front of the calls made through `lib`",
    "sync": "the synchronise itself", "dwt_util_init": _NO_WORK, "dwt_util_finish": "synchronises and frees the context",
    "dwt_util_get_accel": _NO_WORK, "dwt_util_set_accel": _NO_WORK, "dwt_util_viewport": _NO_WORK, "dwt_util_crop21": _NO_WORK,
    "dwt_util_subband_const_s": _NO_WORK, "volume_of": _NO_WORK, "timefreq_bank": "host tables; the bank's upload is a blocking hipMemcpy at first use",
    "prof_enable": "timing instrument: drains the stream", "prof_read": "timing instrument: drains the stream",
    "prof_read_levels": "timing instrument: drains the stream", "features_raw_sums": _NO_WORK,
    "rows_warnings": SYNC("two counters are read back") + ": a query of the last call, no work of its own",
    "volume_perftest_fwd97op_s": "a timing protocol: synchronous by contract",
    "transform2d_interleaved": _MIRROR % "the dwt_*_inplace_* entries (they call it)",
    "fdwt2_cdf97_horizontal_s": _MIRROR % "dwt_cdf97_2f_inplace_s (flavour 1 of the same driver)",
    "fdwt2_cdf97_vertical_s": _MIRROR % "dwt_cdf97_2f_inplace_s", "fdwt2_cdf97_diagonal_s": _MIRROR % "dwt_cdf97_2f_inplace_s",
    "fdwt2_cdf53_horizontal_s": _MIRROR % "dwt_cdf53_2f_inplace_s", "fdwt2_cdf53_vertical_s": _MIRROR % "dwt_cdf53_2f_inplace_s",
    "fdwt2_cdf53_diagonal_s": _MIRROR % "dwt_cdf53_2f_inplace_s",
    "dwt_cdf97_1f_s": _MIRROR % "transform1d_batch (one line)", "dwt_cdf97_1i_s": _MIRROR % "transform1d_batch (one line)",
    "dwt_cdf53_1f_s": _MIRROR % "transform1d_batch (one line)", "dwt_cdf53_1i_s": _MIRROR % "transform1d_batch (one line)",
    "dwt_interp53_1f_s": _MIRROR % "transform1d_batch (one line)", "dwt_interp53_1i_s": _MIRROR % "transform1d_batch (one line)",
    "dwt_cdf97_2f1_s": _MIRROR % "transform1d_batch", "dwt_cdf53_2f1_s": _MIRROR % "transform1d_batch",
    "keep_largest": _MIRROR % "keep_largest_batch (one frame; thr and kept always read back)",
    "map_log_batch": _MIRROR % "map_log (the same driver with a batch count)", "map_exp_batch": _MIRROR % "map_exp",
    "dwt_util_abs_s": _MIRROR % "dwt_hip_abs",
    "dwt_util_shift21_med_s": _MIRROR % "rows_condition", "dwt_util_center21_s": _MIRROR % "rows_condition",
    "dwt_util_center1_s": _MIRROR % "rows_condition", "dwt_util_scale21_s": _MIRROR % "rows_condition",
    "dwt_util_get_center1_s": _MIRROR % "rows_center_index", "dwt_util_find_min_max_s": _MIRROR % "rows_min_max",
    "dwt_util_displace1_s": _MIRROR % "rows_displace", "dwt_util_displace1_zero_s": _MIRROR % "rows_displace",
    "swt_cdf97_f_ex_stride_s": _MIRROR % "swt1d_batch (one level of one line)", "swt_cdf53_f_ex_stride_s": _MIRROR % "swt1d_batch (one level of one line)",
    "gabor_ft_s": _MIRROR % "timefreq_batch (one signal, a bank made for the call)", "gabor_ft_arg_s": _MIRROR % "timefreq_batch",
    "gabor_wt_s": _MIRROR % "timefreq_batch", "gabor_wt_arg_s": _MIRROR % "timefreq_batch", "gabor_st_s": _MIRROR % "timefreq_batch",
    "gabor_st_arg_s": _MIRROR % "timefreq_batch",
    "cdf97_3f_ip_sep_horizontal_s": _MIRROR % "transform3d (struct volume_t in front of it)",
    "cdf97_3i_ip_sep_horizontal_s": _MIRROR % "transform3d", "cdf97_3f_op_sep_horizontal_s": _MIRROR % "transform3d_op",
    "cdf97_3f_op_wrapper_s": _MIRROR % "transform3d_op",
}
for _n in ("wps", "maxidx", "mean", "med", "var", "stdev", "skew", "kurt", "maxnorm", "lpnorm", "norm"):
    EXCLUDED["dwt_util_%s_s" % _n] = _HOST_ONLY + ": features2d with a host vector"
    EXCLUDED["dwt_util_band_%s_s" % _n] = _HOST_ONLY + ": one float returned"
for _n in ("moment", "cmoment", "smoment"):
    EXCLUDED["dwt_util_band_%s_s" % _n] = _HOST_ONLY + ": one float returned"

FAMILIES = ("mallat2d", "mallat2d_batch", "oned", "eaw", "features", "bandops", "nterm", "condition", "swt", "timefreq", "volume")
RUNS = FAMILIES + ("chain", "threads")
DEFAULT_OPTIONS = {"generic": 0, "swt_fused": 1, "swt2d_fused": 1, "timefreq_tiled": 1, "vol_fused": 1, "cond_fused": -1}


# ---- a case ------------------------------------------------------------------------------------------------------------
def same_bytes(got, want):
    """bit for bit"""
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def same_floats(got, want):
    """conftest.same_floats (== swt_model.same, shape_model.same, test_hip_features.equal_bits): the same bits wherever
    neither side is a NaN, NaNs at the same places; integer buffers bit for bit"""
    if not np.issubdtype(want.dtype, np.floating):
        return same_bytes(got, want)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    ng, nw = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(ng, nw) and np.array_equal(got.view(u)[~ng], want.view(u)[~nw])


class Case:
    """name; entry: a key of TABLE; make(seed) -> {buffer name: numpy array} -- every device buffer of the call as it is
    before the call, inputs drawn from `seed`, outputs holding the family's sentinel; names that start with "_" are host
    values that go with the input; call(dwt, P, host) makes the call on the addresses P[name] and returns its host results;
    want(bufs) -> {buffer name: array after the call, "ret": host results}, from the CPU models alone; same: the family's
    comparison of one buffer (same_for: of the buffers named there); check_ret(got, want): of the host results; options: set
    for the call, restored after it; setup(dwt, P) / teardown(dwt): around the call, outside what is timed and while the
    stream is idle (they may synchronise)."""

    def __init__(self, name, entry, make, call, want, same=same_bytes, check_ret=None, options=None, same_for=None, setup=None, teardown=None):
        self.name, self.entry, self.make, self.call, self._want, self.same = name, entry, make, call, want, same
        self.setup, self.teardown = setup, teardown
        self.same_for = same_for or {}
        self.check_ret = check_ret or (lambda got, want: got == want)
        self.options = options or {}
        self._lock = threading.Lock()
        self._real = self._other = self._expected = None

    @property
    def kind(self):
        return TABLE[self.entry]

    @property
    def is_async(self):
        return self.kind == ASYNC

    def data(self):
        """(the real input, another valid input, the expectation for the real one): computed once, never modified"""
        with self._lock:
            if self._expected is None:
                self._real, self._other = self.make(0), self.make(1)
                self._expected = self._want({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self._real.items()})
                for d in (self._real, self._other, self._expected):
                    for v in d.values():
                        if isinstance(v, np.ndarray):
                            v.setflags(write=False)
            return self._real, self._other, self._expected

    def mismatches(self, got, ret):
        _, _, want = self.data()
        bad = [k for k in want if k != "ret" and not k.startswith("_") and not self.same_for.get(k, self.same)(got[k], want[k])]
        if "ret" in want and not self.check_ret(ret, want["ret"]):
            bad.append("host results %r, expected %r" % (ret, want["ret"]))
        return bad


def _crc(text):
    return zlib.crc32(text.encode())  # (hash() of a string changes from process to process)


def _rng(*key):
    return np.random.default_rng([_crc(k) if isinstance(k, str) else int(k) for k in key])


_ORC = None


def orc():
    global _ORC
    if _ORC is None:
        from oraclelib import Oracle

        _ORC = Oracle()
    return _ORC


# ---- 2-D Mallat -------------------------------------------------------------------------------------------------------
# W, H, J = 64, 48, 2: the size tests/test_hip_route.py argues for -- the smallest at which two levels are both >= 2 and
# dense, so that every wavelet takes its fused sweep on an aligned pitch and the 2-byte wavelets their widen / line-pass /
# narrow route on pitch 130.  Comparison: bit for bit (conftest.bits in tests/test_hip_parity.py, test_hip_i16.py,
# test_hip_f16.py, test_hip_interleaved.py).
W, H, J = 64, 48, 2
WAVELETS_2D = {"cdf97_s": np.float32, "cdf53_i": np.int32, "cdf53_s": np.float32, "cdf97_d": np.float64, "cdf53_d": np.float64,
               "cdf97_i": np.int32, "interp53_s": np.float32, "cdf53_i16": np.int16, "cdf97_h": np.float16}
_ORACLE_2D = {"cdf97_s": "cdf97_2%s_s", "cdf53_i": "cdf53_2%s_i", "cdf53_s": "cdf53_2%s_s", "cdf97_d": "cdf97_2%s_d", "cdf53_d": "cdf53_2%s_d",
              "cdf97_i": "cdf97_2%s_i"}
PAD_2D = 77  # what the pitch padding holds: it must come back


def model2d(wavelet, inverse, img, interleaved=False):
    """the J-level transform of the dense (H, W) image, in place, by the CPU restatement of its wavelet"""
    if interleaved:
        name = _ORACLE_2D[wavelet].replace("2%s", "2%s_inplace") % ("i" if inverse else "f")
        (orc().inv if inverse else orc().fwd)(name, img, J)
    elif wavelet in _ORACLE_2D:
        (orc().inv if inverse else orc().fwd)(_ORACLE_2D[wavelet] % ("i" if inverse else "f"), img, J)
    else:
        import f16_model
        import i16_model
        import interp53_model

        m = {"interp53_s": interp53_model, "cdf53_i16": i16_model, "cdf97_h": f16_model}[wavelet]
        (m.inv2d if inverse else m.fwd2d)(img, j_max=J)
    return img


def image2d(dtype, pitch, n, seed, what):
    """n images of H rows of `pitch` bytes one after the other, the padding PAD_2D; float16 holds 8-bit integers (no
    overflow at two levels), the integer types 12-bit ones (tests/test_hip_route.py), the floats uniform [0, 1)"""
    rng = _rng(seed, what)
    a = np.full((n * H, pitch // np.dtype(dtype).itemsize), PAD_2D, dtype)
    if dtype == np.float16:
        a[:, :W] = rng.integers(0, 256, size=(n * H, W))
    elif np.issubdtype(dtype, np.integer):
        a[:, :W] = rng.integers(-2048, 2048, size=(n * H, W))
    else:
        a[:, :W] = rng.random((n * H, W))
    return a


def _want2d(wavelet, inverse, key_in, key_out, n=1, interleaved=False):
    def want(b):
        out = b[key_out]
        for k in range(n):
            img = b[key_in][k * H:(k + 1) * H, :W].copy()  # (a copy: the source of an out-of-place call stays as it is)
            out[k * H:(k + 1) * H, :W] = model2d(wavelet, inverse, img, interleaved)
        return {key_in: b[key_in], key_out: out, "ret": J}
    return want


def _mallat2d():
    cases = []
    for wv, dt in WAVELETS_2D.items():
        es = np.dtype(dt).itemsize
        for inverse in (0, 1):
            fn = ("dwt_" + {**_ORACLE_2D, "interp53_s": "interp53_2%s_s", "cdf53_i16": "cdf53_2%s_i16", "cdf97_h": "cdf97_2%s_h"}[wv]) % ("i" if inverse else "f")
            cases.append(Case(  # the in-place entry on a dense pitch: staging of level 0's subbands, the LL scratch
                "%s in place" % fn, fn, lambda s, dt=dt, es=es, fn=fn: {"x": image2d(dt, W * es, 1, s, fn)},
                lambda dwt, P, h, fn=fn, es=es, inverse=inverse: getattr(dwt, fn)(P["x"], W * es, es, W, H, W, H, J) or (J if inverse else None),
                _want2d(wv, inverse, "x", "x")))
    for inverse in (0, 1):  # the _s2 out-of-place entries (float 9/7 only has them)
        fn = "dwt_cdf97_2%s_s2" % ("i" if inverse else "f")
        cases.append(Case(
            fn, fn, lambda s, fn=fn: {"x": image2d(np.float32, W * 4, 1, s, fn), "y": np.full((H, W), -5.0, F32)},
            lambda dwt, P, h, fn=fn, inverse=inverse: getattr(dwt, fn)(P["x"], P["y"], W * 4, 4, W, H, W, H, J) or (J if inverse else None),
            _want2d("cdf97_s", inverse, "x", "y")))
    for wv in ("cdf97_s", "cdf53_s", "cdf97_i"):  # the interleaved layout: 9/7 and 5/3 float, and the int 9/7 entry
        for inverse in (0, 1):
            fn = "dwt_" + _ORACLE_2D[wv].replace("2%s", "2%s_inplace") % ("i" if inverse else "f")
            dt = WAVELETS_2D[wv]
            cases.append(Case(
                fn, fn, lambda s, dt=dt, fn=fn: {"x": image2d(dt, W * 4, 1, s, fn)},
                lambda dwt, P, h, fn=fn, inverse=inverse: getattr(dwt, fn)(P["x"], W * 4, 4, W, H, W, H, J) or (J if inverse else None),
                _want2d(wv, inverse, "x", "x", interleaved=True)))

    def strided_want(b):  # channel 1 of two interleaved channels; channel 0 must come back
        b["x"][:, 1::2] = model2d("cdf97_s", 0, b["x"][:, 1::2].copy())
        return {"x": b["x"], "ret": J}
    cases.append(Case(  # a strided device image: pack, transform, unpack through the staging frame (tests/test_hip_strided_device.py)
        "dwt_cdf97_2f_s one channel of two", "dwt_cdf97_2f_s", lambda s: {"x": _rng(s, "strided").random((H, 2 * W), dtype=F32)},
        lambda dwt, P, h: dwt.dwt_cdf97_2f_s(P["x"] + 4, W * 8, 8, W, H, W, H, J), strided_want))
    cases.append(Case(  # option "generic": the exact line passes through the staging image
        "dwt_cdf97_2f_s generic", "dwt_cdf97_2f_s", lambda s: {"x": image2d(np.float32, W * 4, 1, s, "generic")},
        lambda dwt, P, h: dwt.dwt_cdf97_2f_s(P["x"], W * 4, 4, W, H, W, H, J), _want2d("cdf97_s", 0, "x", "x"), options={"generic": 1}))
    return cases


def _mallat2d_batch():
    cases = []
    for wv, dt in WAVELETS_2D.items():
        es = np.dtype(dt).itemsize
        for inverse in (0, 1):  # transform2d_batch with 2 images, out of place
            what = "transform2d_batch %s %s" % (wv, "inverse" if inverse else "forward")
            cases.append(Case(
                what, "transform2d_batch",
                lambda s, dt=dt, es=es, what=what: {"x": image2d(dt, W * es, 2, s, what), "y": np.full((2 * H, W), PAD_2D, dt)},
                lambda dwt, P, h, wv=wv, es=es, inverse=inverse: dwt.transform2d_batch(wv, inverse, P["x"], P["y"], W * es * H, 2, W * es, W, H, J),
                _want2d(wv, inverse, "x", "y", n=2)))
    for wv in ("cdf53_i16", "cdf97_h"):  # pitch 128 is the dense case of _mallat2d; pitch 130 (2 mod 4): widen, line passes, narrow
        dt = WAVELETS_2D[wv]
        for inverse in (0, 1):
            fn = "dwt_" + {"cdf53_i16": "cdf53_2%s_i16", "cdf97_h": "cdf97_2%s_h"}[wv] % ("i" if inverse else "f")
            cases.append(Case(
                "%s pitch 130" % fn, fn, lambda s, dt=dt, fn=fn: {"x": image2d(dt, 130, 1, s, fn + "130")},
                lambda dwt, P, h, fn=fn, inverse=inverse: getattr(dwt, fn)(P["x"], 130, 2, W, H, W, H, J) or (J if inverse else None),
                _want2d(wv, inverse, "x", "x")))
            what = "transform2d_batch %s pitch 130 %s" % (wv, "inverse" if inverse else "forward")
            cases.append(Case(
                what, "transform2d_batch", lambda s, dt=dt, what=what: {"x": image2d(dt, 130, 2, s, what), "y": np.full((2 * H, 65), PAD_2D, dt)},
                lambda dwt, P, h, wv=wv, inverse=inverse: dwt.transform2d_batch(wv, inverse, P["x"], P["y"], 130 * H, 2, 130, W, H, J),
                _want2d(wv, inverse, "x", "y", n=2)))
    return cases


# ---- 1-D ---------------------------------------------------------------------------------------------------------------
# 4 lines of 64: the fused kernel, one wave per line (tests/test_hip_route.py's 1-D call).  8200 samples: above N1D_MAX =
# 8192 (tests/test_hip_oned.py), so the exact passes run the first level and the fused kernel the prefix; 8200 rather than
# 8193 keeps the second level even.  Comparison: bit for bit (bits_equal of tests/test_hip_oned.py).
def model1d(wavelet, inverse, lines):
    if wavelet == "interp53_s":
        import interp53_model

        (interp53_model.inv1d if inverse else interp53_model.fwd1d)(lines)
        return lines
    from test_oned import restated

    for row in lines:
        restated(orc(), wavelet[:5], inverse, row, len(row))
    return lines


def _oned():
    cases = []

    def levels(n):
        return int(np.ceil(np.log2(n)))
    for wv in ("cdf97_s", "cdf53_s", "interp53_s"):
        for inverse in (0, 1):
            for n_lines, n, step, oop in ((4, 64, 1, True), (4, 64, 2, False), (2, 8200, 1, False)):
                what = "transform1d_batch %s %s %d x %d%s%s" % (wv, "inverse" if inverse else "forward", n_lines, n,
                                                                ", element stride 8" if step == 2 else "", ", out of place" if oop else "")

                def make(s, what=what, n_lines=n_lines, n=n, step=step, oop=oop):
                    b = {"x": (_rng(s, what).random((n_lines, n * step), dtype=F32) * 2 - 1).astype(F32)}
                    if oop:
                        b["y"] = np.full((n_lines, n), -5.0, F32)
                    return b

                def want(b, wv=wv, inverse=inverse, step=step, oop=oop, n=n):
                    out = model1d(wv, inverse, b["x"][:, ::step].copy())
                    if oop:
                        b["y"][:] = out
                    else:
                        b["x"][:, ::step] = out
                    b["ret"] = -1 if inverse else levels(n)
                    return b

                cases.append(Case(
                    what, "transform1d_batch", make,
                    lambda dwt, P, h, wv=wv, inverse=inverse, n_lines=n_lines, n=n, step=step, oop=oop:
                        dwt.transform1d_batch(wv, inverse, P["x"], P["y" if oop else "x"], n * step * 4, n_lines, n, -1, 4 * step), want))
    return cases


# ---- EAW 5/3 and 9/7 ---------------------------------------------------------------------------------------------------
# 64 x 48, 2 levels: dense Mallat frames with both sides >= 2 take the fused kernel at every size (eaw_fused_ok), so the
# 2-D size is the smallest here too; no line of one sample, so every weight is written.  alpha 1: the reference's bits.
# Comparison: conftest.same_floats for the image, eaw_model.same_weights for the weights (tests/test_hip_eaw.py,
# test_hip_eaw97.py) -- the same criterion as same_floats here where the model writes every weight.
def _eaw():
    import eaw97_model
    import eaw_model

    cases = []
    B, SENT = 2, F32(9.0)

    def models(wavelet, layout):
        if wavelet == "eaw97":
            return eaw97_model.mallat_fwd, eaw97_model.mallat_inv
        return (eaw_model.interleaved_fwd, eaw_model.interleaved_inv) if layout else (eaw_model.mallat_fwd, eaw_model.mallat_inv)

    def weights_ok(got, want):
        return got[0] == want[0] and all(len(g) == len(w) and all(eaw_model.same_weights(a, b) for a, b in zip(g, w)) for g, w in zip(got[1:], want[1:]))

    for wavelet, layout, stem in (("eaw53", 0, "dwt_eaw53_2%s_s"), ("eaw53", 1, "dwt_eaw53_2%s_inplace_s"), ("eaw97", 0, "dwt_eaw97_2%s_s")):
        fwd, inv = models(wavelet, layout)
        for inverse in (0, 1):  # the single-image entries: the weights cross to the host in the wrapper
            fn = stem % ("i" if inverse else "f")

            def make(s, fn=fn, inverse=inverse, fwd=fwd):
                x = (_rng(s, fn).random((H, W), dtype=F32) * 8 - 4).astype(F32)
                if not inverse:
                    return {"x": x}
                _, wH, wV = fwd(x, j_max=J)
                return {"x": x, "_wH": wH, "_wV": wV}

            def want(b, inverse=inverse, fwd=fwd, inv=inv):
                if inverse:
                    inv(b["x"], b["_wH"], b["_wV"], j_max=J)
                    return {"x": b["x"], "ret": J}
                j, wH, wV = fwd(b["x"], j_max=J)
                return {"x": b["x"], "ret": (j, wH, wV)}

            def call(dwt, P, h, fn=fn, inverse=inverse):
                if inverse:
                    return getattr(dwt, fn)(P["x"], W * 4, 4, W, H, W, H, J, 0, 0, h["_wH"], h["_wV"])
                return getattr(dwt, fn)(P["x"], W * 4, 4, W, H, W, H, J, 0, 0, alpha=1.0)
            cases.append(Case(fn, fn, make, call, want, same_floats, (lambda g, w: g == w) if inverse else weights_ok))
    for wavelet in ("eaw53", "eaw97"):  # the batch entries with device weights: one launch per level, nothing crosses to the host
        fwd, inv = models(wavelet, 0)
        fn = wavelet + "_2d_batch"
        for inverse in (0, 1):
            what = "%s %s" % (fn, "inverse" if inverse else "forward")

            def layout():
                import libdwt_amd as dwt

                return dwt.eaw53_weights_layout(dwt.EAW_MALLAT, W, H, W, H, J)

            def flat(wH, wV, into):
                _, hs, vs = layout()
                for k in range(J):
                    for (o, (a, b)), arr in ((hs[k], wH[k]), (vs[k], wV[k])):
                        into[o:o + a * b] = np.asarray(arr, F32).reshape(-1)
                return into

            def make(s, what=what, inverse=inverse, fwd=fwd):
                ws = layout()[0] + 7
                x = (_rng(s, what).random((B * H, W), dtype=F32) * 8 - 4).astype(F32)
                w = np.full(B * ws, SENT, F32)
                if inverse:  # coefficients and weights of a forward transform: what an inverse is called with
                    for k in range(B):
                        img = x[k * H:(k + 1) * H]
                        _, wH, wV = fwd(img, j_max=J)
                        flat(wH, wV, w[k * ws:(k + 1) * ws])
                return {"x": x, "w": w}

            def want(b, inverse=inverse, fwd=fwd, inv=inv):
                total, hs, vs = layout()
                ws = total + 7
                for k in range(B):
                    img, w = b["x"][k * H:(k + 1) * H], b["w"][k * ws:(k + 1) * ws]
                    if inverse:
                        wH = [w[o:o + a * c].reshape(a, c) for o, (a, c) in hs]
                        wV = [w[o:o + a * c].reshape(a, c) for o, (a, c) in vs]
                        inv(img, wH, wV, j_max=J)
                    else:
                        _, wH, wV = fwd(img, j_max=J)
                        flat(wH, wV, w)
                return {"x": b["x"], "w": b["w"], "ret": J}

            def call(dwt, P, h, fn=fn, inverse=inverse):
                ws = layout()[0] + 7
                return getattr(dwt, fn)(inverse, P["x"], H * W * 4, B, W * 4, W, H, P["w"], ws, J, alpha=1.0)
            cases.append(Case(what, fn, make, call, want, same_floats))
    return cases


# ---- features ----------------------------------------------------------------------------------------------------------
# (64, 64, 5) and (4096, 1, 13): the smallest image and the smallest row of EXACT_SHAPES in tests/test_hip_features.py --
# the class of inputs (small integers, every band summing to zero) whose sums are exact in every order, so that every
# feature is compared bit for bit against the sequential float32 restatement (features_model.seq32), the median as a value;
# the median runs its histogram passes.  p = 2.
def _features():
    import features_model as fm
    from test_hip_features import balanced

    cases = []
    names = list(fm.NAMES)

    def block(img, w, h, j_max):
        ref = fm.seq32(img, w, h, w, h, j_max, 2.0)
        return np.concatenate([np.asarray(ref[n], F32) for n in names])

    def same_fv(got, want):  # (test_exact_class_bit_identical: med by value, everything else by bits, NaN == NaN)
        nb = (want.shape[1] - 3) // len(names)
        med = slice(names.index("med") * nb, (names.index("med") + 1) * nb)
        rest = np.ones(want.shape[1], bool)
        rest[med] = False
        return np.array_equal(got[:, med], want[:, med]) and same_floats(np.ascontiguousarray(got[:, rest]), np.ascontiguousarray(want[:, rest]))

    for fn, (w, h, j_max), batch in (("features2d", (64, 64, 5), 1), ("features2d_batch", (64, 64, 5), 2), ("features1d_batch", (4096, 1, 13), 3)):
        nb = fm.count_subbands(w, h, w, h, j_max)
        stride = len(names) * nb + 3

        def make(s, fn=fn, w=w, h=h, j_max=j_max, batch=batch, stride=stride):
            rng = _rng(s, fn)
            return {"x": np.stack([balanced(rng, w, h, w, h, j_max) for _ in range(batch)]), "fv": np.full((batch, stride), np.nan, F32)}

        def want(b, w=w, h=h, j_max=j_max, batch=batch, stride=stride):
            for k in range(batch):
                b["fv"][k, :stride - 3] = block(b["x"][k], w, h, j_max)
            return b

        def call(dwt, P, hh, fn=fn, w=w, h=h, j_max=j_max, batch=batch, stride=stride):
            if fn == "features2d":
                return dwt.features2d(names, P["x"], w * 4, 4, w, h, w, h, j_max, P["fv"], 2.0)
            if fn == "features2d_batch":
                return dwt.features2d_batch(names, P["x"], h * w * 4, batch, w * 4, w, h, j_max, P["fv"], stride, 2.0)
            return dwt.features1d_batch(names, P["x"], w * 4, 4, batch, w, j_max, P["fv"], stride, 2.0)
        cases.append(Case(fn, fn, make, call, want, same_floats, same_for={"fv": same_fv}))
    return cases


# ---- band operators ----------------------------------------------------------------------------------------------------
# 37 x 29 at 3 levels: the frame of test_batch_with_per_image_tables / _one_table in tests/test_hip_shape.py (odd sizes, every
# band non-empty, one chunk per band); the maps on its 21 x 13 frame.  Comparison: that file's check_table (bit for bit
# but COMPRESS magnitudes within 1 ulp of the float64 model, its own bound), maps within 1 ulp of shape_model.apply_op (its
# test_maps), the threshold bit for bit; every word outside the frames bit for bit.
def _bandops():
    import shape_model as sm
    from test_hip_shape import check_table, frames

    cases = []
    sox, soy, JB = 37, 29, 3
    ns = 3 * JB + 1

    def laid(s, what, n, pad, step=1, h=soy, w=sox):
        return frames([sm.make_input(_crc(what) % 1000 + 17 * s + b, h, w) for b in range(n)], pad, step)[0]

    def table_same(tables, n, pad, step=1):
        """the comparison of a laid-out buffer: frame b against tables[b] with check_table, everything else bit for bit"""
        def same(got, want_and_input):
            x = want_and_input  # (the expectation is the INPUT buffer: check_table applies the model itself)
            mask = np.zeros(x.shape, bool)
            mask[:, :soy, :sox * step:step] = True
            if not np.array_equal(got.view(np.uint32)[~mask], x.view(np.uint32)[~mask]):
                return False
            try:
                for b in range(n):
                    ops, params = tables[b]
                    check_table(got[b, :soy, :sox * step:step], x[b, :soy, :sox * step:step], (sox, soy, sox, soy), JB, ops, params)
            except AssertionError as e:
                print("    check_table:", e)
                return False
            return True
        return same

    one = sm.make_table("mixed", ns, shift=1)
    cases.append(Case("bands_apply", "bands_apply", lambda s: {"x": laid(s, "apply", 1, 1)},
                      lambda dwt, P, h: dwt.bands_apply(P["x"], 38 * 4, 4, sox, soy, sox, soy, JB, *one), lambda b: b, table_same([one], 1, 1)))
    cases.append(Case("bands_apply strided frame", "bands_apply", lambda s: {"x": laid(s, "strided", 1, 1, 2)},  # (staged through frame_a)
                      lambda dwt, P, h: dwt.bands_apply(P["x"], 38 * 8, 8, sox, soy, sox, soy, JB, *one), lambda b: b, table_same([one], 1, 1, 2)))
    soft = sm.make_table("soft", ns)
    cases.append(Case("bands_apply_batch one table", "bands_apply_batch", lambda s: {"x": laid(s, "shared", 4, 0)},
                      lambda dwt, P, h: dwt.bands_apply_batch(P["x"], 30 * 37 * 4, 4, 37 * 4, sox, soy, JB, *soft), lambda b: b,
                      table_same([soft] * 4, 4, 0)))
    # per-image tables, twice back to back with different tables and no synchronise in between: the second call refills the
    # host vector the first call's upload was given
    ts = ns + 2
    tabs = []
    for call_no in range(2):
        ops, params = np.zeros((3, ts), np.int32), np.zeros((3, ts), F32)
        for b in range(3):
            ops[b, :ns], params[b, :ns] = sm.make_table("mixed", ns, shift=b + 1 + 3 * call_no)
            params[b, :ns] *= F32(1 + b + call_no)
        ops[:, ns:] = 77  # (behind a table: never read)
        tabs.append((ops, params))

    def twice(dwt, P, h):
        for k, name in enumerate(("x", "y")):
            dwt.bands_apply_batch(P[name], 30 * 38 * 4, 3, 38 * 4, sox, soy, JB, tabs[k][0], tabs[k][1], ts)

    per_image = {name: table_same([(tabs[k][0][b, :ns], tabs[k][1][b, :ns]) for b in range(3)], 3, 1) for k, name in enumerate(("x", "y"))}
    cases.append(Case("bands_apply_batch per-image tables, twice", "bands_apply_batch[per-image tables]",
                      lambda s: {"x": laid(s, "per-image a", 3, 1), "y": laid(s, "per-image b", 3, 1)}, twice, lambda b: b, same_for=per_image))
    for op, fn in ((sm.LOG, "map_log"), (sm.EXP, "map_exp")):
        def want(b, op=op):
            b["x"][0, :13, :21] = sm.apply_op(b["x"][0, :13, :21], op, 1e-5)
            return b

        def same_map(got, want):  # (test_maps: within 1 ulp of the float64 model rounded once; the background bit for bit)
            mask = np.zeros(want.shape, bool)
            mask[:, :13, :21] = True
            return np.array_equal(got.view(np.uint32)[~mask], want.view(np.uint32)[~mask]) and int(sm.ulps(got[mask], want[mask]).max()) <= 1
        cases.append(Case(fn, fn, lambda s, fn=fn: {"x": laid(s, fn, 1, 1, h=13, w=21)},
                          lambda dwt, P, h, fn=fn: getattr(dwt, fn)(P["x"], 22 * 4, 4, 21, 13, 1e-5), want, same_map))

    def thr_make(s):
        with np.errstate(over="ignore"):
            return {"x": frames([sm.threshold_input(sm.make_input(40 + 5 * s + b, soy, sox) * F32(1 + b), sox, soy) for b in range(3)], 4)[0]}

    def thr_want(b):
        b["ret"] = np.array([sm.threshold(b["x"][k, :soy, :sox], sox, soy) for k in range(3)], F32)
        return b
    cases.append(Case("universal_threshold_batch", "universal_threshold_batch", thr_make,
                      lambda dwt, P, h: dwt.universal_threshold_batch(P["x"], 30 * 41 * 4, 3, 41 * 4, sox, soy), thr_want,
                      check_ret=lambda g, w: np.array_equal(g.view(np.uint32), w.view(np.uint32))))
    return cases


# ---- N-term ------------------------------------------------------------------------------------------------------------
# 37 x 29, five groups, five ranks, two channels: test_batch_of_five of tests/test_hip_nterm.py (odd sizes, a pitch that is
# no multiple of 16 bytes, several groups in one launch).  Comparison: exact -- == on the uint32 image of coefficients,
# thresholds and magnitudes, == on the kept counts; the padding (3e38) bit for bit.
def _nterm():
    import nterm_model as nm
    from test_hip_nterm import lay

    cases = []
    w, h, ch, n, pad = 37, 29, 2, 5, 3
    keep = [1, w * h // 2, w * h, 17, 0]

    def make(s, what="keep"):
        xs = np.stack([nm.make_input(40 + 10 * s + b, "normal", ch, h, w) * F32(10.0 ** (b - 2)) for b in range(n)])
        return {"x": lay(xs, pad)[0]}

    def want(b, records=True):
        thr, kept = np.zeros(n, F32), np.zeros(n, np.int32)
        for g in range(n):
            out, thr[g], kept[g] = nm.keep_largest(b["x"][g, :ch, :h, :w], keep[g])
            b["x"][g, :ch, :h, :w] = out
        if records:
            b["ret"] = (thr, kept)
        return b

    bs, cs, sx = (ch + 1) * (h + 1) * (w + pad) * 4, (h + 1) * (w + pad) * 4, (w + pad) * 4  # of lay()'s buffer
    cases.append(Case("keep_largest_batch", "keep_largest_batch", make,
                      lambda dwt, P, hh: dwt.keep_largest_batch(P["x"], bs, n, ch, cs, sx, w, h, keep), want,
                      check_ret=lambda g, wt: np.array_equal(g[0].view(np.uint32), wt[0].view(np.uint32)) and np.array_equal(g[1], wt[1])))

    def no_records(dwt, P, hh):  # thr == NULL && kept == NULL: the header's call that "does not wait for the device"
        k = np.ascontiguousarray(keep, np.int32)
        rc = dwt.lib.dwt_hip_keep_largest_batch(P["x"], bs, n, ch, cs, sx, w, h, -1, 0, k.ctypes.data, None, None)
        assert rc == 0, dwt.last_error()
    cases.append(Case("keep_largest_batch without thr and kept", "keep_largest_batch[no records]", make, no_records, lambda b: want(b, False)))

    def mag_make(s):
        b = make(s)
        b["m"] = np.ascontiguousarray(lay(np.zeros((n, 1, h, w), F32), 7)[0][:, 0])
        return b

    def mag_want(b):
        for g in range(n):
            b["m"][g, :h, :w] = nm.magnitudes(b["x"][g, :ch, :h, :w])
        return b
    cases.append(Case("magnitude_batch", "magnitude_batch", mag_make,
                      lambda dwt, P, hh: dwt.magnitude_batch(P["x"], bs, n, ch, cs, sx, w, h, P["m"], (h + 1) * (w + 7) * 4, (w + 7) * 4), mag_want))
    return cases


# ---- conditioning ------------------------------------------------------------------------------------------------------
# 64 samples, one row of every kind of condition_model.KINDS: the smallest size of tests/test_hip_condition.py with every
# code path of the centring (its reversing row lives at 64 too); 3 canary elements behind each row.  Comparison: that
# file's `same` (bit for bit, zeros by value) for the rows, == for info, centres, minima, maxima and displaced rows.
def _condition():
    import condition_model as cm
    from test_hip_condition import CANARY, frame
    from test_hip_condition import same as same_rows

    cases = []
    N, pad = 64, 3
    ls = (N + pad) * 4

    def rows(s, what):
        x = np.concatenate([cm.make_input(1000 + 17 * k + N + 100 * s + _crc(what) % 50, kind, 1, N) for k, kind in enumerate(cm.KINDS)])
        return np.concatenate([x, cm.reversing_row()[None, :]]) if s == 0 else np.concatenate([x, x[:1]])

    R = len(cm.KINDS) + 1

    def same(got, want):
        return same_rows(got, want) if got.dtype == F32 else np.array_equal(got, want)

    for ops in (1, 2, 4, 7):  # every operator, and all three: the fused kernel (the default for this batch), info in device memory
        for entry, options in (("rows_condition", {}),) + ((("rows_condition[per operation]", {"cond_fused": 0}),) if ops == 7 else ()):
            what = "%s ops %d" % (entry, ops)

            def want(b, ops=ops):
                out, info = cm.condition(b["x"][:R, :N], ops, 20, -1.0, 2.5)
                b["x"][:R, :N] = out
                b["info"][:] = info
                return b
            cases.append(Case(what, entry, lambda s, what=what: {"x": frame(rows(s, what), pad, 1), "info": np.full((R, 4), -99, np.int32)},
                              lambda dwt, P, h, ops=ops: dwt.rows_condition(ops, P["x"], ls, 4, R, N, 20, -1.0, 2.5, P["info"]), want, same, options=options))

    def centres(b):
        return np.array([cm.get_center1(r) for r in b["x"][:R, :N]], np.int32)
    cases.append(Case("rows_center_index", "rows_center_index", lambda s: {"x": frame(rows(s, "centre"), pad, 1)},
                      lambda dwt, P, h: dwt.rows_center_index(P["x"], ls, 4, R, N), lambda b: dict(b, ret=centres(b)), same,
                      check_ret=np.array_equal))
    cases.append(Case("rows_center_index, device result", "rows_center_index[device result]",
                      lambda s: {"x": frame(rows(s, "centre d"), pad, 1), "c": np.full(R, -99, np.int32)},
                      lambda dwt, P, h: dwt.rows_center_index(P["x"], ls, 4, R, N, P["c"]) and None, lambda b: dict(b, c=centres(b)), same))

    def extremes(b):
        mm = [cm.min_max(r) for r in b["x"][:R, :N]]
        return np.array([m[0] for m in mm], F32), np.array([m[1] for m in mm], F32)
    cases.append(Case("rows_min_max", "rows_min_max", lambda s: {"x": frame(rows(s, "minmax"), pad, 1)},
                      lambda dwt, P, h: dwt.rows_min_max(P["x"], ls, 4, R, N), lambda b: dict(b, ret=extremes(b)), same,
                      check_ret=lambda g, w: np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])))
    cases.append(Case("rows_min_max, device result", "rows_min_max[device result]",
                      lambda s: {"x": frame(rows(s, "minmax d"), pad, 1), "mn": np.full(R, CANARY, F32), "mx": np.full(R, CANARY, F32)},
                      lambda dwt, P, h: dwt.rows_min_max(P["x"], ls, 4, R, N, P["mn"], P["mx"]) and None,
                      lambda b: dict(b, mn=extremes(b)[0], mx=extremes(b)[1]), same, same_for={"mn": np.array_equal, "mx": np.array_equal}))
    # the element kernels (dwt_util_shift_s: x += a, dwt_util_scale_s: x *= a, dwt_hip_abs: the sign bit cleared), each one
    # float32 operation per sample: numpy's float32 add, multiply and absolute value are the model; bit for bit
    def element(fn, op):
        def want(b):
            with np.errstate(all="ignore"):
                b["x"][:R, :N] = op(b["x"][:R, :N])
            return b
        call = (lambda dwt, P, h: dwt.dwt_hip_abs(P["x"], ls, 4, N, R)) if fn == "dwt_hip_abs" else \
            (lambda dwt, P, h: getattr(dwt, fn)(P["x"], N, R, ls, 4, 1.75) and None)
        return Case(fn, fn, lambda s: {"x": frame(rows(s, fn), pad, 1)}, call, want, same_floats)
    cases.append(element("dwt_util_shift_s", lambda x: (x + F32(1.75)).astype(F32)))
    cases.append(element("dwt_util_scale_s", lambda x: (x * F32(1.75)).astype(F32)))
    cases.append(element("dwt_hip_abs", lambda x: np.abs(x)))
    ds = np.array([-N - 1, -3, 0, 2, N, 1, -1, N - 1, -(N - 1)], np.int32)[:R]

    def displaced(b, zero):
        b["x"][:R, :N] = np.stack([cm.displace1(r, int(d), zero) for r, d in zip(b["x"][:R, :N].copy(), ds)])
        return b
    class Address:  # (the wrapper takes a bare int for one move for every row: a device array goes in as a tensor would)
        def __init__(self, p):
            self.p = p

        def data_ptr(self):
            return self.p
    cases.append(Case("rows_displace, device array", "rows_displace", lambda s: {"x": frame(rows(s, "displace d"), pad, 1), "d": ds.copy()},
                      lambda dwt, P, h: dwt.rows_displace(P["x"], ls, 4, R, N, Address(P["d"]), zero_fill=True), lambda b: displaced(b, True), same))
    cases.append(Case("rows_displace, host array", "rows_displace[host array]", lambda s: {"x": frame(rows(s, "displace h"), pad, 1)},
                      lambda dwt, P, h: dwt.rows_displace(P["x"], ls, 4, R, N, ds, zero_fill=False), lambda b: displaced(b, False), same))
    return cases


# ---- SWT ---------------------------------------------------------------------------------------------------------------
# 1-D: 3 lines of 64 samples at 3 levels (the smallest N of COEFF_CASES in tests/test_hip_swt.py with more than one level of
# real taps; <= 8192 so that option swt_fused picks between one launch and one per level).  2-D: 2 images of 33 x 40 at 2
# levels (tests/test_hip_swt2d.py's smallest size with both sides above a tile edge's halo; below the 5 fused levels, so
# that option swt2d_fused picks between one launch and two per level).  Comparison: swt_model.same, bitwise with NaN == NaN;
# the features are the order statistics, which tests/test_hip_swt.py compares exactly (median by value).
def _swt():
    import features_model as fm
    import swt2d_model as m2
    import swt_model as sm

    cases = []
    lines, N, L = 3, 64, 3
    CAN = np.array([0xDEADBEEF], np.uint32).view(F32)[0]
    for fused in (1, 0):
        for wv in sm.WAVELETS:
            def want(b, wv=wv):
                Lp, Hp = sm.swt_levels(b["x"], wv, L)
                b["h"][:], b["l"][:] = Hp, Lp
                return b
            cases.append(Case("swt1d_batch %s swt_fused %d" % (wv, fused), "swt1d_batch",
                              lambda s, wv=wv: {"x": sm.make_input(300 + s, "normal", lines, N), "h": np.full((L, lines, N), CAN, F32), "l": np.full((L, lines, N), CAN, F32)},
                              lambda dwt, P, h, wv=wv: dwt.swt1d_batch(wv, P["x"], N * 4, 4, lines, N, L, P["h"], P["l"], 2, lines * N * 4, N * 4),
                              want, same_floats, options={"swt_fused": fused}))
        names = ["maxidx", "med", "maxnorm"]
        stride = len(names) * L + 3

        def fwant(b):
            planes = sm.swt_levels(b["x"], "cdf97_s", L)[1]
            for y in range(lines):
                for i, q in enumerate(n for n in fm.NAMES if n in names):
                    b["fv"][y, i * L:(i + 1) * L] = [fm.order_stats(planes[l, y])[q] for l in range(L)]
            return b

        def fsame(got, want):
            if got.shape != (lines, stride):
                return same_floats(got, want)
            med = slice(1 * L, 2 * L)  # (enum order: maxidx, med, maxnorm)
            rest = np.ones(stride, bool)
            rest[med] = False
            return np.array_equal(got[:, med], want[:, med]) and same_floats(np.ascontiguousarray(got[:, rest]), np.ascontiguousarray(want[:, rest]))
        cases.append(Case("swt_features1d_batch swt_fused %d" % fused, "swt_features1d_batch",
                          lambda s: {"x": sm.make_input(400 + s, "normal", lines, N), "fv": np.full((lines, stride), np.nan, F32)},
                          lambda dwt, P, h: dwt.swt_features1d_batch("cdf97_s", names, P["x"], N * 4, 4, lines, N, L, P["fv"], stride, 0, 2.0),
                          fwant, fsame, options={"swt_fused": fused}))
    B, h2, w2, L2 = 2, 33, 40, 2
    for fused in (1, 0):
        for wv in sm.WAVELETS:
            def want2(b, wv=wv):
                LL, D = m2.swt2d_levels(b["x"], wv, L2)  # (levels, batch, h, w), (levels, 3, batch, h, w)
                b["h"][:] = D.transpose(2, 0, 1, 3, 4).reshape(B, 3 * L2, h2, w2)
                b["l"][:, :L2] = LL.transpose(1, 0, 2, 3)
                return b
            cases.append(Case("swt2d_batch %s swt2d_fused %d" % (wv, fused), "swt2d_batch",
                              lambda s, wv=wv: {"x": np.stack([m2.make_input(500 + 7 * s + k, "normal", h2, w2) for k in range(B)]),
                                                "h": np.full((B, 3 * L2, h2, w2), CAN, F32), "l": np.full((B, 3 * L2, h2, w2), CAN, F32)},
                              lambda dwt, P, h, wv=wv: dwt.swt2d_batch(wv, P["x"], h2 * w2 * 4, B, w2 * 4, 4, w2, h2, L2, P["h"], P["l"], 2,
                                                                       3 * L2 * h2 * w2 * 4, h2 * w2 * 4, w2 * 4),
                              want2, same_floats, options={"swt2d_fused": fused}))
        # (dst_h and dst_l share dst_batch_stride: the LL planes of image b lie 3 * L2 planes apart as well, the rest canary)

        def wantl(b):
            b["ll"][:], b["hl"][:], b["lh"][:], b["hh"][:] = m2.swt2d_level(b["x"], "cdf97_s", 1)
            return b
        cases.append(Case("swt2d_level swt2d_fused %d" % fused, "swt2d_level",
                          lambda s: dict({"x": m2.make_input(600 + s, "normal", h2, w2)}, **{k: np.full((h2, w2), CAN, F32) for k in ("ll", "hl", "lh", "hh")}),
                          lambda dwt, P, h: dwt.swt2d_level("cdf97_s", P["x"], w2 * 4, 4, w2, h2, 1, P["ll"], P["hl"], P["lh"], P["hh"], w2 * 4),
                          wantl, same_floats, options={"swt2d_fused": fused}))
    return cases


# ---- time-frequency planes ---------------------------------------------------------------------------------------------
# 2 lines of 64 samples against the 5 kernels of the S transform: the (64, 5) size of timefreq_model.CASES whose kernels
# are longer than the line at the low bins (zero padding of the tiled kernel) and shorter at the high ones.  Comparison:
# swt_model.same -- complex sums, magnitudes, phase derivative and ridges 1 and 2 are bitwise in tests/test_hip_timefreq.py.
# (Arguments carry that file's ulp bound and detect_ridges kind 3 its excused points: both left to that file.)
def _timefreq():
    import timefreq_model as tm

    cases = []
    lines, N, bins = 2, 64, 5
    CAN = np.array([0xDEADBEEF], np.uint32).view(F32)[0]
    bank = {}

    def the_bank(dwt):
        key = threading.get_ident()  # a bank is used by one thread at a time
        if key not in bank:
            bank[key] = dwt.timefreq_bank("st", bins)
        return bank[key]

    def taps():
        import libdwt_amd as dwt

        return the_bank(dwt).query()  # host tables, generated on the host as the reference generates them

    for tiled in (1, 0):
        for out in ("complex", "abs"):
            wd = 2 if out == "complex" else 1

            def want(b, out=out, wd=wd):
                sizes, centers, tp = taps()
                for y in range(lines):
                    re, im, mag = tm.planes(b["x"][y], sizes, centers, tp)
                    b["p"][y] = np.stack([re, im], axis=-1).reshape(bins, N * 2) if out == "complex" else mag
                return b
            cases.append(Case("timefreq_batch %s timefreq_tiled %d" % (out, tiled), "timefreq_batch",
                              lambda s, wd=wd: {"x": tm.make_input(700 + s, "normal", lines, N), "p": np.full((lines, bins, N * wd), CAN, F32)},
                              lambda dwt, P, h, out=out, wd=wd: dwt.timefreq_batch(the_bank(dwt), P["x"], N * 4, 4, lines, N, out, P["p"], bins * N * wd * 4, N * wd * 4),
                              want, same_floats, options={"timefreq_tiled": tiled}))
    rows = 9

    def planes_in(s, what):
        return {"x": (_rng(s, what).random((2, rows, N), dtype=F32) * 8 - 4).astype(F32), "y": np.full((2, rows, N), CAN, F32)}

    def op_want(f):
        def want(b):
            b["y"][:] = np.stack([f(p) for p in b["x"]])
            return b
        return want
    cases.append(Case("phase_derivative", "phase_derivative", lambda s: planes_in(s, "pd"),
                      lambda dwt, P, h: dwt.phase_derivative(P["x"], P["y"], N * 4, 4, N, rows, tm.LIMIT, 2, rows * N * 4),
                      op_want(lambda p: tm.phase_derivative(p, tm.LIMIT)), same_floats))
    for kind, f in ((1, tm.ridges1), (2, tm.ridges2)):
        cases.append(Case("detect_ridges %d" % kind, "detect_ridges", lambda s, kind=kind: planes_in(s, "ridges%d" % kind),
                          lambda dwt, P, h, kind=kind: dwt.detect_ridges(kind, P["x"], P["y"], N * 4, 4, N, rows, 0.5, 2, rows * N * 4),
                          op_want(lambda p, f=f: f(p, 0.5)), same_floats))
    # The fill of the scratch, seen through a caller-owned workspace: the two bands are the case's buffers.
    # Their "input" arrives behind the delay; a fill that ran early or on another stream is overwritten by it.
    # (It stands in this family because no other case here uses the LL bands: handing them over frees the library's own.)
    FILL = 0xA5C3F00D
    sizes = {"b0": 1000, "b1": 77}

    def own(dwt, P):
        assert dwt.lib.dwt_hip_set_workspace(P["b0"], 4 * sizes["b0"], P["b1"], 4 * sizes["b1"]) == 0, dwt.last_error()

    def hand_back(dwt):
        assert dwt.lib.dwt_hip_set_workspace(None, 0, None, 0) == 0, dwt.last_error()
    cases.append(Case(
        "fill_workspace over a caller-owned workspace", "fill_workspace",
        lambda s: {k: _rng(s, "fill" + k).integers(0, 1 << 31, size=n).astype(np.uint32) for k, n in sizes.items()},
        lambda dwt, P, h: dwt.fill_workspace(FILL), lambda b: {k: np.full(n, FILL, np.uint32) for k, n in sizes.items()},
        setup=own, teardown=hand_back))
    return cases


# ---- 3-D ---------------------------------------------------------------------------------------------------------------
# Out of place: (2, 2, 256) is the smallest volume of test_out_of_place_forward_vs_oracle (tests/test_hip_volume.py) that
# the fused x+y+z kernel takes (128 samples wide or more; forced by vol_fused = 2 as there).  In place: (9, 33, 257), the
# smallest of IP_SHAPES for the one-pass in-place level.  (16, 16, 16) of test_volume_vs_oracle is narrower than the fused
# kernels take: two passes per level through the scratch volume.  Comparison: bit for bit against the oracle.
def _volume():
    from test_hip_volume import oracle_multilevel

    cases = []
    for shape, fused in (((9, 33, 257), 2), ((16, 16, 16), 1)):
        nz, ny, nx = shape
        for inverse in (0, 1):
            what = "transform3d %s %s vol_fused %d" % ("inverse" if inverse else "forward", "x".join(map(str, shape)), fused)
            cases.append(Case(what, "transform3d", lambda s, what=what, shape=shape: {"v": _rng(s, what).random(shape, dtype=F32)},
                              lambda dwt, P, h, inverse=inverse, nz=nz, ny=ny, nx=nx: dwt.transform3d(inverse, P["v"], nx * 4, nx * ny * 4, nx, ny, nz, 1),
                              lambda b, inverse=inverse: {"v": oracle_multilevel(orc(), b["v"], 1, bool(inverse))}, options={"vol_fused": fused}))
    for shape, fused in (((2, 2, 256), 2), ((16, 16, 16), 1)):
        nz, ny, nx = shape
        what = "transform3d_op %s vol_fused %d" % ("x".join(map(str, shape)), fused)
        cases.append(Case(what, "transform3d_op", lambda s, what=what, shape=shape: {"v": _rng(s, what).random(shape, dtype=F32), "o": np.full(shape, -5.0, F32)},
                          lambda dwt, P, h, nz=nz, ny=ny, nx=nx: dwt.transform3d_op(P["v"], P["o"], nx * 4, nx * ny * 4, nx, ny, nz, 1),
                          lambda b: {"v": b["v"], "o": oracle_multilevel(orc(), b["v"].copy(), 1, False)}, options={"vol_fused": fused}))
    return cases


_BUILDERS = {"mallat2d": _mallat2d, "mallat2d_batch": _mallat2d_batch, "oned": _oned, "eaw": _eaw, "features": _features, "bandops": _bandops,
             "nterm": _nterm, "condition": _condition, "swt": _swt, "timefreq": _timefreq, "volume": _volume}
_CASES = {}


def family_cases(family):
    """the case list of a family (built once per process; nothing here touches a device)"""
    if family not in _CASES:
        _CASES[family] = _BUILDERS[family]()
        names = [c.name for c in _CASES[family]]
        assert len(set(names)) == len(names), "case names of %s are not unique" % family
    return _CASES[family]


def pick(family, name):
    return next(c for c in family_cases(family) if c.name == name)


# the chain of part 2: consecutive calls share context scratch (frame_a: the strided 2-D call and the strided band call;
# the widened copy; the condition workspace; the SWT's intermediate planes) and alternate between two streams
def chain_cases():
    return [pick("mallat2d", "dwt_cdf97_2f_s one channel of two"), pick("bandops", "bands_apply strided frame"),
            pick("mallat2d_batch", "dwt_cdf97_2f_h pitch 130"), pick("condition", "rows_condition ops 7"),
            pick("swt", "swt2d_batch cdf97_s swt2d_fused 0"), pick("mallat2d", "dwt_cdf53_2f_i16 in place")]


# the four threads of part 3: all nine 2-D wavelets on both pitches; 1-D, SWT and features; band operators, N-term and
# conditioning; EAW, time-frequency and 3-D
THREAD_FAMILIES = (("mallat2d", "mallat2d_batch"), ("oned", "swt", "features"), ("bandops", "nterm", "condition"), ("eaw", "timefreq", "volume"))


# ---- the GPU side ------------------------------------------------------------------------------------------------------
class Harness:
    """one process, one device: torch first, then the library"""

    def __init__(self):
        import torch  # first: the library then binds to the HIP runtime torch ships

        import libdwt_amd as dwt

        self.torch, self.dwt = torch, dwt
        dwt.dwt_util_init()
        self.failures = []
        # S and T: non-blocking streams (torch creates its streams with hipStreamNonBlocking).  The runtime multiplexes its
        # streams over a few hardware queues, and two streams that share one run in turn: work on such a stream would wait
        # for S's delay like work on S itself, and no harness could tell them apart.  So S is a stream that the null stream
        # does not wait for, and T one that S does not hold up -- found by trying, once per process.
        pool = [torch.cuda.Stream() for _ in range(8)]
        self.S = pool[0]
        self.measure_ms(2_000_000)  # (the first launch loads the kernel)
        self.cycles_per_ms = 2_000_000 / max(self.measure_ms(2_000_000), 1e-3)
        null = torch.cuda.default_stream()
        free = [s for s in pool if self.runs_beside(s, null)]
        pair = next(((s, u) for s in free for u in free if u is not s and self.runs_beside(s, u)), None)  # (the first hit is enough)
        print("streams: %d of %d candidates run beside the null stream; S, T = %s" % (
            len(free), len(pool), [pool.index(x) for x in pair] if pair else None), flush=True)
        if not pair:
            raise RuntimeError("no two non-blocking streams that run beside each other and beside the null stream")
        self.S, self.T = pair

    def runs_beside(self, busy, other):
        """does an event recorded on `other` complete while `busy` is still held up by a 20 ms delay?"""
        t = self.torch
        with t.cuda.stream(busy):
            t.cuda._sleep(int(20 * self.cycles_per_ms))
        ev = t.cuda.Event()
        ev.record(other)
        stop = time.perf_counter() + 0.005
        while not ev.query() and time.perf_counter() < stop:
            pass
        ok = ev.query() and not busy.query()
        t.cuda.synchronize()
        return ok

    # -- device buffers of a case: work buffers X, the staged real input, another valid input, the copy-out
    def buffers(self, case):
        t = self.torch
        real, other, _ = case.data()
        dev = {}
        for k, v in real.items():
            if k.startswith("_"):
                continue
            dev[k] = [t.from_numpy(np.array(a)).to("cuda:0") for a in (other[k], real[k], other[k], other[k])]  # X, staged, other, out
        t.cuda.synchronize()
        return dev

    def run_once(self, case, dev, delay_cycles=0, stream=None):
        """steps 2 to 5 of a case on `stream` -> (enqueue seconds, launches, event done before the call, stream idle after
        step 5, host results).  No host synchronise inside apart from what the entry itself does."""
        t, dwt = self.torch, self.dwt
        S = stream or self.S
        real = case.data()[0]
        for k, (x, _, oth, out) in dev.items():  # canaries: another valid input; the outputs hold the family's sentinel in both
            x.copy_(oth)
            out.copy_(oth)
        t.cuda.synchronize()
        for name, value in case.options.items():
            dwt.set_option(name, value)
        try:
            if case.setup:
                case.setup(dwt, {k: v[0].data_ptr() for k, v in dev.items()})
            n0 = dwt.get_option("stat_launches")
            with t.cuda.stream(S):
                t0 = time.perf_counter()
                if delay_cycles:
                    t.cuda._sleep(int(delay_cycles))
                ev = t.cuda.Event()
                ev.record(S)
                for k, (x, staged, _, _) in dev.items():
                    x.copy_(staged, non_blocking=True)  # the true input reaches the buffer only behind the delay
                dwt.use_torch_stream()
                early = ev.query()
                ret = case.call(dwt, {k: v[0].data_ptr() for k, v in dev.items()}, real)
                for k, (x, _, _, out) in dev.items():
                    out.copy_(x, non_blocking=True)  # no host synchronise in front of it
                t1 = time.perf_counter()
                idle = S.query()
            launches = dwt.get_option("stat_launches") - n0
        finally:
            if case.teardown:
                case.teardown(dwt)
            for name in case.options:
                dwt.set_option(name, DEFAULT_OPTIONS[name])
        return t1 - t0, launches, early, idle, ret

    def collect(self, dev):
        return {k: v[3].cpu().numpy() for k, v in dev.items()}

    def fail(self, case, what):
        self.failures.append("%s: %s" % (case.name, what))
        print("  FAIL %s: %s" % (case.name, what), flush=True)

    def compare(self, case, dev, ret, how):
        bad = case.mismatches(self.collect(dev), ret)
        if bad:
            self.fail(case, "%s: differs from the model in %s" % (how, ", ".join(bad)))
        return not bad

    # -- the delay
    def measure_ms(self, cycles):
        t = self.torch
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        with t.cuda.stream(self.S):
            a.record(self.S)
            t.cuda._sleep(int(cycles))
            b.record(self.S)
        self.S.synchronize()
        return a.elapsed_time(b)

    def calibrate(self, D_ms):
        """the cycle count of a D ms delay: a probe count timed with two events, scaled, measured again"""
        probe = 2_000_000
        ms = max(self.measure_ms(probe), 1e-3)
        cycles = int(probe * D_ms / ms)
        got = self.measure_ms(cycles)
        print("delay: D = %.1f ms, %d cycles (probe: %d cycles in %.3f ms), measured again %.1f ms" % (D_ms, cycles, probe, ms, got), flush=True)
        assert 0.8 * D_ms <= got <= 4 * D_ms, "the delay took %.1f ms, wanted %.1f .. %.1f" % (got, 0.8 * D_ms, 4 * D_ms)
        return cycles

    # -- part 1
    def run_family(self, family, D_override=None):
        t = self.torch
        cases = family_cases(family)
        warm = {}
        longest = 0.0
        for case in cases:  # the warm-up pass, on the idle stream: every workspace grows here (`grow` synchronises the stream)
            dev = self.buffers(case)
            self.run_once(case, dev)
            self.S.synchronize()
            secs, launches, _, _, ret = self.run_once(case, dev)
            self.S.synchronize()
            self.compare(case, dev, ret, "idle stream")
            warm[case.name] = (dev, launches)
            longest = max(longest, secs)
        D = D_FLOOR_MS if D_override is None else D_override
        if D_override is None:
            D = max(D_FLOOR_MS, 4 * longest * 1e3)
        print("%s: %d cases, longest enqueue on the idle stream %.3f ms" % (family, len(cases), longest * 1e3), flush=True)
        cycles = self.calibrate(D) if D > 0 else 0
        for case in cases:
            dev, launches_warm = warm[case.name]
            secs, launches, early, idle, ret = self.run_once(case, dev, cycles)
            self.S.synchronize()
            print("  %-62s %-5s enqueue %7.3f ms  stream %s after the call  launches %d" % (
                case.name, "async" if case.is_async else "sync", secs * 1e3, "idle" if idle else "busy", launches), flush=True)
            self.compare(case, dev, ret, "busy stream")
            if early:
                self.fail(case, "the event in front of the input copy had completed when the call was made: the stream was not busy")
            if case.is_async and secs * 1e3 > D / 2:
                self.fail(case, "classified async, but queuing took %.1f ms of a %.1f ms delay (limit D / 2)" % (secs * 1e3, D))
            if case.is_async and idle:
                self.fail(case, "classified async, but the stream was idle right after the copy-out was queued")
            if launches != launches_warm:
                self.fail(case, "%d launches, %d in the warm-up" % (launches, launches_warm))
        t.cuda.synchronize()
        return D, cycles, longest

    # -- the negative control: the harness sees a wrong stream, with no change to the library
    def negative_control(self, cycles):
        t, dwt = self.torch, self.dwt
        case = pick("mallat2d", "dwt_cdf97_2f_s2")  # out of place: what the wrong stream computed stays readable
        real, other, want = case.data()
        dev = self.buffers(case)
        self.run_once(case, dev)
        t.cuda.synchronize()
        T = self.T
        for x, _, oth, _ in dev.values():
            x.copy_(oth)
        t.cuda.synchronize()
        dwt.set_stream(T.cuda_stream)  # before anything is queued on S
        with t.cuda.stream(self.S):
            t.cuda._sleep(int(cycles))
            dev["x"][0].copy_(dev["x"][1], non_blocking=True)  # (the input alone: the copy must not cover what T wrote to y)
        case.call(dwt, {k: v[0].data_ptr() for k, v in dev.items()}, real)  # runs on T, against the wrong image
        self.S.synchronize()
        T.synchronize()
        got = dev["y"][0].cpu().numpy()
        wrong = case._want({k: v.copy() for k, v in other.items()})["y"]
        with t.cuda.stream(self.S):
            dwt.use_torch_stream()
        ok = not same_bytes(got, want["y"]) and same_bytes(got, wrong)
        print("negative control: a call on another stream %s (equal to the expectation: %s, to the wrong image's transform: %s, untouched: %s)" % (
            "is seen" if ok else "was NOT seen", same_bytes(got, want["y"]), same_bytes(got, wrong), same_bytes(got, other["y"])), flush=True)
        if not ok:
            self.failures.append("negative control: the result of a call on the wrong stream equals the expectation, or is not the wrong image's transform")

    # -- part 2
    def run_chain(self):
        t, dwt = self.torch, self.dwt
        cases = chain_cases()
        assert all(c.is_async for c in cases)
        devs = [self.buffers(c) for c in cases]
        for c, dev in zip(cases, devs):  # warm-up
            self.run_once(c, dev)
            self.S.synchronize()
        cycles = self.calibrate(D_FLOOR_MS)
        self.negative_control(cycles)
        S = [self.T, self.S]
        for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
            for c, dev in zip(cases, devs):
                for k, (x, _, oth, out) in dev.items():
                    x.copy_(oth)
                    out.copy_(oth)
            t.cuda.synchronize()
            with t.cuda.stream(S[1]):
                t.cuda._sleep(int(cycles))  # S1 carries a delay at its head
                delay_done = t.cuda.Event()
                delay_done.record(S[1])
            rets = {}
            for pos, i in enumerate(order):
                c, dev = cases[i], devs[i]
                for name, value in c.options.items():
                    dwt.set_option(name, value)
                with t.cuda.stream(S[(pos + 1) & 1]):  # S1 first: behind the delay
                    for k, (x, staged, _, _) in dev.items():
                        x.copy_(staged, non_blocking=True)
                    dwt.use_torch_stream()
                    rets[i] = c.call(dwt, {k: v[0].data_ptr() for k, v in dev.items()}, c.data()[0])
                    for k, (x, _, _, out) in dev.items():
                        out.copy_(x, non_blocking=True)
                for name in c.options:
                    dwt.set_option(name, DEFAULT_OPTIONS[name])
            # The last call of the chain, in either direction, went to the stream WITHOUT a delay.  Its calls take
            # microseconds: left to itself that stream is through them long before the 5 ms below are over.  It may only
            # still be busy because every change of stream ordered it behind the other stream's queue, delay included.
            last_on_free = t.cuda.Event()
            last_on_free.record(S[0])
            time.sleep(0.005)
            held, pending = not last_on_free.query(), not delay_done.query()
            t.cuda.synchronize()  # the one final synchronise
            print("chain %s: 5 ms after queuing, the delay on stream 1 was %s and the stream without a delay was %s" % (
                order, "pending" if pending else "OVER", "held behind it" if held else "THROUGH its calls"), flush=True)
            if not pending:
                self.failures.append("chain %s: the delay was over 5 ms after the last call had been queued: nothing was shown" % order)
            elif not held:
                self.failures.append("chain %s: the stream without a delay finished its calls while the other stream's delay was pending: "
                                     "the change of stream did not order it behind the old stream's queue" % order)
            for i in order:
                self.compare(cases[i], devs[i], rets[i], "chain %s" % order)

    # -- part 3
    def run_threads(self):
        t, dwt = self.torch, self.dwt
        self.negative_control(self.calibrate(D_FLOOR_MS))
        for fams in THREAD_FAMILIES:  # the expectations, once, before the threads start
            for f in fams:
                for c in family_cases(f):
                    c.data()
        barrier = threading.Barrier(len(THREAD_FAMILIES))
        lock = threading.Lock()

        def work(fams):
            try:
                dwt.set_device(0)
                S = t.cuda.Stream()
                barrier.wait()
                for rep in range(3):
                    for f in fams:
                        for c in family_cases(f):
                            dev = self.buffers(c)
                            _, _, _, _, ret = self.run_once(c, dev, 0, S)
                            S.synchronize()
                            bad = c.mismatches(self.collect(dev), ret)
                            if bad:
                                with lock:
                                    self.failures.append("thread %s, round %d, %s: differs from the model in %s" % (fams, rep, c.name, ", ".join(bad)))
                dwt.dwt_util_finish()
            except Exception as e:  # noqa: BLE001
                with lock:
                    self.failures.append("thread %s: %r" % (fams, e))
                try:
                    barrier.abort()
                except Exception:  # noqa: BLE001
                    pass
        ts = [threading.Thread(target=work, args=(fams,)) for fams in THREAD_FAMILIES]
        for th in ts:
            th.start()
        for th in ts:
            th.join()
        print("threads: %d threads, 3 rounds each" % len(ts), flush=True)


def main(argv):
    run = argv[1]
    D_override = float(argv[2]) if len(argv) > 2 else None  # (D = 0 shows that the teeth are conditions: every case then fails them)
    h = Harness()
    print("device:", h.dwt.device_name(), flush=True)
    if run == "chain":
        h.run_chain()
    elif run == "threads":
        h.run_threads()
    else:
        D, cycles, longest = h.run_family(run, D_override)
        print("%s: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (run, D, cycles, longest * 1e3), flush=True)
        if cycles:
            h.negative_control(cycles)
    h.torch.cuda.synchronize()
    h.dwt.dwt_util_finish()
    if h.failures:
        print("%d FAILURES" % len(h.failures))
        for f in h.failures:
            print(" ", f)
        return 1
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
