"""The windowed inverse on a busy caller's stream, run as a process of its own by tests/test_hip_window.py: the cases below
go through the harness of tests/stream_cases.py -- a warm-up on the idle stream, then once on a non-blocking stream behind a
bounded delay, the true input reaching its buffer only behind that delay.  The result must be the model's bits
(tests/window_model.py), the entry must have queued its work without waiting for the stream, and the launch count must be
that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import stream_cases as sc
import window_model as wm

KINDS = {"inverse_window_batch": sc.ASYNC}
B, H, W, J = 2, 67, 131, 3
# (wavelet, discard, window): across the tile seam at full resolution; a border window of LL(1)
WINDOWS = [("cdf97_s", 0, (60, 5, 12, 9)), ("cdf53_i16", 1, (50, 20, 16, 14)), ("cdf53_i", 3, (2, 1, 9, 5))]
_ORACLE = []


def oracle():
    if not _ORACLE:
        from oraclelib import Oracle

        _ORACLE.append(Oracle())
    return _ORACLE[0]


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def cases():
    from libdwt_amd import window

    out = []
    for route in (2, 0):
        for wv, r, (x0, y0, ww, wh) in WINDOWS:
            dt = np.dtype(wm.DTYPE[wv])
            es = dt.itemsize
            sentinel = np.array([-77], np.int16).astype(dt)[0]

            def make(seed, wv=wv, dt=dt, ww=ww, wh=wh, sentinel=sentinel):
                return {"x": np.stack([wm.make_frame(wv, 9800 + 5 * seed + b, H, W) for b in range(B)]), "y": np.full((B, wh, ww), sentinel, dt)}

            def want(b, wv=wv, r=r, win=(x0, y0, ww, wh)):
                b["y"][:] = np.stack([wm.expected(oracle(), wv, f, J, r, *win) for f in b["x"]])
                return b

            out.append(Case("inverse_window_batch %s discard %d window_fused %d" % (wv, r, route), "inverse_window_batch", make,
                            lambda dwt, P, h, wv=wv, r=r, win=(x0, y0, ww, wh), es=es: window.inverse_window_batch(
                                wv, P["x"], es * W * H, B, es * W, W, H, J, r, *win, P["y"], es * win[2] * win[3], es * win[2]),
                            want, sc.same_floats, options={"window_fused": route}))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # The harness is driven through two names of tests/stream_cases.py that are not part of its interface, as
    # tests/quant_stream.py drives it: family_cases() serves a family from the cache _CASES, and Harness.run_once restores a
    # case's options from DEFAULT_OPTIONS.  Both are set here for this process alone; if either is renamed there, the
    # assertions below say so.
    assert isinstance(getattr(sc, "_CASES", None), dict) and isinstance(getattr(sc, "DEFAULT_OPTIONS", None), dict), "stream_cases.py changed"
    sc.DEFAULT_OPTIONS = dict(sc.DEFAULT_OPTIONS, window_fused=1)
    sc._CASES["window"] = cases()
    assert sc.family_cases("window") is sc._CASES["window"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("window")
    print("window: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
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
    sys.exit(main())
