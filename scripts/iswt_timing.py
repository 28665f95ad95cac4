"""Timing of the inverse stationary wavelet transforms (dwt_hip_iswt1d_batch, dwt_hip_iswt2d_batch) on
device-resident batches: 65536 rows of 4096 samples at 10 levels, one 8192 x 8192 image at 5 levels and 16 images of
4096 x 4096 at 4 levels, float 9/7 and 5/3, every plane kept.  One process; the median over --reps timed calls after
--warmup, device events around each call, the buffers rotated over --rotate sets so that no call finds its planes in the
Infinity Cache because the call before it left them there.  Next to each figure:

* (a) the byte floor of the mode over 8 TB/s: rows 4 * (levels + 2) bytes a sample; images 20 bytes a sample and level;
* (b) the generic route of the same build (options swt_fused / swt2d_fused = 0);
* (c) the forward call of the same shape under the symmetric border, alternated with the inverse call by call.

--parent-lib PATH (optional): a build of the parent commit's libdwt_hip.so.  The replicate forward of this build is then
alternated call by call against the parent's, and the parent against a second copy of itself (--parent-lib-copy PATH, the
same file under another name): the border template must cost the replicate forward nothing, that is, stay within the
spread that parent-against-parent shows in the same run.  Both are recorded.

Every GPU step runs under its own time limit: the process ends if a step overruns it.

    python scripts/iswt_timing.py [--reps 100] [--warmup 10] [--rotate 3] [--step-limit 150] [--out profiles/iswt_timing.json]"""
import argparse
import contextlib
import ctypes as C
import json
import os
import signal
import sys

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdwt_amd as dwt  # noqa: E402
from libdwt_amd import stationary as st  # noqa: E402

PEAK = 8e12
ROWS = (65536, 4096, 10)  # lines, samples, levels
IMAGES = [(1, 8192, 8192, 5), (16, 4096, 4096, 4)]  # batch, size_y, size_x, levels
WAVELETS = ("cdf97_s", "cdf53_s")


@contextlib.contextmanager
def step_limit(seconds, what):
    """the default action of SIGALRM ends the process: a step that hangs does not keep the device"""
    print("step:", what, "(limit %d s)" % seconds, flush=True)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def timed(calls, reps, warmup):
    """calls: one callable per series, each taking the repetition index; the series alternate call by call -> medians (ms)"""
    for i in range(warmup):
        for f in calls:
            f(i)
    torch.cuda.synchronize()
    ms = [[] for _ in calls]
    for i in range(reps):
        for k, f in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f(i)
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [float(np.median(m)) for m in ms]


def foreign(path):
    """another build of the library, loaded beside this one: its replicate forward entries on this process's device"""
    lib = C.CDLL(path)
    _I, _P, _S = C.c_int, C.c_void_p, C.c_size_t
    lib.dwt_hip_swt1d_batch.argtypes = [_I, _P, _S, _S, _I, _I, _I, _P, _P, _I, _S, _S]
    lib.dwt_hip_swt2d_batch.argtypes = [_I, _P, _S, _I, _I, _I, _I, _I, _I, _P, _P, _I, _S, _S, _I]
    assert lib.dwt_hip_init() == 0
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=150)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-lib-copy", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iswt_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    parents = [foreign(p) for p in (a.parent_lib, a.parent_lib_copy) if p]
    R = a.rotate
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "rotating_buffer_sets": R, "peak_bytes_per_s": PEAK,
           "iswt2d_fused_levels": st.ISWT2D_FUSED_LEVELS, "rows": {}, "images": []}

    def series(name, fused_opt, inverse, forward, replicate, floor_bytes, parent_calls):
        out = {"floor_bytes": floor_bytes, "floor_ms": floor_bytes / PEAK * 1e3}
        with step_limit(a.step_limit, name + " inverse and forward, alternated"):
            out["inverse_ms"], out["forward_symmetric_ms"] = timed([inverse, forward], a.reps, a.warmup)
        dwt.set_option(fused_opt, 0)
        try:
            with step_limit(a.step_limit, name + " generic route"):
                out["inverse_generic_route_ms"] = timed([inverse], max(a.reps // 4, 5), 2)[0]
        finally:
            dwt.set_option(fused_opt, 1)
        out["floor_share"] = out["floor_ms"] / out["inverse_ms"]
        out["speedup_over_generic_route"] = out["inverse_generic_route_ms"] / out["inverse_ms"]
        out["inverse_over_forward"] = out["inverse_ms"] / out["forward_symmetric_ms"]
        if parent_calls:
            with step_limit(a.step_limit, name + " replicate forward against the parent build"):
                t = timed([replicate] + parent_calls, a.reps, a.warmup)
            out["replicate_forward_ms"], out["parent_replicate_forward_ms"] = t[0], t[1]
            if len(t) > 2:
                out["parent_copy_replicate_forward_ms"] = t[2]
                out["parent_against_parent_spread"] = abs(t[1] - t[2]) / min(t[1], t[2])
            out["this_build_over_parent"] = t[0] / t[1]
        print(name, out, flush=True)
        return out

    lines, n, levels = ROWS
    with step_limit(a.step_limit, "allocate %d rows of %d, %d levels" % ROWS):
        x = [torch.randn((lines, n), dtype=torch.float32, device="cuda") for _ in range(R)]
        h = [torch.empty((levels, lines, n), dtype=torch.float32, device="cuda") for _ in range(R)]
        l = [torch.empty((lines, n), dtype=torch.float32, device="cuda") for _ in range(R)]
        y = [torch.empty((lines, n), dtype=torch.float32, device="cuda") for _ in range(R)]
        torch.cuda.synchronize()
    plane = 4 * lines * n
    for wv in WAVELETS:
        wid = dwt.WAVELET_ID[wv]
        fwd = lambda i, b=st.BORDER_SYMMETRIC: st.swt1d_batch(wv, x[i % R], 4 * n, 4, lines, n, levels, h[i % R], l[i % R], 1, plane, 4 * n, border=b)  # noqa: E731
        for i in range(R):
            fwd(i)
        inv = lambda i: st.iswt1d_batch(wv, st.BORDER_SYMMETRIC, h[i % R], l[i % R], plane, 4 * n, lines, n, levels, y[i % R], 4 * n)  # noqa: E731
        pc = [lambda i, p=p: p.dwt_hip_swt1d_batch(wid, x[i % R].data_ptr(), 4 * n, 4, lines, n, levels, h[i % R].data_ptr(), l[i % R].data_ptr(), 1, plane, 4 * n)
              for p in parents]
        res["rows"][wv] = dict(series("rows %s" % wv, "swt_fused", inv, fwd, lambda i: fwd(i, st.BORDER_REPLICATE), (levels + 2) * plane, pc),
                               lines=lines, size=n, levels=levels)
    del x, h, l, y
    torch.cuda.empty_cache()

    for batch, hh, ww, levels in IMAGES:
        with step_limit(a.step_limit, "allocate %d x %d x %d, %d levels" % (batch, hh, ww, levels)):
            x = [torch.randn((batch, hh, ww), dtype=torch.float32, device="cuda") for _ in range(R)]
            d = [torch.empty((batch, 3 * levels + 1, hh, ww), dtype=torch.float32, device="cuda") for _ in range(R)]  # the last LL behind the details
            y = [torch.empty((batch, hh, ww), dtype=torch.float32, device="cuda") for _ in range(R)]
            torch.cuda.synchronize()
        plane = 4 * hh * ww
        per = (3 * levels + 1) * plane
        entry = {"batch": batch, "size_y": hh, "size_x": ww, "levels": levels, "wavelets": {}}
        for wv in WAVELETS:
            wid = dwt.WAVELET_ID[wv]
            ll = [t.data_ptr() + 3 * levels * plane for t in d]
            fwd = lambda i, b=st.BORDER_SYMMETRIC: st.swt2d_batch(wv, x[i % R], plane, batch, 4 * ww, 4, ww, hh, levels, d[i % R], ll[i % R], 1, per, plane, 4 * ww, border=b)  # noqa: E731
            for i in range(R):
                fwd(i)
            inv = lambda i: st.iswt2d_batch(wv, st.BORDER_SYMMETRIC, d[i % R], ll[i % R], per, plane, 4 * ww, batch, ww, hh, levels, y[i % R], plane, 4 * ww)  # noqa: E731
            pc = [lambda i, p=p: p.dwt_hip_swt2d_batch(wid, x[i % R].data_ptr(), plane, batch, 4 * ww, 4, ww, hh, levels, d[i % R].data_ptr(), ll[i % R], 1, per, plane, 4 * ww)
                  for p in parents]
            entry["wavelets"][wv] = series("images %d x %d x %d %s" % (batch, hh, ww, wv), "swt2d_fused", inv, fwd, lambda i: fwd(i, st.BORDER_REPLICATE),
                                           5 * levels * batch * plane, pc)
        res["images"].append(entry)
        del x, d, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
