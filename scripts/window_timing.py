"""Timing of the windowed inverse (dwt_hip_inverse_window_batch) on device-resident Mallat frames: one
8192 x 8192 frame at 5 levels -- windows of 256^2, 512^2, 2048^2 and the whole frame at discard 0, 512^2 at discard 2 -- and
16 frames of 4096 x 4096 at 5 levels with a 512^2 window, float 9/7 and int16 5/3.  One process; the median over --reps
timed calls after --warmup, device events around each call, the frames rotated over --rotate sets so that no call finds its
coefficients in the Infinity Cache because the call before it left them there.  Per case:

* route 2 (the window kernels) against route 0 of the same build (the inverse driver into scratch and a rectangle copy: what a
  caller without the entry does), alternated call by call;
* route 2 against the byte floor of dwt_hip_window_regions: the regions' bytes read, the window's bytes written, over 8 TB/s;
* the window's share of LL(discard), the figure the rule of option "window_fused" = 1 is stated in.

Every GPU step runs under its own time limit: the process ends if a step overruns it.

    python scripts/window_timing.py [--reps 100] [--warmup 10] [--rotate 3] [--step-limit 150] [--out profiles/window_timing.json]"""
import argparse
import contextlib
import json
import os
import signal
import sys

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdwt_amd as dwt  # noqa: E402
from libdwt_amd import window  # noqa: E402

PEAK = 8e12
LEVELS = 5
WAVELETS = {"cdf97_s": torch.float32, "cdf53_i16": torch.int16}
# batch, size, [(discard, window side; 0: the whole band)]
SHAPES = [(1, 8192, [(0, 256), (0, 512), (0, 2048), (0, 0), (2, 512)]), (16, 4096, [(0, 512)])]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    R = a.rotate
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "rotating_buffer_sets": R, "peak_bytes_per_s": PEAK, "levels": LEVELS,
           "cases": []}
    for batch, size, windows in SHAPES:
        for wv, dt in WAVELETS.items():
            es = window.ELEM_BYTES[dwt.WAVELET_ID[wv]]
            with step_limit(a.step_limit, "allocate %d x %d x %d %s" % (batch, size, size, wv)):
                if dt == torch.float32:
                    x = [torch.randn((batch, size, size), dtype=dt, device="cuda") for _ in range(R)]
                else:
                    x = [torch.randint(-2000, 2000, (batch, size, size), dtype=dt, device="cuda") for _ in range(R)]
                torch.cuda.synchronize()
            for discard, side in windows:
                band = -(-size // (1 << discard))
                side = side or band
                x0 = y0 = ((band - side) // 2) | 1 if side < band else 0  # an odd origin in the middle
                y = [torch.empty((batch, side, side), dtype=dt, device="cuda") for _ in range(R)]
                reg = window.window_regions(wv, size, size, LEVELS, discard, x0, y0, side, side)
                floor_bytes = batch * (window.region_bytes(wv, reg) + es * side * side)

                def call(i, route):
                    dwt.set_option("window_fused", route)
                    window.inverse_window_batch(wv, x[i % R], es * size * size, batch, es * size, size, size, LEVELS, discard, x0, y0, side, side,
                                                y[i % R], es * side * side, es * side)

                name = "%s %d x %d^2 discard %d window %d^2" % (wv, batch, size, discard, side)
                try:
                    with step_limit(a.step_limit, name):
                        t2, t0 = timed([lambda i: call(i, 2), lambda i: call(i, 0)], a.reps, a.warmup)
                finally:
                    dwt.set_option("window_fused", 1)
                out = {"wavelet": wv, "batch": batch, "size": size, "discard": discard, "window": side, "origin": x0,
                       "window_share_of_band": side * side / (band * band), "kernels_ms": t2, "inverse_and_copy_ms": t0,
                       "speedup_over_inverse_and_copy": t0 / t2, "floor_bytes": floor_bytes, "frame_bytes": batch * es * size * size,
                       "floor_ms": floor_bytes / PEAK * 1e3, "floor_share": floor_bytes / PEAK * 1e3 / t2,
                       "default_route": window.window_route(wv, batch, size, size, LEVELS, discard, x0, y0, side, side)}
                print(name, out, flush=True)
                res["cases"].append(out)
                del y
            del x
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
