"""Timing of the wavelet packet transforms (dwt_hip_wp1d_batch, dwt_hip_wp2d_batch) on device-resident data, float CDF 9/7,
forward, out of place:

* 65536 rows of 4096 samples at 6 and at 12 levels;
* 64 images of 4096 x 4096 at 3 levels; one image of 8192 x 8192 at 3 levels (and the same calls at 1 and 2 levels, so
  that the cost of each level of the 2-D route is visible as a difference).

Per shape the fused route and the level-by-level route of the same build (option wp_fused = 0) are timed ALTERNATELY, one
call of each per round, on buffers that rotate over --sets source / destination pairs, device events around each call:
median and minimum over --reps rounds after --warmup.  Next to them

* the byte floor -- 8 bytes a sample per call in 1-D, 8 bytes a sample per level in 2-D -- over the measured streaming
  ceiling of 6.29 TB/s and over the 8 TB/s of the data sheet;
* the yardstick: dwt_hip_transform1d_batch / dwt_hip_transform2d_batch (the Mallat tree) of the same shape and depth,
  timed the same way.

Every GPU step runs under its own time limit: the process ends if a step overruns it.

    python scripts/wp_timing.py [--reps 100] [--warmup 10] [--sets 3] [--step-limit 300] [--out profiles/wp_timing.json]"""
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
from libdwt_amd import packets  # noqa: E402

PEAK = 8e12
STREAM = 6.29e12
LINES = [(65536, 4096, 6), (65536, 4096, 12)]          # n_lines, N, levels
IMAGES = [(64, 4096, 4096, (3,)), (1, 8192, 8192, (1, 2, 3))]  # batch, size_y, size_x, depths timed


@contextlib.contextmanager
def step_limit(seconds, what):
    """the default action of SIGALRM ends the process: a step that hangs does not keep the device"""
    print("step:", what, "(limit %d s)" % seconds, flush=True)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def timed_alternately(calls, reps, warmup):
    """calls: {name: f(set index)}; one call of each per round, buffers rotating -> {name: (min ms, median ms)}"""
    ms = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f(r)
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[k].append(a.elapsed_time(b))
    return {k: (float(np.min(v)), float(np.median(v))) for k, v in ms.items()}


def with_option(value, f):
    def g(r):
        dwt.set_option("wp_fused", value)
        try:
            f(r)
        finally:
            dwt.set_option("wp_fused", 1)
    return g


def count(f):
    n0 = dwt.get_option("stat_launches")
    f(0)
    return dwt.get_option("stat_launches") - n0


def report(name, t, floor_bytes, launches):
    out = {"floor_bytes": floor_bytes, "streaming_ms": floor_bytes / STREAM * 1e3, "peak_ms": floor_bytes / PEAK * 1e3, "launches": launches}
    for k, (mn, med) in t.items():
        out[k] = {"ms_min": mn, "ms_median": med, "share_of_streaming_floor": floor_bytes / STREAM * 1e3 / med}
    out["fused_over_level_by_level"] = t["level_by_level"][1] / t["fused"][1]
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wp_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "buffer_sets": a.sets, "peak_bytes_per_s": PEAK,
           "streaming_bytes_per_s": STREAM, "wavelet": "cdf97_s", "lines": [], "images": []}
    W = dwt.CDF97_S
    for n_lines, N, levels in LINES:
        with step_limit(a.step_limit, "allocate %d x %d" % (n_lines, N)):
            xs = [torch.randn((n_lines, N), dtype=torch.float32, device="cuda") for _ in range(a.sets)]
            ys = [torch.empty_like(x) for x in xs]
            torch.cuda.synchronize()
        wp = lambda r: packets.wp1d_batch(W, False, xs[r % a.sets], ys[r % a.sets], 4 * N, 4, n_lines, N, levels)  # noqa: E731
        calls = {"fused": wp, "level_by_level": with_option(0, wp),
                 "mallat_yardstick": lambda r: dwt.transform1d_batch(W, 0, xs[r % a.sets], ys[r % a.sets], 4 * N, n_lines, N, levels)}
        with step_limit(a.step_limit, "%d x %d, %d levels" % (n_lines, N, levels)):
            launches = {k: count(f) for k, f in calls.items()}
            t = timed_alternately(calls, a.reps, a.warmup)
        entry = report("lines %d x %d, %d levels" % (n_lines, N, levels), t, 8 * n_lines * N, launches)
        entry.update({"n_lines": n_lines, "N": N, "levels": levels})
        res["lines"].append(entry)
        del xs, ys
        torch.cuda.empty_cache()
    for batch, h, w, depths in IMAGES:
        with step_limit(a.step_limit, "allocate %d x %d x %d" % (batch, h, w)):
            xs = [torch.randn((batch, h, w), dtype=torch.float32, device="cuda") for _ in range(a.sets)]
            ys = [torch.empty_like(x) for x in xs]
            torch.cuda.synchronize()
        for levels in depths:
            wp = lambda r: packets.wp2d_batch(W, False, xs[r % a.sets], ys[r % a.sets], 4 * h * w, batch, 4 * w, 4, w, h, levels)  # noqa: E731
            calls = {"fused": wp, "level_by_level": with_option(0, wp),
                     "mallat_yardstick": lambda r: dwt.transform2d_batch(W, 0, xs[r % a.sets], ys[r % a.sets], 4 * h * w, batch, 4 * w, w, h, levels)}
            with step_limit(a.step_limit, "%d x %d x %d, %d levels" % (batch, h, w, levels)):
                launches = {k: count(f) for k, f in calls.items()}
                t = timed_alternately(calls, a.reps, a.warmup)
            entry = report("images %d x %d x %d, %d levels" % (batch, h, w, levels), t, 8 * batch * h * w * levels, launches)
            entry.update({"batch": batch, "size_y": h, "size_x": w, "levels": levels})
            res["images"].append(entry)
        del xs, ys
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
