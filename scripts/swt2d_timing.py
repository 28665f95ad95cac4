"""Timing of the stationary wavelet transform of image batches (dwt_hip_swt2d_batch) on device-resident images: one
8192 x 8192 image at 5 levels and 16 images of 4096 x 4096 at 4 levels, both wavelets, l_mode 0 (detail planes only) and 2
(detail and LL planes).  One process; median and minimum over --reps timed calls after --warmup, device events around the
call.  Next to each:

* the byte floor of the mode over 8 TB/s: per level one plane read and HL, LH, HH written, plus LL wherever the mode or
  the next level needs it (l_mode 0: every level but the last; l_mode 2: every level), 4 bytes a sample;
* the same bytes over the project's measured streaming ceiling of 6.29 TB/s;
* the generic route of the same build (option swt2d_fused = 0: a row pass and a column pass per level through library
  scratch), timed over the same number of calls.

Every GPU step (allocation, warm-up and timing of one configuration) runs under its own time limit: the process ends
if a step overruns it.

    python scripts/swt2d_timing.py [--reps 100] [--warmup 20] [--step-limit 120] [--out profiles/swt2d_timing.json]"""
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

PEAK = 8e12
STREAM = 6.29e12
SHAPES = [(1, 8192, 8192, 5), (16, 4096, 4096, 4)]  # batch, size_y, size_x, levels


@contextlib.contextmanager
def step_limit(seconds, what):
    """the default action of SIGALRM ends the process: a step that hangs does not keep the device"""
    print("step:", what, "(limit %d s)" % seconds, flush=True)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def timed(f, reps, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.min(ms)), float(np.median(ms))


def count(call):
    n0 = dwt.get_option("stat_launches")
    call()
    return dwt.get_option("stat_launches") - n0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swt2d_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "peak_bytes_per_s": PEAK, "streaming_bytes_per_s": STREAM,
           "fused_levels": dwt.SWT2D_FUSED_LEVELS, "tile": [dwt.SWT2D_TILE_W, dwt.SWT2D_TILE_H], "shapes": []}
    for batch, h, w, levels in SHAPES:
        with step_limit(a.step_limit, "allocate %d x %d x %d, %d levels" % (batch, h, w, levels)):
            x = torch.randn((batch, h, w), dtype=torch.float32, device="cuda")
            dh = torch.empty((batch, 3 * levels, h, w), dtype=torch.float32, device="cuda")
            # (one batch stride serves dst_h and dst_l: the LL stacks lie 3 * levels planes apart too, `levels` of them used)
            dl = torch.empty((batch, 3 * levels, h, w), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
        plane = 4 * h * w
        entry = {"batch": batch, "size_y": h, "size_x": w, "levels": levels, "wavelets": {}}
        for wv in ("cdf97_s", "cdf53_s"):
            out = {}
            for l_mode in (0, 2):
                call = lambda: dwt.swt2d_batch(wv, x, plane, batch, 4 * w, 4, w, h, levels, dh, dl, l_mode, 3 * levels * plane, plane, 4 * w)  # noqa: E731
                planes = batch * (4 * levels + (levels - 1 if l_mode == 0 else levels))
                floor_bytes = planes * plane
                with step_limit(a.step_limit, "%s l_mode %d fused" % (wv, l_mode)):
                    launches = count(call)
                    mn, med = timed(call, a.reps, a.warmup)
                dwt.set_option("swt2d_fused", 0)
                try:
                    with step_limit(a.step_limit, "%s l_mode %d generic" % (wv, l_mode)):
                        g_launches = count(call)
                        gmn, gmed = timed(call, a.reps, a.warmup)
                finally:
                    dwt.set_option("swt2d_fused", 1)
                out["l_mode_%d" % l_mode] = {
                    "launches": launches, "ms_min": mn, "ms_median": med, "floor_bytes": floor_bytes, "floor_ms": floor_bytes / PEAK * 1e3,
                    "floor_share": floor_bytes / PEAK * 1e3 / med, "streaming_ms": floor_bytes / STREAM * 1e3,
                    "streaming_share": floor_bytes / STREAM * 1e3 / med, "achieved_floor_bytes_per_s": floor_bytes / (med * 1e-3),
                    "generic_route": {"launches": g_launches, "ms_min": gmn, "ms_median": gmed}, "speedup_over_generic_route": gmed / med}
                print(batch, h, w, levels, wv, "l_mode", l_mode, out["l_mode_%d" % l_mode], flush=True)
            entry["wavelets"][wv] = out
        res["shapes"].append(entry)
        del x, dh, dl
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
