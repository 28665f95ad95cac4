"""Timing of the N-term approximation (dwt_hip_keep_largest_batch) on device-resident coefficients: 64
frames of 4096 x 4096 with one channel, 32 groups of two channels of 4096 x 4096, one frame of 8192 x 8192, each at keep =
1 %, 10 % and 50 % of the positions.  The coefficients are a real 5-level forward CDF 9/7 of smooth-plus-noise images
(constant or all-random data would make the select's histograms unrepresentative).  The call zeroes what it reads, so
every timed call runs on a fresh device copy of the coefficients, made before the first event.  One process; median and
minimum over --reps timed calls after --warmup, device events around the call.  Next to each:

* the byte floor 4 * C * (P + 2) bytes a position over 8 TB/s (P = 3 histogram passes read, the apply pass reads and
  writes), and the same bytes over the project's measured streaming ceiling of 6.29 TB/s;
* the route that exists without this entry: the same planes copied to pinned host memory and back (D2H + H2D, timed in
  this script, the host sort between them NOT included);
* the per-launch kernel times (three histogram passes, apply), device events around each launch
  (dwt_hip_prof_enable(2)), from a run of their own.

Every GPU step (allocation, warm-up and timing of one configuration) runs under its own time limit: the process ends
if a step overruns it.

    python scripts/nterm_timing.py [--reps 100] [--warmup 10] [--step-limit 120] [--out profiles/nterm_timing.json]"""
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
PASSES = 3
SHAPES = [(64, 1, 4096, 4096), (32, 2, 4096, 4096), (1, 1, 8192, 8192)]  # groups, channels, size_y, size_x
SHARES = (0.01, 0.10, 0.50)


@contextlib.contextmanager
def step_limit(seconds, what):
    """the default action of SIGALRM ends the process: a step that hangs does not keep the device"""
    print("step:", what, "(limit %d s)" % seconds, flush=True)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def timed(f, reps, warmup, before=lambda: None):
    for _ in range(warmup):
        before()
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.min(ms)), float(np.median(ms))


def coefficients(frames, h, w):
    """frames x h x w: the 5-level forward 9/7 of smooth images with noise on them"""
    y, x = torch.meshgrid(torch.arange(h, device="cuda") / h, torch.arange(w, device="cuda") / w, indexing="ij")
    src = torch.empty((frames, h, w), dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    for b in range(frames):
        src[b] = torch.sin(6.0 * x + 0.3 * b) * torch.cos(4.0 * y - 0.2 * b) + 0.5 * x * y
        src[b] += 0.02 * torch.randn((h, w), device="cuda", generator=gen)
    dst = torch.empty_like(src)
    j = dwt.transform2d_batch("cdf97_s", 0, src, dst, 4 * h * w, frames, 4 * w, w, h, 5)
    torch.cuda.synchronize()
    del src
    return dst, j


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nterm_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "peak_bytes_per_s": PEAK, "streaming_bytes_per_s": STREAM,
           "histogram_passes": PASSES, "shapes": []}
    for groups, ch, h, w in SHAPES:
        frames, plane = groups * ch, 4 * h * w
        with step_limit(a.step_limit, "coefficients of %d x %d x %d x %d" % (groups, ch, h, w)):
            pristine, j = coefficients(frames, h, w)
            work = torch.empty_like(pristine)
            pinned = torch.empty(pristine.shape, dtype=torch.float32, pin_memory=True)
            torch.cuda.synchronize()
        M = h * w
        floor_bytes = 4 * ch * (PASSES + 2) * M * groups
        entry = {"groups": groups, "channels": ch, "size_y": h, "size_x": w, "levels": j, "floor_bytes": floor_bytes,
                 "floor_ms": floor_bytes / PEAK * 1e3, "streaming_ms": floor_bytes / STREAM * 1e3, "keep": {}}

        def round_trip():
            pinned.copy_(work, non_blocking=True)
            work.copy_(pinned, non_blocking=True)

        with step_limit(a.step_limit, "PCIe round trip"):
            work.copy_(pristine)
            mn, med = timed(round_trip, max(3, a.reps // 10), 2)
        entry["pcie_round_trip"] = {"ms_min": mn, "ms_median": med, "bytes_each_way": frames * plane}
        for share in SHARES:
            keep = int(M * share)
            call = lambda: dwt.lib.dwt_hip_keep_largest_batch(work.data_ptr(), ch * plane, groups, ch, plane, 4 * w, w, h, j, 0,  # noqa: E731
                                                              keeps.ctypes.data, None, None)
            keeps = np.full(groups, keep, np.int32)
            fresh = lambda: work.copy_(pristine)  # noqa: E731
            with step_limit(a.step_limit, "keep %d %%" % round(100 * share)):
                fresh()
                n0 = dwt.get_option("stat_launches")
                thr, kept = dwt.keep_largest_batch(work, ch * plane, groups, ch, plane, 4 * w, w, h, keep, j)
                launches = dwt.get_option("stat_launches") - n0
                mn, med = timed(call, a.reps, a.warmup, fresh)
            with step_limit(a.step_limit, "keep %d %%, per launch" % round(100 * share)):
                dwt.prof_enable(2)
                dwt.prof_read_levels(4)
                for _ in range(max(3, a.reps // 10)):
                    fresh()
                    call()
                per_launch, _ = dwt.prof_read_levels(4)
                dwt.prof_enable(0)
            out = {"keep": keep, "launches": launches, "ms_min": mn, "ms_median": med, "floor_share": entry["floor_ms"] / med,
                   "streaming_share": entry["streaming_ms"] / med, "achieved_floor_bytes_per_s": floor_bytes / (med * 1e-3),
                   "speedup_over_pcie_round_trip": entry["pcie_round_trip"]["ms_median"] / med,
                   "launch_ms": {"hist0": per_launch[0], "hist1": per_launch[1], "hist2": per_launch[2], "apply": per_launch[3]},
                   "pass_bytes": 4 * ch * M * groups, "thr_first_group": float(thr[0]), "kept_first_group": int(kept[0])}
            entry["keep"]["%d%%" % round(100 * share)] = out
            print(groups, ch, h, w, out, flush=True)
        res["shapes"].append(entry)
        del pristine, work, pinned
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
