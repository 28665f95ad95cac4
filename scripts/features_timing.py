"""Timing of the per-subband feature statistics (dwt_hip_features1d_batch / dwt_hip_features2d_batch) on device-resident
coefficients: 65536 rows of 4096 samples at 12 levels (one k_feat_lines launch), 64 images of 4096^2 and one of 8192^2 at
5 levels (the slab passes).  Per workload three masks -- WPS alone, every sum-type feature, every feature with the
median -- min and median over --reps timed calls after --warmup, device events around the call (the call itself ends
synchronised: the raw records cross to the host and the finished vector returns).  The yardsticks come from the same
run: the byte floor, the bytes each pass must read (rows: the line once; images: the detail bands once per pass --
pass 1, pass 2 for central moments, four select passes for the median) over 8 TB/s; and the route a user has without
these entries, the device-to-host copy of the same coefficients into pinned memory (the CPU statistics they would
still have to run afterwards are not in it).  --kernel-stats DIR merges the per-kernel times of a separate
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/features_timing.py --reps 3 --warmup 1
--out /dev/null` run into the JSON.

    python scripts/features_timing.py [--reps 100] [--warmup 20] [--out profiles/features_timing.json]"""
import argparse
import csv
import glob
import json
import os
import re
import sys

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import libdwt_amd as dwt  # noqa: E402
from features_model import bands  # noqa: E402

PEAK = 8e12
SUMS = ["wps", "mean", "var", "stdev", "skew", "kurt", "maxnorm", "maxidx", "lpnorm", "norm"]
MASKS = [("wps", ["wps"], 1), ("sums", SUMS, 2), ("all", SUMS + ["med"], 6)]  # name, features, passes over the bands


def timed(f, reps, warmup):
    for _ in range(warmup):
        f()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.min(ms)), float(np.median(ms))


def workload(name, batch, w, h, levels, reps, warmup):
    x = torch.randn((batch, h, w), dtype=torch.float32, device="cuda")
    j_max = levels + 1
    bs = bands(w, h, w, h, j_max)
    nb = len(bs)
    band_bytes = 4 * batch * sum(b[2] * b[3] for b in bs)
    fv = torch.empty((batch, 11 * nb), dtype=torch.float32, device="cuda")
    host = torch.empty((batch, h, w), dtype=torch.float32).pin_memory()
    d2h = timed(lambda: (host.copy_(x, non_blocking=True), torch.cuda.synchronize()), max(5, reps // 10), 2)
    out = {"shape": [batch, h, w], "levels": levels, "bands": nb, "coefficient_bytes": x.numel() * 4, "band_bytes": band_bytes,
           "d2h_copy_ms": {"min": d2h[0], "median": d2h[1]}, "masks": {}}
    for mname, feats, passes in MASKS:
        if h == 1:
            call = lambda: dwt.features1d_batch(feats, x, w * 4, 4, batch, w, j_max, fv, 11 * nb, 1.5)  # noqa: E731
            floor_bytes = x.numel() * 4  # the line is read once, whatever the mask
        else:
            call = lambda: dwt.features2d_batch(feats, x, h * w * 4, batch, w * 4, w, h, j_max, fv, 11 * nb, 1.5)  # noqa: E731
            floor_bytes = band_bytes * passes
        n0 = dwt.get_option("stat_launches")
        call()
        launches = dwt.get_option("stat_launches") - n0
        mn, med = timed(call, reps, warmup)
        floor_ms = floor_bytes / PEAK * 1e3
        out["masks"][mname] = {"features": feats, "launches": launches, "ms_min": mn, "ms_median": med, "floor_bytes": floor_bytes,
                               "floor_ms": floor_ms, "floor_share": floor_ms / med, "ratio_to_d2h_copy": med / d2h[1]}
        print(name, mname, out["masks"][mname], flush=True)
    return out


def kernel_stats(d):
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_feat_\w+(<[^>]*>)?", r.get("Name", ""))
            if m:
                rows[m.group(0)] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "total_ms": float(r["TotalDurationNs"]) / 1e6}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_timing.json"))
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:  # merge only
        res = json.load(open(a.out))
        res["rocprofv3_kernel_stats"] = {"how": "separate run under rocprofv3 --kernel-trace --stats, --reps 3 --warmup 1, all workloads and masks",
                                         "kernels": kernel_stats(a.kernel_stats)}
        json.dump(res, open(a.out, "w"), indent=1)
        return
    dwt.dwt_util_init()
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "peak_bytes_per_s": PEAK, "p": 1.5, "workloads": {}}
    for name, batch, w, h, levels in (("rows_65536x4096", 65536, 4096, 1, 12), ("images_64x4096^2", 64, 4096, 4096, 5),
                                      ("image_1x8192^2", 1, 8192, 8192, 5)):
        res["workloads"][name] = workload(name, batch, w, h, levels, a.reps, a.warmup)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
