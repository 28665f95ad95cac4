"""Timing of the stationary wavelet transform of row batches (dwt_hip_swt1d_batch / dwt_hip_swt_features1d_batch) on
device-resident rows: 65536 rows of 4096 samples, 10 levels, both wavelets.  Coefficient mode with l_mode 0 (H planes
only) and 2 (H and L planes); feature mode over the H planes with WPS alone, every sum-type feature, and every feature
with the median.  Median and minimum over --reps timed calls after --warmup, one process, device events around the call
(a feature call ends synchronised: the raw records cross to the host and the finished matrix returns).  Next to each:

* its byte floor over 8 TB/s -- per row 4N bytes in and 4*J*N (l_mode 0) or 8*J*N (l_mode 2) out for coefficients, 4N in
  for features;
* the level-by-level route of the same build (option swt_fused = 0: one k_swt_level launch per level through global
  memory; for features the planes go to library scratch and are reduced there), the only other device route, timed over
  fewer calls (--reps / 10, at least 10).

    python scripts/swt_timing.py [--reps 100] [--warmup 20] [--rows 65536] [--out profiles/swt_timing.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdwt_amd as dwt  # noqa: E402

PEAK = 8e12
SUMS = ["wps", "mean", "var", "stdev", "skew", "kurt", "maxnorm", "maxidx", "lpnorm", "norm"]
MASKS = [("wps", ["wps"]), ("sums", SUMS), ("all", SUMS + ["med"])]


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


def both_routes(call, floor_bytes, reps, warmup):
    n0 = dwt.get_option("stat_launches")
    call()
    launches = dwt.get_option("stat_launches") - n0
    mn, med = timed(call, reps, warmup)
    dwt.set_option("swt_fused", 0)
    try:
        n0 = dwt.get_option("stat_launches")
        call()
        level_launches = dwt.get_option("stat_launches") - n0
        lmn, lmed = timed(call, max(10, reps // 10), 2)
    finally:
        dwt.set_option("swt_fused", 1)
    floor_ms = floor_bytes / PEAK * 1e3
    return {"launches": launches, "ms_min": mn, "ms_median": med, "floor_bytes": floor_bytes, "floor_ms": floor_ms,
            "floor_share": floor_ms / med, "level_route": {"launches": level_launches, "ms_min": lmn, "ms_median": lmed},
            "speedup_over_level_route": lmed / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--levels", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swt_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    rows, n, J = a.rows, a.n, a.levels
    x = torch.randn((rows, n), dtype=torch.float32, device="cuda")
    h = torch.empty((J, rows, n), dtype=torch.float32, device="cuda")
    lo = torch.empty((J, rows, n), dtype=torch.float32, device="cuda")
    fv = torch.empty((rows, 11 * J), dtype=torch.float32, device="cuda")
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "peak_bytes_per_s": PEAK, "rows": rows, "n": n, "levels": J,
           "p": 1.5, "wavelets": {}}
    for w in ("cdf97_s", "cdf53_s"):
        out = {}
        for l_mode in (0, 2):
            call = lambda: dwt.swt1d_batch(w, x, n * 4, 4, rows, n, J, h, lo, l_mode, rows * n * 4, n * 4)  # noqa: E731
            out["coefficients_l_mode_%d" % l_mode] = both_routes(call, rows * (4 * n + (4 if l_mode == 0 else 8) * J * n), a.reps, a.warmup)
            print(w, "coefficients l_mode", l_mode, out["coefficients_l_mode_%d" % l_mode], flush=True)
        for mname, feats in MASKS:
            call = lambda: dwt.swt_features1d_batch(w, feats, x, n * 4, 4, rows, n, J, fv, 11 * J, 0, 1.5)  # noqa: E731
            out["features_" + mname] = dict(both_routes(call, rows * 4 * n, a.reps, a.warmup), features=feats)
            print(w, "features", mname, out["features_" + mname], flush=True)
        res["wavelets"][w] = out
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
