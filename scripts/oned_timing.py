"""Timing of the 1-D transforms: the fused all-levels kernel against the per-level line passes (option "generic"),
alternated in one process on a seeded input, device events after a warm-up.  One JSON line per case and path.

    python scripts/oned_timing.py [--reps 20] [--out profiles/oned_timing.json]

Cases: (a) 65536 x 4096 rows, (b) 262144 x 256 rows, (c) one 2^24-sample signal -- device resident, forward and
inverse at full depth -- and (d) one 4096-sample host-memory signal (mostly latency; host wall clock, the call is
synchronous).  Share of peak: 8 B of HBM traffic per sample (read once, written once) against 8 TB/s."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libdwt_amd as dwt  # noqa: E402

PEAK = 8e12


def device_case(name, n_lines, n, reps):
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.random((n_lines, n), dtype=np.float32)).cuda()
    y = torch.empty_like(x)
    dwt.use_torch_stream()
    out = []
    for inverse in (0, 1):
        times = {0: [], 1: []}
        for generic in (0, 1, 0, 1):  # warm-up round first, then measured rounds alternate
            dwt.set_option("generic", generic)
            dwt.transform1d_batch("cdf97_s", inverse, x, y, n * 4, n_lines, n)
        for _ in range(reps):
            for generic in (0, 1):
                dwt.set_option("generic", generic)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                dwt.transform1d_batch("cdf97_s", inverse, x, y, n * 4, n_lines, n)
                b.record()
                b.synchronize()
                times[generic].append(a.elapsed_time(b) * 1e3)
        dwt.set_option("generic", 0)
        for generic in (0, 1):
            us = float(np.median(times[generic]))
            samples = n_lines * n
            out.append({"case": name, "lines": n_lines, "n": n, "levels": int(np.ceil(np.log2(n))),
                        "dir": "inverse" if inverse else "forward", "path": "generic" if generic else "fused",
                        "us": round(us, 2), "us_min": round(float(np.min(times[generic])), 2),
                        "gsamples_s": round(samples / us / 1e3, 2), "peak_share": round(samples * 8 / (us * 1e-6) / PEAK, 4)})
    del x, y
    torch.cuda.empty_cache()
    return out


def host_case(reps):
    rng = np.random.default_rng(2)
    a = rng.random(4096, dtype=np.float32)
    out = []
    for inverse in (0, 1):
        times = {0: [], 1: []}
        for _ in range(reps + 2):
            for generic in (0, 1):
                dwt.set_option("generic", generic)
                b = a.copy()
                t0 = time.perf_counter()
                (dwt.dwt_cdf97_1i_s if inverse else dwt.dwt_cdf97_1f_s)(b, 4, 4096, 4096)
                times[generic].append((time.perf_counter() - t0) * 1e6)
        dwt.set_option("generic", 0)
        for generic in (0, 1):
            us = float(np.median(times[generic][2:]))
            out.append({"case": "d_host_4096", "lines": 1, "n": 4096, "levels": 12, "dir": "inverse" if inverse else "forward",
                        "path": "generic" if generic else "fused", "us": round(us, 2), "clock": "host",
                        "gsamples_s": round(4096 / us / 1e3, 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="abcd")
    args = ap.parse_args()
    dwt.dwt_util_init()
    rows = []
    cases = {"a": ("a_65536x4096", 65536, 4096), "b": ("b_262144x256", 262144, 256), "c": ("c_1x2^24", 1, 1 << 24)}
    for k in args.cases:
        res = host_case(args.reps) if k == "d" else device_case(*cases[k], args.reps)
        for r in res:
            print(json.dumps(r), flush=True)
        rows += res
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": dwt.device_name(), "reps": args.reps, "results": rows}, f, indent=1)


if __name__ == "__main__":
    main()
