#!/usr/bin/env python3
"""Times the row conditioning (dwt_hip_rows_condition) on one MI355X -> profiles/condition_timing.json.

Workload: 65536 rows of 4096 `spectrum` samples (tests/condition_model.py), device resident.  Per configuration the
median of --reps calls after --warmup; conditioning is not idempotent, so the batch is restored from a pristine device
copy before every call, outside the timed region (events around the call alone).  Compared with the byte floor (read +
write of the batch at 8 TB/s), the per-operation route of the same build (option "cond_fused" = 0) and the D2H + H2D
copy of the batch through pinned memory -- the route a caller takes without this feature -- and with the route the
library picks by itself (option "cond_fused" = -1).  A second, small batch shows the other end of that choice.

    python scripts/condition_timing.py [--rows 65536 2048] [--size 4096] [--reps 100] [--warmup 20] [--out F | -]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/condition_timing.py --reps 5 --warmup 1 --out -
        (a run of its own: per-kernel times -> profiles/condition_kernel_stats.csv)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import condition_model as cm  # noqa: E402
import libdwt_amd as dwt  # noqa: E402


def timed(fn, restore, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def rows_per_workgroup(n):
    """cond_rows_per_group of dwt_condition.hip: the rows whose LDS lines fit into 152 KiB, 64 at the most"""
    return min(64, 152 * 1024 // (4 * (((n + 3) & ~3) + 4)))


def measure(rows, n, reps, warmup):
    base = cm.make_input(1, "spectrum", 256, n)  # 256 distinct rows, repeated with a roll that depends on the block
    host = np.empty((rows, n), np.float32)
    for y in range(0, rows, 256):
        host[y:y + 256] = np.roll(base, (y // 256) * 7 % n, axis=1)[:min(256, rows - y)]
    pristine = torch.from_numpy(host).cuda()
    work = torch.empty_like(pristine)
    info = torch.zeros((rows, 4), dtype=torch.int32, device="cuda")
    nbytes = host.nbytes
    res = {"rows": rows, "size": n, "batch_bytes": nbytes, "byte_floor_ms": 2 * nbytes / 8e12 * 1e3,
           "rows_per_workgroup": rows_per_workgroup(n), "default_route_fused": None, "configs": {}}

    def restore():
        work.copy_(pristine)

    for name, ops in (("med_shift", 1), ("med_shift+center20", 3), ("med_shift+center20+scale", 7)):
        def call():
            dwt.rows_condition(ops, work, 4 * n, 4, rows, n, 20, 0.0, 1.0, info)

        out = {}
        for route, opt in (("fused", 1), ("per_operation", 0), ("default", -1)):
            dwt.set_option("cond_fused", opt)
            out[route] = timed(call, restore, reps, warmup)
        out["fused_over_floor"] = out["fused"]["median_ms"] / res["byte_floor_ms"]
        out["per_operation_over_fused"] = out["per_operation"]["median_ms"] / out["fused"]["median_ms"]
        res["configs"][name] = out
        if ops == 3:
            moves = info[:, 1].cpu().numpy()
            res["moves_per_row"] = {str(k): int(v) for k, v in zip(*np.unique(moves, return_counts=True))}
        print(rows, name, {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in out.items()}, flush=True)
    pinned = torch.empty((rows, n), dtype=torch.float32).pin_memory()
    res["pcie_round_trip"] = timed(lambda: (pinned.copy_(work, non_blocking=True), work.copy_(pinned, non_blocking=True)), lambda: None, reps, warmup)
    print(rows, "pcie", res["pcie_round_trip"]["median_ms"], flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 2048])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "condition_timing.json"))
    args = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    res = {"device": dwt.device_name(), "method": "HIP events around each call; median of %d calls after %d warm-ups; the batch is restored "
           "from a pristine device copy before every call, outside the timed region" % (args.reps, args.warmup),
           "batches": [measure(r, args.size, args.reps, args.warmup) for r in args.rows]}
    dwt.set_option("cond_fused", -1)
    if args.out != "-":
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
