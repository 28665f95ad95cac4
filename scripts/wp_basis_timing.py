"""Timing of the best-basis search and of the pruned packet trees (dwt_hip_wp_best1d_batch, dwt_hip_wp_tree1d_batch;
DESIGN.md s28) on device-resident rows: 65536 rows of 4096 samples, float CDF 9/7, Shannon cost, 6 and 10 levels, out of place.

Per depth, ALTERNATELY call by call on buffers that rotate over --sets source / destination pairs, device events around
each call, median and minimum over --reps rounds after --warmup:

* `search`        the one-launch search with dst (costs, trees, totals and the rows in their trees);
* `search_no_dst` the search with dst == NULL (costs and trees only: 4 B a sample of global traffic);
* `tree`          dwt_hip_wp_tree1d_batch in the trees the search found;
* `wp1d`          dwt_hip_wp1d_batch of the same depth from the same build -- the yardstick: the search lifts twice and adds
                  the costs, so about 2 - 2.5 x is the expectation to confirm or refute.

The cross-check route (option "wp_fused" = 0: the full tree level by level twice, a cost kernel behind every level) is
timed on its own over --cross-reps calls: it takes hundreds of launches a call.  Also recorded: the pinned D2H copy of the
batch, which a caller without these entries pays per level to get the same answer on the host.

Every GPU step runs under its own time limit: the process ends if a step overruns it.

    python scripts/wp_basis_timing.py [--reps 100] [--warmup 10] [--sets 3] [--cross-reps 3] [--step-limit 300]
                                      [--out profiles/wp_basis_timing.json]"""
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

STREAM = 6.29e12  # the measured streaming ceiling
N_LINES, N = 65536, 4096
DEPTHS = (6, 10)


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
    """calls: {name: f(round)}; one call of each per round -> {name: {"ms_min", "ms_median"}}"""
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
    return {k: {"ms_min": float(np.min(v)), "ms_median": float(np.median(v))} for k, v in ms.items()}


def count(f):
    n0 = dwt.get_option("stat_launches")
    f(0)
    return dwt.get_option("stat_launches") - n0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--cross-reps", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wp_basis_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    W, cost = dwt.CDF97_S, packets.COST_SHANNON
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "buffer_sets": a.sets, "cross_reps": a.cross_reps,
           "wavelet": "cdf97_s", "cost": "shannon", "n_lines": N_LINES, "N": N, "streaming_bytes_per_s": STREAM, "depths": []}
    with step_limit(a.step_limit, "allocate %d x %d" % (N_LINES, N)):
        xs = [torch.randn((N_LINES, N), dtype=torch.float32, device="cuda") for _ in range(a.sets)]
        ys = [torch.empty_like(x) for x in xs]
        trees = torch.zeros((N_LINES, packets.TREE_WORDS), dtype=torch.int32, device="cuda")
        totals = torch.zeros(N_LINES, dtype=torch.float64, device="cuda")
        pinned = torch.empty((N_LINES, N), dtype=torch.float32).pin_memory()
        torch.cuda.synchronize()
    with step_limit(a.step_limit, "pinned D2H copy of the batch"):
        res["pinned_d2h"] = timed_alternately({"copy": lambda r: pinned.copy_(xs[r % a.sets], non_blocking=True)}, 10, 2)["copy"]
    for levels in DEPTHS:
        table = torch.zeros((N_LINES, 2 << levels), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def search(r, dst=True):
            packets.wp_best1d_batch(W, cost, 0.0, xs[r % a.sets], ys[r % a.sets] if dst else None, 4 * N, 4, N_LINES, N, levels, tree=trees,
                                    total=totals, node_cost=table)

        calls = {"search": search, "search_no_dst": lambda r: search(r, False),
                 "tree": lambda r: packets.wp_tree1d_batch(W, False, xs[r % a.sets], ys[r % a.sets], 4 * N, 4, N_LINES, N, levels, trees,
                                                           4 * packets.TREE_WORDS),
                 "wp1d": lambda r: packets.wp1d_batch(W, False, xs[r % a.sets], ys[r % a.sets], 4 * N, 4, N_LINES, N, levels)}
        with step_limit(a.step_limit, "%d levels, one-launch route" % levels):
            launches = {k: count(f) for k, f in calls.items()}
            t = timed_alternately(calls, a.reps, a.warmup)
        entry = {"levels": levels, "launches": launches, **t}
        entry["search_over_wp1d"] = t["search"]["ms_median"] / t["wp1d"]["ms_median"]
        entry["search_bytes"] = 12 * N_LINES * N
        entry["search_streaming_ms"] = 12 * N_LINES * N / STREAM * 1e3
        if a.cross_reps > 0:
            dwt.set_option("wp_fused", 0)
            try:
                with step_limit(a.step_limit, "%d levels, cross-check route" % levels):
                    entry["cross_check_launches"] = count(search)
                    entry["cross_check"] = timed_alternately({"search": search}, a.cross_reps, 1)["search"]
            finally:
                dwt.set_option("wp_fused", 1)
        print(json.dumps(entry), flush=True)
        res["depths"].append(entry)
        del table
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
