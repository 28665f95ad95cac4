"""Timing of the best-basis search over packet quadtrees and of the pruned 2-D packet trees (dwt_hip_wp_best2d_batch,
dwt_hip_wp_tree2d_batch) on device-resident images, float CDF 9/7, Shannon cost, out of place:
64 images of 4096 x 4096 at 3 levels and one image of 8192 x 8192 at 5 levels.

Per shape, ALTERNATELY call by call on buffers that rotate over --sets source / destination pairs, device events around
each call, median and minimum over --reps rounds after --warmup:

* `search`        the search with dst (costs, trees, totals and the images in their trees): 3 * levels + 2 launches;
* `search_no_dst` the search with dst == NULL (costs and trees only): 2 * levels + 2 launches;
* `tree`          dwt_hip_wp_tree2d_batch in the trees the search found;
* `wp2d`          dwt_hip_wp2d_batch of the same depth from the same build -- the yardstick.

Each call is reported as a multiple of `wp2d` and of its own byte floor over the measured streaming ceiling: a level
kernel moves 8 B a sample, a cost kernel reads 4 B a sample, so the search with dst has 4 (levels + 1) + 16 levels bytes a
sample, without dst 4 (levels + 1) + 8 levels, `tree` and `wp2d` 8 levels.  No target ratio is set.

The cross-check route (option "wp_fused" = 0: the staged frame level by level through the line passes, one thread per
node in the cost kernel) is timed on its own over --cross-reps calls.  Also recorded: the pinned D2H copy of the batch,
which a caller without these entries pays per level to get the same answer on the host.

Every GPU step runs under its own time limit: the process ends if a step overruns it.

    python scripts/wp_basis2d_timing.py [--reps 100] [--warmup 10] [--sets 3] [--cross-reps 1] [--step-limit 300]
                                        [--out profiles/wp_basis2d_timing.json]"""
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
SHAPES = ((64, 4096, 4096, 3), (1, 8192, 8192, 5))  # batch, rows, columns, levels


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
    ap.add_argument("--cross-reps", type=int, default=1)
    ap.add_argument("--step-limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wp_basis2d_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    W, cost = dwt.CDF97_S, packets.COST_SHANNON
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "buffer_sets": a.sets, "cross_reps": a.cross_reps,
           "wavelet": "cdf97_s", "cost": "shannon", "streaming_bytes_per_s": STREAM, "shapes": []}
    for batch, size_y, size_x, levels in SHAPES:
        samples = batch * size_y * size_x
        geom = (4 * size_x * size_y, batch, 4 * size_x, 4, size_x, size_y, levels)
        with step_limit(a.step_limit, "allocate %d x %d x %d" % (batch, size_y, size_x)):
            # (|c| < 1, where the Shannon term rewards concentration; a smooth ramp under the noise so that the trees are mixed)
            ramp = torch.linspace(0, 0.2, size_x, device="cuda")
            xs = [torch.randn((batch, size_y, size_x), dtype=torch.float32, device="cuda") * 0.02 + ramp for _ in range(a.sets)]
            ys = [torch.empty_like(x) for x in xs]
            trees = torch.zeros((batch, packets.QTREE_WORDS), dtype=torch.int32, device="cuda")
            totals = torch.zeros(batch, dtype=torch.float64, device="cuda")
            table = torch.zeros((batch, packets.qtree_nodes(levels)), dtype=torch.float64, device="cuda")
            pinned = torch.empty((batch, size_y, size_x), dtype=torch.float32).pin_memory()
            torch.cuda.synchronize()
        with step_limit(a.step_limit, "pinned D2H copy of the batch"):
            d2h = timed_alternately({"copy": lambda r: pinned.copy_(xs[r % a.sets], non_blocking=True)}, 10, 2)["copy"]

        def search(r, dst=True):
            packets.wp_best2d_batch(W, cost, 0.0, xs[r % a.sets], ys[r % a.sets] if dst else None, *geom, tree=trees, total=totals, node_cost=table)

        calls = {"search": search, "search_no_dst": lambda r: search(r, False),
                 "tree": lambda r: packets.wp_tree2d_batch(W, False, xs[r % a.sets], ys[r % a.sets], *geom, trees, 4 * packets.QTREE_WORDS),
                 "wp2d": lambda r: packets.wp2d_batch(W, False, xs[r % a.sets], ys[r % a.sets], *geom)}
        floor_bytes = {"search": 4 * (levels + 1) + 16 * levels, "search_no_dst": 4 * (levels + 1) + 8 * levels, "tree": 8 * levels, "wp2d": 8 * levels}
        with step_limit(a.step_limit, "%d levels, fused route" % levels):
            launches = {k: count(f) for k, f in calls.items()}
            t = timed_alternately(calls, a.reps, a.warmup)
        leaves = [len(packets.wp_qtree_leaves(size_x, size_y, levels, [int(v) & 0xFFFFFFFF for v in row])) for row in trees.cpu().tolist()]
        entry = {"batch": batch, "size_y": size_y, "size_x": size_x, "levels": levels, "launches": launches, "leaves_min_max": [min(leaves), max(leaves)],
                 "pinned_d2h": d2h, **t}
        for k in calls:
            floor_ms = floor_bytes[k] * samples / STREAM * 1e3
            entry[k].update(bytes_per_sample=floor_bytes[k], floor_ms=floor_ms, over_floor=t[k]["ms_median"] / floor_ms,
                            over_wp2d=t[k]["ms_median"] / t["wp2d"]["ms_median"])
        if a.cross_reps > 0:
            dwt.set_option("wp_fused", 0)
            try:
                with step_limit(a.step_limit, "%d levels, cross-check route" % levels):
                    entry["cross_check_launches"] = count(search)
                    entry["cross_check"] = timed_alternately({"search": search}, a.cross_reps, 0)["search"]
                    entry["cross_check"]["over_wp2d"] = entry["cross_check"]["ms_median"] / t["wp2d"]["ms_median"]
            finally:
                dwt.set_option("wp_fused", 1)
        print(json.dumps(entry), flush=True)
        res["shapes"].append(entry)
        del xs, ys, table, pinned
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
