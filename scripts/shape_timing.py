#!/usr/bin/env python3
"""Times the per-band coefficient operators, the LOG map and the threshold estimate on one MI355X
-> profiles/shape_timing.json.

Shapes: 64 x 4096^2 and one 8192^2 image, 5 levels, device resident, filled with seeded normal samples (coefficient-like:
both signs, no specials).  Configurations: SCALE on all slots, SOFT and COMPRESS on the detail slots, LOG over the
frames, the universal threshold.  Per configuration the median of --reps calls after --warmup, device events around the
call alone; the operators are not idempotent, so the images are restored from a pristine device copy before every call,
outside the timed region.  Next to each time: the byte floor (8 bytes per touched sample, 4 per sample read by the
threshold, at 8 TB/s), the per-band route of the same build where one exists (3J + 1 dwt_hip_scale calls per image) and
the pinned D2H + H2D copy of the same coefficients -- the two routes a caller has without this feature.

Also measures, on the fixture of tests/golden/shape.npz, the device's largest distance in ulp to the float64 model and to
the host libm's powf / logf / expf values (what tests/test_hip_shape.py reads as LIBM_ULPS).

    python scripts/shape_timing.py [--reps 100] [--warmup 10] [--out F | -]
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
import libdwt_amd as dwt  # noqa: E402
import shape_model as sm  # noqa: E402


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


def measure(batch, n, J, reps, warmup):
    g = torch.Generator(device="cuda").manual_seed(batch * 7 + n)
    pristine = torch.randn((batch, n, n), generator=g, device="cuda", dtype=torch.float32)
    work = torch.empty_like(pristine)
    image, sx, ns = n * n * 4, n * 4, 3 * J + 1
    geo = sm.slots(n, n, n, n, J)
    detail = sum(w * h for _, _, w, h in geo[:-1])
    res = {"batch": batch, "size": n, "levels": J, "coefficient_bytes": batch * image, "configs": {}}

    def restore():
        work.copy_(pristine)

    def table(op, a, ll):
        ops = np.full(ns, sm.KEEP if not ll else op, np.int32)
        ops[:3 * J] = op
        return ops, np.full(ns, a, np.float32)

    def per_band_scale():
        for b in range(batch):
            for x0, y0, w, h in geo:
                dwt.dwt_util_scale_s(work.data_ptr() + b * image + y0 * sx + 4 * x0, w, h, sx, 4, 0.5)

    for name, op, a, ll in (("scale_all", sm.SCALE, 0.5, True), ("soft_detail", sm.SOFT, 0.5, False), ("compress_detail", sm.COMPRESS, 0.7, False)):
        ops, params = table(op, a, ll)
        out = {"one_launch": timed(lambda: dwt.bands_apply_batch(work, image, batch, sx, n, n, J, ops, params), restore, reps, warmup)}
        touched = batch * (n * n if ll else detail)
        out["touched_samples"] = touched
        out["byte_floor_ms"] = 8 * touched / 8e12 * 1e3
        out["over_floor"] = out["one_launch"]["median_ms"] / out["byte_floor_ms"]
        if name == "scale_all":
            out["per_band_route"] = timed(per_band_scale, restore, max(5, reps // 10), 2)
            out["per_band_route"]["calls"] = batch * ns
        res["configs"][name] = out
        print(batch, n, name, {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in out.items()}, flush=True)
    # LOG reads positive samples
    positive = pristine.abs()

    def restore_log():
        work.copy_(positive)

    out = {"one_launch": timed(lambda: dwt.map_log_batch(work, image, batch, sx, n, n, 1e-5), restore_log, reps, warmup),
           "touched_samples": batch * n * n, "byte_floor_ms": 8 * batch * n * n / 8e12 * 1e3}
    out["over_floor"] = out["one_launch"]["median_ms"] / out["byte_floor_ms"]
    res["configs"]["log"] = out
    print(batch, n, "log", out["one_launch"]["median_ms"], out["byte_floor_ms"], flush=True)
    restore()
    lam = np.zeros(batch, np.float32)
    out = {"call": timed(lambda: dwt.universal_threshold_batch(work, image, batch, sx, n, n, lam), lambda: None, reps, warmup),
           "read_samples": batch * (n // 2) ** 2, "byte_floor_ms": 4 * batch * (n // 2) ** 2 / 8e12 * 1e3,
           "note": "four histogram rounds over HH(1), then one float per image crosses to the host (the call ends synchronised)"}
    out["over_floor"] = out["call"]["median_ms"] / out["byte_floor_ms"]
    res["configs"]["threshold"] = out
    print(batch, n, "threshold", out["call"]["median_ms"], out["byte_floor_ms"], flush=True)
    pinned = torch.empty((batch, n, n), dtype=torch.float32).pin_memory()
    res["pcie_round_trip"] = timed(lambda: (pinned.copy_(work, non_blocking=True), work.copy_(pinned, non_blocking=True)), lambda: None,
                                   max(5, reps // 10), 2)
    print(batch, n, "pcie", res["pcie_round_trip"]["median_ms"], flush=True)
    return res


def libm_distance():
    """the device over the fixture: largest distance in ulp to the float64 model and to the host libm"""
    z = np.load(sm.GOLDEN)
    out = {}

    def dist(got, model, libm):
        return {"to_float64_model": int(sm.ulps(got, z[model]).max()), "to_libm": int(sm.ulps(got, z[libm]).max())}

    for case in ("compress", "hdr"):
        sox, soy = sm.CASES[case][:2]
        x = z["hdr.eaw"].copy() if case == "hdr" else sm.case_arrays(case)[0]
        J = sm.levels(sox, soy, sm.CASES[case][4])
        ops, params = sm.make_table("compress", 3 * J + 1)
        d = torch.from_numpy(x).cuda()
        dwt.bands_apply(d, sox * 4, 4, sox, soy, sox, soy, J, ops, params)
        if case == "hdr":
            out["compress_hdr_coefficients"] = dist(d.cpu().numpy(), "hdr.compressed", "hdr.compressed.libm")
        else:
            out["compress"] = dist(d.cpu().numpy(), "compress.out", "compress.libm")
    m = sm.make_input(99, 13, 21)
    for op, f in ((sm.LOG, dwt.map_log), (sm.EXP, dwt.map_exp)):
        d = torch.from_numpy(m).cuda()
        f(d, 21 * 4, 4, 21, 13, 1e-5)
        out[op] = dist(d.cpu().numpy(), "map." + op, "map.%s.libm" % op)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shape_timing.json"))
    args = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    res = {"device": dwt.device_name(),
           "method": "HIP events around each call; median of %d calls after %d warm-ups (per-band route and PCIe copy: a tenth of the calls); "
                     "the images are restored from a pristine device copy before every call, outside the timed region" % (args.reps, args.warmup),
           "ulp_distance_over_fixture": libm_distance(),
           "shapes": [measure(64, 4096, 5, args.reps, args.warmup), measure(1, 8192, 5, args.reps, args.warmup)]}
    print(json.dumps(res["ulp_distance_over_fixture"]), flush=True)
    if args.out != "-":
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
