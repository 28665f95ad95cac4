"""Timing of the edge-avoiding 5/3 transforms (dwt_hip_eaw53_2d_batch): the fused one-launch-per-level kernels against
the two-pass route (option "eaw_two_pass"), alternated in one process on a seeded input, device events after a warm-up,
median of --reps.  Cases: one 8192^2 image and 64 x 1024^2 images, J = 5, forward and inverse, alpha 1 and 0.8.  The
reference CPU library (oracle/_ref/libdwt_ref.so, where it was built) is timed on the 8192^2 image once, wall clock.
Share of peak: 16 B per sample of every level (image in and out, both weights out / in) against 6.29 TB/s.

    python scripts/eaw_timing.py [--reps 10] [--out profiles/eaw_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import libdwt_amd as dwt  # noqa: E402

PEAK = 6.29e12
J = 5


def level_samples(w, h, j):
    return sum(((w + (1 << k) - 1) >> k) * ((h + (1 << k) - 1) >> k) for k in range(j))


def device_case(name, batch, w, h, reps):
    x0 = torch.from_numpy(np.random.default_rng(1).random((batch, h, w), dtype=np.float32)).cuda()
    x = x0.clone()
    total, _, _ = dwt.eaw53_weights_layout(dwt.EAW_MALLAT, w, h, w, h, J)
    wb = torch.zeros(batch * total, dtype=torch.float32, device="cuda")
    dwt.use_torch_stream()
    out = []
    for alpha in (1.0, 0.8):
        for inverse in (0, 1):
            times = {0: [], 1: []}
            for two in (0, 1, 0, 1):  # warm-up round
                if not inverse:
                    x.copy_(x0)
                dwt.set_option("eaw_two_pass", two)
                dwt.eaw53_2d_batch(inverse, x, h * w * 4, batch, w * 4, w, h, wb, total, J, alpha=alpha)
            for _ in range(reps):
                for two in (0, 1):
                    dwt.set_option("eaw_two_pass", two)
                    if not inverse:
                        x.copy_(x0)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    dwt.eaw53_2d_batch(inverse, x, h * w * 4, batch, w * 4, w, h, wb, total, J, alpha=alpha)
                    b.record()
                    b.synchronize()
                    times[two].append(a.elapsed_time(b) * 1e3)
            dwt.set_option("eaw_two_pass", 0)
            samples = batch * level_samples(w, h, J)
            for two in (0, 1):
                us = float(np.median(times[two]))
                out.append({"case": name, "batch": batch, "w": w, "h": h, "levels": J, "alpha": alpha,
                            "dir": "inverse" if inverse else "forward", "path": "two_pass" if two else "fused",
                            "us": round(us, 1), "us_min": round(float(np.min(times[two])), 1),
                            "peak_share": round(samples * 16 / (us * 1e-6) / PEAK, 4)})
                print(json.dumps(out[-1]), flush=True)
    del x, x0, wb
    torch.cuda.empty_cache()
    return out


def reference_case(w, h):
    import eaw_model as M

    if not M.have_ref():
        return []
    ref = M.RefEaw()
    img = np.random.default_rng(1).random((h, w), dtype=np.float32)
    t0 = time.perf_counter()
    j, wH, wV = ref.fwd(img, j_max=J)
    t1 = time.perf_counter()
    ref.inv(img, wH, wV, j_max=j)
    t2 = time.perf_counter()
    rows = [{"case": "reference_cpu", "w": w, "h": h, "levels": J, "alpha": 1.0, "dir": d, "path": "reference",
             "us": round(t * 1e6, 1), "threads": os.environ.get("OMP_NUM_THREADS", "")}
            for d, t in (("forward", t1 - t0), ("inverse", t2 - t1))]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eaw_timing.json"))
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    dwt.dwt_util_init()
    rows = device_case("8192^2", 1, 8192, 8192, a.reps) + device_case("64x1024^2", 64, 1024, 1024, a.reps)
    if not a.no_reference:
        rows += reference_case(8192, 8192)
    with open(a.out, "w") as f:
        json.dump({"device": dwt.device_name(), "reps": a.reps, "rows": rows}, f, indent=1)
    dwt.dwt_util_finish()


if __name__ == "__main__":
    main()
