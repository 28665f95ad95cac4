"""Timing of the edge-avoiding 9/7 transforms (dwt_hip_eaw97_2d_batch) and, in the same process on the same buffers, of
the 5/3 ones (dwt_hip_eaw53_2d_batch): the fused one-launch-per-level kernels against the two-pass route (option
"eaw_two_pass"), alternated on a seeded input, device events after a warm-up, median of --reps.  Cases: one 8192^2
image and 64 x 1024^2 images, J = 5, forward and inverse, alpha 1 and 0.8.  Share of peak: 16 B per sample of every
level (image in and out, both weights out / in) against 6.29 TB/s.  The summary rows give the 9/7 : 5/3 ratio of the
fused times.

    python scripts/eaw97_timing.py [--reps 10] [--out profiles/eaw97_timing.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdwt_amd as dwt  # noqa: E402

PEAK = 6.29e12
J = 5
BATCH = {"eaw97": dwt.eaw97_2d_batch, "eaw53": dwt.eaw53_2d_batch}


def level_samples(w, h, j):
    return sum(((w + (1 << k) - 1) >> k) * ((h + (1 << k) - 1) >> k) for k in range(j))


def device_case(name, batch, w, h, reps):
    x0 = torch.from_numpy(np.random.default_rng(1).random((batch, h, w), dtype=np.float32)).cuda()
    x = x0.clone()
    total, _, _ = dwt.eaw53_weights_layout(dwt.EAW_MALLAT, w, h, w, h, J)
    wb = torch.zeros(batch * total, dtype=torch.float32, device="cuda")
    dwt.use_torch_stream()
    out = []
    runs = [(wv, two) for wv in ("eaw97", "eaw53") for two in (0, 1)]
    for alpha in (1.0, 0.8):
        for inverse in (0, 1):
            times = {r: [] for r in runs}

            def once(wv, two, keep):
                # the inverse needs the wavelet's own forward in x and wb: run it (untimed) first
                dwt.set_option("eaw_two_pass", two)
                x.copy_(x0)
                if inverse:
                    BATCH[wv](0, x, h * w * 4, batch, w * 4, w, h, wb, total, J, alpha=alpha)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                BATCH[wv](inverse, x, h * w * 4, batch, w * 4, w, h, wb, total, J, alpha=alpha)
                b.record()
                b.synchronize()
                if keep:
                    times[(wv, two)].append(a.elapsed_time(b) * 1e3)
            for wv, two in runs + runs:  # warm-up rounds
                once(wv, two, False)
            for _ in range(reps):
                for wv, two in runs:
                    once(wv, two, True)
            dwt.set_option("eaw_two_pass", 0)
            samples = batch * level_samples(w, h, J)
            med = {}
            for wv, two in runs:
                t = times[(wv, two)]
                us = med[(wv, two)] = float(np.median(t))
                out.append({"case": name, "wavelet": wv, "batch": batch, "w": w, "h": h, "levels": J, "alpha": alpha,
                            "dir": "inverse" if inverse else "forward", "path": "two_pass" if two else "fused",
                            "us": round(us, 1), "us_min": round(float(np.min(t)), 1), "us_max": round(float(np.max(t)), 1),
                            "peak_share": round(samples * 16 / (us * 1e-6) / PEAK, 4)})
                print(json.dumps(out[-1]), flush=True)
            out.append({"case": name, "summary": True, "alpha": alpha, "dir": "inverse" if inverse else "forward",
                        "fused_97_over_53": round(med[("eaw97", 0)] / med[("eaw53", 0)], 3),
                        "eaw97_two_pass_over_fused": round(med[("eaw97", 1)] / med[("eaw97", 0)], 3)})
            print(json.dumps(out[-1]), flush=True)
    del x, x0, wb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eaw97_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    rows = device_case("8192^2", 1, 8192, 8192, a.reps) + device_case("64x1024^2", 64, 1024, 1024, a.reps)
    with open(a.out, "w") as f:
        json.dump({"device": dwt.device_name(), "reps": a.reps, "rows": rows}, f, indent=1)
    dwt.dwt_util_finish()


if __name__ == "__main__":
    main()
