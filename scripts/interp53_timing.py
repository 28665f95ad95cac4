"""Timing of the interpolating 5/3 transforms (DWT_HIP_INTERP53_S): the fused tile sweeps against the exact line-pass
route (option "generic"), and interp53 against CDF 5/3 float on the same buffers, alternated in one process on a seeded
input, device events after a warm-up round, median of --reps.  Cases, J = 5: a batch of 64 x 4096^2 images
(dwt_hip_transform2d_batch; the line-pass route takes no batches, so its row runs the 64 images one call each) and one
8192^2 image (dwt_hip_transform2d, out of place), forward and inverse; then one batch of 65536 lines of 4096 samples
at J = 12 (dwt_hip_transform1d_batch).  The same run compares the fused and line-pass outputs of the timed inputs bit
for bit.  Share of peak: algorithmic bytes -- 8 B per sample of every level for the 2-D transforms (each level's input
read once, its output written once), 8 B per sample for the 1-D batch (all levels of a line in one pass) -- against
8 TB/s.

    python scripts/interp53_timing.py [--reps 10] [--out profiles/interp53_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdwt_amd as dwt  # noqa: E402

PEAK = 8e12
J = 5


def level_samples(w, h, j):
    return sum(((w + (1 << k) - 1) >> k) * ((h + (1 << k) - 1) >> k) for k in range(j))


def bits_equal(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def case2d(name, batch, w, h, reps):
    x0 = torch.from_numpy(np.random.default_rng(1).random((batch, h, w), dtype=np.float32)).cuda()
    src = x0.clone()
    dst = torch.empty_like(x0)
    bs = h * w * 4

    def call(wav, inverse, generic):
        a, b = (dst, src) if inverse else (src, dst)
        if not generic:
            if batch == 1:
                j = C.c_int(J)
                rc = dwt.lib.dwt_hip_transform2d(dwt.WAVELET_ID[wav], inverse, a.data_ptr(), b.data_ptr(), w * 4, 4, w, h, w, h,
                                                 C.byref(j), 0, 0)
                assert rc == 0, dwt.last_error()
            else:
                dwt.transform2d_batch(wav, inverse, a, b, bs, batch, w * 4, w, h, J)
        else:
            for k in range(batch):
                j = C.c_int(J)
                rc = dwt.lib.dwt_hip_transform2d(dwt.WAVELET_ID[wav], inverse, a[k].data_ptr(), b[k].data_ptr(), w * 4, 4, w, h, w, h,
                                                 C.byref(j), 0, 0)
                assert rc == 0, dwt.last_error()

    variants = [("interp53_s", 0), ("interp53_s", 1), ("cdf53_s", 0)]
    rows = []
    for inverse in (0, 1):
        times = {v: [] for v in variants}
        outs = {}
        for rep in range(reps + 1):  # round 0: warm-up
            for wav, generic in variants:
                src.copy_(x0)
                if inverse:  # the inverse reads the fused forward's coefficients of this wavelet
                    call(wav, 0, 0)
                dwt.set_option("generic", generic)
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                call(wav, inverse, generic)
                ev1.record()
                ev1.synchronize()
                dwt.set_option("generic", 0)
                if rep > 0:
                    times[(wav, generic)].append(ev0.elapsed_time(ev1) * 1e3)
                if rep == reps and wav == "interp53_s":
                    outs[generic] = (src if inverse else dst).clone()
        same = bits_equal(outs[0], outs[1])
        del outs
        samples = batch * level_samples(w, h, J)
        for wav, generic in variants:
            us = float(np.median(times[(wav, generic)]))
            rows.append({"case": name, "batch": batch, "w": w, "h": h, "levels": J, "dir": "inverse" if inverse else "forward",
                         "wavelet": wav, "path": "generic" if generic else "fused", "us": round(us, 1),
                         "us_min": round(float(np.min(times[(wav, generic)])), 1),
                         "peak_share": round(samples * 8 / (us * 1e-6) / PEAK, 4)})
            if wav == "interp53_s" and generic:
                rows[-1]["bits_equal_fused"] = same
            print(json.dumps(rows[-1]), flush=True)
        f53 = next(r for r in rows[-3:] if r["wavelet"] == "cdf53_s")["us"]
        fi = next(r for r in rows[-3:] if r["wavelet"] == "interp53_s" and r["path"] == "fused")["us"]
        rows.append({"case": name, "dir": "inverse" if inverse else "forward", "interp53_rate_over_cdf53_rate": round(f53 / fi, 4),
                     "target": 0.95, "met": f53 / fi >= 0.95})
        print(json.dumps(rows[-1]), flush=True)
    del x0, src, dst
    torch.cuda.empty_cache()
    return rows


def case1d(n_lines, size, levels, reps):
    x0 = torch.from_numpy(np.random.default_rng(2).random((n_lines, size), dtype=np.float32)).cuda()
    x = x0.clone()
    rows = []
    for inverse in (0, 1):
        times = {0: [], 1: [], 2: []}
        outs = {}
        for rep in range(reps + 1):
            for v in (0, 1, 2):  # 0: interp53 fused, 1: interp53 line passes, 2: cdf53 fused
                wav = "cdf53_s" if v == 2 else "interp53_s"
                x.copy_(x0)
                if inverse:
                    dwt.transform1d_batch(wav, 0, x, x, size * 4, n_lines, size, levels)
                dwt.set_option("generic", 1 if v == 1 else 0)
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                dwt.transform1d_batch(wav, inverse, x, x, size * 4, n_lines, size, levels)
                ev1.record()
                ev1.synchronize()
                dwt.set_option("generic", 0)
                if rep > 0:
                    times[v].append(ev0.elapsed_time(ev1) * 1e3)
                if rep == reps and v < 2:
                    outs[v] = x.clone()
        same = bits_equal(outs[0], outs[1])
        for v in (0, 1, 2):
            us = float(np.median(times[v]))
            rows.append({"case": "1d_%dx%d" % (n_lines, size), "lines": n_lines, "size": size, "levels": levels,
                         "dir": "inverse" if inverse else "forward", "wavelet": "cdf53_s" if v == 2 else "interp53_s",
                         "path": "generic" if v == 1 else "fused", "us": round(us, 1), "us_min": round(float(np.min(times[v])), 1),
                         "peak_share": round(n_lines * size * 8 / (us * 1e-6) / PEAK, 4)})
            if v == 1:
                rows[-1]["bits_equal_fused"] = same
            print(json.dumps(rows[-1]), flush=True)
    del x, x0
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp53_timing.json"))
    ap.add_argument("--cases", default="batch,single,1d")
    a = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    rows = []
    cases = a.cases.split(",")
    if "batch" in cases:
        rows += case2d("64x4096^2", 64, 4096, 4096, a.reps)
    if "single" in cases:
        rows += case2d("8192^2", 1, 8192, 8192, a.reps)
    if "1d" in cases:
        rows += case1d(65536, 4096, 12, a.reps)
    with open(a.out, "w") as f:
        json.dump({"device": dwt.device_name(), "reps": a.reps, "peak_Bps": PEAK, "rows": rows}, f, indent=1)
    dwt.dwt_util_finish()


if __name__ == "__main__":
    main()
