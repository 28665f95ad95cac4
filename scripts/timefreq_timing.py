"""Timing of the time-frequency planes (dwt_hip_timefreq_batch) on device-resident lines at the settings of the reference's
examples/spectra-tf: --lines lines of 4096 samples, 256 bins; FT with sigma 40, WT with sigma 1 and frequency 0.999 pi,
ST; magnitude output, and FT once more with argument output.  Median and minimum over --reps timed calls after --warmup,
one process, device events around the call.  Next to each:

* the arithmetic floor: the taps the reference would run (clipped at the line's ends) x 4 flops over the non-fused f32
  vector peak, half of the 157.3 TF FMA peak -- which assumes that packed multiplications and additions issue at full rate;
* the plain kernel of the same build (option timefreq_tiled = 0: one thread per output, signal and taps from global
  memory), timed over fewer calls (--reps / 10, at least 5);
* the reference's CPU rate: 0.29 Gtaps/s on one core, gabor_ft_s with N = 1024, bins = 64, sigma = 40, measured on the
  build machine (the reference is not built on the GPU machine's host).

Also recorded: the largest error of the device's argument planes against float64 atan2 of the device's own (re, im) over
the fixtures of tests/golden/timefreq.npz, in float32 ulps, next to the reference's own (manifest).

    python scripts/timefreq_timing.py [--reps 100] [--warmup 10] [--lines 64] [--out profiles/timefreq_timing.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import libdwt_amd as dwt  # noqa: E402
import timefreq_model as tm  # noqa: E402

PEAK_FLOPS = 157.3e12 / 2
REF_TAPS_PER_S = 0.29e9


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


def clipped_taps(sizes, centers, n):
    """taps the reference runs for one line: per bin and output, min(t, centre) + min(n-1-t, size-centre-1) + 1"""
    t = np.arange(n, dtype=np.int64)
    return int(sum((np.minimum(t, c) + np.minimum(n - 1 - t, s - c - 1) + 1).sum() for s, c in zip(sizes.astype(np.int64), centers.astype(np.int64))))


def arg_error():
    gold = np.load(tm.GOLDEN)
    worst = 0.0
    for i, c in enumerate(tm.CASES):
        n, bins = c[3], c[4]
        sizes = gold["sizes_%d" % i]
        bank = dwt.timefreq_bank(kernels=np.split(gold["taps_%d" % i], np.cumsum(sizes)[:-1]), centers=gold["centers_%d" % i])
        x = np.ascontiguousarray(gold["x_%d" % i])
        z, a = np.zeros((bins, n, 2), np.float32), np.zeros((bins, n), np.float32)
        dwt.timefreq_batch(bank, x, n * 4, 4, 1, n, "complex", z, bins * n * 8, n * 8)
        dwt.timefreq_batch(bank, x, n * 4, 4, 1, n, "arg", a, bins * n * 4, n * 4)
        bank.free()
        with np.errstate(all="ignore"):
            e = tm.ulps(a, np.arctan2(z[..., 1].astype(np.float64), z[..., 0].astype(np.float64)))
        if np.isfinite(e).any():
            worst = max(worst, float(e[np.isfinite(e)].max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lines", type=int, default=64)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timefreq_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    lines, n, bins = a.lines, a.n, a.bins
    x = torch.randn((lines, n), dtype=torch.float32, device="cuda")
    out = torch.empty((lines, bins, n), dtype=torch.float32, device="cuda")
    with open(tm.MANIFEST) as f:
        ref_arg = json.load(f)["arg_ref_max_ulp"]
    res = {"device": dwt.device_name(), "reps": a.reps, "warmup": a.warmup, "lines": lines, "n": n, "bins": bins, "peak_flops_unfused_f32": PEAK_FLOPS,
           "reference_cpu_taps_per_s": REF_TAPS_PER_S, "reference_cpu_rate_source": "one core of the build machine: gabor_ft_s, N 1024, bins 64, sigma 40",
           "arg_max_ulp_device": arg_error(), "arg_max_ulp_reference": ref_arg, "shapes": {}}
    print("arg error: device", res["arg_max_ulp_device"], "ulp, reference", ref_arg, "ulp", flush=True)
    for name, kind, sigma, freq, kind_out in (("ft", "ft", 40.0, 0.0, "abs"), ("wt", "wt", 1.0, tm.FREQ_TF, "abs"), ("st", "st", 0.0, 0.0, "abs"),
                                              ("ft_arg", "ft", 40.0, 0.0, "arg")):
        bank = dwt.timefreq_bank(kind, bins, sigma, freq)
        sizes, centers, _ = bank.query()
        taps = clipped_taps(sizes, centers, n) * lines
        call = lambda: dwt.timefreq_batch(bank, x, n * 4, 4, lines, n, kind_out, out, bins * n * 4, n * 4)  # noqa: E731
        mn, med = timed(call, a.reps, a.warmup)
        dwt.set_option("timefreq_tiled", 0)
        try:
            pmn, pmed = timed(call, max(5, a.reps // 10), 1)
        finally:
            dwt.set_option("timefreq_tiled", 1)
        bank.free()
        floor_ms = taps * 4 / PEAK_FLOPS * 1e3
        res["shapes"][name] = {"kernel_taps_min": int(sizes.min()), "kernel_taps_max": int(sizes.max()), "taps": taps, "taps_run_by_tiled_kernel": int(sizes.sum()) * n * lines,
                               "ms_min": mn, "ms_median": med, "gtaps_per_s": taps / med / 1e6, "floor_ms": floor_ms, "floor_share": floor_ms / med,
                               "plain": {"ms_min": pmn, "ms_median": pmed}, "speedup_over_plain": pmed / med,
                               "reference_cpu_s": taps / REF_TAPS_PER_S, "speedup_over_reference_core": taps / REF_TAPS_PER_S / (med / 1e3)}
        print(name, res["shapes"][name], flush=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
