"""Timing of the float CDF 9/7 on binary16 storage (DWT_HIP_CDF97_H) against the float CDF 9/7 (DWT_HIP_CDF97_S) of the
same build on the same shapes: one 8192^2 image (dwt_hip_transform2d, out of place) and a batch of 64 x 8192^2
(dwt_hip_transform2d_batch), 5 levels, forward and inverse.  Device events around every call, a warm-up round, then the
median of --reps calls; the calls rotate over --sets source / destination pairs so that no call finds its input in the
Infinity Cache, and the two wavelets alternate call by call.  The same run checks the binary16 round trip on the timed
input: within one grey level of the 8-bit data.

Per row: microseconds, Gsamples/s (samples of level 0 of every image per second), the binary16 rate over the float rate,
and the fraction of the byte floor -- 2 * 2 B (binary16) or 2 * 4 B (float) per sample of every level, each level's input
read once and its output written once, against 8 TB/s.

    python scripts/h16_timing.py [--reps 100] [--sets 2] [--out profiles/h16_timing.json]"""
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
WAVELETS = (("cdf97_h", torch.float16, 2), ("cdf97_s", torch.float32, 4))


def level_samples(w, h, j):
    return sum(((w + (1 << k) - 1) >> k) * ((h + (1 << k) - 1) >> k) for k in range(j))


def call(wav, es, inverse, a, b, batch, w, h):
    if batch == 1:
        j = C.c_int(J)
        rc = dwt.lib.dwt_hip_transform2d(dwt.WAVELET_ID[wav], inverse, a.data_ptr(), b.data_ptr(), w * es, es, w, h, w, h, C.byref(j), 0, 0)
        assert rc == 0, dwt.last_error()
    else:
        dwt.transform2d_batch(wav, inverse, a, b, w * h * es, batch, w * es, w, h, J)


def case(name, batch, w, h, reps, sets):
    g = torch.Generator(device="cuda").manual_seed(16)
    bufs, round_trip = {}, {}
    for wav, dt, es in WAVELETS:
        src = [torch.randint(0, 256, (batch, h, w), dtype=torch.int16, device="cuda", generator=g).to(dt) for _ in range(sets)]
        coef = [torch.empty_like(s) for s in src]
        keep = src[0][0].clone()
        for k in range(sets):  # warm-up, and the coefficients the inverse calls read; the inverse puts the round trip in place of the source
            call(wav, es, 0, src[k], coef[k], batch, w, h)
            call(wav, es, 1, coef[k], src[k], batch, w, h)
        torch.cuda.synchronize()
        round_trip[wav] = float((src[0][0].float() - keep.float()).abs().max())
        assert round_trip[wav] <= 1.0, (wav, round_trip[wav])
        del keep
        bufs[wav] = (src, coef)
    rows = []
    for inverse in (0, 1):
        times = {wav: [] for wav, _, _ in WAVELETS}
        for rep in range(reps):
            for wav, dt, es in WAVELETS:
                src, coef = bufs[wav]
                k = rep % sets
                a, b = (coef[k], src[k]) if inverse else (src[k], coef[k])
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                call(wav, es, inverse, a, b, batch, w, h)
                ev1.record()
                ev1.synchronize()
                times[wav].append(ev0.elapsed_time(ev1) * 1e3)
        us = {wav: float(np.median(times[wav])) for wav, _, _ in WAVELETS}
        for wav, dt, es in WAVELETS:
            floor_us = batch * level_samples(w, h, J) * 2 * es / PEAK * 1e6
            rows.append({"case": name, "batch": batch, "w": w, "h": h, "levels": J, "dir": "inverse" if inverse else "forward", "wavelet": wav,
                         "us": round(us[wav], 1), "us_min": round(float(np.min(times[wav])), 1), "us_p90": round(float(np.percentile(times[wav], 90)), 1),
                         "gsamples_per_s": round(batch * w * h / us[wav] * 1e-3, 2), "byte_floor_us": round(floor_us, 1),
                         "fraction_of_floor": round(floor_us / us[wav], 4), "round_trip_max_error_grey_levels": round_trip[wav]})
            print(json.dumps(rows[-1]), flush=True)
        rows.append({"case": name, "dir": "inverse" if inverse else "forward",
                     "half_rate_over_float_rate": round(us["cdf97_s"] / us["cdf97_h"], 4)})
        print(json.dumps(rows[-1]), flush=True)
    del bufs
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "h16_timing.json"))
    ap.add_argument("--cases", default="single,batch")
    a = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    rows = []
    if "single" in a.cases.split(","):
        rows += case("8192^2", 1, 8192, 8192, a.reps, max(a.sets, 4))
    if "batch" in a.cases.split(","):
        rows += case("64x8192^2", 64, 8192, 8192, a.reps, a.sets)
    with open(a.out, "w") as f:
        json.dump({"device": dwt.device_name(), "reps": a.reps, "sets": a.sets, "peak_Bps": PEAK, "rows": rows,
                   "bound_by": "not determined: the sweeps keep no LDS ring, run 3 waves per SIMD and fetch the halo of the row ends "
                               "sample by sample; none of it was timed apart"}, f, indent=1)
        f.write("\n")
    dwt.dwt_util_finish()


if __name__ == "__main__":
    main()
