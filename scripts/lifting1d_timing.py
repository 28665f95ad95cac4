"""Timing of the user-defined lifting wavelets of line batches (dwt_hip_lifting1d_batch) on the shape of the
spectra workload: 65536 rows of 4096 samples, full depth (12 levels), forward and inverse, out of place.  Device events around
every call, a warm-up round, then the median of --reps calls on --sets rotating buffer sets, so that no call finds its input
in the Infinity Cache.

Per direction three routes are ALTERNATED call by call on the same buffers:
  * the fused route with the CDF 9/7 table (k_lift_lines: every level in one launch);
  * the yardstick: dwt_hip_transform1d_batch(DWT_HIP_CDF97_S) of the same build, the specialised one-launch kernel;
  * the step-by-step route with the same table (option "lifting_fused" = 0);
then D4 and HAAR_INT run on the fused route.  Every row states microseconds, the byte floor -- 8 bytes per sample, whatever
the depth, over 8 TB/s -- and its share; the ratio rows divide medians.  Before anything is timed the three CDF 9/7 routes are
compared on the timed shape: the same bits.

    python scripts/lifting1d_timing.py [--reps 100] [--sets 3] [--out profiles/lifting1d_timing.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdwt_amd as dwt  # noqa: E402
from libdwt_amd import lifting as L  # noqa: E402

PEAK = 8e12
ROWS, SIZE, LEVELS = 65536, 4096, 12


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def row(case, what, us, **more):
    med = float(np.median(us))
    floor = 8.0 * ROWS * SIZE / PEAK * 1e6
    r = dict({"case": case, "what": what, "calls": len(us), "us": round(med, 1), "us_min": round(float(np.min(us)), 1),
              "us_p90": round(float(np.percentile(us, 90)), 1), "byte_floor_us": round(floor, 1), "fraction_of_floor": round(floor / med, 4),
              "Gsamples_per_s": round(ROWS * SIZE / med * 1e-3, 2)}, **more)
    print(json.dumps(r), flush=True)
    return r


def ratio(case, what, a, b):
    r = {"case": case, "what": what, "ratio": round(a["us"] / b["us"], 3)}
    print(json.dumps(r), flush=True)
    return r


def measure(reps, sets):
    rows = []
    geom = (4 * SIZE, 4, ROWS, SIZE)
    gen = torch.Generator(device="cuda").manual_seed(5)
    src = [torch.rand((ROWS, SIZE), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1 for _ in range(sets)]
    dst = [torch.empty_like(s) for s in src]
    chk = torch.empty_like(src[0])

    def lifting(scheme, fused, inverse, a, b):
        dwt.set_option("lifting_fused", fused)
        assert L.lifting1d_batch(scheme, inverse, a, b, *geom, LEVELS) == LEVELS

    def special(inverse, a, b):
        assert dwt.transform1d_batch("cdf97_s", inverse, a, b, 4 * SIZE, ROWS, SIZE, LEVELS) == LEVELS

    same = lambda a, b: bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    for inverse in (False, True):
        case = "%d x %d, %s, %d levels" % (ROWS, SIZE, "inverse" if inverse else "forward", LEVELS)
        for tname, ttype in (("CDF97", torch.float32), ("D4", torch.float32), ("HAAR_INT", torch.int32)):
            scheme = L.builtin(tname)
            assert L.route1d(scheme, SIZE) == L.FUSED
            ins = [(s * 32767.0).to(torch.int32) for s in src] if ttype == torch.int32 else src
            if inverse:  # the coefficients by this scheme
                coef = []
                for a in ins:
                    c = torch.empty_like(a)
                    lifting(scheme, 1, False, a, c)
                    coef.append(c)
                ins = coef
            outs = [d.view(ttype) for d in dst]
            fused = lambda k: lifting(scheme, 1, inverse, ins[k], outs[k])
            steps = lambda k: lifting(scheme, 0, inverse, ins[k], outs[k])
            more = {"scheme": tname, "reach": L.check(scheme)}
            if tname == "CDF97":
                spec = lambda k: special(inverse, ins[k], outs[k])
                # the same bits on the timed shape, and the warm-up
                fused(0)
                torch.cuda.synchronize()
                chk.copy_(outs[0])
                steps(0)
                same_steps = same(chk, outs[0])
                spec(0)
                same_spec = same(chk, outs[0])
                for k in range(sets):
                    fused(k), spec(k), steps(k)
                torch.cuda.synchronize()
                us_f, us_y, us_s = [], [], []
                for rep in range(reps):
                    k = rep % sets
                    us_f.append(timed(lambda: fused(k)))
                    us_y.append(timed(lambda: spec(k)))
                    if rep < max(10, reps // 5):  # (some seventy launches a call: fewer calls say the same)
                        us_s.append(timed(lambda: steps(k)))
                rf = row(case, "fused route, CDF 9/7 table", us_f, same_bits_as_steps=same_steps, same_bits_as_specialised=same_spec, **more)
                ry = row(case, "yardstick: transform1d_batch(CDF97_S), the specialised kernel", us_y)
                rs = row(case, "step-by-step route, CDF 9/7 table", us_s, **more)
                rows += [rf, ry, rs, ratio(case, "fused over the specialised kernel (medians)", rf, ry),
                         ratio(case, "step-by-step over fused (medians)", rs, rf)]
            else:
                for k in range(sets):
                    fused(k)
                torch.cuda.synchronize()
                us_f = [timed(lambda: fused(rep % sets)) for rep in range(reps)]
                rows.append(row(case, "fused route, %s" % tname, us_f, **more))
            del ins, outs
            torch.cuda.empty_cache()
    dwt.set_option("lifting_fused", 1)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lifting1d_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    res = {"device": dwt.device_name(), "reps": a.reps, "sets": a.sets, "peak_Bps": PEAK, "rows_of_samples": [ROWS, SIZE], "levels": LEVELS,
           "byte_floor": "8 bytes per sample, whatever the depth", "rows": measure(a.reps, a.sets)}
    dwt.dwt_util_finish()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
