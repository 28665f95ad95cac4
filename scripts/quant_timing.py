"""Timing of the deadzone quantizer (dwt_hip_quantize_batch / dwt_hip_dequantize_batch / dwt_hip_codeblock_bitplanes_batch;
DESIGN.md s26) on the shapes of the workload: 64 frames of 4096^2 and one of 8192^2, holding the 5-level float 9/7
coefficients of the library's test image.  Device events around every call, a warm-up round, then the median of --reps
calls on --sets rotating buffer sets, so that no call finds its input in the Infinity Cache.

Per row: microseconds and the fraction of the byte floor -- every sample's bytes read once and written once, against
8 TB/s (quantize binary32 -> int16: 6 bytes per sample).  The same run times, ALTERNATED call by call with the quantizer,
  * the yardstick: dwt_hip_bands_apply_batch with SCALE (by 1) on every slot of the same batch, the library's existing
    in-place elementwise operator over the same band tables, 8 bytes per sample;
and
  * the bit-plane map once more under option "quant_wide" = 0 (element by element);
  * the route that exists without the quantizer: the float planes copied to pinned host memory (one 8192^2 frame,
    median of max(5, reps / 5) copies).  Every row states its number of calls.

    python scripts/quant_timing.py [--reps 100] [--sets 2] [--out profiles/quant_timing.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdwt_amd as dwt  # noqa: E402
from libdwt_amd import quant as Q  # noqa: E402

PEAK = 8e12
LEVELS = 5
SHAPES = (("64x4096^2", 64, 4096, 4096), ("8192^2", 1, 8192, 8192))
BASE_STEP = 1.0 / 128


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(us):
    return {"us": round(float(np.median(us)), 1), "us_min": round(float(np.min(us)), 1), "us_p90": round(float(np.percentile(us, 90)), 1)}


def row(case, what, nbytes, us, **more):
    floor_us = nbytes / PEAK * 1e6
    r = dict({"case": case, "what": what, "bytes": nbytes, "calls": len(us)}, **stats(us), byte_floor_us=round(floor_us, 1),
             fraction_of_floor=round(floor_us / float(np.median(us)), 4), TB_per_s=round(nbytes / float(np.median(us)) * 1e-6, 3), **more)
    print(json.dumps(r), flush=True)
    return r


def coefficients(batch, w, h, sets):
    """`sets` stacks of `batch` frames: the test image, transformed LEVELS levels on the device"""
    img = np.zeros((h, w), np.float32)
    dwt.lib.dwt_util_test_image_fill_s(img.ctypes.data, img.strides[0], 4, w, h, 0)
    one = torch.from_numpy(img).cuda()
    out = []
    for k in range(sets):
        src = (one * (1.0 + 0.25 * k)).unsqueeze(0).expand(batch, h, w).contiguous()
        dst = torch.empty_like(src)
        assert dwt.transform2d_batch(dwt.CDF97_S, False, src, dst, 4 * w * h, batch, 4 * w, w, h, LEVELS) == LEVELS
        out.append(dst)
        del src
    torch.cuda.synchronize()
    return out


def measure(reps, sets):
    rows = []
    steps = Q.quant_steps(dwt.CDF97_S, LEVELS, BASE_STEP)
    ns = 3 * LEVELS + 1
    scale_ops, scale_params = ["scale"] * ns, [1.0] * ns
    for name, batch, w, h in SHAPES:
        n = batch * w * h
        coef = coefficients(batch, w, h, sets)
        i16 = [torch.empty((batch, h, w), dtype=torch.int16, device="cuda") for _ in range(sets)]
        i32 = [torch.empty((batch, h, w), dtype=torch.int32, device="cuda") for _ in range(sets)]
        back = torch.empty_like(coef[0])
        total = int(Q.codeblock_layout(w, h, LEVELS, 6, 6)[0][-1])
        planes = torch.empty((batch, total), dtype=torch.uint8, device="cuda")
        f32, s16, s32 = (4 * w * h, 4 * w), (2 * w * h, 2 * w), (4 * w * h, 4 * w)
        frames = (batch, w, h, LEVELS)
        assert Q.quant_route(Q.S, coef[0], *f32, Q.I16, i16[0], *s16, batch, w, h) == Q.WIDE_COEF | Q.WIDE_INDEX
        q16 = lambda k: Q.quantize_batch(Q.S, coef[k], *f32, Q.I16, i16[k], *s16, *frames, steps)
        q32 = lambda k: Q.quantize_batch(Q.S, coef[k], *f32, Q.I32, i32[k], *s32, *frames, steps)
        d16 = lambda k: Q.dequantize_batch(Q.I16, i16[k], *s16, Q.S, back, *f32, *frames, steps, r=0.5)
        bp = lambda k: Q.codeblock_bitplanes_batch(Q.I16, i16[k], *s16, *frames, 6, 6, planes, total)
        scale = lambda k: dwt.bands_apply_batch(coef[k], 4 * w * h, batch, 4 * w, w, h, LEVELS, scale_ops, scale_params)
        for k in range(sets):  # warm-up; the indices the later calls read
            q16(k), q32(k), d16(k), bp(k), scale(k)
        counters = Q.quantize_batch(Q.S, coef[0], *f32, Q.I16, i16[0], *s16, *frames, steps, stats=True)
        torch.cuda.synchronize()
        share = {"nonzero_share": round(float(counters[:, :, 0].sum()) / n, 4), "clipped": int(counters[:, :, 2].sum()),
                 "largest_magnitude": int(counters[:, :, 1].max())}
        # quantize to int16 and the yardstick, alternated call by call
        us_q, us_s = [], []
        for rep in range(reps):
            us_q.append(timed(lambda: q16(rep % sets)))
            us_s.append(timed(lambda: scale(rep % sets)))
        rq = row(name, "quantize binary32 -> int16", 6 * n, us_q, **share)
        rs = row(name, "yardstick: bands_apply_batch SCALE, in place", 8 * n, us_s)
        rows += [rq, rs, {"case": name, "what": "quantize -> int16 over the yardstick (medians)", "ratio": round(rq["us"] / rs["us"], 4)}]
        print(json.dumps(rows[-1]), flush=True)
        rows.append(row(name, "quantize binary32 -> int32", 8 * n, [timed(lambda: q32(rep % sets)) for rep in range(reps)]))
        rows.append(row(name, "quantize binary32 -> int16 with the band counters (ends synchronised)", 6 * n,
                        [timed(lambda: Q.quantize_batch(Q.S, coef[rep % sets], *f32, Q.I16, i16[rep % sets], *s16, *frames, steps, stats=True))
                         for rep in range(reps)]))
        rows.append(row(name, "dequantize int16 -> binary32", 6 * n, [timed(lambda: d16(rep % sets)) for rep in range(reps)]))
        rows.append(row(name, "bit-plane map of int16 indices, 64 x 64 blocks", 2 * n + batch * total, [timed(lambda: bp(rep % sets)) for rep in range(reps)]))
        dwt.set_option("quant_wide", 0)  # the cross-check route: the same map read element by element
        try:
            bp(0)
            rows.append(row(name, "bit-plane map of int16 indices, 64 x 64 blocks, element by element (quant_wide 0)", 2 * n + batch * total,
                            [timed(lambda: bp(rep % sets)) for rep in range(reps)]))
        finally:
            dwt.set_option("quant_wide", 1)
        if batch == 1:
            host = torch.empty((h, w), dtype=torch.float32).pin_memory()
            host.copy_(coef[0][0], non_blocking=True)
            torch.cuda.synchronize()
            us = [timed(lambda: host.copy_(coef[0][0], non_blocking=True)) for _ in range(max(5, reps // 5))]
            rows.append(dict({"case": name, "what": "without the quantizer: the float planes to pinned host memory", "bytes": 4 * n, "calls": len(us)},
                             **stats(us), GB_per_s=round(4 * n / float(np.median(us)) * 1e-3, 2)))
            print(json.dumps(rows[-1]), flush=True)
            del host
        del coef, i16, i32, back, planes
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    res = {"device": dwt.device_name(), "reps": a.reps, "sets": a.sets, "peak_Bps": PEAK, "levels": LEVELS, "base_step": BASE_STEP,
           "rows": measure(a.reps, a.sets)}
    dwt.dwt_util_finish()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
