"""Timing of the sparse coefficient streams (dwt_hip_sparse_pack_batch / dwt_hip_sparse_unpack_batch) on the
shapes of the workload: 64 frames of 4096^2 and one of 8192^2, holding what the two flows that end in sparse planes leave
of the 5-level float 9/7 coefficients of the library's test image -- int16 indices at base step 1/128 (quantize_batch),
float coefficients after keep_largest_batch at keep = 1 % and 10 %.  Device events around every call, a warm-up round, then
the median of --reps calls on --sets rotating buffer sets, so that no call finds its input in the Infinity Cache.

Per row: microseconds and the fraction of the byte floor against 8 TB/s -- count only: the planes read once; pack: the
planes read twice plus 4 + (element size) bytes an entry written; unpack: the planes written once plus the entries read.
The same run times, ALTERNATED call by call with pack,
  * the yardstick: dwt_hip_bands_apply_batch with SCALE (by 1) on every slot of a float batch of the same shape, the
    library's one-pass in-place kernel, 8 bytes per sample;
and, with a host clock around work that ends synchronised (median of max(5, reps / 5)),
  * the route without this feature: the planes copied to pinned host memory;
  * the route with it: count to a host array (the sizing call), pack, and the streams and offsets copied to pinned memory.
Every row states its number of calls.

    python scripts/sparse_timing.py [--reps 100] [--sets 2] [--out profiles/sparse_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdwt_amd as dwt  # noqa: E402
from libdwt_amd import quant as Q  # noqa: E402
from libdwt_amd import sparse as S  # noqa: E402

PEAK = 8e12
LEVELS = 5
WORDS = 3 * LEVELS + 2
SHAPES = (("64x4096^2", 64, 4096, 4096), ("8192^2", 1, 8192, 8192))
BASE_STEP = 1.0 / 128


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def walled(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def stats(us):
    return {"us": round(float(np.median(us)), 1), "us_min": round(float(np.min(us)), 1), "us_p90": round(float(np.percentile(us, 90)), 1)}


def row(case, what, nbytes, us, **more):
    floor_us = nbytes / PEAK * 1e6
    r = dict({"case": case, "what": what, "bytes": nbytes, "calls": len(us)}, **stats(us), byte_floor_us=round(floor_us, 1),
             fraction_of_floor=round(floor_us / float(np.median(us)), 4), TB_per_s=round(nbytes / float(np.median(us)) * 1e-6, 3), **more)
    print(json.dumps(r), flush=True)
    return r


def plain(case, what, us, **more):
    r = dict({"case": case, "what": what, "calls": len(us)}, **stats(us), **more)
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


def inputs(kind, coef, batch, w, h):
    """the planes of one flow, per set -> (element type, torch dtype, list of planes)"""
    if kind == "int16 indices, base step 1/128":
        steps = Q.quant_steps(dwt.CDF97_S, LEVELS, BASE_STEP)
        out = [torch.empty((batch, h, w), dtype=torch.int16, device="cuda") for _ in coef]
        for c, q in zip(coef, out):
            Q.quantize_batch(Q.S, c, 4 * w * h, 4 * w, Q.I16, q, 2 * w * h, 2 * w, batch, w, h, LEVELS, steps)
        return S.I16, torch.int16, out
    keep = w * h // (100 if "1 %" in kind else 10)
    out = [c.clone() for c in coef]
    for c in out:
        dwt.keep_largest_batch(c, 4 * w * h, batch, 1, 0, 4 * w, w, h, keep, LEVELS)
    return S.F32, torch.float32, out


def measure(reps, sets):
    rows = []
    ns = 3 * LEVELS + 1
    scale_ops, scale_params = ["scale"] * ns, [1.0] * ns
    few = max(5, reps // 5)
    for name, batch, w, h in SHAPES:
        n = batch * w * h
        coef = coefficients(batch, w, h, sets)
        scale = lambda k: dwt.bands_apply_batch(coef[k], 4 * w * h, batch, 4 * w, w, h, LEVELS, scale_ops, scale_params)
        for kind in ("int16 indices, base step 1/128", "binary32 coefficients, keep_largest 1 %", "binary32 coefficients, keep_largest 10 %"):
            etype, tdtype, planes = inputs(kind, coef, batch, w, h)
            es = S.ELEM_BYTES[etype]
            strides = (es * w * h, es * w)
            frames = (batch, w, h)
            case = "%s, %s" % (name, kind)
            assert S.sparse_route(etype, planes[0], *strides, *frames) == 1
            totals = [S.count_batch(etype, p, *strides, *frames, LEVELS)[:, -1].astype(np.int64) for p in planes]
            cap, entries = max(int(t.max()) for t in totals), int(totals[0].sum())  # (the floors below: the entries of set 0)
            share = {"entries": entries, "nonzero_share": round(entries / n, 5), "stream_stride": cap}
            pos = torch.empty((batch, cap), dtype=torch.int32, device="cuda")
            val = torch.empty((batch, cap), dtype=tdtype, device="cuda")
            off = torch.empty((batch, WORDS), dtype=torch.int32, device="cuda")
            back = [torch.empty((batch, h, w), dtype=tdtype, device="cuda") for _ in range(sets)]
            count = lambda k: S.count_batch(etype, planes[k], *strides, *frames, LEVELS, off)
            pack = lambda k: S.pack_batch(etype, planes[k], *strides, *frames, LEVELS, pos, val, cap, off)
            unpack = lambda k: S.unpack_batch(etype, pos, val, cap, off.data_ptr() + 4 * (WORDS - 1), WORDS, back[k], *strides, *frames)
            ibits = torch.int16 if es == 2 else torch.int32
            for k in range(sets):  # warm-up; does the round trip give the planes' bits back (a -0.0 would not come back)
                count(k), pack(k), unpack(k), scale(k)
                torch.cuda.synchronize()
                share["round_trip_same_bits"] = share.get("round_trip_same_bits", True) and bool(torch.equal(back[k].view(ibits), planes[k].view(ibits)))
            us_p, us_s = [], []
            for rep in range(reps):
                us_p.append(timed(lambda: pack(rep % sets)))
                us_s.append(timed(lambda: scale(rep % sets)))
            rp = row(case, "pack (3 launches)", 2 * es * n + (4 + es) * entries, us_p, **share)
            rs = row(case, "yardstick: bands_apply_batch SCALE on the float batch of this shape, in place", 8 * n, us_s)
            rows += [rp, rs, {"case": case, "what": "pack over the yardstick (medians)", "ratio": round(rp["us"] / rs["us"], 4)}]
            print(json.dumps(rows[-1]), flush=True)
            rows.append(row(case, "count only (2 launches)", es * n, [timed(lambda: count(rep % sets)) for rep in range(reps)]))
            rows.append(row(case, "unpack (2 launches)", es * n + (4 + es) * entries, [timed(lambda: unpack(rep % sets)) for rep in range(reps)]))
            # across PCIe, with a host clock: the planes; against count + pack + the streams
            host = torch.empty((batch, h, w), dtype=tdtype).pin_memory()
            host.copy_(planes[0], non_blocking=True)
            us = [walled(lambda: host.copy_(planes[0], non_blocking=True)) for _ in range(few)]
            rows.append(plain(case, "without the streams: the planes to pinned host memory", us, bytes=es * n, GB_per_s=round(es * n / float(np.median(us)) * 1e-3, 2)))
            del host
            hpos, hval = torch.empty((batch, cap), dtype=torch.int32).pin_memory(), torch.empty((batch, cap), dtype=tdtype).pin_memory()

            def through(k):
                t = S.count_batch(etype, planes[k], *strides, *frames, LEVELS)  # host offsets: the sizing call, ends synchronised
                c = int(t[:, -1].max())
                assert c <= cap
                S.pack_batch(etype, planes[k], *strides, *frames, LEVELS, pos, val, cap, off)
                hpos[:, :c].copy_(pos[:, :c], non_blocking=True)
                hval[:, :c].copy_(val[:, :c], non_blocking=True)

            through(0)
            us = [walled(lambda: through(rep % sets)) for rep in range(few)]
            rows.append(plain(case, "with them: count to the host, pack, positions and values to pinned host memory", us, bytes=(4 + es) * batch * cap))
            del hpos, hval, pos, val, off, back, planes
            torch.cuda.empty_cache()
        del coef
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    res = {"device": dwt.device_name(), "reps": a.reps, "sets": a.sets, "peak_Bps": PEAK, "levels": LEVELS, "base_step": BASE_STEP,
           "tile_samples": S.TILE_SAMPLES, "rows": measure(a.reps, a.sets)}
    dwt.dwt_util_finish()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
