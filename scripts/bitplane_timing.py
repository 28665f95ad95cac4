"""Timing of the embedded bit-plane streams of code-blocks (dwt_hip_bitplane_pack_batch / dwt_hip_bitplane_unpack_batch;
DESIGN.md s36) on the shapes of the workload: 64 frames of 4096^2 and one of 8192^2, holding the int16 indices of the 5-level
float 9/7 coefficients of the library's test image under white noise (standard deviation 1/64) at three base steps -- 4, 1
and 0.5 standard deviations --, 64 x 64 code-blocks.  Device events around every
call, a warm-up round, then the median of --reps calls on --sets rotating buffer sets, so that no call finds its input in
the Infinity Cache.

Per row: microseconds and the fraction of the byte floor against 8 TB/s -- count only: the planes read once; pack: the
planes read twice plus the words written; unpack: the words read plus the planes written.  The same run times, ALTERNATED
call by call with pack,
  * the one-read yardstick: dwt_hip_codeblock_bitplanes_batch of the same planes, 2 bytes per sample;
  * dwt_hip_sparse_pack_batch of the same planes;
reports the stream bytes against the plane bytes; and, with a host clock around work that ends synchronised (median of
max(5, reps / 5)),
  * the route without this feature: the planes copied to pinned host memory;
  * the route with it: count to a host array (the sizing call), pack, and the words and offsets copied to pinned memory.
Every row states its number of calls.

    python scripts/bitplane_timing.py [--reps 100] [--sets 2] [--out profiles/bitplane_timing.json]"""
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
from libdwt_amd import bitplanes as BP  # noqa: E402
from libdwt_amd import quant as Q  # noqa: E402
from libdwt_amd import sparse as S  # noqa: E402

PEAK = 8e12
LEVELS = 5
CB = (6, 6)
SHAPES = (("64x4096^2", 64, 4096, 4096), ("8192^2", 1, 8192, 8192))
NOISE = 1.0 / 64  # sensor noise on the test image, which alone is smooth enough to leave 0.1 % of the indices nonzero
BASE_STEPS = (1.0 / 256, 1.0 / 64, 1.0 / 32)  # 4, 1 and 0.5 standard deviations of that noise


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
    """`sets` stacks of `batch` frames: the test image under white noise of NOISE standard deviation (every frame its own),
    transformed LEVELS levels on the device"""
    img = np.zeros((h, w), np.float32)
    dwt.lib.dwt_util_test_image_fill_s(img.ctypes.data, img.strides[0], 4, w, h, 0)
    one = torch.from_numpy(img).cuda()
    gen = torch.Generator(device="cuda").manual_seed(36)
    out = []
    for k in range(sets):
        src = (one * (1.0 + 0.25 * k)).unsqueeze(0).expand(batch, h, w).contiguous()
        src += torch.randn(src.shape, generator=gen, device="cuda") * NOISE
        dst = torch.empty_like(src)
        assert dwt.transform2d_batch(dwt.CDF97_S, False, src, dst, 4 * w * h, batch, 4 * w, w, h, LEVELS) == LEVELS
        out.append(dst)
        del src
    torch.cuda.synchronize()
    return out


def measure(reps, sets):
    rows = []
    few = max(5, reps // 5)
    for name, batch, w, h in SHAPES:
        n = batch * w * h
        coef = coefficients(batch, w, h, sets)
        strides = (2 * w * h, 2 * w)
        frames = (batch, w, h, LEVELS)
        blocks = int(BP.bands(w, h, LEVELS, *CB)[-1, 4])
        total = int(Q.codeblock_layout(w, h, LEVELS, *CB)[0][-1])
        assert total == blocks
        for base in BASE_STEPS:
            case = "%s, int16 indices, base step 1/%d" % (name, round(1 / base))
            steps = Q.quant_steps(dwt.CDF97_S, LEVELS, base)
            planes = [torch.empty((batch, h, w), dtype=torch.int16, device="cuda") for _ in coef]
            for c, q in zip(coef, planes):
                Q.quantize_batch(Q.S, c, 4 * w * h, 4 * w, Q.I16, q, *strides, batch, w, h, LEVELS, steps)
            totals = [BP.count_batch(BP.I16, p, *strides, *frames, *CB)[:, -1].astype(np.int64) for p in planes]
            cap, words_all = max(int(t.max()) for t in totals), int(totals[0].sum())  # (the floors below: the words of set 0)
            nonzero = int(torch.count_nonzero(planes[0]).item())
            share = {"words": words_all, "stream_bytes": 8 * words_all + 4 * batch * (blocks + 1), "plane_bytes": 2 * n,
                     "stream_over_planes": round((8 * words_all + 4 * batch * (blocks + 1)) / (2 * n), 4), "bits_per_sample": round(64 * words_all / n, 3),
                     "nonzero_share": round(nonzero / n, 5), "stream_stride": cap, "blocks_per_frame": blocks}
            words = torch.empty((batch, cap), dtype=torch.int64, device="cuda")
            off = torch.empty((batch, blocks + 1), dtype=torch.int32, device="cuda")
            back = [torch.empty((batch, h, w), dtype=torch.int16, device="cuda") for _ in range(sets)]
            bmap = torch.empty((batch, total), dtype=torch.uint8, device="cuda")
            s_tot = [S.count_batch(S.I16, p, *strides, batch, w, h, LEVELS)[:, -1].astype(np.int64) for p in planes]
            s_cap, entries = max(int(t.max()) for t in s_tot), int(s_tot[0].sum())
            pos = torch.empty((batch, s_cap), dtype=torch.int32, device="cuda")
            val = torch.empty((batch, s_cap), dtype=torch.int16, device="cuda")
            s_off = torch.empty((batch, 3 * LEVELS + 2), dtype=torch.int32, device="cuda")
            count = lambda k: BP.count_batch(BP.I16, planes[k], *strides, *frames, *CB, off)
            pack = lambda k: BP.pack_batch(BP.I16, planes[k], *strides, *frames, *CB, words, cap, off)
            unpack = lambda k: BP.unpack_batch(BP.I16, words, cap, off, back[k], *strides, *frames, *CB)
            yard = lambda k: Q.codeblock_bitplanes_batch(Q.I16, planes[k], *strides, batch, w, h, LEVELS, *CB, bmap, total)
            spack = lambda k: S.pack_batch(S.I16, planes[k], *strides, batch, w, h, LEVELS, pos, val, s_cap, s_off)
            for k in range(sets):  # warm-up; does the round trip give the planes back
                count(k), pack(k), unpack(k), yard(k), spack(k)
                torch.cuda.synchronize()
                share["round_trip_same_bits"] = share.get("round_trip_same_bits", True) and bool(torch.equal(back[k], planes[k]))
            us_p, us_y, us_s = [], [], []
            for rep in range(reps):
                us_p.append(timed(lambda: pack(rep % sets)))
                us_y.append(timed(lambda: yard(rep % sets)))
                us_s.append(timed(lambda: spack(rep % sets)))
            rp = row(case, "pack (3 launches)", 4 * n + 8 * words_all, us_p, **share)
            ry = row(case, "yardstick: codeblock_bitplanes_batch of the same planes (one read)", 2 * n, us_y)
            rs = row(case, "sparse_pack_batch of the same planes", 4 * n + 6 * entries, us_s, entries=entries, sparse_stream_bytes=6 * entries)
            rows += [rp, ry, rs, {"case": case, "what": "pack over the yardstick; pack over sparse pack (medians)", "ratio_yardstick": round(rp["us"] / ry["us"], 4),
                                  "ratio_sparse": round(rp["us"] / rs["us"], 4)}]
            print(json.dumps(rows[-1]), flush=True)
            rows.append(row(case, "count only (2 launches)", 2 * n, [timed(lambda: count(rep % sets)) for rep in range(reps)]))
            pack(0)
            rows.append(row(case, "unpack (1 launch)", 2 * n + 8 * words_all, [timed(lambda: unpack(rep % sets)) for rep in range(reps)]))
            # across PCIe, with a host clock: the planes; against count + pack + the words and offsets
            host = torch.empty((batch, h, w), dtype=torch.int16).pin_memory()
            host.copy_(planes[0], non_blocking=True)
            us = [walled(lambda: host.copy_(planes[0], non_blocking=True)) for _ in range(few)]
            rows.append(plain(case, "without the streams: the planes to pinned host memory", us, bytes=2 * n, GB_per_s=round(2 * n / float(np.median(us)) * 1e-3, 2)))
            del host
            hwords, hoff = torch.empty((batch, cap), dtype=torch.int64).pin_memory(), torch.empty((batch, blocks + 1), dtype=torch.int32).pin_memory()

            def through(k):
                t = BP.count_batch(BP.I16, planes[k], *strides, *frames, *CB)  # host offsets: the sizing call, ends synchronised
                assert int(t[:, -1].max()) <= cap
                BP.pack_batch(BP.I16, planes[k], *strides, *frames, *CB, words, cap, off)
                hwords.copy_(words, non_blocking=True)  # (whole, at the capacity: one contiguous copy)
                hoff.copy_(off, non_blocking=True)

            through(0)
            us = [walled(lambda: through(rep % sets)) for rep in range(few)]
            rows.append(plain(case, "with them: count to the host, pack, words and offsets to pinned host memory", us, bytes=8 * batch * cap + 4 * batch * (blocks + 1)))
            del hwords, hoff, words, off, back, planes, pos, val, s_off, bmap
            torch.cuda.empty_cache()
        del coef
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitplane_timing.json"))
    a = ap.parse_args()
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    res = {"device": dwt.device_name(), "reps": a.reps, "sets": a.sets, "peak_Bps": PEAK, "levels": LEVELS, "code_block_exponents": list(CB),
           "base_steps": list(BASE_STEPS), "noise_sigma": NOISE, "rows": measure(a.reps, a.sets)}
    dwt.dwt_util_finish()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
