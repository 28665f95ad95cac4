"""Timing of the pixel front end (dwt_hip_pixels_to_planes_batch / dwt_hip_planes_to_pixels_batch) on the
shapes of the workload: 64 interleaved RGB8 pictures of 4096^2 and one of 8192^2, to int16 planes with the RCT and to
binary32 planes with the ICT, both directions.  Device events around every call, a warm-up round, then the median of
--reps calls on --sets rotating buffer pairs, so that no call finds its input in the Infinity Cache.

Per row: microseconds and the fraction of the byte floor -- the pixels' bytes plus the planes' bytes, each crossing once,
against 8 TB/s.  The same run times
  * the yardstick: k_strided_move (dwt_strided.hip), the library's existing kernel of the same kind -- one element per
    lane, gather or scatter -- inside a strided dwt_hip_transform2d call of about as many bytes.  No public entry runs it
    alone, so a child process makes the calls under `rocprofv3 --kernel-trace` and the kernel's own durations are read from
    the trace (--no-yardstick leaves it out);
  * the route that exists without the front end: the planes widened on the host and copied from pinned memory
    (hipMemcpyAsync, one 8192^2 picture: 6 or 12 bytes per pixel against the 3 of the pixels themselves).

    python scripts/pixels_timing.py [--reps 100] [--sets 2] [--out profiles/pixels_timing.json]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch  # first: the library then shares torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libdwt_amd as dwt  # noqa: E402
from libdwt_amd import pixels as P  # noqa: E402

PEAK = 8e12
SHAPES = (("64x4096^2", 64, 4096, 4096), ("8192^2", 1, 8192, 8192))
ROUTES = (("rgb8 -> int16, RCT", P.I16, P.RCT, torch.int16, 2), ("rgb8 -> binary32, ICT", P.S, P.ICT, torch.float32, 4))
STRIDED = ((8192, 8192), (32768, 32768))  # the yardstick's images: floats 8 bytes apart


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(us):
    return {"us": round(float(np.median(us)), 1), "us_min": round(float(np.min(us)), 1), "us_p90": round(float(np.percentile(us, 90)), 1)}


def conversions(reps, sets):
    rows = []
    for name, batch, w, h in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(25)
        pix = [torch.randint(0, 256, (batch, h, w, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
        for route, plane, colour, dt, es in ROUTES:
            planes = [torch.empty((batch * 3, h, w), dtype=dt, device="cuda") for _ in range(sets)]
            back = torch.empty_like(pix[0])
            args = lambda p, q: (P.U8, p, 3 * w * h, 3 * w, 3, 1, batch, 3, P.RGB, 8, 128, 1.0, colour, plane, q, es * w * h, es * w, w, h)
            assert P.pixels_route(P.U8, False, pix[0], 3 * w * h, 3 * w, 3, 1, batch, 3, plane, planes[0], es * w * h, es * w, w, h) == P.WIDE_PIX | P.WIDE_PLANES
            for k in range(sets):  # warm-up; the planes the inverse calls read
                P.pixels_to_planes_batch(*args(pix[k], planes[k]))
            P.planes_to_pixels_batch(*args(back, planes[0]))
            torch.cuda.synchronize()
            assert torch.equal(back, pix[0]), "the round trip changed pixels"
            nbytes = batch * w * h * 3 * (1 + es)
            for inverse in (False, True):
                f = P.planes_to_pixels_batch if inverse else P.pixels_to_planes_batch
                us = [timed(lambda k=rep % sets: f(*args(back if inverse else pix[k], planes[k]))) for rep in range(reps)]
                floor_us = nbytes / PEAK * 1e6
                rows.append(dict({"case": name, "route": route, "dir": "planes to pixels" if inverse else "pixels to planes", "bytes": nbytes},
                                 **stats(us), byte_floor_us=round(floor_us, 1), fraction_of_floor=round(floor_us / float(np.median(us)), 4),
                                 TB_per_s=round(nbytes / float(np.median(us)) * 1e-6, 3)))
                print(json.dumps(rows[-1]), flush=True)
            del planes, back
            torch.cuda.empty_cache()
        del pix
        torch.cuda.empty_cache()
    return rows


def host_route(reps):
    """today's route: planes widened on the host, copied from pinned memory; and the pixels' own bytes the same way"""
    rows = []
    n = 8192 * 8192 * 3
    for what, bytes_per_sample in (("rgb8 pixels (the front end's upload)", 1), ("host-widened int16 planes", 2), ("host-widened binary32 planes", 4)):
        host = torch.empty(n * bytes_per_sample, dtype=torch.uint8).pin_memory()
        dev = torch.empty(n * bytes_per_sample, dtype=torch.uint8, device="cuda")
        dev.copy_(host, non_blocking=True)
        torch.cuda.synchronize()
        us = [timed(lambda: dev.copy_(host, non_blocking=True)) for _ in range(max(5, reps // 5))]
        rows.append(dict({"case": "8192^2", "copy": what, "bytes": n * bytes_per_sample}, **stats(us),
                         GB_per_s=round(n * bytes_per_sample / float(np.median(us)) * 1e-3, 2)))
        print(json.dumps(rows[-1]), flush=True)
        del host, dev
    return rows


def yardstick_child(reps):
    """strided dwt_hip_transform2d calls (one level): each packs the source and the destination and spreads the result"""
    import ctypes as C

    dwt.dwt_util_init()
    dwt.use_torch_stream()
    for w, h in STRIDED:
        img = torch.zeros((h, 2 * w), dtype=torch.float32, device="cuda")
        for _ in range(reps + 1):
            j = C.c_int(1)
            rc = dwt.lib.dwt_hip_transform2d(dwt.WAVELET_ID["cdf53_s"], 0, img.data_ptr(), img.data_ptr(), 8 * w, 8, w, h, w, h, C.byref(j), 0, 0)
            assert rc == 0, dwt.last_error()
        torch.cuda.synchronize()
        del img
        torch.cuda.empty_cache()
    dwt.dwt_util_finish()


def yardstick(reps):
    """k_strided_move's durations from a kernel trace of yardstick_child, by grid size (one per image size) and direction"""
    tool = shutil.which("rocprofv3")
    if not tool:
        return [{"yardstick": "not measured: rocprofv3 is not installed"}]
    out = tempfile.mkdtemp(prefix="pixels_yardstick_")
    found = {}
    try:
        run = subprocess.run([tool, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
                              "--yardstick-child", "--reps", str(reps)], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
        if run.returncode:
            return [{"yardstick": "not measured: the traced run ended with status %d: %s" % (run.returncode, run.stderr[-300:])}]
        for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    if "k_strided_move" in r["Kernel_Name"]:
                        key = (r["Kernel_Name"], int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"]))
                        found.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    rows = []
    sizes = sorted({k[1] for k in found})
    for (kernel, grid), us in sorted(found.items()):
        w, h = STRIDED[sizes.index(grid)] if len(sizes) == len(STRIDED) else (0, 0)
        us = us[len(us) // (reps + 1):]  # (the first call's launches: cold)
        useful, touched = 8 * w * h, 12 * w * h  # 4 B read + 4 B written per element; the gather touches both floats of every pair
        rows.append(dict({"kernel": kernel, "w": w, "h": h, "launches": len(us), "bytes_moved": useful, "bytes_touched": touched}, **stats(us),
                         fraction_of_floor_moved=round(useful / PEAK * 1e6 / float(np.median(us)), 4),
                         fraction_of_floor_touched=round(touched / PEAK * 1e6 / float(np.median(us)), 4)))
        print(json.dumps(rows[-1]), flush=True)
    return rows or [{"yardstick": "not measured: no k_strided_move dispatch in the trace"}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixels_timing.json"))
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--yardstick-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.yardstick_child:
        return yardstick_child(a.reps)
    dwt.dwt_util_init()
    dwt.use_torch_stream()
    res = {"device": dwt.device_name(), "reps": a.reps, "sets": a.sets, "peak_Bps": PEAK, "pixels_per_lane": P.PIXELS_PER_LANE,
           "conversions": conversions(a.reps, a.sets), "host_route": host_route(a.reps)}
    dwt.dwt_util_finish()
    res["k_strided_move"] = [{"yardstick": "left out (--no-yardstick)"}] if a.no_yardstick else yardstick(max(3, a.reps // 10))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
