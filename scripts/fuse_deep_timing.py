#!/usr/bin/env python3
"""fuse_deep 0 against 2 in one process, on buffers from dwt_hip_alloc_batch, the whole J = 5 call.
Phase A: the candidates of the deeper pair's launch (ring, direction, height) set by hand, untuned, against the untuned
level-by-level tail.  Phase B: as the benchmark runs it (dwt_hip_tune for either setting), fuse_deep 0 / 2 / 1.
usage: scripts/fuse_deep_timing.py NB N [phases: A, B, C]   (writes bench_outputs/fuse_deep/NBxN.json; profiles/fuse_deep_summary.md)"""
import json, os, statistics as st, sys, time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import libdwt_amd as dwt

nb, n = int(sys.argv[1]), int(sys.argv[2])
phases = sys.argv[3] if len(sys.argv) > 3 else "AB"
J, K, ROUNDS, DROP = 5, 5, 8, 2
dev = torch.device("cuda:0")
out_dir = "bench_outputs/fuse_deep"
os.makedirs(out_dir, exist_ok=True)


def raw_tensor(ptr, shape):
    class _Dev:
        pass
    o = _Dev()
    o.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 3, "strides": None}
    return torch.as_tensor(o, device=dev)


dwt.dwt_util_init()
dwt.use_torch_stream()
t0 = time.perf_counter()
p_src, p_dst = dwt.alloc_batch("cdf97_s", nb, n, n, J)
print("alloc_batch %.1f s" % (time.perf_counter() - t0), dwt.alloc_batch_note(), dwt.alloc_batch_report(), flush=True)
src, dst = raw_tensor(p_src, (nb, n, n)), raw_tensor(p_dst, (nb, n, n))
gen = torch.Generator(device=dev)
for i in range(nb):
    gen.manual_seed(1234 + i)
    torch.rand((n, n), generator=gen, out=src[i])
torch.cuda.synchronize()
img_bytes = n * n * 4
DEFAULTS = {"fuse_deep": 1, "fuse01_ring": 0, "fuse01_updown": -1, "tile_pairs": 0}


def call(d=dst):
    assert dwt.transform2d_batch("cdf97_s", 0, src, d, img_bytes, nb, n * 4, n, n, J) == J


def setopts(o):
    for k, v in {**DEFAULTS, **o}.items():
        if dwt.get_option(k) != v:
            dwt.set_option(k, v)


# ---- the bits first: fuse_deep 0 against 2 (rule) and against every candidate, the whole batch, on the device ----
ref = torch.empty((nb, n, n), device=dev, dtype=torch.float32)
got = torch.empty((nb, n, n), device=dev, dtype=torch.float32)
setopts({"fuse_deep": 0})
before = dwt.get_option("stat_launches")
call(ref)
print("fuse_deep 0: launches", dwt.get_option("stat_launches") - before, "deep", dwt.get_option("fuse_deep_last"), flush=True)
CANDS = [{"fuse_deep": 2, "fuse01_ring": ring, "fuse01_updown": ud, "tile_pairs": tp} for ring in (8, 16) for ud in (0, 1) for tp in (64, 32, 128)]
equal = {}
for o in [{"fuse_deep": 2}, {"fuse_deep": 1}] + CANDS:
    setopts(o)
    got.fill_(7.0)
    before = dwt.get_option("stat_launches")
    call(got)
    torch.cuda.synchronize()
    name = json.dumps(o, sort_keys=True)
    equal[name] = {"equal_words": bool(torch.equal(got.view(torch.int32), ref.view(torch.int32))),
                   "launches": dwt.get_option("stat_launches") - before, "deep": dwt.get_option("fuse_deep_last")}
    print("bits", name, equal[name], flush=True)
del ref, got
torch.cuda.empty_cache()
setopts({})


def measure(variants, tag):
    """variants: {name: options}.  Rounds of K profiled calls (per-level timer) and K calls timed by events, per variant;
    alternated within a round, the order reversed every other round; DROP rounds discarded."""
    names = list(variants)
    rec = {v: {"levels_ms": [], "step_ms": []} for v in names}
    for r in range(ROUNDS):
        order = names if r % 2 == 0 else names[::-1]
        for v in order:
            setopts(variants[v])
            call()
            dwt.prof_enable(2)
            for _ in range(K):
                call()
            lv, cnt = dwt.prof_read_levels(8)
            dwt.prof_enable(0)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(K + 1)]
            ev[0].record()
            for i in range(K):
                call()
                ev[i + 1].record()
            torch.cuda.synchronize()
            if r >= DROP:
                rec[v]["levels_ms"].append(lv[:J])
                rec[v]["step_ms"] += [ev[i].elapsed_time(ev[i + 1]) for i in range(K)]
        print(tag, "round", r, flush=True)
    setopts({})
    res = {}
    for v in names:
        L = np.array(rec[v]["levels_ms"]) * 1e3  # us, rounds x levels
        tail23 = L[:, 2] + L[:, 3]
        s = rec[v]["step_ms"]
        res[v] = {"options": variants[v],
                  "level_us_median": [round(float(x), 1) for x in np.median(L, axis=0)],
                  "l2_plus_l3_us": {"median": round(float(np.median(tail23)), 1), "min": round(float(tail23.min()), 1), "max": round(float(tail23.max()), 1)},
                  "fused01_us": {"median": round(float(np.median(L[:, 0])), 1), "min": round(float(L[:, 0].min()), 1), "max": round(float(L[:, 0].max()), 1)},
                  "step_ms": {"median": round(st.median(s), 4), "min": round(min(s), 4), "max": round(max(s), 4), "n": len(s)},
                  "raw": rec[v]}
        print("%s %-28s levels us %s  L2+L3 %.1f (%.1f-%.1f)  step %.4f (%.4f-%.4f) ms" % (
            tag, v, res[v]["level_us_median"], res[v]["l2_plus_l3_us"]["median"], res[v]["l2_plus_l3_us"]["min"], res[v]["l2_plus_l3_us"]["max"],
            res[v]["step_ms"]["median"], res[v]["step_ms"]["min"], res[v]["step_ms"]["max"]), flush=True)
    return res


result = {"batch": nb, "size": n, "levels": J, "calls_per_round": K, "rounds_kept": ROUNDS - DROP, "bits": equal,
          "placement": dwt.alloc_batch_report()}
if "A" in phases:
    variants = {"levels": {"fuse_deep": 0}}
    for o in CANDS:
        variants["r%d u%d p%d" % (o["fuse01_ring"], o["fuse01_updown"], o["tile_pairs"])] = o
    result["A_untuned_candidates"] = measure(variants, "A")
if "C" in phases:  # nothing tuned: the rule of the deeper pair against the levels' own rule
    result["C_untuned_rule"] = measure({"fuse_deep 0": {"fuse_deep": 0}, "fuse_deep 1": {"fuse_deep": 1}}, "C")
if "B" in phases:
    setopts({"fuse_deep": 0})
    dwt.tune("cdf97_s", 0, src, dst, img_bytes, nb, n * 4, n, n, J)
    setopts({"fuse_deep": 2})
    dwt.tune("cdf97_s", 0, src, dst, img_bytes, nb, n * 4, n, n, J)
    print("tile cache", dwt.get_option("tile_cache_size"), flush=True)
    result["B_tuned"] = measure({"fuse_deep 0": {"fuse_deep": 0}, "fuse_deep 2": {"fuse_deep": 2}, "fuse_deep 1": {"fuse_deep": 1}}, "B")
json.dump(result, open("%s/%dx%d%s.json" % (out_dir, nb, n, "" if phases == "AB" else "_" + phases), "w"), indent=1)
dwt.lib.dwt_hip_free(p_src)
dwt.lib.dwt_hip_free(p_dst)
dwt.dwt_util_finish()
print("done", flush=True)
