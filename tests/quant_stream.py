"""The quantizer on a busy caller's stream, run as a process of its own by tests/test_hip_quant.py: the cases below go
through the harness of tests/stream_cases.py -- a warm-up on the idle stream, then once on a non-blocking stream behind a
bounded delay, the true input reaching its buffer only behind that delay.  The result must be the model's bits
(tests/quant_model.py), the entries classified async must have queued their work without waiting for the stream, and the
launch count must be that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import quant_model as qm
import stream_cases as sc

_STATS = sc.SYNC("the band counters are read back and folded on the host")
KINDS = {"quantize_batch": sc.ASYNC, "quantize_batch[stats]": _STATS, "dequantize_batch": sc.ASYNC, "codeblock_bitplanes_batch": sc.ASYNC}
BATCH, SIZE_X, SIZE_Y, LEVELS = 3, 72, 40, 3
SLOTS = 3 * LEVELS + 1
CB = (3, 2)


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def table():
    return np.random.default_rng(9500).uniform(0.05, 2.0, SLOTS).astype(np.float32)


def coefficients(seed):
    return np.random.default_rng(9600 + seed).normal(0, 30, (BATCH, SIZE_Y, SIZE_X)).astype(np.float32)


def indices(seed):
    return np.random.default_rng(9700 + seed).integers(-3000, 3001, (BATCH, SIZE_Y, SIZE_X)).astype(np.int16)


def cases():
    from libdwt_amd import quant as Q

    f32, i16 = (4 * SIZE_X * SIZE_Y, 4 * SIZE_X), (2 * SIZE_X * SIZE_Y, 2 * SIZE_X)
    frames = (BATCH, SIZE_X, SIZE_Y, LEVELS)
    steps = table()
    total = int(qm.codeblock_layout(SIZE_X, SIZE_Y, LEVELS, *CB)[0][-1])
    out = []
    for wide in (1, 0):
        opts = {"quant_wide": wide}
        out.append(Case("quantize_batch f32 int16 quant_wide %d" % wide, "quantize_batch",
                        lambda seed: {"coef": coefficients(seed), "index": np.full((BATCH, SIZE_Y, SIZE_X), -77, np.int16)},
                        lambda dwt, D, host: Q.quantize_batch(Q.S, D["coef"], *f32, Q.I16, D["index"], *i16, *frames, steps),
                        lambda b: {"coef": b["coef"], "index": qm.quantize_frames(b["coef"], steps, LEVELS, qm.I16)[0], "ret": None},
                        same=sc.same_floats, options=opts))
        out.append(Case("dequantize_batch int16 f32 quant_wide %d" % wide, "dequantize_batch",
                        lambda seed: {"coef": np.full((BATCH, SIZE_Y, SIZE_X), -7.5, np.float32), "index": indices(seed)},
                        lambda dwt, D, host: Q.dequantize_batch(Q.I16, D["index"], *i16, Q.S, D["coef"], *f32, *frames, steps, r=0.5),
                        lambda b: {"coef": qm.dequantize_frames(b["index"], steps, LEVELS, 0.5, qm.S), "index": b["index"], "ret": None},
                        same=sc.same_floats, options=opts))
    out.append(Case("quantize_batch f32 int16 with counters", "quantize_batch[stats]",
                    lambda seed: {"coef": coefficients(seed), "index": np.full((BATCH, SIZE_Y, SIZE_X), -77, np.int16)},
                    lambda dwt, D, host: Q.quantize_batch(Q.S, D["coef"], *f32, Q.I16, D["index"], *i16, *frames, steps, stats=True),
                    lambda b: dict(zip(("index", "ret"), qm.quantize_frames(b["coef"], steps, LEVELS, qm.I16)), coef=b["coef"]),
                    same=sc.same_floats, check_ret=np.array_equal))
    out.append(Case("codeblock_bitplanes_batch int16 8 x 4", "codeblock_bitplanes_batch",
                    lambda seed: {"index": indices(seed), "planes": np.full((BATCH, total), 99, np.uint8)},
                    lambda dwt, D, host: Q.codeblock_bitplanes_batch(Q.I16, D["index"], *i16, *frames, *CB, D["planes"], total),
                    lambda b: {"index": b["index"], "planes": qm.codeblock_bitplanes(b["index"], LEVELS, *CB), "ret": None}))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # The harness is driven through two names of tests/stream_cases.py that are not part of its interface: family_cases()
    # serves a family from the cache _CASES, and Harness.run_once restores a case's options from DEFAULT_OPTIONS.  Both are
    # set here for this process alone; if either is renamed there, the assertions below say so.
    assert isinstance(getattr(sc, "_CASES", None), dict) and isinstance(getattr(sc, "DEFAULT_OPTIONS", None), dict), "stream_cases.py changed"
    sc.DEFAULT_OPTIONS = dict(sc.DEFAULT_OPTIONS, quant_wide=1)
    sc._CASES["quant"] = cases()
    assert sc.family_cases("quant") is sc._CASES["quant"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("quant")
    print("quant: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
    h.torch.cuda.synchronize()
    h.dwt.dwt_util_finish()
    if h.failures:
        print("%d FAILURES" % len(h.failures))
        for f in h.failures:
            print(" ", f)
        return 1
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
