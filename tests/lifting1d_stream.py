"""The user-defined lifting wavelets of line batches on a busy caller's stream, run as a process of its own by
tests/test_hip_lifting1d.py: the cases below go through the harness of tests/stream_cases.py -- a warm-up on the idle stream,
then once on a non-blocking stream behind a bounded delay, the true input reaching its buffer only behind that delay.  The
result must be the model's bits (tests/lifting1d_model.py), the entry -- classified async for device pointers -- must have
queued its work without waiting for the stream, and the launch count must be that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import lifting1d_model as l1
import lifting_model as lm
import stream_cases as sc

KINDS = {"lifting1d_batch": sc.ASYNC}
N_LINES, SIZE, LEVELS = 5, 600, 4
SENTINEL = 0xEEEEEEEE


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def lines(s, seed):
    rng = np.random.default_rng(9910 + seed)
    if s.type == lm.I32:
        return rng.integers(-(1 << 20), 1 << 20, (N_LINES, SIZE)).astype(np.int32)
    return rng.uniform(-1, 1, (N_LINES, SIZE)).astype(np.float32)


def sentinel(s):
    return np.full((N_LINES, SIZE), SENTINEL, np.uint32).view(s.dtype)


def cases():
    from libdwt_amd import lifting as L

    geom = (4 * SIZE, 4, N_LINES, SIZE)
    out = []
    for name in ("D4", "HAAR_INT"):
        s, sl = lm.builtin(name), L.builtin(name)
        for fused in (1, 0):
            opts = {"lifting_fused": fused}
            for inverse in (False, True):
                model = l1.inv1d if inverse else l1.fwd1d
                source = (lambda seed, s=s: l1.fwd1d(s, lines(s, seed), LEVELS)[0]) if inverse else (lambda seed, s=s: lines(s, seed))
                what = "%s %s lifting_fused %d" % (name, "inverse" if inverse else "forward", fused)
                out.append(Case("lifting1d_batch " + what, "lifting1d_batch",
                                lambda seed, s=s, source=source: {"x": source(seed), "y": sentinel(s)},
                                lambda dwt, D, host, sl=sl, inverse=inverse: L.lifting1d_batch(sl, inverse, D["x"], D["y"], *geom, LEVELS),
                                lambda b, s=s, model=model: {"x": b["x"], "y": model(s, b["x"], LEVELS)[0], "ret": LEVELS}, options=opts))
                out.append(Case("lifting1d_batch in place " + what, "lifting1d_batch",
                                lambda seed, source=source: {"x": source(seed)},
                                lambda dwt, D, host, sl=sl, inverse=inverse: L.lifting1d_batch(sl, inverse, D["x"], D["x"], *geom, LEVELS),
                                lambda b, s=s, model=model: {"x": model(s, b["x"], LEVELS)[0], "ret": LEVELS}, options=opts))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # The harness is driven through two names of tests/stream_cases.py that are not part of its interface, as
    # tests/lifting_stream.py drives it: family_cases() serves a family from the cache _CASES, and Harness.run_once restores a
    # case's options from DEFAULT_OPTIONS.  Both are set here for this process alone; if either is renamed there, the
    # assertions below say so.
    assert isinstance(getattr(sc, "_CASES", None), dict) and isinstance(getattr(sc, "DEFAULT_OPTIONS", None), dict), "stream_cases.py changed"
    sc.DEFAULT_OPTIONS = dict(sc.DEFAULT_OPTIONS, lifting_fused=1)
    sc._CASES["lifting1d"] = cases()
    assert sc.family_cases("lifting1d") is sc._CASES["lifting1d"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("lifting1d")
    print("lifting1d: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
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
