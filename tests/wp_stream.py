"""The wavelet packet entries on a busy caller's stream, run as a process of its own by tests/test_hip_wp.py: the cases
below go through the harness of tests/stream_cases.py -- a warm-up on the idle stream, then once on a non-blocking stream
behind a bounded delay, the true input reaching its buffer only behind that delay.  The result must be the model's
bits (tests/wp_model.py; the feature entries on inputs whose sums are exact, against features_model.seq32_band); a transform entry must have queued its work without waiting for the stream; the launch count must be
that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import stream_cases as sc
import wp_model as wp

F32 = np.float32
RECORDS = sc.SYNC("the per-node records are read back and finished on the host")
KINDS = {"wp1d_batch": sc.ASYNC, "wp2d_batch": sc.ASYNC, "wp_features1d_batch": RECORDS, "wp_features2d_batch": RECORDS}
N_LINES, N, LEVELS_1D = 5, 1000, 6
BATCH, SIZE_X, SIZE_Y, LEVELS_2D = 2, 130, 66, 3


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def lines(seed):
    return wp.make_input(9100 + seed, "normal", N_LINES, N)


def images(seed):
    return np.stack([wp.make_input(9200 + 10 * seed + b, "normal", SIZE_Y, SIZE_X) for b in range(BATCH)])


def sentinel(shape):
    return np.full(shape, F32(-7.5), F32)


def balanced(rng, shape, spans):
    """values of {-3 .. 3} with every span summing to exactly 0 (pairs x, -x, shuffled), one span all zero: the class of
    tests/test_hip_features.py's `balanced`, whose sums are exact in every order, so that the double sums of the kernels and
    the sequential float32 sums of features_model.seq32_band give the same bits"""
    a = np.zeros(shape, F32)
    for k, sl in enumerate(spans):
        n = a[sl].size
        half = rng.integers(-3, 4, n // 2).astype(F32)
        v = np.concatenate([half, -half, np.zeros(n % 2, F32)])
        if k == 1:
            v[:] = 0
        a[sl] = rng.permutation(v).reshape(a[sl].shape)
    return a


def node_features(a, spans, level):
    """every feature of fm.NAMES of every span, one block of len(spans) floats per feature: features_model.seq32_band on
    the span's values in row order, j = level, p = 2"""
    import features_model as fm

    per = [fm.seq32_band(np.ascontiguousarray(a[sl], dtype=F32).reshape(-1), level, 2.0) for sl in spans]
    return np.array([q[n] for n in fm.NAMES for q in per], F32)


def same_fv(got, want):
    """as the feature cases of tests/stream_cases.py: the median by value, everything else by bits, NaN == NaN"""
    import features_model as fm

    nb = want.shape[1] // len(fm.NAMES)
    med = slice(fm.NAMES.index("med") * nb, (fm.NAMES.index("med") + 1) * nb)
    rest = np.ones(want.shape[1], bool)
    rest[med] = False
    return got.shape == want.shape and np.array_equal(got[:, med], want[:, med]) and sc.same_floats(
        np.ascontiguousarray(got[:, rest]), np.ascontiguousarray(want[:, rest]))


def cases():
    from libdwt_amd import packets

    out = []
    for fused in (1, 0):
        opts = {"wp_fused": fused}
        for inverse in (False, True):
            f1 = wp.inv1d if inverse else wp.fwd1d
            out.append(Case("wp1d_batch cdf97_s %s wp_fused %d" % ("inverse" if inverse else "forward", fused), "wp1d_batch",
                            lambda seed: {"x": lines(seed)},
                            lambda dwt, P, host, inverse=inverse: packets.wp1d_batch(dwt.CDF97_S, inverse, P["x"], P["x"], 4 * N, 4, N_LINES, N, LEVELS_1D),
                            lambda b, f1=f1: {"x": f1("cdf97_s", b["x"], LEVELS_1D)}, same=sc.same_floats, options=opts))
            f2 = wp.inv2d if inverse else wp.fwd2d
            out.append(Case("wp2d_batch cdf53_s %s out of place wp_fused %d" % ("inverse" if inverse else "forward", fused), "wp2d_batch",
                            lambda seed: {"x": images(seed), "y": sentinel((BATCH, SIZE_Y, SIZE_X))},
                            lambda dwt, P, host, inverse=inverse: packets.wp2d_batch(dwt.CDF53_S, inverse, P["x"], P["y"], 4 * SIZE_X * SIZE_Y, BATCH,
                                                                                      4 * SIZE_X, 4, SIZE_X, SIZE_Y, LEVELS_2D),
                            lambda b, f2=f2: {"x": b["x"], "y": np.stack([f2("cdf53_s", a, LEVELS_2D) for a in b["x"]])},
                            same=sc.same_floats, options=opts))
    import features_model as fm

    lev1, lev2 = 4, 2
    n1, nx, ny = wp.nodes_recursive(N, lev1), wp.nodes_recursive(SIZE_X, lev2), wp.nodes_recursive(SIZE_Y, lev2)
    g1, g2 = wp.freq_order(lev1), wp.freq_order(lev2)
    names, nf = list(fm.NAMES), len(fm.NAMES)
    # the nodes in natural order (what an input is balanced over) and in frequency order (what the calls below return)
    nat1 = [np.s_[s:s + n] for s, n in n1]
    nat2 = [np.s_[sy:sy + h, sx:sx + w] for sy, h in ny for sx, w in nx]
    frq1 = [nat1[k] for k in g1]
    frq2 = [nat2[ky * len(nx) + kx] for ky in g2 for kx in g2]

    def make1(seed):
        rng = sc._rng(seed, "wp_features1d_batch")
        return {"x": np.stack([balanced(rng, (N,), nat1) for _ in range(N_LINES)]), "fv": sentinel((N_LINES, nf << lev1))}

    def make2(seed):
        rng = sc._rng(seed, "wp_features2d_batch")
        return {"x": np.stack([balanced(rng, (SIZE_Y, SIZE_X), nat2) for _ in range(BATCH)]), "fv": sentinel((BATCH, nf << (2 * lev2)))}

    def want1(b):
        return {"x": b["x"], "fv": np.stack([node_features(row, frq1, lev1) for row in b["x"]])}

    def want2(b):
        return {"x": b["x"], "fv": np.stack([node_features(a, frq2, lev2) for a in b["x"]])}

    out.append(Case("wp_features1d_batch frequency order", "wp_features1d_batch", make1,
                    lambda dwt, P, host: packets.wp_features1d_batch(names, P["x"], 4 * N, 4, N_LINES, N, lev1, packets.FREQUENCY, P["fv"], nf << lev1),
                    want1, same=sc.same_floats, same_for={"fv": same_fv}))
    out.append(Case("wp_features2d_batch frequency order", "wp_features2d_batch", make2,
                    lambda dwt, P, host: packets.wp_features2d_batch(names, P["x"], 4 * SIZE_X * SIZE_Y, BATCH, 4 * SIZE_X, SIZE_X, SIZE_Y, lev2,
                                                                      packets.FREQUENCY, P["fv"], nf << (2 * lev2)),
                    want2, same=sc.same_floats, same_for={"fv": same_fv}))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # The harness is driven through two names of tests/stream_cases.py that are not part of its interface: family_cases()
    # serves a family from the cache _CASES, and Harness.run_once restores a case's options from DEFAULT_OPTIONS.  Both are
    # set here for this process alone; if either is renamed there, the assertions below say so.
    assert isinstance(getattr(sc, "_CASES", None), dict) and isinstance(getattr(sc, "DEFAULT_OPTIONS", None), dict), "stream_cases.py changed"
    sc.DEFAULT_OPTIONS = dict(sc.DEFAULT_OPTIONS, wp_fused=1)
    sc._CASES["wp"] = cases()
    assert sc.family_cases("wp") is sc._CASES["wp"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("wp")
    print("wp: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
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
