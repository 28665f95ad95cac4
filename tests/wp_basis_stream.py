"""The best-basis and pruned-tree entries on a busy caller's stream, run as a process of its own by
tests/test_hip_wp_basis.py, in the style of tests/wp_stream.py: the cases below go through the harness of
tests/stream_cases.py -- a warm-up on the idle stream, then once on a non-blocking stream behind a bounded delay, the true
input reaching its buffer only behind that delay.  Both device entries, on the one-launch route and under "wp_fused" = 0,
must have queued their work without waiting for the stream (nothing is read back: the selection runs on the device); the
result must be the model's (tests/wp_basis_model.py) and the launch count that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import stream_cases as sc
import wp_basis_model as bm
import wp_model as wp

F32 = np.float32
KINDS = {"wp_best1d_batch": sc.ASYNC, "wp_tree1d_batch": sc.ASYNC}
N_LINES, N, LEVELS = 5, 1000, 6
NT = 2 << LEVELS
WAVELET = "cdf97_s"
THRESHOLD = (bm.THRESHOLD, 1.0)  # exact counts: every table compares bit for bit
SHANNON = (bm.SHANNON, 0.0)      # rounding differs from the model's fsum: the tree and the coefficients compare


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def lines(seed):
    return wp.make_input(9300 + seed, "normal", N_LINES, N)


def searched(x, cost):
    """-> (coefficients, trees as (lines, 32) uint32, totals, tables with the total at entry 0) of the model"""
    stages = bm.full_levels(WAVELET, x, LEVELS)
    c, _, _ = bm.cost_tables(cost[0], cost[1], stages, LEVELS)
    coef, trees, totals = np.empty_like(x), np.zeros((N_LINES, bm.TREE_WORDS), np.uint32), np.zeros(N_LINES)
    for y in range(N_LINES):
        tree, totals[y], _ = bm.select(c[y], LEVELS)
        trees[y] = tree
        for j, k, s, n in bm.leaves(N, LEVELS, tree):
            coef[y, s:s + n] = stages[j][y, s:s + n]
        c[y, 0] = totals[y]
    return coef, trees, totals, c


def cases():
    from libdwt_amd import packets

    wid = wp.WAVELET_ID[WAVELET]
    out = []
    for fused in (1, 0):
        opts = {"wp_fused": fused}

        def make_all(seed):
            return {"x": lines(seed), "y": np.full((N_LINES, N), F32(-7.5), F32), "tree": np.full((N_LINES, bm.TREE_WORDS), 0x5A5A5A5A, np.uint32),
                    "total": np.full(N_LINES, -7.5), "cost": np.full((N_LINES, NT), -7.5)}

        def want_all(b):
            coef, trees, totals, c = searched(b["x"], THRESHOLD)
            return {"x": b["x"], "y": coef, "tree": trees, "total": totals, "cost": c}

        out.append(Case("wp_best1d_batch threshold, every output, wp_fused %d" % fused, "wp_best1d_batch", make_all,
                        lambda dwt, P, host: packets.wp_best1d_batch(wid, THRESHOLD[0], THRESHOLD[1], P["x"], P["y"], 4 * N, 4, N_LINES, N, LEVELS,
                                                                     tree=P["tree"], total=P["total"], node_cost=P["cost"]),
                        want_all, same=sc.same_floats, options=opts))

        def make_ip(seed):
            return {"x": lines(seed), "tree": np.full((N_LINES, bm.TREE_WORDS), 0x5A5A5A5A, np.uint32)}

        def want_ip(b):
            coef, trees, _, _ = searched(b["x"], SHANNON)
            return {"x": coef, "tree": trees}

        out.append(Case("wp_best1d_batch shannon in place, wp_fused %d" % fused, "wp_best1d_batch", make_ip,
                        lambda dwt, P, host: packets.wp_best1d_batch(wid, SHANNON[0], SHANNON[1], P["x"], P["x"], 4 * N, 4, N_LINES, N, LEVELS,
                                                                     tree=P["tree"]),
                        want_ip, same=sc.same_floats, options=opts))

        for inverse in (False, True):
            def make_tree(seed):
                x = lines(seed)
                return {"x": x, "tree": searched(x, SHANNON)[1]}

            def want_tree(b, inverse=inverse):
                f = bm.inv_tree if inverse else bm.fwd_tree
                return {"x": np.concatenate([f(WAVELET, b["x"][y:y + 1], LEVELS, b["tree"][y]) for y in range(N_LINES)]), "tree": b["tree"]}

            out.append(Case("wp_tree1d_batch %s, per-line trees, wp_fused %d" % ("inverse" if inverse else "forward", fused), "wp_tree1d_batch",
                            make_tree,
                            lambda dwt, P, host, inverse=inverse: packets.wp_tree1d_batch(wid, inverse, P["x"], P["x"], 4 * N, 4, N_LINES, N, LEVELS,
                                                                                           P["tree"], 4 * bm.TREE_WORDS),
                            want_tree, same=sc.same_floats, options=opts))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # as tests/wp_stream.py: two names of tests/stream_cases.py that are not part of its interface, set for this process alone
    assert isinstance(getattr(sc, "_CASES", None), dict) and isinstance(getattr(sc, "DEFAULT_OPTIONS", None), dict), "stream_cases.py changed"
    sc.DEFAULT_OPTIONS = dict(sc.DEFAULT_OPTIONS, wp_fused=1)
    sc._CASES["wp_basis"] = cases()
    assert sc.family_cases("wp_basis") is sc._CASES["wp_basis"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("wp_basis")
    print("wp_basis: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
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
