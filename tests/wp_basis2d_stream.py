"""The 2-D best-basis and pruned-quadtree entries on a busy caller's stream, run as a process of its own by
tests/test_hip_wp_basis2d.py, in the style of tests/wp_basis_stream.py: the cases below go through the harness of
tests/stream_cases.py -- a warm-up on the idle stream, then once on a non-blocking stream behind a bounded delay, the true
input reaching its buffer only behind that delay.  Both device entries, on the fused route and under "wp_fused" = 0, must
have queued their work without waiting for the stream (nothing is read back: the selection runs on the device); the result
must be the model's (tests/wp_basis2d_model.py) and the launch count that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import stream_cases as sc
import wp_basis2d_model as qm
import wp_model as wp

F32 = np.float32
KINDS = {"wp_best2d_batch": sc.ASYNC, "wp_tree2d_batch": sc.ASYNC}
SIZE_Y, SIZE_X, LEVELS, BATCH = 150, 200, 3, 3
NQ = qm.nq(LEVELS)
WAVELET = "cdf97_s"
THRESHOLD = (qm.THRESHOLD, 1.0)  # exact counts: every table compares bit for bit
LOG_ENERGY = (qm.LOG_ENERGY, 0.0)  # rounding differs from the model's fsum: the tree and the coefficients compare


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def images(seed):
    return np.stack([qm.texture(9400 + 10 * seed + b, SIZE_Y, SIZE_X) for b in range(BATCH)])


def searched(x, cost):
    """-> (coefficients, trees as (batch, 16) uint32, totals, tables) of the model"""
    stages = qm.full_levels(WAVELET, x, LEVELS)
    c, _, _ = qm.cost_tables(cost[0], cost[1], stages, LEVELS)
    coef, trees, totals = np.empty_like(x), np.zeros((BATCH, qm.QTREE_WORDS), np.uint32), np.zeros(BATCH)
    for b in range(BATCH):
        tree, totals[b], _ = qm.select(c[b], LEVELS)
        trees[b] = tree
        for j, ky, kx, x0, y0, w, h in qm.leaves(SIZE_X, SIZE_Y, LEVELS, tree):
            coef[b, y0:y0 + h, x0:x0 + w] = stages[j][b, y0:y0 + h, x0:x0 + w]
    return coef, trees, totals, c


def cases():
    from libdwt_amd import packets

    wid = wp.WAVELET_ID[WAVELET]
    geom = (4 * SIZE_X * SIZE_Y, BATCH, 4 * SIZE_X, 4, SIZE_X, SIZE_Y, LEVELS)
    out = []
    for fused in (1, 0):
        opts = {"wp_fused": fused}

        def make_all(seed):
            return {"x": images(seed), "y": np.full((BATCH, SIZE_Y, SIZE_X), F32(-7.5), F32),
                    "tree": np.full((BATCH, qm.QTREE_WORDS), 0x5A5A5A5A, np.uint32), "total": np.full(BATCH, -7.5), "cost": np.full((BATCH, NQ), -7.5)}

        def want_all(b):
            coef, trees, totals, c = searched(b["x"], THRESHOLD)
            return {"x": b["x"], "y": coef, "tree": trees, "total": totals, "cost": c}

        out.append(Case("wp_best2d_batch threshold, every output, wp_fused %d" % fused, "wp_best2d_batch", make_all,
                        lambda dwt, P, host: packets.wp_best2d_batch(wid, THRESHOLD[0], THRESHOLD[1], P["x"], P["y"], *geom, tree=P["tree"],
                                                                     total=P["total"], node_cost=P["cost"]),
                        want_all, same=sc.same_floats, options=opts))

        def make_ip(seed):
            return {"x": images(seed), "tree": np.full((BATCH, qm.QTREE_WORDS), 0x5A5A5A5A, np.uint32)}

        def want_ip(b):
            coef, trees, _, _ = searched(b["x"], LOG_ENERGY)
            return {"x": coef, "tree": trees}

        out.append(Case("wp_best2d_batch log energy in place, wp_fused %d" % fused, "wp_best2d_batch", make_ip,
                        lambda dwt, P, host: packets.wp_best2d_batch(wid, LOG_ENERGY[0], LOG_ENERGY[1], P["x"], P["x"], *geom, tree=P["tree"]),
                        want_ip, same=sc.same_floats, options=opts))

        for inverse in (False, True):
            def make_tree(seed):
                x = images(seed)
                return {"x": x, "tree": searched(x, LOG_ENERGY)[1]}

            def want_tree(b, inverse=inverse):
                f = qm.inv_qtree if inverse else qm.fwd_qtree
                return {"x": np.stack([f(WAVELET, b["x"][i], LEVELS, b["tree"][i]) for i in range(BATCH)]), "tree": b["tree"]}

            out.append(Case("wp_tree2d_batch %s, per-image trees, wp_fused %d" % ("inverse" if inverse else "forward", fused), "wp_tree2d_batch",
                            make_tree,
                            lambda dwt, P, host, inverse=inverse: packets.wp_tree2d_batch(wid, inverse, P["x"], P["x"], *geom, P["tree"],
                                                                                           4 * qm.QTREE_WORDS),
                            want_tree, same=sc.same_floats, options=opts))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # as tests/wp_basis_stream.py: two names of tests/stream_cases.py that are not part of its interface, set for this process alone
    assert isinstance(getattr(sc, "_CASES", None), dict) and isinstance(getattr(sc, "DEFAULT_OPTIONS", None), dict), "stream_cases.py changed"
    sc.DEFAULT_OPTIONS = dict(sc.DEFAULT_OPTIONS, wp_fused=1)
    sc._CASES["wp_basis2d"] = cases()
    assert sc.family_cases("wp_basis2d") is sc._CASES["wp_basis2d"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("wp_basis2d")
    print("wp_basis2d: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
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
