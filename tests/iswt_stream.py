"""The stationary transforms of libdwt_amd.stationary on a busy caller's stream, run as a process of its own by
tests/test_hip_iswt.py: the cases below go through the harness of tests/stream_cases.py -- a warm-up on the idle stream, then
once on a non-blocking stream behind a bounded delay, the true input reaching its buffer only behind that delay.  The
result must be the model's bits (tests/iswt_model.py), the four entries must have queued their work without waiting for
the stream, and the launch count must be that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import iswt_model as im
import stream_cases as sc
import swt2d_model as m2
import swt_model as sm

KINDS = {"swt1d_batch": sc.ASYNC, "swt2d_batch": sc.ASYNC, "iswt1d_batch": sc.ASYNC, "iswt2d_batch": sc.ASYNC}
F32 = np.float32
LINES, N, L = 3, 64, 3  # the row shape of the swt family of tests/stream_cases.py
B, H2, W2, L2 = 2, 33, 40, 2  # ... and its image shape
CAN = np.array([0xDEADBEEF], np.uint32).view(F32)[0]


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def tables(n):
    ops = np.array([(im.SOFT, im.KEEP, im.HARD, im.SCALE)[i % 4] for i in range(n)], np.int32)
    return ops, np.array([0.3 if o != im.SCALE else -1.5 for o in ops], F32)


def cases():
    from libdwt_amd import stationary as st

    out = []
    for fused in (1, 0):
        for wv in sm.WAVELETS:
            def want(b, wv=wv):
                Lp, Hp = im.swt_levels(b["x"], wv, L)
                b["h"][:], b["l"][:] = Hp, Lp
                return b
            out.append(Case("swt1d_batch symmetric %s swt_fused %d" % (wv, fused), "swt1d_batch",
                            lambda s: {"x": sm.make_input(300 + s, "normal", LINES, N), "h": np.full((L, LINES, N), CAN, F32), "l": np.full((L, LINES, N), CAN, F32)},
                            lambda dwt, P, h, wv=wv: st.swt1d_batch(wv, P["x"], N * 4, 4, LINES, N, L, P["h"], P["l"], 2, LINES * N * 4, N * 4, border=st.BORDER_SYMMETRIC),
                            want, sc.same_floats, options={"swt_fused": fused}))
            ops, params = tables(L)

            def make_i(s, wv=wv):
                Lp, Hp = im.swt_levels(sm.make_input(310 + s, "normal", LINES, N), wv, L)
                return {"h": Hp, "l": Lp[-1].copy(), "y": np.full((LINES, N), CAN, F32)}

            def want_i(b, wv=wv, ops=ops, params=params):
                b["y"][:] = im.iswt_levels(b["l"], b["h"], wv, ops, params)
                return b
            out.append(Case("iswt1d_batch %s swt_fused %d" % (wv, fused), "iswt1d_batch", make_i,
                            lambda dwt, P, h, wv=wv, ops=ops, params=params: st.iswt1d_batch(wv, st.BORDER_SYMMETRIC, P["h"], P["l"], LINES * N * 4, N * 4, LINES, N, L, P["y"],
                                                                                             N * 4, ops=ops, params=params),
                            want_i, sc.same_floats, options={"swt_fused": fused}))
    plane = H2 * W2 * 4
    for fused in (1, 0):
        for wv in sm.WAVELETS:
            def want2(b, wv=wv):
                LL, D = im.swt2d_levels(b["x"], wv, L2)
                b["h"][:] = D.transpose(2, 0, 1, 3, 4).reshape(B, 3 * L2, H2, W2)
                b["l"][:, :L2] = LL.transpose(1, 0, 2, 3)
                return b
            out.append(Case("swt2d_batch symmetric %s swt2d_fused %d" % (wv, fused), "swt2d_batch",
                            lambda s: {"x": np.stack([m2.make_input(500 + 7 * s + k, "normal", H2, W2) for k in range(B)]),
                                       "h": np.full((B, 3 * L2, H2, W2), CAN, F32), "l": np.full((B, 3 * L2, H2, W2), CAN, F32)},
                            lambda dwt, P, h, wv=wv: st.swt2d_batch(wv, P["x"], plane, B, W2 * 4, 4, W2, H2, L2, P["h"], P["l"], 2, 3 * L2 * plane, plane, W2 * 4,
                                                                    border=st.BORDER_SYMMETRIC),
                            want2, sc.same_floats, options={"swt2d_fused": fused}))
            ops, params = tables(3 * L2)

            def make_i2(s, wv=wv):
                LL, D = im.swt2d_levels(np.stack([m2.make_input(520 + 7 * s + k, "normal", H2, W2) for k in range(B)]), wv, L2)
                ll = np.full((B, 3 * L2, H2, W2), CAN, F32)  # (src_h and src_l share the batch stride: plane 0 of every image)
                ll[:, 0] = LL[-1]
                return {"h": np.ascontiguousarray(D.transpose(2, 0, 1, 3, 4).reshape(B, 3 * L2, H2, W2)), "l": ll, "y": np.full((B, H2, W2), CAN, F32)}

            def want_i2(b, wv=wv, ops=ops, params=params):
                D = b["h"].reshape(B, L2, 3, H2, W2).transpose(1, 2, 0, 3, 4)
                b["y"][:] = im.iswt2d_levels(b["l"][:, 0], D, wv, ops, params)
                return b
            out.append(Case("iswt2d_batch %s swt2d_fused %d" % (wv, fused), "iswt2d_batch", make_i2,
                            lambda dwt, P, h, wv=wv, ops=ops, params=params: st.iswt2d_batch(wv, st.BORDER_SYMMETRIC, P["h"], P["l"], 3 * L2 * plane, plane, W2 * 4, B, W2, H2, L2,
                                                                                             P["y"], plane, W2 * 4, ops=ops, params=params),
                            want_i2, sc.same_floats, options={"swt2d_fused": fused}))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # The harness is driven through two names of tests/stream_cases.py that are not part of its interface, as tests/quant_stream.py
    # drives it: family_cases() serves a family from the cache _CASES.  If it is renamed there, the assertion below says so.
    assert isinstance(getattr(sc, "_CASES", None), dict) and {"swt_fused", "swt2d_fused"} <= set(sc.DEFAULT_OPTIONS), "stream_cases.py changed"
    sc._CASES["iswt"] = cases()
    assert sc.family_cases("iswt") is sc._CASES["iswt"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("iswt")
    print("iswt: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
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
