"""The pixel front end on a busy caller's stream, run as a process of its own by tests/test_hip_pixels.py: the cases below
go through the harness of tests/stream_cases.py -- a warm-up on the idle stream, then once on a non-blocking stream behind
a bounded delay, the true input reaching its buffer only behind that delay.  The result must be the model's bits
(tests/pixels_model.py; the composite entries with the float 9/7 oracle), every entry must have queued its work without
waiting for the stream, and the launch count must be that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import pixels_model as pm
import stream_cases as sc

KINDS = {"pixels_to_planes_batch": sc.ASYNC, "planes_to_pixels_batch": sc.ASYNC, "picture_forward_batch": sc.ASYNC,
         "picture_inverse_batch": sc.ASYNC}
BATCH, SIZE_X, SIZE_Y, LEVELS = 2, 64, 48, 5
N_PLANES = 3 * BATCH


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def pictures(seed):
    return np.random.default_rng(9300 + seed).integers(0, 256, (BATCH, SIZE_Y, SIZE_X, 3)).astype(np.uint8)


def planes_of(pix, colour, plane):
    """(B, H, W, 3) pixels -> (3 B, H, W) planes, level shift 128"""
    out = pm.to_planes(pix, pm.RGB, 128, 1.0, colour, plane)
    return np.ascontiguousarray(out.transpose(1, 0, 2, 3)).reshape(N_PLANES, SIZE_Y, SIZE_X)


def pixels_of(planes, colour):
    p = planes.reshape(BATCH, 3, SIZE_Y, SIZE_X).transpose(1, 0, 2, 3)
    return pm.to_pixels(p, pm.U8, pm.RGB, 8, 128, 1.0, colour)


def int_planes(seed):
    return np.random.default_rng(9400 + seed).integers(-200, 201, (N_PLANES, SIZE_Y, SIZE_X)).astype(np.int16)


def transformed(planes, inverse):
    import f16_model

    orc = f16_model.oracle()
    out = np.array(planes, np.float32)
    for a in out:
        t = a.copy()
        if inverse:
            orc.inv("cdf97_2i_s", t, LEVELS)
        else:
            assert orc.fwd("cdf97_2f_s", t, LEVELS) == LEVELS
        a[:] = t
    return out


def coefficients(seed):
    return transformed(planes_of(pictures(seed), pm.ICT, pm.S), False)


def cases():
    from libdwt_amd import pixels as P

    pix_args = (P.U8,), (3 * SIZE_X * SIZE_Y, 3 * SIZE_X, 3, 1, BATCH, 3, P.RGB, 8, 128, 1.0)
    i16 = (2 * SIZE_X * SIZE_Y, 2 * SIZE_X, SIZE_X, SIZE_Y)
    f32 = (4 * SIZE_X * SIZE_Y, 4 * SIZE_X, SIZE_X, SIZE_Y)
    out = []
    for wide in (1, 0):
        opts = {"pixels_wide": wide}
        out.append(Case("pixels_to_planes_batch rgb8 rct int16 pixels_wide %d" % wide, "pixels_to_planes_batch",
                        lambda seed: {"pix": pictures(seed), "planes": np.full((N_PLANES, SIZE_Y, SIZE_X), -77, np.int16)},
                        lambda dwt, D, host: P.pixels_to_planes_batch(*pix_args[0], D["pix"], *pix_args[1], P.RCT, P.I16, D["planes"], *i16),
                        lambda b: {"pix": b["pix"], "planes": planes_of(b["pix"], pm.RCT, pm.I16)}, same=sc.same_floats, options=opts))
        out.append(Case("planes_to_pixels_batch rgb8 rct int16 pixels_wide %d" % wide, "planes_to_pixels_batch",
                        lambda seed: {"pix": np.full((BATCH, SIZE_Y, SIZE_X, 3), 77, np.uint8), "planes": int_planes(seed)},
                        lambda dwt, D, host: P.planes_to_pixels_batch(*pix_args[0], D["pix"], *pix_args[1], P.RCT, P.I16, D["planes"], *i16),
                        lambda b: {"pix": pixels_of(b["planes"], pm.RCT), "planes": b["planes"]}, same=sc.same_floats, options=opts))
    out.append(Case("picture_forward_batch rgb8 ict cdf97_s", "picture_forward_batch",
                    lambda seed: {"pix": pictures(seed), "planes": np.full((N_PLANES, SIZE_Y, SIZE_X), -7.5, np.float32)},
                    lambda dwt, D, host: P.picture_forward_batch(dwt.CDF97_S, *pix_args[0], D["pix"], *pix_args[1], P.ICT, D["planes"], *f32, LEVELS),
                    lambda b: {"pix": b["pix"], "planes": transformed(planes_of(b["pix"], pm.ICT, pm.S), False), "ret": LEVELS},
                    same=sc.same_floats))
    out.append(Case("picture_inverse_batch rgb8 ict cdf97_s", "picture_inverse_batch",
                    lambda seed: {"pix": np.full((BATCH, SIZE_Y, SIZE_X, 3), 77, np.uint8), "planes": coefficients(seed)},
                    lambda dwt, D, host: P.picture_inverse_batch(dwt.CDF97_S, *pix_args[0], D["pix"], *pix_args[1], P.ICT, D["planes"], *f32, LEVELS),
                    lambda b: {"pix": pixels_of(transformed(b["planes"], True), pm.ICT), "planes": b["planes"]}, same=sc.same_floats))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # The harness is driven through two names of tests/stream_cases.py that are not part of its interface: family_cases()
    # serves a family from the cache _CASES, and Harness.run_once restores a case's options from DEFAULT_OPTIONS.  Both are
    # set here for this process alone; if either is renamed there, the assertions below say so.
    assert isinstance(getattr(sc, "_CASES", None), dict) and isinstance(getattr(sc, "DEFAULT_OPTIONS", None), dict), "stream_cases.py changed"
    sc.DEFAULT_OPTIONS = dict(sc.DEFAULT_OPTIONS, pixels_wide=1)
    sc._CASES["pixels"] = cases()
    assert sc.family_cases("pixels") is sc._CASES["pixels"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("pixels")
    print("pixels: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
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
