"""The sparse coefficient streams on a busy caller's stream, run as a process of its own by tests/test_hip_sparse.py: the
cases below go through the harness of tests/stream_cases.py -- a warm-up on the idle stream, then once on a non-blocking
stream behind a bounded delay, the true input reaching its buffer only behind that delay.  The result must be the model's
bits (tests/sparse_model.py), the entries classified async must have queued their work without waiting for the stream, and
the launch count must be that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import sparse_model as spm
import stream_cases as sc

KINDS = {"pack_batch": sc.ASYNC, "count_batch": sc.ASYNC, "unpack_batch": sc.ASYNC,
         "pack_batch[host offsets]": sc.SYNC("the offsets are copied to the caller's host array")}
BATCH, SIZE_X, SIZE_Y, LEVELS = 3, 72, 40, 3
CAP = SIZE_X * SIZE_Y // 2
WORDS = 3 * LEVELS + 2
SENTINEL = 0xEEEEEEEE


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def indices(seed):
    rng = np.random.default_rng(9800 + seed)
    q = rng.integers(-3000, 3001, (BATCH, SIZE_Y, SIZE_X)).astype(np.int16)
    q[rng.random(q.shape) >= 0.2] = 0
    return q


def empty_stream():
    # (positions and offsets as int32 views of their uint32 bits: the harness moves the buffers as torch tensors)
    return {"pos": np.full((BATCH, CAP), SENTINEL, np.uint32).view(np.int32), "val": np.full((BATCH, CAP), SENTINEL & 0xFFFF, np.uint16).view(np.int16),
            "off": np.full((BATCH, WORDS), SENTINEL, np.uint32).view(np.int32)}


def packed(planes):
    pos, val, off = spm.pack(planes, spm.I16, LEVELS, CAP, fill=SENTINEL)
    assert off[:, -1].max() < CAP
    return {"pos": pos.view(np.int32), "val": val, "off": off.view(np.int32)}


def cases():
    from libdwt_amd import sparse as S

    i16 = (2 * SIZE_X * SIZE_Y, 2 * SIZE_X)
    frames = (BATCH, SIZE_X, SIZE_Y)
    out = []
    for wide in (1, 0):
        opts = {"sparse_wide": wide}
        out.append(Case("pack_batch int16 sparse_wide %d" % wide, "pack_batch",
                        lambda seed: dict(empty_stream(), planes=indices(seed)),
                        lambda dwt, D, host: S.pack_batch(S.I16, D["planes"], *i16, *frames, LEVELS, D["pos"], D["val"], CAP, D["off"]),
                        lambda b: dict(packed(b["planes"]), planes=b["planes"], ret=None), options=opts))
        out.append(Case("count_batch int16 sparse_wide %d" % wide, "count_batch",
                        lambda seed: {"planes": indices(seed), "off": empty_stream()["off"]},
                        lambda dwt, D, host: S.count_batch(S.I16, D["planes"], *i16, *frames, LEVELS, D["off"]),
                        lambda b: {"planes": b["planes"], "off": packed(b["planes"])["off"], "ret": None}, options=opts))
        out.append(Case("unpack_batch int16 sparse_wide %d" % wide, "unpack_batch",
                        lambda seed: dict(packed(indices(seed)), planes=np.full((BATCH, SIZE_Y, SIZE_X), -77, np.int16)),
                        lambda dwt, D, host: S.unpack_batch(S.I16, D["pos"], D["val"], CAP, D["off"] + 4 * (WORDS - 1), WORDS, D["planes"], *i16, *frames),
                        lambda b: dict(b, planes=spm.unpack(b["pos"].view(np.uint32), b["val"], b["off"].view(np.uint32)[:, -1], spm.I16, SIZE_Y, SIZE_X), ret=None), options=opts))
    out.append(Case("pack_batch int16, offsets to the host", "pack_batch[host offsets]",
                    lambda seed: dict(empty_stream(), planes=indices(seed)),
                    lambda dwt, D, host: S.pack_batch(S.I16, D["planes"], *i16, *frames, LEVELS, D["pos"], D["val"], CAP),
                    lambda b: dict(packed(b["planes"]), planes=b["planes"], off=empty_stream()["off"], ret=packed(b["planes"])["off"].view(np.uint32)),
                    check_ret=np.array_equal))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # The harness is driven through two names of tests/stream_cases.py that are not part of its interface: family_cases()
    # serves a family from the cache _CASES, and Harness.run_once restores a case's options from DEFAULT_OPTIONS.  Both are
    # set here for this process alone; if either is renamed there, the assertions below say so.
    assert isinstance(getattr(sc, "_CASES", None), dict) and isinstance(getattr(sc, "DEFAULT_OPTIONS", None), dict), "stream_cases.py changed"
    sc.DEFAULT_OPTIONS = dict(sc.DEFAULT_OPTIONS, sparse_wide=1)
    sc._CASES["sparse"] = cases()
    assert sc.family_cases("sparse") is sc._CASES["sparse"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("sparse")
    print("sparse: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
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
