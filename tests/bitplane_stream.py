"""The embedded bit-plane streams on a busy caller's stream, run as a process of its own by tests/test_hip_bitplanes.py:
the cases below go through the harness of tests/stream_cases.py -- a warm-up on the idle stream, then once on a
non-blocking stream behind a bounded delay, the true input reaching its buffer only behind that delay.  The result must be
the model's bits (tests/bitplane_model.py), the entries classified async must have queued their work without waiting for
the stream, and the launch count must be that of the warm-up.  Prints OK as its last line."""
import sys

import numpy as np

import bitplane_model as bpm
import stream_cases as sc

KINDS = {"pack_batch": sc.ASYNC, "count_batch": sc.ASYNC, "unpack_batch": sc.ASYNC,
         "pack_batch[host offsets]": sc.SYNC("the offsets are copied to the caller's host array")}
BATCH, SIZE_X, SIZE_Y, LEVELS, CB = 3, 72, 40, 3, (3, 5)
BLOCKS = int(bpm.bands(SIZE_X, SIZE_Y, LEVELS, *CB)[-1, 4])
CAP = SIZE_X * SIZE_Y // 2  # words: 32 bits a sample, room for 13 planes and the partial blocks' padding
SENTINEL = 0xEEEEEEEE
SENTINEL64 = 0xEEEEEEEEEEEEEEEE


class Case(sc.Case):
    @property
    def kind(self):
        return KINDS[self.entry]


def indices(seed):
    rng = np.random.default_rng(9900 + seed)
    q = rng.integers(-3000, 3001, (BATCH, SIZE_Y, SIZE_X)).astype(np.int16)
    q[rng.random(q.shape) >= 0.2] = 0
    q[:, :8, :] = 0  # (blocks of zeros)
    return q


def empty_stream():
    # (words and offsets as signed views of their bits: the harness moves the buffers as torch tensors)
    return {"words": np.full((BATCH, CAP), SENTINEL64, np.uint64).view(np.int64), "off": np.full((BATCH, BLOCKS + 1), SENTINEL, np.uint32).view(np.int32)}


def packed(planes):
    words, off = bpm.pack(planes, bpm.I16, LEVELS, *CB, capacity=CAP, fill=SENTINEL64)
    assert off[:, -1].max() < CAP
    return {"words": words.view(np.int64), "off": off.view(np.int32)}


def cases():
    from libdwt_amd import bitplanes as BP

    i16 = (2 * SIZE_X * SIZE_Y, 2 * SIZE_X)
    frames = (BATCH, SIZE_X, SIZE_Y, LEVELS) + CB
    out = []
    for wave in (1, 0):
        opts = {"bitplane_wave": wave}
        out.append(Case("pack_batch int16 bitplane_wave %d" % wave, "pack_batch",
                        lambda seed: dict(empty_stream(), planes=indices(seed)),
                        lambda dwt, D, host: BP.pack_batch(BP.I16, D["planes"], *i16, *frames, D["words"], CAP, D["off"]),
                        lambda b: dict(packed(b["planes"]), planes=b["planes"], ret=None), options=opts))
        out.append(Case("count_batch int16 bitplane_wave %d" % wave, "count_batch",
                        lambda seed: {"planes": indices(seed), "off": empty_stream()["off"]},
                        lambda dwt, D, host: BP.count_batch(BP.I16, D["planes"], *i16, *frames, D["off"]),
                        lambda b: {"planes": b["planes"], "off": packed(b["planes"])["off"], "ret": None}, options=opts))
        out.append(Case("unpack_batch int16 bitplane_wave %d" % wave, "unpack_batch",
                        lambda seed: dict(packed(indices(seed)), planes=np.full((BATCH, SIZE_Y, SIZE_X), -77, np.int16)),
                        lambda dwt, D, host: BP.unpack_batch(BP.I16, D["words"], CAP, D["off"], D["planes"], *i16, *frames, 1, BP.SHIFT),
                        lambda b: dict(b, planes=bpm.unpack(b["words"].view(np.uint64), b["off"].view(np.uint32), bpm.I16, SIZE_X, SIZE_Y, LEVELS, *CB, 1,
                                                            bpm.SHIFT), ret=None), options=opts))
    out.append(Case("pack_batch int16, offsets to the host", "pack_batch[host offsets]",
                    lambda seed: dict(empty_stream(), planes=indices(seed)),
                    lambda dwt, D, host: BP.pack_batch(BP.I16, D["planes"], *i16, *frames, D["words"], CAP),
                    lambda b: dict(packed(b["planes"]), planes=b["planes"], off=empty_stream()["off"], ret=packed(b["planes"])["off"].view(np.uint32)),
                    check_ret=np.array_equal))
    return out


def main():
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch ships)

    # The harness is driven through two names of tests/stream_cases.py that are not part of its interface: family_cases()
    # serves a family from the cache _CASES, and Harness.run_once restores a case's options from DEFAULT_OPTIONS.  Both are
    # set here for this process alone; if either is renamed there, the assertions below say so.
    assert isinstance(getattr(sc, "_CASES", None), dict) and isinstance(getattr(sc, "DEFAULT_OPTIONS", None), dict), "stream_cases.py changed"
    sc.DEFAULT_OPTIONS = dict(sc.DEFAULT_OPTIONS, bitplane_wave=1)
    sc._CASES["bitplane"] = cases()
    assert sc.family_cases("bitplane") is sc._CASES["bitplane"]
    h = sc.Harness()
    print("device:", h.dwt.device_name(), flush=True)
    D, cycles, longest = h.run_family("bitplane")
    print("bitplane: D = %.1f ms, %d cycles, longest enqueue %.3f ms" % (D, cycles, longest * 1e3), flush=True)
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
