#!/usr/bin/env python3
"""Writes tests/golden/nterm.npz and tests/golden/nterm_manifest.json: for every two-channel case of tests/nterm_model.py
the magnitude plane, and the threshold and kept count for every keep of nterm_model.keeps_of, as a literal C restatement
of examples/displ-vectors/vectors.c:254-297 gives them (libc sqrtf and qsort; the function below, compiled with the
reference's release flags); for the "flow" cases also the coefficient planes, which are the reference's own
dwt_cdf97_2f_s / dwt_cdf53_2f_s over the two displacement fields of nterm_model.flow_fields.

The reference's sources are compiled from where they lie (oracle/Makefile: REF_CFLAGS) into a temporary directory outside
the repository, loaded from there, and the directory is deleted: no reference text or binary enters the tree.

    python scripts/gen_nterm_golden.py [--ref /path/to/libdwt]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import nterm_model as nm  # noqa: E402
from gen_swt_golden import REF_SRCS, ref_cflags  # noqa: E402

RESTATEMENT = r"""
#include <math.h>
#include <stdlib.h>
static int cmp_desc(const void *a, const void *b)
{
	const float x = *(const float *)a, y = *(const float *)b;
	return x < y ? 1 : (x > y ? -1 : 0);
}
/* the magnitudes of count positions -> map; the threshold for N of them -> return; positions not below it -> *kept */
float nterm_restated(const float *dx, const float *dy, float *map, int count, int N, int *kept)
{
	float *array = malloc(sizeof(float) * count);
	for (int i = 0; i < count; i++)
		array[i] = map[i] = sqrtf(dx[i] * dx[i] + dy[i] * dy[i]);
	qsort(array, count, sizeof(float), cmp_desc);
	if (N < 1 || N > count)
		N = count;
	const float thr = array[N - 1];
	*kept = 0;
	for (int i = 0; i < count; i++)
		if (!(map[i] < thr))
			++*kept;
	free(array);
	return thr;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    tmp = tempfile.mkdtemp(prefix="nterm_golden_")
    try:
        cc, flags = os.environ.get("CC", "gcc"), ref_cflags(args.ref)
        so = os.path.join(tmp, "libdwt_ref.so")
        subprocess.check_call([cc] + flags + ["-I" + src, "-shared", "-Wl,-Bsymbolic", "-o", so] +
                              [os.path.join(src, f) for f in REF_SRCS] + ["-lm", "-lrt"])
        with open(os.path.join(tmp, "restated.c"), "w") as f:
            f.write(RESTATEMENT)
        so2 = os.path.join(tmp, "librestated.so")
        subprocess.check_call([cc] + flags + ["-shared", "-o", so2, os.path.join(tmp, "restated.c"), "-lm"])
        ref, own = C.CDLL(so), C.CDLL(so2)
        own.nterm_restated.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        own.nterm_restated.restype = C.c_float
        out, cases = {}, []
        for name, (source, seed, wavelet, size_y, size_x) in nm.CASES.items():
            if source == "flow":
                planes = nm.flow_fields(size_y, size_x)
                fwd = getattr(ref, "dwt_%s_2f_s" % wavelet)
                fwd.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_int]
                fwd.restype = None
                for c in range(2):
                    j = C.c_int(-1)
                    fwd(planes[c].ctypes.data, 4 * size_x, 4, size_x, size_y, size_x, size_y, C.addressof(j), 0, 0)
                out[name + ".coef"] = planes
            else:
                planes = nm.make_input(seed, source, 2, size_y, size_x)
            M = size_y * size_x
            mag, kept = np.zeros((size_y, size_x), np.float32), C.c_int(0)
            keeps = nm.keeps_of(M)
            thr, cnt = np.zeros(len(keeps), np.float32), np.zeros(len(keeps), np.int32)
            for i, n in enumerate(keeps):
                thr[i] = own.nterm_restated(planes[0].ctypes.data, planes[1].ctypes.data, mag.ctypes.data, M, n, C.addressof(kept))
                cnt[i] = kept.value
            out[name + ".mag"], out[name + ".thr"], out[name + ".kept"] = mag, thr, cnt
            cases.append({"name": name, "source": source, "seed": seed, "wavelet": wavelet, "size_y": size_y, "size_x": size_x})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(nm.GOLDEN, **out)
    with open(nm.GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(nm.MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_nterm_golden.py",
                   "reference": "libdwt (src/libdwt.c: dwt_cdf97_2f_s, dwt_cdf53_2f_s; examples/displ-vectors/vectors.c:254-297 restated; "
                                "oracle/Makefile REF_CFLAGS)",
                   "files": {"nterm.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", nm.GOLDEN, os.path.getsize(nm.GOLDEN), "bytes,", len(cases), "cases,", sum(a.size for a in out.values()), "values")


if __name__ == "__main__":
    main()
