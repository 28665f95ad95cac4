#!/usr/bin/env python3
"""Per-kernel resource figures of device assembly files, and the comparison of two sets of them:
    scripts/sweep_isa_table.py PARENT_DIR HEAD_DIR            (every *.s of PARENT_DIR against the file of that name in HEAD_DIR)
The assembly comes from the Makefile's HIPFLAGS plus `--cuda-device-only -S` (and -DDWT_FLOAT_END_FORMS=0 for the plain
build).  Kernels are matched by demangled name; the geometry argument's type name is ignored.  Prints per-file totals
and every kernel whose figures differ; exit status 1 if the kernel sets differ, a kernel of the head has scratch or
spilled vector registers, or an occupancy falls.  (Scalar registers spilled to lanes of a vector register -- the
parent's kernels have up to 189 -- are counted as `sspill` and compared like the other figures.)"""
import glob
import os
import re
import subprocess
import sys

FIELDS = ("vgpr", "sgpr", "lds", "scratch", "sspill", "vspill", "insts", "occ")


def kernels(path):
    text = open(path).read()
    out = {}
    # a kernel: its label, its code, its .amdhsa_kernel block, then the "Kernel info" comments up to the occupancy
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\t\.amdhsa_kernel \1\n(.*?)^; Occupancy: (\d+)", text, re.S | re.M):
        name, body, tail, occ = m.groups()
        num = lambda pat: int(re.search(pat, tail).group(1))
        out[name] = dict(
            vgpr=num(r"; NumVgprs: (\d+)"), sgpr=num(r"; TotalNumSgprs: (\d+)"), lds=num(r"\.amdhsa_group_segment_fixed_size (\d+)"),
            scratch=num(r"\.amdhsa_private_segment_fixed_size (\d+)"), sspill=0, vspill=0,
            insts=sum(1 for ln in body.splitlines() if re.match(r"\t[a-z]\w*(\s|$)", ln)), occ=int(occ))
    # spill counts: the metadata at the end of the file
    for md in text[text.rfind("amdhsa.kernels:"):].split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(_Z\w+)", md).group(1)
        if name in out:
            out[name]["sspill"] = int(re.search(r"\.sgpr_spill_count: (\d+)", md).group(1))
            out[name]["vspill"] = int(re.search(r"\.vgpr_spill_count: (\d+)", md).group(1))
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    norm = lambda d: re.sub(r"dwt::(\(anonymous namespace\)::)?SweepGeomD?", "SweepGeom", d)
    return {norm(d): out[n] for n, d in zip(names, dem)}


def main():
    parent, head = sys.argv[1], sys.argv[2]
    bad = False
    for pf in sorted(glob.glob(os.path.join(parent, "*.s"))):
        f = os.path.basename(pf)
        kp, kh = kernels(pf), kernels(os.path.join(head, f))
        tot = lambda k, x: sum(v[x] for v in k.values())
        mx = lambda k, x: max(v[x] for v in k.values())
        print(f"| `{f}` | {len(kp)} / {len(kh)} | {tot(kp, 'insts')} / {tot(kh, 'insts')} | {mx(kp, 'vgpr')} / {mx(kh, 'vgpr')} | "
              f"{mx(kp, 'scratch') + mx(kp, 'vspill')} / {mx(kh, 'scratch') + mx(kh, 'vspill')} | {mx(kp, 'sspill')} / {mx(kh, 'sspill')} | "
              f"{sum(1 for n in kp if n in kh and kp[n] != kh[n])} |")
        if set(kp) != set(kh):
            bad = True
            print("  kernel sets differ:", sorted(set(kp) ^ set(kh)))
        for n in sorted(kp):
            if n not in kh:
                continue
            a, b = kp[n], kh[n]
            if b["scratch"] or b["vspill"] or b["occ"] < a["occ"]:
                bad = True
            if a != b:
                print("  differs: `" + n.split("(")[0] + "` " + ", ".join(f"{x} {a[x]} -> {b[x]}" for x in FIELDS if a[x] != b[x]))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
