"""Every device entry holds to the caller's stream, on a busy stream.

The cases, the table of kinds (async / sync(reason)) and the harness live in tests/stream_cases.py.  Each GPU test here
starts that module once, in a process of its own -- torch must be imported before the library -- and asserts its final
"OK": one run per family (part 1: every entry behind a bounded delay on a non-blocking stream, with the negative control
of that process), one for the chain across families and two streams (part 2) and one for four threads (part 3).  The CPU
test holds the table to the package: a new public entry cannot be forgotten."""
import os
import subprocess
import sys

import pytest

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_public_entry_is_classified():
    """Every public callable of libdwt_amd is in the table of kinds or in the exclusion list with a reason, never in both;
    every row of the table is async or sync(reason) and has at least one case; every case names a row."""
    import libdwt_amd as dwt

    names = {n for n in dir(dwt) if not n.startswith("_") and callable(getattr(dwt, n))}
    rows = {k.split("[")[0] for k in sc.TABLE}
    assert not rows & set(sc.EXCLUDED), sorted(rows & set(sc.EXCLUDED))
    assert not names - rows - set(sc.EXCLUDED), "neither classified nor excluded: %s" % sorted(names - rows - set(sc.EXCLUDED))
    assert not (rows | set(sc.EXCLUDED)) - names, "no such entry: %s" % sorted((rows | set(sc.EXCLUDED)) - names)
    assert all(isinstance(r, str) and len(r) > 10 for r in sc.EXCLUDED.values())
    for k, kind in sc.TABLE.items():
        assert kind == sc.ASYNC or (kind.startswith("sync(") and len(kind) > 16), (k, kind)
    used = {}
    for family in sc.FAMILIES:
        for c in sc.family_cases(family):
            assert c.entry in sc.TABLE, (family, c.name, c.entry)
            assert set(c.options) <= set(sc.DEFAULT_OPTIONS), (family, c.name)
            used.setdefault(c.entry, []).append(family)
    assert not set(sc.TABLE) - set(used), "rows without a case: %s" % sorted(set(sc.TABLE) - set(used))
    # what the issue lists per family: the routes that an option picks run under both settings
    by_name = {c.name for f in sc.FAMILIES for c in sc.family_cases(f)}
    for stem in ("swt1d_batch cdf97_s swt_fused %d", "swt_features1d_batch swt_fused %d", "swt2d_batch cdf97_s swt2d_fused %d",
                 "swt2d_level swt2d_fused %d", "timefreq_batch complex timefreq_tiled %d"):
        assert stem % 0 in by_name and stem % 1 in by_name, stem
    assert all(c.is_async for c in sc.chain_cases())
    assert sorted(f for fams in sc.THREAD_FAMILIES for f in fams) == sorted(sc.FAMILIES)


def test_poison_mode_wraps_every_entry_that_is_not_denied():
    """The poison mode of the package (libdwt_amd.poison_workspace): every name on its deny list is an exported
    symbol of the library; every dwt_hip_* symbol the headers declare is on the list or comes back behind a fill while the
    switch is on; with the switch off `lib` hands out the plain CDLL functions.  No device is touched."""
    import re

    import libdwt_amd as dwt

    missing = sorted(n for n in dwt.NEVER_PREFILLED if not hasattr(dwt._cdll, n))
    assert not missing, "on the deny list, not exported: %s" % missing
    declared = set()
    inc = os.path.join(ROOT, "include")
    for header in os.listdir(inc):
        if header.endswith(".h"):
            declared.update(re.findall(r"\b(dwt_hip_\w+)\s*\(", open(os.path.join(inc, header)).read()))
    exported = sorted(n for n in declared if hasattr(dwt._cdll, n))
    assert len(exported) > 100 and "dwt_hip_fill_workspace" in exported and "dwt_hip_transform2d_batch" in exported
    assert dwt.poison_workspace(None) is None, "the switch was left on"
    for n in exported:
        assert getattr(dwt.lib, n) is getattr(dwt._cdll, n), n
    try:
        dwt.poison_workspace(0xFFFFFFFF)
        for n in exported:
            fn = getattr(dwt.lib, n)
            if n in dwt.NEVER_PREFILLED:
                assert fn is getattr(dwt._cdll, n), n
            else:
                assert isinstance(fn, dwt._Prefilled) and fn._fn is getattr(dwt._cdll, n), n
                assert fn.argtypes is getattr(dwt._cdll, n).argtypes  # (the function's own attributes)
        assert isinstance(dwt.lib.dwt_cdf97_2f_s, dwt._Prefilled), "the libdwt.h entries are wrapped too"
        for n in ("dwt_hip_fill_workspace", "dwt_hip_rows_warnings", "dwt_hip_memcpy_d2h", "dwt_hip_set_workspace", "dwt_hip_last_error"):
            assert n in dwt.NEVER_PREFILLED
        for n in ("dwt_hip_transform2d", "dwt_hip_rows_condition", "dwt_hip_quantize_batch", "dwt_hip_picture_forward_batch", "dwt_hip_tune"):
            assert n not in dwt.NEVER_PREFILLED
    finally:
        assert dwt.poison_workspace(None) == 0xFFFFFFFF
    assert dwt.lib.dwt_hip_transform2d is dwt._cdll.dwt_hip_transform2d


@pytest.mark.gpu
@pytest.mark.parametrize("run", sc.RUNS)
def test_entries_hold_to_the_callers_stream(run):
    pytest.importorskip("torch")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_cases.py"), run], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "OK", out.stdout[-6000:] + out.stderr[-3000:]
