"""The cells of tests/alignment_cases.py stand on both sides of every term of every family's 16-byte predicate (DESIGN.md
s35).  A condition on the matrix, read from the restated predicates alone -- not a measurement: it keeps the GPU test
(tests/test_hip_alignment.py) from passing on one path only.  Needs no GPU."""
import pytest

import alignment_cases as ac

FAMILIES = sorted(ac.FAMILIES)


@pytest.mark.parametrize("name", FAMILIES)
def test_cells_on_both_sides_of_every_term(name):
    """(a) for every term of the predicate -- every base, the pitch, every other stride -- a cell where it holds and one
    where it alone fails; and a cell where the whole predicate holds."""
    f = ac.FAMILIES[name]
    rows = [f.terms(c) for c in f.cells]
    assert rows and any(all(r.values()) for r in rows), "%s: no cell takes the 16-byte path" % name
    for term in rows[0]:
        assert any(r[term] for r in rows), (name, term, "never holds")
        assert any(not r[term] and all(v for k, v in r.items() if k != term) for r in rows), (name, term, "never fails alone")
    assert all(r.keys() == rows[0].keys() for r in rows)


@pytest.mark.parametrize("name", [n for n in FAMILIES if ac.FAMILIES[n].kind == "vec"])
def test_wide_path_meets_every_tail(name):
    """(b) the predicate holds together with each of n % 4 = 0, 1, 2, 3: the 16-byte loop and its tail run in one call; and
    fails with each of them: the element path sees every length too."""
    f = ac.FAMILIES[name]
    for wide in (True, False):
        seen = {f.length(c) % 4 for c in f.cells if f.predicate(c) == wide}
        assert seen == {0, 1, 2, 3}, (name, "16-byte path" if wide else "element path", sorted(seen))


@pytest.mark.parametrize("name", [n for n in FAMILIES if ac.FAMILIES[n].kind == "peel"])
def test_peeling_kernels_peel_every_count(name):
    """(c) the two kernels that peel elements up to a 16-byte boundary: every count 0 to 3, of every peel the family names."""
    f = ac.FAMILIES[name]
    for what in f.peels:
        seen = set().union(*(f.peel(c)[what] for c in f.cells))
        assert seen >= {0, 1, 2, 3}, (name, what, sorted(seen))


@pytest.mark.parametrize("name", FAMILIES)
def test_every_cell_runs_in_some_variant(name):
    """the GPU test is parametrised over the family's variants: together they cover the cells"""
    f = ac.FAMILIES[name]
    assert f.variants and len(set(f.variants)) == len(f.variants)
    covered = {id(c) for v in f.variants for c in f.cells_of(v)}
    assert covered == {id(c) for c in f.cells}


def test_row_family_axes():
    """the axes of the row families as the matrix was specified: every base offset and pitch residue at 64 .. 67 samples in 5
    lines, offsets and residues {0, 4} at 2049 .. 2052 in 2 lines"""
    for name in ("oned", "lifting1d"):
        f = ac.FAMILIES[name]
        plain = [c for c in f.cells if not c.more.get("staged") and c.more.get("es", 4) == 4]
        for n in ac.SHORT:
            here = [c for c in plain if c.n == n]
            assert all(c.lines == 5 for c in here)
            assert {(c.offs[0], c.pitch % 16) for c in here if not c.apart} == {(o, r) for o in ac.OFFSETS for r in ac.RESIDUES}
            assert {(c.offs, c.pitch % 16) for c in here if c.apart} == {(p, r) for p in ac.PAIRS for r in ac.RESIDUES}
            assert all(c.pitch - 16 < n * 4 <= c.pitch for c in here)
        for n in ac.LONG:
            here = [c for c in plain if c.n == n]
            assert all(c.lines == 2 for c in here)
            assert {(c.offs[0], c.pitch % 16) for c in here if not c.apart} == {(o, r) for o in (0, 4) for r in (0, 4)}
