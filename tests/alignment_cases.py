"""Every 16-byte fast path at every base, pitch and length residue (tests/test_alignment_matrix.py and
tests/test_hip_alignment.py read this module).

Almost every driver touches a line in one of two ways: 16 bytes per lane, or one element per lane.  The choice is made per
call from the alignment of the base pointers and strides, so it is a function of three residues -- base address mod 16,
pitch mod 16, line length mod 4.  The other GPU tests reach those by accident of their shapes.  Here every family has

  * its predicate, restated from the code as a function of a cell (the source line is cited beside it), term by term, and
  * its cells: (byte offset of every device buffer of the call, pitch, length).

A plain module like gridlimits.py and stream_cases.py: it needs no GPU to be imported, and the CPU test asserts from the
predicates alone that the cells stand on both sides of every term.  The GPU side (`run`) lays every buffer of a call into a
hipdev.Dev allocation -- which the runtime aligns far beyond 16 bytes -- 16 + off bytes in, every word outside the samples
a canary: the words in front of the frame, the row padding, the gaps between frames or planes and the words behind must
come back as they were, and so must the source of an out-of-place call.  Expected values come from the CPU side only, by
the model or oracle call that the family's own GPU test uses, compared as that test compares: bit for bit, a NaN equal to
a NaN (only the band operators' inputs hold any), and by value where that test compares by value (a median, a conditioned
row: -0 counts as +0).  No tolerance is introduced.  A base 2 bytes off a sample boundary has one cell per family: the entry
either stages such a frame (the model's bits are expected) or refuses it (a message, and every byte as it was)."""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F32, I32 = np.float32, np.int32
LEAD = 16            # bytes of canary in front of every frame, before its offset
TAIL = 64            # bytes of canary behind it
CANARY = 0x5CA1AB1E  # what every word outside the samples holds
OFFSETS = (0, 4, 8, 12)                                # base offsets in bytes of an in-place call
PAIRS = ((0, 0), (0, 4), (4, 0), (8, 8), (12, 4))      # (source, destination) offsets of an out-of-place call
RESIDUES = (0, 4, 8, 12)                               # pitch mod 16
SHORT = (64, 65, 66, 67)      # 5 lines: one wave per line, four lines per workgroup, the fifth alone in its workgroup
LONG = (2049, 2050, 2051, 2052)  # 2 lines of the 256-thread class, at offsets {0, 4} and pitch residues {0, 4} only
LONG_OFFSETS, LONG_PAIRS, LONG_RESIDUES = (0, 4), ((0, 0), (0, 4), (4, 0)), (0, 4)
DEPTH = 3


def pitch_for(line_bytes, residue):
    """the smallest pitch >= line_bytes with pitch % 16 == residue"""
    return line_bytes + (residue - line_bytes) % 16


def _rng(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def finite(shape, *key):
    """floatends.finite_floats: no transform of any depth overflows, so every sample of a result is compared"""
    from floatends import finite_floats

    return finite_floats(_rng(*key), shape, F32)


_ORC = None


def orc():
    global _ORC
    if _ORC is None:
        from oraclelib import Oracle

        _ORC = Oracle()
    return _ORC


# ---- a frame inside an allocation full of canaries ---------------------------------------------------------------------
class Frame:
    """Samples of `dtype` at byte `strides` (slowest first), the first one LEAD + off bytes into the allocation."""

    def __init__(self, off, shape, strides, dtype=F32):
        self.off, self.shape, self.strides, self.dtype = off, tuple(shape), tuple(strides), np.dtype(dtype)
        span = sum((n - 1) * s for n, s in zip(self.shape, self.strides)) + self.dtype.itemsize
        self.nbytes = (LEAD + off + span + TAIL + 3) // 4 * 4

    def view(self, raw):
        return np.ndarray(self.shape, self.dtype, buffer=raw, offset=LEAD + self.off, strides=self.strides)

    def host(self, samples=None):
        """the allocation's bytes: canaries, and `samples` where the frame's samples lie"""
        raw = np.full(self.nbytes // 4, CANARY, np.uint32).view(np.uint8)
        if samples is not None:
            self.view(raw)[...] = samples
        return raw

    def diff(self, got, want):
        """None where the allocation came back as expected, otherwise what differs"""
        if got.tobytes() == want.tobytes():
            return None
        g, w = np.ascontiguousarray(self.view(got)), np.ascontiguousarray(self.view(want))
        bad = g.view(np.uint8).reshape(g.shape + (-1,)) != w.view(np.uint8).reshape(w.shape + (-1,))
        bad = bad.any(axis=-1)
        if self.dtype.kind == "f":
            bad &= ~(np.isnan(g) & np.isnan(w))
        inside = np.zeros(got.shape, bool)
        np.ndarray(self.shape + (self.dtype.itemsize,), bool, buffer=inside, offset=LEAD + self.off, strides=self.strides + (1,))[...] = True
        out = np.flatnonzero((got != want) & ~inside)
        msg = []
        if bad.any():
            msg.append("%d of %d samples differ, the first at %s" % (int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0])))
        if out.size:
            msg.append("%d bytes outside the samples written, at %d .. %d from the frame's first byte" % (
                out.size, int(out[0]) - LEAD - self.off, int(out[-1]) - LEAD - self.off))
        return "; ".join(msg) or None


def run_call(dwt, frames, before, call, after, by_value=None):
    """frames: {name: Frame}; before / after: {name: samples}.  Uploads every allocation, makes the call on the frames'
    addresses, and compares every byte of every allocation.  by_value: {name: index of the samples that the family's own
    test compares by value}: there -0 counts as +0.  -> list of differences"""
    from hipdev import Dev

    devs = {k: Dev(dwt, f.host(before[k])) for k, f in frames.items()}
    try:
        call({k: devs[k].ptr + LEAD + f.off for k, f in frames.items()})
        bad = []
        for k, f in frames.items():
            got, want = devs[k].get(), f.host(after[k])
            if by_value and k in by_value:
                for raw in (got, want):
                    f.view(raw)[by_value[k]] += F32(0)  # (-0 + +0 is +0; every other value stays)
            d = f.diff(got, want)
            if d:
                bad.append("%s: %s" % (k, d))
        return bad
    finally:
        for d in devs.values():
            d.free()


def run_refused(dwt, frames, before, call, text="multiples of 4 bytes"):
    """a call with a base 2 bytes off a sample boundary that the entry refuses: an error that says `text`, and every byte of
    every allocation as it was.  -> list of differences"""
    said = []

    def guarded(P):
        try:
            call(P)
            said.append("accepted")
        except dwt.DwtError as e:
            said.append(str(e))
    bad = run_call(dwt, frames, before, guarded, before)
    if text not in said[0]:
        bad.append("not refused with %r: %s" % (text, said[0]))
    return ["a base 2 bytes off: %s" % b for b in bad]


class Options:
    """library options for the calls inside, put back to `default` afterwards"""

    def __init__(self, dwt, values, default):
        self.dwt, self.values, self.default = dwt, values, default

    def __enter__(self):
        for k, v in self.values.items():
            self.dwt.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.dwt.set_option(k, self.default[k])


DEFAULTS = {"generic": 0, "swt_fused": 1, "lifting_fused": 1, "vol_fused": 1, "cond_fused": -1, "window_fused": 1}


# ---- cells -----------------------------------------------------------------------------------------------------------------
class Cell:
    """offs: the byte offset of every device buffer of the call, in the family's order; pitch: bytes from line to line (row
    to row); n: samples a line (columns a row); lines: lines, or rows; more: what else the family varies"""

    def __init__(self, offs, pitch, n, lines, **more):
        self.offs, self.pitch, self.n, self.lines, self.more = tuple(offs), pitch, n, lines, more

    def __getattr__(self, name):
        try:
            return self.more[name]
        except KeyError:
            raise AttributeError(name)

    def __repr__(self):
        more = "".join(" %s=%s" % kv for kv in sorted(self.more.items()))
        return "offs=%s pitch=%d n=%d lines=%d%s" % ("/".join(map(str, self.offs)), self.pitch, self.n, self.lines, more)


def row_cells(n_bufs, place=lambda s, d: (s, d), in_place=True, apart=True, es=4):
    """The cells of a row family: 5 short lines at every offset and pitch residue, 2 long ones at offsets and residues {0, 4}.
    In place: every buffer at the same offset.  Apart: `place(source offset, destination offset)` gives every buffer's."""
    cells = []
    for ns, lines, offsets, pairs, residues in ((SHORT, 5, OFFSETS, PAIRS, RESIDUES), (LONG, 2, LONG_OFFSETS, LONG_PAIRS, LONG_RESIDUES)):
        for n in ns:
            for r in residues:
                pitch = pitch_for(n * es, r)
                if in_place:
                    cells += [Cell((o,) * n_bufs, pitch, n, lines, apart=False) for o in offsets]
                if apart:
                    cells += [Cell(place(s, d), pitch, n, lines, apart=True) for s, d in pairs]
    return cells


class Family:
    """name; where: the source lines of the choice; kind: "vec" (16 bytes per lane where the predicate holds, with a tail of
    n % 4 samples), "peel" (elements peeled up to a 16-byte boundary: peels names the counts, peel(cell) -> {count: the values
    the cell's rows meet}), "tile" (the 3-D tiles) or "route" (the 2-D entries: which driver runs); terms(cell) -> {term:
    bool}, the predicate being their conjunction; cells; variants: the ids the GPU test is parametrised over, cells_of(variant)
    the cells each runs; run(dwt, variant) -> differences, one line per cell and buffer that differs."""

    kind = "vec"
    where = ""
    variants = ()

    def terms(self, c):
        raise NotImplementedError

    def predicate(self, c):
        return all(self.terms(c).values())

    def length(self, c):
        return c.n

    def cells_of(self, variant):
        return self.cells

    def run(self, dwt, variant):
        raise NotImplementedError


def alone(family, candidates):
    """for every term of the family's predicate the first candidate cell in which that term alone fails (strides that are
    sums of others seldom fail alone: a gap of 4, 8 or 12 bytes elsewhere has to make up for them)"""
    out = []
    for term in family.terms(candidates[0]):
        for c in candidates:
            t = family.terms(c)
            if not t[term] and all(v for k, v in t.items() if k != term):
                out.append(c)
                break
    return out


# ---- 1-D Mallat lines: transform1d_batch ---------------------------------------------------------------------------------------
class Oned(Family):
    """dwt_line1d.hip:152 (line_levels_t): vec = elem_stride == 4 && line_stride % 16 == 0 && src % 16 == 0 && dst % 16 == 0;
    the loads of dwt_line_lds.h and the paired store of the inverse (dwt_line1d.hip:132) follow it.  A base 2 bytes off is
    staged (dwt_backend_1d.hip:93-99 fall through to frame_stage; dwt_strided.hip moves such elements byte by byte)."""
    name, where = "oned", "dwt_line1d.hip:152"
    wavelets = ("cdf97_s", "cdf53_s", "interp53_s")

    def __init__(self):
        self.cells = row_cells(2)
        self.cells.append(Cell((0, 0), pitch_for(65 * 8, 0), 65, 5, apart=False, es=8))  # the element stride's own term
        self.cells.append(Cell((2, 2), pitch_for(65 * 4, 0), 65, 5, apart=False, staged=True))  # 2 bytes off a sample: staged
        self.cells.append(Cell((2, 0), pitch_for(65 * 4, 0), 65, 5, apart=True, staged=True))
        self.variants = ["%s-%s" % (w, d) for w in self.wavelets for d in ("fwd", "inv")]
        self._want = {}

    def terms(self, c):
        return {"elem_stride == 4": c.more.get("es", 4) == 4, "line_stride % 16": c.pitch % 16 == 0, "src % 16": c.offs[0] % 16 == 0,
                "dst % 16": c.offs[1] % 16 == 0}

    def model(self, wv, inverse, lines):
        if wv == "interp53_s":
            import interp53_model

            (interp53_model.inv1d if inverse else interp53_model.fwd1d)(lines, j_max=DEPTH)
            return lines
        from test_oned import restated

        for row in lines:
            restated(orc(), wv[:5], inverse, row, len(row), None, DEPTH)
        return lines

    def data(self, wv, inverse, n, lines):
        key = (wv, inverse, n, lines)
        if key not in self._want:
            x = finite((lines, n), "oned", n)
            self._want[key] = (x, self.model(wv, inverse, x.copy()))
        return self._want[key]

    def run(self, dwt, variant):
        wv, direction = variant.rsplit("-", 1)
        inverse = int(direction == "inv")
        bad = []
        for c in self.cells:
            es = c.more.get("es", 4)
            x, y = self.data(wv, inverse, c.n, c.lines)
            fr = Frame(c.offs[0], (c.lines, c.n), (c.pitch, es))
            if c.apart:
                frames = {"src": fr, "dst": Frame(c.offs[1], (c.lines, c.n), (c.pitch, es))}
                before, after = {"src": x, "dst": None}, {"src": x, "dst": y}
            else:
                frames, before, after = {"src": fr}, {"src": x}, {"src": y}

            def call(P, c=c, es=es):
                j = dwt.transform1d_batch(wv, inverse, P["src"], P["dst" if c.apart else "src"], c.pitch, c.lines, c.n, DEPTH, es)
                assert j == DEPTH, j
            bad += ["%r: %s" % (c, d) for d in run_call(dwt, frames, before, call, after)]
        return bad


# ---- user lifting of rows: lifting1d_batch -------------------------------------------------------------------------------------
class Lifting1d(Family):
    """dwt_lifting.hip:533 (launch_lift_lines): vec = elem_stride == 4 && line_stride % 16 == 0 && src % 16 == 0 && dst % 16
    == 0; the split-by-parity quad load of the forward (:435-441), the whole-line load of the inverse (:470-476) and its paired
    store (:504-507) follow it.  Under lifting_fused 0 every level runs step by step through dense scratch (no predicate:
    one element per lane on the caller's side).  A base 2 bytes off is staged (dwt_backend_lifting.hip:334-348)."""
    name, where = "lifting1d", "dwt_lifting.hip:533"
    schemes = ("D4", "CDF53_INT")

    def __init__(self):
        self.cells = row_cells(2)
        self.cells.append(Cell((0, 0), pitch_for(65 * 8, 0), 65, 5, apart=False, es=8))
        self.cells.append(Cell((2, 2), pitch_for(65 * 4, 0), 65, 5, apart=False, staged=True))
        self.cells.append(Cell((2, 0), pitch_for(65 * 4, 0), 65, 5, apart=True, staged=True))
        self.variants = ["%s-%s-fused%d" % (s, d, f) for s in self.schemes for d in ("fwd", "inv") for f in (1, 0)]
        self._want = {}

    terms = Oned.terms

    def data(self, name, inverse, n, lines):
        import lifting1d_model as l1
        import lifting_model as lm

        key = (name, inverse, n, lines)
        if key not in self._want:
            s = lm.builtin(name)
            if s.type == lm.I32:
                x = _rng("lifting1d", n).integers(-(1 << 20), 1 << 20, (lines, n)).astype(I32)
            else:
                x = finite((lines, n), "lifting1d", n)
            y = (l1.inv1d if inverse else l1.fwd1d)(s, x.copy(), DEPTH)[0]
            self._want[key] = (x, np.ascontiguousarray(y, x.dtype))
        return self._want[key]

    def run(self, dwt, variant):
        from libdwt_amd import lifting as L

        name, direction, fused = variant.split("-")
        inverse, sl = int(direction == "inv"), L.builtin(name)
        bad = []
        with Options(dwt, {"lifting_fused": int(fused[-1])}, DEFAULTS):
            for c in self.cells:
                es = c.more.get("es", 4)
                x, y = self.data(name, inverse, c.n, c.lines)
                fr = Frame(c.offs[0], (c.lines, c.n), (c.pitch, es), x.dtype)
                if c.apart:
                    frames = {"src": fr, "dst": Frame(c.offs[1], (c.lines, c.n), (c.pitch, es), x.dtype)}
                    before, after = {"src": x, "dst": None}, {"src": x, "dst": y}
                else:
                    frames, before, after = {"src": fr}, {"src": x}, {"src": y}

                def call(P, c=c, es=es):
                    j = L.lifting1d_batch(sl, inverse, P["src"], P["dst" if c.apart else "src"], c.pitch, es, c.lines, c.n, DEPTH)
                    assert j == DEPTH, j
                bad += ["%r: %s" % (c, d) for d in run_call(dwt, frames, before, call, after)]
        return bad


# ---- SWT rows and their features -----------------------------------------------------------------------------------------------
class Swt(Family):
    """dwt_backend_swt.hip:16 (swt_fused_ok: the one-launch route needs src % 4 == 0 and line_stride % 4 == 0, which
    check_dev_align at :26 has already demanded) and :36: vec = line_stride % 16 == 0 && src % 16 == 0 -- the load alone
    (dwt_line_lds.h); every store is one element per lane.  Buffers: src, dst_h, dst_l (l_mode 2).  A base 2 bytes off is
    refused (:26)."""
    name, where = "swt", "dwt_backend_swt.hip:36"
    wavelets = ("cdf97_s", "cdf53_s")

    def __init__(self):
        self.cells = row_cells(3, place=lambda s, d: (s, d, (d + 8) % 16), in_place=False)
        self.variants = ["%s-fused%d" % (w, f) for w in self.wavelets for f in (1, 0)]
        self._want = {}

    def terms(self, c):
        return {"line_stride % 16": c.pitch % 16 == 0, "src % 16": c.offs[0] % 16 == 0}

    def data(self, wv, n, lines):
        import swt_model as sm

        key = (wv, n, lines)
        if key not in self._want:
            x = finite((lines, n), "swt", n)
            self._want[key] = (x,) + sm.swt_levels(x, wv, DEPTH)
        return self._want[key]

    def run(self, dwt, variant):
        wv, fused = variant.split("-")
        bad = []
        with Options(dwt, {"swt_fused": int(fused[-1])}, DEFAULTS):
            for c in self.cells:
                x, Lp, Hp = self.data(wv, c.n, c.lines)
                plane = c.pitch * c.lines + 16  # (a gap of canaries between the planes)
                frames = {"src": Frame(c.offs[0], x.shape, (c.pitch, 4)), "h": Frame(c.offs[1], Hp.shape, (plane, c.pitch, 4)),
                          "l": Frame(c.offs[2], Lp.shape, (plane, c.pitch, 4))}

                def call(P, c=c, plane=plane):
                    dwt.swt1d_batch(wv, P["src"], c.pitch, 4, c.lines, c.n, DEPTH, P["h"], P["l"], 2, plane, c.pitch)
                bad += ["%r: %s" % (c, d) for d in run_call(dwt, frames, {"src": x, "h": None, "l": None}, call, {"src": x, "h": Hp, "l": Lp})]
            bad += self.refused(dwt, wv)
        return bad

    def refused(self, dwt, wv):
        """a source 2 bytes off a sample: refused with a message, every byte as it was"""
        x, Lp, Hp = self.data(wv, 65, 5)
        pitch = plane = 65 * 4
        frames = {"src": Frame(2, x.shape, (pitch, 4)), "h": Frame(0, Hp.shape, (plane * 5, pitch, 4)), "l": Frame(0, Lp.shape, (plane * 5, pitch, 4))}
        return run_refused(dwt, frames, {"src": x, "h": None, "l": None},
                           lambda P: dwt.swt1d_batch(wv, P["src"], pitch, 4, 5, 65, DEPTH, P["h"], P["l"], 2, plane * 5, pitch))


class SwtFeatures(Family):
    """dwt_backend_features.hip:405 (swt_features_device): vec = line_stride % 16 == 0 && src % 16 == 0, on the one-launch
    route of swt_fused_ok (dwt_backend_swt.hip:16).  Buffers: src, fv.  The order statistics maxidx, med and maxnorm are
    compared exactly, the median by value (tests/stream_cases.py: the SWT family).  A base 2 bytes off is refused (:573)."""
    name, where = "swt_features", "dwt_backend_features.hip:405"
    names = ["maxidx", "med", "maxnorm"]

    def __init__(self):
        self.cells = row_cells(2, in_place=False)
        self.variants = ["fused1", "fused0"]
        self._want = {}

    terms = Swt.terms

    def data(self, n, lines):
        import features_model as fm
        import swt_model as sm

        key = (n, lines)
        if key not in self._want:
            x = finite((lines, n), "swt features", n)
            planes = sm.swt_levels(x, "cdf97_s", DEPTH)[1]
            fv = np.zeros((lines, len(self.names) * DEPTH), F32)
            for y in range(lines):
                for i, q in enumerate(k for k in fm.NAMES if k in self.names):
                    fv[y, i * DEPTH:(i + 1) * DEPTH] = [fm.order_stats(planes[l, y])[q] for l in range(DEPTH)]
            self._want[key] = (x, fv)
        return self._want[key]

    def run(self, dwt, variant):
        bad = []
        nf = len(self.names) * DEPTH
        stride = nf + 3  # floats from row to row of fv: 3 canaries behind every row
        with Options(dwt, {"swt_fused": int(variant[-1])}, DEFAULTS):
            for c in self.cells:
                x, fv = self.data(c.n, c.lines)
                frames = {"src": Frame(c.offs[0], x.shape, (c.pitch, 4)), "fv": Frame(c.offs[1], fv.shape, (stride * 4, 4))}

                def call(P, c=c):
                    dwt.swt_features1d_batch("cdf97_s", self.names, P["src"], c.pitch, 4, c.lines, c.n, DEPTH, P["fv"], stride, 0, 2.0)
                # (the median by value, as tests/test_hip_swt.py and tests/stream_cases.py compare it: a zero's sign is not told)
                med = (slice(None), slice(DEPTH, 2 * DEPTH))
                bad += ["%r: %s" % (c, d) for d in run_call(dwt, frames, {"src": x, "fv": None}, call, {"src": x, "fv": fv}, {"fv": med})]
            x, fv = self.data(65, 5)
            bad += run_refused(dwt, {"src": Frame(2, x.shape, (260, 4)), "fv": Frame(0, fv.shape, (stride * 4, 4))}, {"src": x, "fv": None},
                               lambda P: dwt.swt_features1d_batch("cdf97_s", self.names, P["src"], 260, 4, 5, 65, DEPTH, P["fv"], stride, 0, 2.0))
        return bad


# ---- 3-D levels ----------------------------------------------------------------------------------------------------------------
class Vol3d(Family):
    """dwt_vol3d.hip:519-523 (vol_fused_vec_ok): in % 16 == 0 && in_sy % 16 == 0 && in_sz % 16 == 0 (bytes) and the same of
    out; :247 full = MODE >= 1 || (vec_ok && the tile lies inside the row); :250 halo16 = full && the tile is interior
    (c0 >= 4 && c0 + 260 <= nx, c0 a multiple of 256).  The multi-level modes and the whole-tile variant (MODE 4, what an
    out-of-place level runs as by default) address every row as a buffer and take `full`, hence `halo16`, whatever the
    alignment: an interior tile fetches each halo as one 16-byte piece from a row that may be only 4-byte aligned.  :707: the
    lattice merge of the two-pass levels (16-byte pieces of the destination) needs dst % 16 == 0 and strides % 16 == 0.
    Buffers: src, dst (transform3d_op), or the volume alone.  A base 2 bytes off is refused (dwt_backend_vol.hip)."""
    name, where, kind = "vol3d", "dwt_vol3d.hip:247-281, :519-523, :707", "tile"  # (every nx here is a multiple of 4: the tail is the tile's overhang)
    shapes = (((6, 9, 768), 1), ((6, 9, 300), 1), ((7, 34, 516), 2))  # (z, y, x), levels: an interior tile; overhang; the smallest nx with an interior tile, levels 0 and 1 merged

    def __init__(self):
        self.cells = []
        for (nz, ny, nx), levels in self.shapes:
            for fused in (2, 0):
                for r in RESIDUES:
                    for zpad in (0, 4):
                        sy = nx * 4 + r
                        for apart, offs in [(False, (o, o)) for o in OFFSETS] + [(True, p) for p in PAIRS]:
                            self.cells.append(Cell(offs, sy, nx, ny, nz=nz, sz=sy * ny + zpad, levels=levels, fused=fused, apart=apart))
        self.variants = ["%dx%dx%d-%s" % (s + (e,)) for s, _ in self.shapes for e in ("op", "fwd", "inv")]
        self._want = {}

    def terms(self, c):
        return {"an interior tile": any(c0 >= 4 and c0 + 260 <= c.n for c0 in range(0, c.n, 256)), "in % 16": c.offs[0] % 16 == 0,
                "out % 16": c.offs[1] % 16 == 0, "stride_y % 16": c.pitch % 16 == 0, "stride_z % 16": c.sz % 16 == 0}

    def cells_of(self, variant):
        shape, entry = variant.split("-")
        nz, ny, nx = map(int, shape.split("x"))
        return [c for c in self.cells if (c.nz, c.lines, c.n) == (nz, ny, nx) and c.apart == (entry == "op")]

    def data(self, shape, levels, inverse):
        from test_hip_volume import oracle_multilevel

        key = (shape, levels, inverse)
        if key not in self._want:
            x = _rng("vol3d", *shape).random(shape, dtype=F32)  # [0, 1): the reflected ends do not show (tests/test_hip_sweep_matrix.py)
            self._want[key] = (x, oracle_multilevel(orc(), x.copy(), levels, bool(inverse)))
        return self._want[key]

    def run(self, dwt, variant):
        entry = variant.split("-")[1]
        inverse = int(entry == "inv")
        bad = []
        for c in self.cells_of(variant):
            shape = (c.nz, c.lines, c.n)
            x, y = self.data(shape, c.levels, inverse)
            with Options(dwt, {"vol_fused": c.fused}, DEFAULTS):
                if entry == "op":
                    frames = {"src": Frame(c.offs[0], shape, (c.sz, c.pitch, 4)), "dst": Frame(c.offs[1], shape, (c.sz, c.pitch, 4))}

                    def call(P, c=c):
                        dwt.transform3d_op(P["src"], P["dst"], c.pitch, c.sz, c.n, c.lines, c.nz, c.levels)
                    got = run_call(dwt, frames, {"src": x, "dst": None}, call, {"src": x, "dst": y})
                else:
                    frames = {"vol": Frame(c.offs[0], shape, (c.sz, c.pitch, 4))}

                    def call(P, c=c):
                        dwt.transform3d(inverse, P["vol"], c.pitch, c.sz, c.n, c.lines, c.nz, c.levels)
                    got = run_call(dwt, frames, {"vol": x}, call, {"vol": y})
            bad += ["%r: %s" % (c, d) for d in got]
        sy, sz = c.n * 4, c.n * 4 * c.lines
        if entry == "op":
            frames = {"src": Frame(0, shape, (sz, sy, 4)), "dst": Frame(2, shape, (sz, sy, 4))}
            bad += run_refused(dwt, frames, {"src": x, "dst": None}, lambda P: dwt.transform3d_op(P["src"], P["dst"], sy, sz, c.n, c.lines, c.nz, c.levels))
        else:
            bad += run_refused(dwt, {"vol": Frame(2, shape, (sz, sy, 4))}, {"vol": x}, lambda P: dwt.transform3d(inverse, P["vol"], sy, sz, c.n, c.lines, c.nz, c.levels))
        return bad


# ---- inverse SWT rows ----------------------------------------------------------------------------------------------------------
class Iswt(Family):
    """dwt_backend_iswt.hip:63 (iswt1d_device): vec = all16(src_h, src_l, plane stride where levels > 1, source line stride):
    the L line (dwt_line_lds.h) and every level's H line (detail_to_lds, dwt_iswt1d.hip:35-50) load 16 bytes per lane; every
    store is one element per lane.  Buffers: src_h, src_l, dst.  A base 2 bytes off is refused (:50)."""
    name, where = "iswt", "dwt_backend_iswt.hip:63"
    wavelets = ("cdf97_s", "cdf53_s")

    def __init__(self):
        self.cells = row_cells(3, place=lambda s, d: (s, d, (s + 8) % 16), in_place=False)
        for c in self.cells:
            c.more["pgap"] = 16  # bytes of canary between the H planes
        # (5 lines: the plane stride follows the line stride unless the gap makes up for it)
        self.cells += alone(self, [Cell((0, 0, 4), pitch_for(65 * 4, r), 65, 5, apart=True, pgap=g) for r in RESIDUES for g in (16, 4, 8, 12)])
        self.variants = ["%s-fused%d" % (w, f) for w in self.wavelets for f in (1, 0)]
        self._want = {}

    def terms(self, c):
        return {"src_h % 16": c.offs[0] % 16 == 0, "src_l % 16": c.offs[1] % 16 == 0, "plane_stride % 16": (c.pitch * c.lines + c.pgap) % 16 == 0,
                "src_line_stride % 16": c.pitch % 16 == 0}

    def tables(self):
        import iswt_model as im

        return np.array([im.SOFT, im.KEEP, im.HARD], I32), np.array([0.3, 0.0, 0.3], F32)  # (tests/iswt_stream.py: operators on load)

    def data(self, wv, n, lines):
        import iswt_model as im

        key = (wv, n, lines)
        if key not in self._want:
            H, L = finite((DEPTH, lines, n), "iswt h", n), finite((lines, n), "iswt l", n)
            self._want[key] = (H, L, im.iswt_levels(L, H, wv, *self.tables()))
        return self._want[key]

    def run(self, dwt, variant):
        from libdwt_amd import stationary as st

        wv, fused = variant.split("-")
        ops, params = self.tables()
        bad = []
        with Options(dwt, {"swt_fused": int(fused[-1])}, DEFAULTS):
            for c in self.cells:
                H, L, y = self.data(wv, c.n, c.lines)
                plane = c.pitch * c.lines + c.pgap
                frames = {"h": Frame(c.offs[0], H.shape, (plane, c.pitch, 4)), "l": Frame(c.offs[1], L.shape, (c.pitch, 4)),
                          "dst": Frame(c.offs[2], y.shape, (c.pitch, 4))}

                def call(P, c=c, plane=plane):
                    st.iswt1d_batch(wv, st.BORDER_SYMMETRIC, P["h"], P["l"], plane, c.pitch, c.lines, c.n, DEPTH, P["dst"], c.pitch, ops=ops, params=params)
                bad += ["%r: %s" % (c, d) for d in run_call(dwt, frames, {"h": H, "l": L, "dst": None}, call, {"h": H, "l": L, "dst": y})]
            H, L, y = self.data(wv, 65, 5)
            frames = {"h": Frame(0, H.shape, (260 * 5, 260, 4)), "l": Frame(2, L.shape, (260, 4)), "dst": Frame(0, y.shape, (260, 4))}
            bad += run_refused(dwt, frames, {"h": H, "l": L, "dst": None},
                               lambda P: st.iswt1d_batch(wv, st.BORDER_SYMMETRIC, P["h"], P["l"], 260 * 5, 260, 5, 65, DEPTH, P["dst"], 260))
        return bad


# ---- packets and pruned trees of rows ------------------------------------------------------------------------------------------
class Wp(Family):
    """dwt_wp1d.hip:69 (wp_lines_t) and dwt_wp_basis.hip:230 (wp_tree_t; :270 wp_best_t is the same rule): vec = elem_stride ==
    4 && line_stride % 16 == 0 && src % 16 == 0 && dst % 16 == 0; the load of dwt_line_lds.h and the whole-line store of
    dwt_wp_level.h:96-101 follow it.  A base 2 bytes off is refused (dwt_backend_wp.hip:185, :378)."""
    name, where = "wp", "dwt_wp1d.hip:69, dwt_wp_basis.hip:230"
    SPLITS = (1, 2, 5)  # a pruned tree of depth 3: leaves at levels 1, 2, 3 and 3

    def __init__(self):
        self.cells = row_cells(2)
        self.cells.append(Cell((0, 0), pitch_for(65 * 8, 0), 65, 5, apart=False, es=8))
        self.variants = ["%s-%s-%s" % (e, w, d) for e, w in (("packets", "cdf97_s"), ("packets", "interp53_s"), ("tree", "cdf53_s")) for d in ("fwd", "inv")]
        self._want = {}

    terms = Oned.terms

    def data(self, entry, wv, inverse, n, lines):
        import wp_basis_model as bm
        import wp_model as wp

        key = (entry, wv, inverse, n, lines)
        if key not in self._want:
            x = finite((lines, n), "wp", n)
            if entry == "packets":
                y = (wp.inv1d if inverse else wp.fwd1d)(wv, x, DEPTH)
            else:
                y = (bm.inv_tree if inverse else bm.fwd_tree)(wv, x, DEPTH, bm.tree_of(self.SPLITS))
            self._want[key] = (x, y)
        return self._want[key]

    def run(self, dwt, variant):
        import wp_basis_model as bm
        import wp_model as wp
        from libdwt_amd import packets

        entry, wv, direction = variant.split("-")
        inverse, wid, tree = int(direction == "inv"), wp.WAVELET_ID[wv], bm.tree_of(self.SPLITS)

        def entry_call(src, dst, pitch, es, lines, n):
            if entry == "packets":
                packets.wp1d_batch(wid, inverse, src, dst, pitch, es, lines, n, DEPTH)
            else:
                packets.wp_tree1d_batch(wid, inverse, src, dst, pitch, es, lines, n, DEPTH, tree, 0)
        bad = []
        for c in self.cells:
            es = c.more.get("es", 4)
            x, y = self.data(entry, wv, inverse, c.n, c.lines)
            fr = Frame(c.offs[0], (c.lines, c.n), (c.pitch, es))
            if c.apart:
                frames = {"src": fr, "dst": Frame(c.offs[1], (c.lines, c.n), (c.pitch, es))}
                before, after = {"src": x, "dst": None}, {"src": x, "dst": y}
            else:
                frames, before, after = {"src": fr}, {"src": x}, {"src": y}
            bad += ["%r: %s" % (c, d) for d in run_call(
                dwt, frames, before, lambda P, c=c, es=es: entry_call(P["src"], P["dst" if c.apart else "src"], c.pitch, es, c.lines, c.n), after)]
        x, _ = self.data(entry, wv, inverse, 65, 5)
        bad += run_refused(dwt, {"src": Frame(2, x.shape, (260, 4))}, {"src": x}, lambda P: entry_call(P["src"], P["src"], 260, 4, 5, 65))
        return bad


# ---- conditioning --------------------------------------------------------------------------------------------------------------
class Condition(Family):
    """dwt_backend_condition.hip:200 (dwt_hip_rows_condition, the fused route): vec = line_stride % 16 == 0 && ptr % 16 == 0;
    the rows come in through dwt_line_lds.h and go out by the store of dwt_condition.hip:178-181.  Under cond_fused 0 every
    operation is a kernel of its own, one element per lane.  Buffers: the rows, info.  Compared as tests/test_hip_condition.py
    compares: bit for bit, zeros by value.  A base 2 bytes off is refused (check_rows, :81)."""
    name, where = "condition", "dwt_backend_condition.hip:200"
    KINDS = ("spectrum", "two_peaks", "edge", "tiny", "exact")

    def __init__(self):
        self.cells = row_cells(2, apart=False)
        self.variants = ["fused1", "fused0"]
        self._want = {}

    def terms(self, c):
        return {"line_stride % 16": c.pitch % 16 == 0, "ptr % 16": c.offs[0] % 16 == 0}

    def data(self, n, lines):
        import condition_model as cm

        key = (n, lines)
        if key not in self._want:
            x = np.concatenate([cm.make_input(2000 + 17 * k + n, kind, 1, n) for k, kind in enumerate(self.KINDS[:lines])])
            self._want[key] = (x,) + cm.condition(x, 7, 20, -1.0, 2.5)
        return self._want[key]

    def run(self, dwt, variant):
        bad = []
        with Options(dwt, {"cond_fused": int(variant[-1])}, DEFAULTS):
            for c in self.cells:
                x, y, info = self.data(c.n, c.lines)
                frames = {"rows": Frame(c.offs[0], x.shape, (c.pitch, 4)), "info": Frame(c.offs[1], info.shape, (16, 4), I32)}

                def call(P, c=c):
                    dwt.rows_condition(7, P["rows"], c.pitch, 4, c.lines, c.n, 20, -1.0, 2.5, P["info"])
                bad += ["%r: %s" % (c, d) for d in run_call(dwt, frames, {"rows": x, "info": None}, call, {"rows": y, "info": info}, {"rows": Ellipsis})]
            x, _, info = self.data(65, 5)
            frames = {"rows": Frame(2, x.shape, (260, 4)), "info": Frame(0, info.shape, (16, 4), I32)}
            bad += run_refused(dwt, frames, {"rows": x, "info": None}, lambda P: dwt.rows_condition(7, P["rows"], 260, 4, 5, 65, 20, -1.0, 2.5, P["info"]))
        return bad


# ---- frame families: N-term and band operators ---------------------------------------------------------------------------------
FRAME_W, FRAME_H, FRAME_BATCH, FRAME_LEVELS = (36, 37, 38, 39), 29, 2, 3  # subband origins then fall on every residue


def frame_cells(n_bufs, **more):
    """every base offset and pitch residue at every width; `more`: the family's further strides (their gaps)"""
    cells = []
    for w in FRAME_W:
        for r in RESIDUES:
            pitch = pitch_for(w * 4, r)
            cells += [Cell((o,) if n_bufs == 1 else o, pitch, w, FRAME_H, **more) for o in (OFFSETS if n_bufs == 1 else PAIRS)]
    return cells


class Nterm(Family):
    """dwt_backend_nterm.hip:65-73, :99 (stage_groups): vec = all_16(img; pitch, batch stride, channel stride), and :237 for
    the magnitude map: && all_16(map; map pitch, map batch stride).  dwt_nterm.hip:149: a lane's four samples are one 16-byte
    access where vec holds and all four lie in the row (`quad`), single elements otherwise -- so with w % 4 != 0 a row's last
    lane takes the element path inside a vec call.  Buffers: the groups (keep_largest_batch), or the groups and the map
    (magnitude_batch).  A base 2 bytes off is refused (:115, :217)."""
    name, where = "nterm", "dwt_backend_nterm.hip:65-73, :99, :237; dwt_nterm.hip:149"
    CH = 2

    def __init__(self):
        gaps = (0, 4, 8, 12)
        self.keep_cells = frame_cells(1, entry="keep", cgap=0, bgap=0, mres=0, mgap=0)
        self.keep_cells += alone(self, [Cell((o,), pitch_for(37 * 4, r), 37, FRAME_H, entry="keep", cgap=cg, bgap=bg, mres=0, mgap=0)
                                        for o in OFFSETS for r in RESIDUES for cg in gaps for bg in gaps])
        self.map_cells = frame_cells(2, entry="map", cgap=0, bgap=0, mres=0, mgap=0)
        self.map_cells += alone(self, [Cell(p, pitch_for(37 * 4, r), 37, FRAME_H, entry="map", cgap=cg, bgap=bg, mres=mr, mgap=mg)
                                       for p in PAIRS for r in RESIDUES for cg in gaps for bg in gaps for mr in gaps for mg in gaps])
        self.cells = self.keep_cells + self.map_cells
        self.variants = ["keep_largest_batch", "magnitude_batch"]
        self._want = {}

    def strides(self, c):
        cs = c.pitch * c.lines + c.cgap
        mp = c.pitch + c.mres
        return cs, cs * self.CH + c.bgap, mp, mp * c.lines + c.mgap

    def terms(self, c):
        cs, bs, mp, mbs = self.strides(c)
        t = {"img % 16": c.offs[0] % 16 == 0, "pitch % 16": c.pitch % 16 == 0, "channel_stride % 16": cs % 16 == 0, "batch_stride % 16": bs % 16 == 0}
        # (a call of keep_largest_batch has no map: its terms hold there)
        m = c.entry == "map"
        t.update({"map % 16": not m or c.offs[1] % 16 == 0, "map_pitch % 16": not m or mp % 16 == 0, "map_batch_stride % 16": not m or mbs % 16 == 0})
        return t

    def cells_of(self, variant):
        return self.keep_cells if variant == "keep_largest_batch" else self.map_cells

    def data(self, w):
        import nterm_model as nm

        if w not in self._want:
            x = np.stack([nm.make_input(600 + 10 * w + b, "normal", self.CH, FRAME_H, w) * F32(10.0 ** (b - 1)) for b in range(FRAME_BATCH)])
            keep = [w * FRAME_H // 2, 17]
            kept = [nm.keep_largest(x[b], keep[b]) for b in range(FRAME_BATCH)]
            self._want[w] = (x, keep, np.stack([k[0] for k in kept]), np.array([k[1] for k in kept], F32), np.array([k[2] for k in kept], I32),
                             np.stack([nm.magnitudes(x[b]) for b in range(FRAME_BATCH)]))
        return self._want[w]

    def run(self, dwt, variant):
        bad = []
        for c in self.cells_of(variant):
            x, keep, y, thr, kept, mag = self.data(c.n)
            cs, bs, mp, mbs = self.strides(c)
            fr = Frame(c.offs[0], x.shape, (bs, cs, c.pitch, 4))
            if c.entry == "keep":
                records = []

                def call(P, c=c, cs=cs, bs=bs):
                    records.extend(dwt.keep_largest_batch(P["x"], bs, FRAME_BATCH, self.CH, cs, c.pitch, c.n, c.lines, keep))
                got = run_call(dwt, {"x": fr}, {"x": x}, call, {"x": y})
                if not (np.array_equal(records[0].view(np.uint32), thr.view(np.uint32)) and np.array_equal(records[1], kept)):
                    got.append("thresholds %s and kept counts %s, expected %s and %s" % (records[0], records[1], thr, kept))
            else:
                def call(P, c=c, cs=cs, bs=bs, mp=mp, mbs=mbs):
                    dwt.magnitude_batch(P["x"], bs, FRAME_BATCH, self.CH, cs, c.pitch, c.n, c.lines, P["m"], mbs, mp)
                got = run_call(dwt, {"x": fr, "m": Frame(c.offs[1], mag.shape, (mbs, mp, 4))}, {"x": x, "m": None}, call, {"x": x, "m": mag})
            bad += ["%r: %s" % (c, d) for d in got]
        x, keep, y, thr, kept, mag = self.data(37)
        cs, bs = 160 * FRAME_H, 160 * FRAME_H * self.CH
        if variant == "keep_largest_batch":
            bad += run_refused(dwt, {"x": Frame(2, x.shape, (bs, cs, 160, 4))}, {"x": x},
                               lambda P: dwt.keep_largest_batch(P["x"], bs, FRAME_BATCH, self.CH, cs, 160, 37, FRAME_H, keep))
        else:
            bad += run_refused(dwt, {"x": Frame(0, x.shape, (bs, cs, 160, 4)), "m": Frame(2, mag.shape, (cs, 160, 4))}, {"x": x, "m": None},
                               lambda P: dwt.magnitude_batch(P["x"], bs, FRAME_BATCH, self.CH, cs, 160, 37, FRAME_H, P["m"], cs, 160))
        return bad


def band_slots(w, h, levels):
    """shape_model.slots of a dense frame: [(x0, y0, w, h)] of the 3 J + 1 subbands"""
    import shape_model as sm

    return sm.slots(w, h, w, h, levels)


class Bandops(Family):
    """dwt_bandops.hip:45 (walk_rows): per row of a band, lead = ((16 - (row address & 15)) & 15) >> 2 elements are peeled up to
    the first 16-byte boundary, the rest goes as aligned 16-byte accesses, and what is left behind the last boundary is
    peeled again.  A band starts ceil(size / 2^j) elements into a row: there is no predicate, every call mixes the paths.
    Operators: zero, scale, hard and soft threshold (bit for bit; no COMPRESS).  A base 2 bytes off is refused
    (dwt_backend_bandops.hip:122)."""
    name, where, kind = "bandops", "dwt_bandops.hip:45", "peel"
    peels = ("lead", "tail")

    def __init__(self):
        self.cells = frame_cells(1, bgap=0)
        self.cells += alone(self, [Cell((o,), pitch_for(37 * 4, r), 37, FRAME_H, bgap=g) for o in OFFSETS for r in RESIDUES for g in (0, 4, 8, 12)])
        self.variants = ["bands_apply_batch"]
        self._want = {}

    def terms(self, c):
        # (no predicate; the terms say what the row addresses depend on, and the cells stand on both sides of each)
        return {"ptr % 16": c.offs[0] % 16 == 0, "pitch % 16": c.pitch % 16 == 0, "batch_stride % 16": (c.pitch * c.lines + c.bgap) % 16 == 0}

    def table(self):
        import shape_model as sm

        ops = [(sm.ZERO, sm.SCALE, sm.HARD, sm.SOFT)[k % 4] for k in range(3 * FRAME_LEVELS + 1)]
        return np.array(ops, I32), np.array([sm.PARAM[o] for o in ops], F32)

    def peel(self, c):
        """the lead and tail counts of every row of every band of every frame of the cell"""
        out = {"lead": set(), "tail": set()}
        for b in range(FRAME_BATCH):
            for x0, y0, w, h in band_slots(c.n, c.lines, FRAME_LEVELS):
                for r in range(h):
                    addr = c.offs[0] + b * (c.pitch * c.lines + c.bgap) + (y0 + r) * c.pitch + 4 * x0  # (LEAD is a multiple of 16)
                    lead = ((16 - (addr & 15)) & 15) >> 2
                    head = min(lead, w)
                    out["lead"].add(lead)
                    out["tail"].add((w - head) & 3)
        return out

    def data(self, w):
        import shape_model as sm

        if w not in self._want:
            x = np.stack([sm.make_input(700 + 10 * w + b, FRAME_H, w) for b in range(FRAME_BATCH)])
            ops, params = self.table()
            self._want[w] = (x, np.stack([sm.apply_table(x[b], w, FRAME_H, w, FRAME_H, FRAME_LEVELS, ops, params) for b in range(FRAME_BATCH)]))
        return self._want[w]

    def run(self, dwt, variant):
        ops, params = self.table()
        bad = []
        for c in self.cells:
            x, y = self.data(c.n)
            bs = c.pitch * c.lines + c.bgap

            def call(P, c=c, bs=bs):
                dwt.bands_apply_batch(P["x"], bs, FRAME_BATCH, c.pitch, c.n, c.lines, FRAME_LEVELS, ops, params)
            bad += ["%r: %s" % (c, d) for d in run_call(dwt, {"x": Frame(c.offs[0], x.shape, (bs, c.pitch, 4))}, {"x": x}, call, {"x": y})]
        x, _ = self.data(37)
        bad += run_refused(dwt, {"x": Frame(2, x.shape, (160 * FRAME_H, 160, 4))}, {"x": x},
                           lambda P: dwt.bands_apply_batch(P["x"], 160 * FRAME_H, FRAME_BATCH, 160, 37, FRAME_H, FRAME_LEVELS, ops, params))
        return bad


# ---- windows of the inverse ----------------------------------------------------------------------------------------------------
class Window(Family):
    """dwt_window2d.hip:115 (store_run16): a row of the window goes out in 16-byte runs counted from the aligned address below
    it: head = (address & 15) / element size elements lie between that address and the row, a run that lies in the row whole
    is one access, the runs at its ends go element by element.  Both routes end in it: the window kernel's last level (route
    2, per tile: a window across the seam of two 64-column tiles has two row pieces) and the copy out of the full inverse
    (route 0, k_window_copy).  No predicate: every call mixes the paths.  Both element sizes: float 9/7 (4 bytes, head 0 .. 3)
    and the int16 5/3 (2 bytes, head 0 .. 7).  The window's x origin and width take every residue mod 4.  Buffers: the frames,
    the windows.  A base that is no multiple of the element is refused (dwt_backend_window.hip:63, :66)."""
    name, where, kind = "window", "dwt_window2d.hip:115", "peel"
    peels = ("head",)
    B, H, W, J, Y0, WH, TILE = 2, 67, 131, 3, 5, 9, 64
    wavelets = {"cdf97_s": (4, OFFSETS, RESIDUES), "cdf53_i16": (2, (0, 2, 4, 6, 8, 10, 12, 14), (0, 2, 8, 14))}

    def __init__(self):
        self.cells = []
        for wv, (es, offsets, residues) in self.wavelets.items():
            for x0 in (60, 61, 62, 63):          # every residue mod 4; the window crosses the tile seam at column 64
                for ww in (12, 13, 14, 15):
                    for off in offsets:
                        for r in residues:
                            self.cells.append(Cell((off, off), pitch_for(ww * es, r), ww, self.WH, wv=wv, es=es, x0=x0))
        self.variants = ["%s-route%d" % (w, r) for w in self.wavelets for r in (2, 0)]
        self._want = {}

    def terms(self, c):
        # (no predicate; what the row addresses of the destination depend on)
        return {"dst % 16": c.offs[1] % 16 == 0, "dst_pitch % 16": c.pitch % 16 == 0}

    def peel(self, c):
        """the head counts of every row piece: the rows of the window (route 0), cut at the tile seams (route 2)"""
        out = set()
        starts = [0] + [t - c.x0 for t in range(self.TILE, self.W, self.TILE) if c.x0 < t < c.x0 + c.n]
        for y in range(c.lines):
            for k in starts:
                out.add(((c.offs[1] + y * c.pitch + k * c.es) & 15) // c.es)
        return {"head": out}

    def cells_of(self, variant):
        return [c for c in self.cells if c.wv == variant.split("-")[0]]

    def data(self, wv):
        import window_model as wm

        if wv not in self._want:
            x = np.stack([wm.make_frame(wv, 9900 + b, self.H, self.W) for b in range(self.B)])
            self._want[wv] = (x, np.stack([wm.full_inverse(orc(), wv, f, self.J, 0) for f in x]))
        return self._want[wv]

    def run(self, dwt, variant):
        from libdwt_amd import window

        wv, route = variant.split("-")
        x, full = self.data(wv)
        es = x.dtype.itemsize
        bad = []
        with Options(dwt, {"window_fused": int(route[-1])}, DEFAULTS):
            for c in self.cells_of(variant):
                y = full[:, self.Y0:self.Y0 + c.lines, c.x0:c.x0 + c.n]
                dbs = c.pitch * c.lines + 16
                frames = {"src": Frame(c.offs[0], x.shape, (es * self.W * self.H, es * self.W, es), x.dtype),
                          "dst": Frame(c.offs[1], y.shape, (dbs, c.pitch, es), x.dtype)}

                def call(P, c=c, dbs=dbs):
                    window.inverse_window_batch(wv, P["src"], es * self.W * self.H, self.B, es * self.W, self.W, self.H, self.J, 0,
                                                c.x0, self.Y0, c.n, c.lines, P["dst"], dbs, c.pitch)
                bad += ["%r: %s" % (c, d) for d in run_call(dwt, frames, {"src": x, "dst": None}, call, {"src": x, "dst": y})]
            frames = {"src": Frame(0, x.shape, (es * self.W * self.H, es * self.W, es), x.dtype), "dst": Frame(es // 2, (self.B, 9, 12), (16 * 9 * es, 16 * es, es), x.dtype)}
            bad += run_refused(dwt, frames, {"src": x, "dst": None},
                               lambda P: window.inverse_window_batch(wv, P["src"], es * self.W * self.H, self.B, es * self.W, self.W, self.H, self.J, 0,
                                                                     60, 5, 12, 9, P["dst"], 16 * 9 * es, 16 * es), "bad strides of the destination")
        return bad


# ---- 2-D Mallat and interleaved entries ----------------------------------------------------------------------------------------
class Mallat2d(Family):
    """dwt_abi.hip:396 (dwt_hip_transform2d) and dwt_backend_il.hip:451 (the interleaved entries): a device image runs where
    it lies if its elements are adjacent and base and pitch are multiples of the element size; anything else takes the
    staging detour (dwt_strided.hip packs such elements byte by byte).  dwt_hip_transform2d_batch has no detour: it refuses
    such a base.  The sweeps address every row as a buffer, so 4 bytes of alignment suffice for them; the rule that is left is
    Call2d::aligned (dwt_backend.hip:50-67): the 2-byte wavelets take their fused sweeps (dwt_sweep2d_i16.hip:35,
    dwt_sweep2d_h.hip:36: a lane's own bytes of a row are dword-aligned) only if every base, pitch and batch stride is a
    multiple of 4 bytes, the exact line passes otherwise; and dwt_backend_il.hip:171, :312-359 ask the same of the bases of an
    interleaved call.  Buffers: the image (in-place entries), or source and destination (transform2d_batch, 2 images)."""
    name, where, kind = "mallat2d", "dwt_abi.hip:396; dwt_backend.hip:50-67; dwt_backend_il.hip:171, :312-359, :451", "route"
    SHAPES = ((48, 64, 2), (67, 259, 7))  # (h, w, levels): two dense levels; odd sizes at every level, at full depth
    ORACLE = {"cdf97_s": "cdf97_2%s_s", "cdf53_i": "cdf53_2%s_i", "cdf53_s": "cdf53_2%s_s", "cdf97_d": "cdf97_2%s_d", "cdf53_d": "cdf53_2%s_d",
              "cdf97_i": "cdf97_2%s_i"}
    ENTRY = dict(ORACLE, interp53_s="interp53_2%s_s", cdf53_i16="cdf53_2%s_i16", cdf97_h="cdf97_2%s_h")
    INTERLEAVED = ("cdf97_s", "cdf53_s", "cdf97_i")

    def __init__(self):
        from stream_cases import WAVELETS_2D

        self.dtypes = dict(WAVELETS_2D)
        self.cells = []
        for wv, dt in self.dtypes.items():
            es = np.dtype(dt).itemsize
            offsets = {2: (0, 2, 4, 8), 4: (0, 4, 8, 12), 8: (0, 8)}[es]
            for layout in ("mallat",) + (("interleaved",) if wv in self.INTERLEAVED else ()):
                for h, w, levels in self.SHAPES:
                    for pad in (0, es):  # a pitch residue of 0 and of one element
                        for k, off in enumerate(offsets):
                            more = dict(wv=wv, es=es, levels=levels, layout=layout)
                            self.cells.append(Cell((off, off), w * es + pad, w, h, entry="inplace", **more))
                            if layout == "mallat":
                                self.cells.append(Cell((off, offsets[(k + 1) % len(offsets)]), w * es + pad, w, h, entry="batch", **more))
            # a base that is no multiple of the element: the in-place entry stages it, the batch entry refuses it
            if es >= 4:
                self.cells.append(Cell((es // 2, es // 2), 64 * es, 64, 48, entry="inplace", wv=wv, es=es, levels=2, layout="mallat", odd=True))
        self.variants = ["%s-%s" % (w, d) for w in self.dtypes for d in ("fwd", "inv")]
        self._want = {}

    def terms(self, c):
        return {"base % element": all(o % c.es == 0 for o in c.offs), "base % 4": all(o % 4 == 0 for o in c.offs), "pitch % 4": c.pitch % 4 == 0}

    def cells_of(self, variant):
        return [c for c in self.cells if c.wv == variant.split("-")[0]]

    def model(self, wv, inverse, img, levels, interleaved):
        if interleaved:
            name = self.ORACLE[wv].replace("2%s", "2%s_inplace") % ("i" if inverse else "f")
            (orc().inv if inverse else orc().fwd)(name, img, levels)
        elif wv in self.ORACLE:
            (orc().inv if inverse else orc().fwd)(self.ORACLE[wv] % ("i" if inverse else "f"), img, levels)
        else:
            import f16_model
            import i16_model
            import interp53_model

            m = {"interp53_s": interp53_model, "cdf53_i16": i16_model, "cdf97_h": f16_model}[wv]
            (m.inv2d if inverse else m.fwd2d)(img, j_max=levels)
        return img

    def data(self, wv, inverse, h, w, levels, interleaved):
        key = (wv, inverse, h, w, interleaved)
        if key not in self._want:
            dt, rng = self.dtypes[wv], _rng("mallat2d", wv, h, w)
            if dt == np.float16:  # small integers: nothing overflows at either depth (tests/stream_cases.py)
                x = rng.integers(0, 256 if levels <= 2 else 16, size=(2, h, w)).astype(dt)
            elif np.issubdtype(dt, np.integer):
                x = rng.integers(-2048, 2048, size=(2, h, w)).astype(dt)
            else:
                from floatends import finite_floats

                x = finite_floats(rng, (2, h, w), dt)
            self._want[key] = (x, np.stack([self.model(wv, inverse, img.copy(), levels, interleaved) for img in x]))
        return self._want[key]

    def run(self, dwt, variant):
        wv, direction = variant.split("-")
        inverse = int(direction == "inv")
        bad = []
        for c in self.cells_of(variant):
            il = c.layout == "interleaved"
            x, y = self.data(wv, inverse, c.lines, c.n, c.levels, il)
            es, dt = c.es, x.dtype
            if c.entry == "inplace":
                stem = self.ORACLE[wv].replace("2%s", "2%s_inplace") if il else self.ENTRY[wv]
                fn = getattr(dwt, "dwt_" + stem % ("i" if inverse else "f"))
                frames = {"x": Frame(c.offs[0], x[0].shape, (c.pitch, es), dt)}
                got = run_call(dwt, frames, {"x": x[0]}, lambda P, c=c: fn(P["x"], c.pitch, es, c.n, c.lines, c.n, c.lines, c.levels), {"x": y[0]})
            else:
                bs = c.pitch * c.lines + 16  # (16 bytes of canary between the images)
                frames = {"src": Frame(c.offs[0], x.shape, (bs, c.pitch, es), dt), "dst": Frame(c.offs[1], x.shape, (bs, c.pitch, es), dt)}
                got = run_call(dwt, frames, {"src": x, "dst": None},
                               lambda P, c=c, bs=bs: dwt.transform2d_batch(wv, inverse, P["src"], P["dst"], bs, 2, c.pitch, c.n, c.lines, c.levels),
                               {"src": x, "dst": y})
            bad += ["%r: %s" % (c, d) for d in got]
        es = np.dtype(self.dtypes[wv]).itemsize
        if es >= 4:
            x, _ = self.data(wv, inverse, 48, 64, 2, False)
            bs = 64 * es * 48
            frames = {"src": Frame(es // 2, x.shape, (bs, 64 * es, es), x.dtype), "dst": Frame(0, x.shape, (bs, 64 * es, es), x.dtype)}
            bad += run_refused(dwt, frames, {"src": x, "dst": None},
                               lambda P: dwt.transform2d_batch(wv, inverse, P["src"], P["dst"], bs, 2, 64 * es, 64, 48, 2), "multiples of the element size")
        return bad


FAMILIES = {f.name: f for f in (Oned(), Lifting1d(), Swt(), SwtFeatures(), Iswt(), Wp(), Condition(), Nterm(), Bandops(), Window(), Mallat2d(), Vol3d())}
