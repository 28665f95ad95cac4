"""CPU checks of the embedded bit-plane streams of code-blocks: the numpy model (tests/bitplane_model.py) against the
format's own promises -- the round trip, dropped planes, a cut stream, the size rule against the bit-plane map of
tests/quant_model.py -- and the library's host geometry (dwt_hip_bitplane_bands / _block / _words) against that model.  The
device entries are held to the model in tests/test_hip_bitplanes.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import bitplane_model as bpm
import quant_model as qm
import shape_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 3, 2), (1, 37, -1), (37, 1, -1), (72, 40, 3), (264, 136, 3)]
EXPONENTS = [(2, 2), (3, 5), (6, 6), (10, 2), (2, 10)]


@pytest.fixture(scope="module")
def dwt():
    import __graft_entry__ as g

    if not os.path.exists(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")):
        g.build()
    import libdwt_amd as d
    from libdwt_amd import bitplanes

    d.bitplanes = bitplanes
    return d


def frames_of(index_type, B, H, W, seed, bits=None):
    """frame 0 all zero; the others: blocks of very different magnitudes -- zeros, +-1, a few bits, the whole range -- by
    regions of 8 x 8 samples, with the extremes somewhere"""
    rng = np.random.default_rng([seed, index_type, B, H, W])
    info = np.iinfo(bpm.DTYPE[index_type])
    top = bits if bits is not None else rng.integers(0, info.bits + 1, (B, -(-H // 8), -(-W // 8)))
    top = np.broadcast_to(top, (B, -(-H // 8), -(-W // 8)))
    lim = np.repeat(np.repeat((1 << np.asarray(top, np.int64)) - 1, 8, 1), 8, 2)[:, :H, :W]
    v = (rng.random((B, H, W)) * (lim + 1)).astype(np.int64).clip(0, lim) * rng.choice([-1, 1], (B, H, W))
    v = v.clip(info.min, info.max)
    v[0] = 0
    if B > 1:
        flat = v[B - 1].reshape(-1)
        special = [info.min, -1, 1, info.max]
        at = rng.choice(flat.size, min(len(special), flat.size), replace=False)
        flat[at] = special[:len(at)]
    return v.astype(bpm.DTYPE[index_type])


def truncate(v, index_type):
    u = np.uint16 if index_type == bpm.I16 else np.uint32
    return (np.asarray(v, np.int64) & np.iinfo(u).max).astype(u).view(bpm.DTYPE[index_type])


# ---- the model against the format -----------------------------------------------------------------------------------
@pytest.mark.parametrize("index_type", [bpm.I16, bpm.I32])
@pytest.mark.parametrize("cbx, cby", EXPONENTS)
@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_pack_then_unpack_is_the_input(W, H, j_max, cbx, cby, index_type):
    """zero frames, zero blocks, +-1, INT_MIN: everything comes back; offsets are monotone, end at the total, and every
    block's size is a multiple of its G"""
    q = frames_of(index_type, 3, H, W, 1)
    words, off = bpm.pack(q, index_type, j_max, cbx, cby)
    assert (np.diff(off.astype(np.int64), axis=1) >= 0).all() and off[0, -1] == 0 and words.shape[1] == off[:, -1].max()
    for s, (x, y, w, h) in enumerate(bpm.blocks(W, H, j_max, cbx, cby)):
        assert not ((off[:, s + 1] - off[:, s]) % -(-w * h // 64)).any()
        if s % 7 == 0:  # the definition, block by block
            assert np.array_equal(words[2, off[2, s]:off[2, s + 1]], bpm.block_words(q[2, y:y + h, x:x + w]))
    back = bpm.unpack(words, off, index_type, W, H, j_max, cbx, cby)
    assert back.dtype == q.dtype and np.array_equal(back, q)


@pytest.mark.parametrize("index_type", [bpm.I16, bpm.I32])
def test_extremes_and_units(index_type):
    info = np.iinfo(bpm.DTYPE[index_type])
    q = np.zeros((4, 8, 8), bpm.DTYPE[index_type])
    q[0, 3, 5], q[1, 0, 0], q[2, 7, 7] = info.min, 1, -1
    words, off = bpm.pack(q, index_type, 0, 3, 3)
    assert off[:, -1].tolist() == [info.bits + 1, 2, 2, 0]  # (64 samples: G = 1; p = 16 / 32, 1, 1, 0)
    assert words[0, 0] == 1 << 29 and words[0, 1] == 1 << 29 and not words[0, 2:info.bits + 1].any()
    assert words[1, 0] == 0 and words[1, 1] == 1 and words[2, 0] == 1 << 63 and words[2, 1] == 1 << 63
    assert np.array_equal(bpm.unpack(words, off, index_type, 8, 8, 0, 3, 3), q)


@pytest.mark.parametrize("index_type", [bpm.I16, bpm.I32])
@pytest.mark.parametrize("cbx, cby", [(2, 2), (3, 5), (6, 6)])
def test_dropped_planes(cbx, cby, index_type):
    """drop = d: KEEP gives sign(q) * ((|q| >> d) << d), SHIFT sign(q) * (|q| >> d), with d capped by every block's own p"""
    W, H, j_max = 72, 40, 3
    q = frames_of(index_type, 3, H, W, 2)
    words, off = bpm.pack(q, index_type, j_max, cbx, cby)
    mag, sign = np.abs(q.astype(np.int64)), np.sign(q.astype(np.int64))
    p_of = np.zeros(q.shape, np.int64)
    for x, y, w, h in bpm.blocks(W, H, j_max, cbx, cby):
        for b in range(3):
            p_of[b, y:y + h, x:x + w] = bpm.bit_length(mag[b, y:y + h, x:x + w].max())
    pmax = int(p_of.max())
    assert pmax == bpm.PMAX[index_type]
    for d in list(range(0, pmax + 2)):
        if d > 32:
            continue
        dk = np.minimum(d, p_of)
        keep = bpm.unpack(words, off, index_type, W, H, j_max, cbx, cby, d, bpm.KEEP)
        shift = bpm.unpack(words, off, index_type, W, H, j_max, cbx, cby, d, bpm.SHIFT)
        assert np.array_equal(keep, truncate(sign * ((mag >> dk) << dk), index_type)), d
        assert np.array_equal(shift, truncate(sign * (mag >> dk), index_type)), d
    assert not bpm.unpack(words, off, index_type, W, H, j_max, cbx, cby, 32, bpm.KEEP).any()


def test_a_cut_stream_is_a_prefix_of_the_blocks():
    """a capacity that ends inside a block: the blocks in front of it come back, that block and every later one as zeros;
    the words behind the last written block keep the fill"""
    W, H, j_max, cbx, cby = 72, 40, 3, 3, 3
    q = frames_of(bpm.I16, 2, H, W, 3, bits=5)
    q[0] = q[1]
    _, off = bpm.pack(q, bpm.I16, j_max, cbx, cby)
    rects = bpm.blocks(W, H, j_max, cbx, cby)
    s = len(rects) // 2
    assert off[1, s + 1] - off[1, s] > 1
    cap = int(off[1, s]) + 1
    words, off2 = bpm.pack(q, bpm.I16, j_max, cbx, cby, capacity=cap, fill=0xA5A5A5A5A5A5A5A5)
    assert np.array_equal(off2, off) and (words[:, int(off[1, s]):] == 0xA5A5A5A5A5A5A5A5).all()
    want = np.zeros_like(q)
    for x, y, w, h in rects[:s]:
        want[:, y:y + h, x:x + w] = q[:, y:y + h, x:x + w]
    assert np.array_equal(bpm.unpack(words, off, bpm.I16, W, H, j_max, cbx, cby), want)


def test_malformed_blocks_are_zeros():
    W, H, j_max, cbx, cby = 72, 40, 3, 3, 3
    q = frames_of(bpm.I16, 2, H, W, 4, bits=6)
    words, off = bpm.pack(q, bpm.I16, j_max, cbx, cby)
    rects = bpm.blocks(W, H, j_max, cbx, cby)
    bad = off.astype(np.int64).copy()
    s = 7
    bad[1, s + 1] = bad[1, s] - 1  # not monotone: block s, and block s + 1 grows (to a p it may not have)
    got = bpm.unpack(words, bad.astype(np.uint32), bpm.I16, W, H, j_max, cbx, cby)
    x, y, w, h = rects[s]
    assert q[1, y:y + h, x:x + w].any() and not got[1, y:y + h, x:x + w].any()
    for k, (x, y, w, h) in enumerate(rects):
        if k not in (s, s + 1):
            assert np.array_equal(got[:, y:y + h, x:x + w], q[:, y:y + h, x:x + w]), k
    # an end beyond the capacity, a length that is no multiple of G, more planes than the type has bits
    assert bpm.stream_planes(0, 5, 4, 1, bpm.I16) == 0 and bpm.stream_planes(0, 5, 8, 2, bpm.I16) == 0
    assert bpm.stream_planes(0, 18, 99, 1, bpm.I16) == 0 and bpm.stream_planes(0, 17, 99, 1, bpm.I16) == 16
    assert bpm.stream_planes(3, 36, 99, 1, bpm.I32) == 32 and bpm.stream_planes(3, 37, 99, 1, bpm.I32) == 0


@pytest.mark.parametrize("cbx, cby", EXPONENTS)
@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_block_sizes_follow_the_bit_plane_map(W, H, j_max, cbx, cby):
    """every block's size is the size rule of the value dwt_hip_codeblock_bitplanes_batch stores for it (slot order there,
    stream order here)"""
    import sparse_model as spm

    J = sm.levels(W, H, j_max)
    q = frames_of(bpm.I32, 2, H, W, 5)
    _, off = bpm.pack(q, bpm.I32, j_max, cbx, cby)
    planes = qm.codeblock_bitplanes(q, j_max, cbx, cby)
    first, _ = qm.codeblock_layout(W, H, j_max, cbx, cby)
    table = bpm.bands(W, H, j_max, cbx, cby)
    s = 0
    for k, slot in enumerate(spm.stream_order(J)):
        n_blocks = int(first[slot + 1] - first[slot])
        assert table[k, 4] == s and table[k + 1, 4] - table[k, 4] == n_blocks
        for i in range(n_blocks):
            x, y, w, h = bpm.block(table, cbx, cby, s)
            for b in range(2):
                assert off[b, s + 1] - off[b, s] == bpm.words_of(w * h, int(planes[b, first[slot] + i]))
            s += 1
    assert s == table[-1, 4] == first[-1]


# ---- the library's host geometry against the model ---------------------------------------------------------------------
@pytest.mark.parametrize("cbx, cby", EXPONENTS)
@pytest.mark.parametrize("W, H, j_max", SHAPES + [(4096, 4096, 5), (8, 1050000, 2)])
def test_geometry_of_the_library(dwt, W, H, j_max, cbx, cby):
    BP = dwt.bitplanes
    table = BP.bands(W, H, j_max, cbx, cby)
    model = bpm.bands(W, H, j_max, cbx, cby)
    assert table.dtype == np.int32 and np.array_equal(table, model)
    S = int(table[-1, 4])
    rects = bpm.blocks(W, H, j_max, cbx, cby) if S <= 70000 else None
    picks = range(S) if S <= 3000 else sorted({0, 1, S // 3, S // 2, S - 2, S - 1} | {int(v) for v in table[:-1, 4] if v < S} |
                                               {int(v) - 1 for v in table[1:, 4] if v > 0})
    for s in picks:
        assert BP.block(table, cbx, cby, s) == bpm.block(model, cbx, cby, s), s
        if rects is not None:
            assert BP.block(table, cbx, cby, s) == rects[s]
    if rects is not None:
        assert len(rects) == S and sum(w * h for _, _, w, h in rects) == W * H


def test_size_rule_of_the_library(dwt):
    BP = dwt.bitplanes
    for n in (1, 16, 63, 64, 65, 185, 4095, 4096):
        for p in range(33):
            assert BP.words_of(n, p) == bpm.words_of(n, p)
    assert BP.words_of(185, 3) == 12 and BP.words_of(4096, 32) == 33 * 64 and BP.words_of(4096, 0) == 0


def test_host_refusals(dwt):
    BP = dwt.bitplanes
    lib = dwt.lib
    table = np.full(5 * 8, -5, np.int32)
    for args in ((64, 64, 2, 1, 6), (64, 64, 2, 6, 11), (64, 64, 2, 7, 6), (64, 64, 2, 6, 1), (-1, 64, 2, 6, 6), (64, -1, 2, 6, 6),
                 (65536, 32768, 2, 6, 6)):
        assert lib.dwt_hip_bitplane_bands(*args, table.ctypes.data) == -1, args
    assert lib.dwt_hip_bitplane_bands(64, 64, 2, 6, 6, None) == -1
    assert (table == -5).all(), "a refused call wrote"
    with pytest.raises(dwt.DwtError):
        BP.bands(64, 64, 2, 1, 6)
    good = BP.bands(72, 40, 3, 3, 3)
    S = int(good[-1, 4])
    for s in (-1, S, S + 5):
        with pytest.raises(dwt.DwtError):
            BP.block(good, 3, 3, s)
    with pytest.raises(dwt.DwtError):
        BP.block(good, 1, 3, 0)
    for n, p in ((0, 1), (4097, 1), (64, -1), (64, 33), (-3, 0)):
        assert lib.dwt_hip_bitplane_words(n, p) == -1
        with pytest.raises(dwt.DwtError):
            BP.words_of(n, p)


def test_constants_and_namespace(dwt):
    import libdwt_amd

    BP = dwt.bitplanes
    assert (BP.I16, BP.I32, BP.KEEP, BP.SHIFT) == (bpm.I16, bpm.I32, bpm.KEEP, bpm.SHIFT)
    header = open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()
    for name, value in (("KEEP", BP.KEEP), ("SHIFT", BP.SHIFT), ("GRID_BLOCKS", BP.GRID_BLOCKS), ("GRID_BATCH", BP.GRID_BATCH)):
        assert re.search(r"#define DWT_HIP_BITPLANE_%s %d\s" % (name, value), header), name
    assert not [n for n in ("count_batch", "words_of", "route") if n in vars(libdwt_amd)]


def test_geometry_under_asan_ubsan(tmp_path):
    """tests/san/san_bitplanes.c: a stand-alone program around libdwt_amd/csrc/dwt_bitplane_geom.c (and the band table of
    dwt_sparse_geom.c that it calls), built with -fsanitize=address,undefined and run on the CPU; any report aborts it"""
    exe = tmp_path / "san_bitplanes"
    csrc = os.path.join(ROOT, "libdwt_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g",
                           "-O1", os.path.join(ROOT, "tests", "san", "san_bitplanes.c"), os.path.join(csrc, "dwt_bitplane_geom.c"),
                           os.path.join(csrc, "dwt_sparse_geom.c"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "san_bitplanes: OK" in out.stdout, out.stdout + out.stderr
