"""CPU checks of the sparse coefficient streams (include/libdwt_hip.h): the numpy model against itself, the
library's stream order and band table (host code) against the model, and the tile geometry under the sanitizers.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import sparse_model as spm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 3, 2), (1, 37, -1), (37, 1, -1), (72, 40, 3), (264, 136, 3)]


@pytest.fixture(scope="module")
def dwt():
    import __graft_entry__ as g

    if not os.path.exists(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")):
        g.build()
    import libdwt_amd as d
    from libdwt_amd import sparse

    d.sparse = sparse
    return d


def frames_of(elem_type, B, H, W, density, seed):
    """random frames of that density, with the values whose bits matter: both zeros, NaN, infinities, subnormals, the extremes"""
    rng = np.random.default_rng([seed, elem_type, B, H, W])
    dt = spm.DTYPE[elem_type]
    if dt.kind == "f":
        v = rng.normal(0, 30, (B, H, W)).astype(dt)
        special = np.array([-0.0, np.nan, np.inf, -np.inf, 1e-45 if dt.itemsize == 4 else 6e-8, -(1e-40 if dt.itemsize == 4 else 3e-7)], dt)
    else:
        info = np.iinfo(dt)
        v = rng.integers(info.min, int(info.max) + 1, (B, H, W)).astype(dt)
        special = np.array([info.min, -1, 1, info.max], dt)
    v[rng.random((B, H, W)) >= density] = 0
    flat = v.reshape(-1)
    at = rng.choice(flat.size, min(len(special), flat.size), replace=False)
    flat[at] = special[:len(at)]
    return v


@pytest.mark.parametrize("elem_type", spm.TYPES)
@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_pack_then_unpack_is_the_input(W, H, j_max, elem_type):
    """the round trip changes one thing: -0.0 comes back as +0.0; offsets are monotone and end at the total"""
    import shape_model as sm

    J = sm.levels(W, H, j_max)
    for density in (0.0, 0.05, 1.0):
        v = frames_of(elem_type, 3, H, W, density, 1)
        pos, val, off = spm.pack(v, elem_type, J)
        assert off.shape == (3, 3 * J + 2) and (np.diff(off.astype(np.int64), axis=1) >= 0).all()
        assert np.array_equal(off[:, -1], spm.kept(v, elem_type).reshape(3, -1).sum(1))
        back = spm.unpack(pos, val, off[:, -1], elem_type, H, W)
        want = spm.bits(v).copy()
        want[~spm.kept(v, elem_type)] = 0
        assert np.array_equal(spm.bits(back), want)
        if spm.DTYPE[elem_type].kind == "f" and density:
            assert (spm.bits(v) != want).any(), "no -0.0 in the input"
        for b in range(3):  # positions ascend inside a band, and lie in it
            for k, (x0, y0, w, h) in enumerate(spm.bands(W, H, J)):
                p = pos[b, off[b, k]:off[b, k + 1]].astype(np.int64)
                assert (np.diff(p) > 0).all() and ((p % W >= x0) & (p % W < x0 + w) & (p // W >= y0) & (p // W < y0 + h)).all()


@pytest.mark.parametrize("W, H, j_max", SHAPES)
def test_a_prefix_is_a_coarser_frame(W, H, j_max):
    """a stream cut at off[k] unpacks to the frame with the stream bands k .. zeroed"""
    import shape_model as sm

    J = sm.levels(W, H, j_max)
    v = frames_of(spm.F32, 1, H, W, 0.5, 2)
    pos, val, off = spm.pack(v, spm.F32, J)
    for k in range(3 * J + 2):
        back = spm.unpack(pos, val, off[:, k], spm.F32, H, W)
        assert np.array_equal(spm.bits(back), spm.bits(spm.coarser(v, spm.F32, J, k)))
    # the same through the capacity: truncation keeps the first entries in stream order
    k = (3 * J + 1) // 2
    cut = spm.pack(v, spm.F32, J, capacity=int(off[0, k]))
    assert np.array_equal(cut[2], off) and np.array_equal(cut[0][0], pos[0, :off[0, k]])
    assert np.array_equal(spm.bits(spm.unpack(cut[0], cut[1], off[:, -1], spm.F32, H, W)), spm.bits(spm.coarser(v, spm.F32, J, k)))


@pytest.mark.parametrize("J", range(6))
def test_stream_order_of_the_library(dwt, J):
    assert dwt.sparse.stream_order(J).tolist() == spm.stream_order(J)
    assert sorted(spm.stream_order(J)) == list(range(3 * J + 1))


def test_stream_order_refusals(dwt):
    for J in (-1, 32):
        with pytest.raises(dwt.DwtError):
            dwt.sparse.stream_order(J)


@pytest.mark.parametrize("W, H, j_max", SHAPES + [(130, 66, 0), (4096, 4096, 5), (8, 1050000, 2)])
def test_band_table_of_the_library(dwt, W, H, j_max):
    """dwt_hip_sparse_bands: the model's rectangles in stream order (empty bands as zeros), the tiles' prefix"""
    S = dwt.sparse
    J = dwt.band_levels(W, H, j_max)
    table = S.stream_bands(W, H, j_max)
    first = 0
    for row, (x0, y0, w, h) in zip(table, spm.bands(W, H, J)):
        assert row[:4].tolist() == ([x0, y0, w, h] if w and h else [row[0], row[1], 0, 0]) and row[4] == first
        first += -(-w * h // S.TILE_SAMPLES)
    assert table[-1].tolist() == [0, 0, 0, 0, first]


def test_constants_and_namespace(dwt):
    import libdwt_amd

    S = dwt.sparse
    assert (S.F32, S.F16, S.I16, S.I32) == (spm.F32, spm.F16, spm.I16, spm.I32)
    assert {t: np.dtype(S.ELEM_DTYPE[t]) for t in spm.TYPES} == spm.DTYPE
    assert S.TILE_SAMPLES > 0 and S.GRID_TILES > 0 and S.GRID_BATCH > 0
    header = open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()
    for name, value in (("TILE_SAMPLES", S.TILE_SAMPLES), ("GRID_TILES", S.GRID_TILES), ("GRID_BATCH", S.GRID_BATCH)):
        assert re.search(r"#define DWT_HIP_SPARSE_%s %d\s" % (name, value), header), name
    assert not [n for n in ("pack_batch", "count_batch", "unpack_batch", "stream_order", "sparse_route") if n in vars(libdwt_amd)]


def test_geometry_under_asan_ubsan(tmp_path):
    """tests/san/san_sparse.c: a stand-alone program around libdwt_amd/csrc/dwt_sparse_geom.c, built with
    -fsanitize=address,undefined and run on the CPU; any report aborts it"""
    exe = tmp_path / "san_sparse"
    subprocess.check_call(["gcc", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g",
                           "-O1", os.path.join(ROOT, "tests", "san", "san_sparse.c"), os.path.join(ROOT, "libdwt_amd", "csrc", "dwt_sparse_geom.c"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "san_sparse: OK" in out.stdout, out.stdout + out.stderr
