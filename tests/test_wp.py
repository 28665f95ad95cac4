"""CPU checks of the wavelet packet transforms: the model (tests/wp_model.py: the CPU oracle's one-level transforms node
by node) against the compiled reference's functions node by node (tests/golden/wp.npz, written by
scripts/gen_wp_golden.py), the node geometry, the frequency order and the conditions on the input kinds."""
import hashlib
import json
import os

import numpy as np
import pytest

import wp_model as wp

GOLD = np.load(wp.GOLDEN)
CASES = [(1, i) for i in range(len(wp.CASES_1D))] + [(2, i) for i in range(len(wp.CASES_2D))]


def case(dim, i):
    seed, wavelet, kind, size_y, size_x, levels = (wp.CASES_1D if dim == 1 else wp.CASES_2D)[i]
    return wavelet, kind, levels, wp.make_input(seed, kind, size_y, size_x, image=dim == 2)


def test_manifest():
    with open(wp.MANIFEST) as f:
        info = json.load(f)["files"]["wp.npz"]
    with open(wp.GOLDEN, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == info["sha256"]
    one = [(c["seed"], c["wavelet"], c["kind"], c["n_lines"], c["N"], c["levels"]) for c in info["cases"] if c["dim"] == 1]
    two = [(c["seed"], c["wavelet"], c["kind"], c["size_y"], c["size_x"], c["levels"]) for c in info["cases"] if c["dim"] == 2]
    assert one == wp.CASES_1D and two == wp.CASES_2D
    assert os.path.getsize(wp.GOLDEN) < 1 << 20
    assert sorted(GOLD.files) == sorted(d + wp.case_key(dim, i) for d in ("F_", "I_") for dim, i in CASES)


def test_cases_stay_small():
    assert all(c[4] <= 1025 for c in wp.CASES_1D) and all(c[3] <= 64 and c[4] <= 64 for c in wp.CASES_2D)
    assert all(1 <= c[5] <= wp.max_levels_1d(c[4]) for c in wp.CASES_1D)
    assert all(1 <= c[5] <= wp.max_levels_2d(c[3], c[4]) for c in wp.CASES_2D)
    for cases in (wp.CASES_1D, wp.CASES_2D):
        assert {c[2] for c in cases} == set(wp.KINDS) and {c[1] for c in cases} == set(wp.WAVELETS)
        assert all(c[5] <= 3 for c in cases if c[2] == "float_range")


@pytest.mark.parametrize("dim,i", CASES)
def test_model_equals_golden(dim, i):
    """forward and inverse, bit for bit (a NaN on both sides is not compared)"""
    wavelet, kind, levels, x = case(dim, i)
    fwd, inv = (wp.fwd1d, wp.inv1d) if dim == 1 else (wp.fwd2d, wp.inv2d)
    for tag, f in (("F_", fwd), ("I_", inv)):
        want = GOLD[tag + wp.case_key(dim, i)]
        got = f(wavelet, x, levels)
        assert got.shape == want.shape == x.shape and got.dtype == np.float32
        assert wp.same(got, want), (tag, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


@pytest.mark.parametrize("dim,i", CASES)
def test_input_kind_conditions(dim, i):
    """on the golden itself: float_range holds at most 25 % non-finite samples, every other kind none"""
    _, kind, _, x = case(dim, i)
    for tag in ("F_", "I_"):
        share = wp.nonfinite_share(GOLD[tag + wp.case_key(dim, i)])
        if kind == "float_range":
            assert share <= wp.NONFINITE_CAP, (tag, share)
        else:
            assert share == 0, (tag, share)
    if kind == "float_range":
        assert not np.isfinite(x).all()  # (the special values are there)
    if kind == "tiny":
        assert (np.abs(x) < np.finfo(np.float32).tiny).all()


def test_round_trip_of_the_model():
    x = wp.make_input(77, "normal", 2, 100)
    for wavelet in wp.WAVELETS:
        back = wp.inv1d(wavelet, wp.fwd1d(wavelet, x, 6), 6)
        assert np.abs(back - x).max() < 1e-4
    img = wp.make_input(78, "normal", 33, 47)
    for wavelet in wp.WAVELETS:
        back = wp.inv2d(wavelet, wp.fwd2d(wavelet, img, 4), 4)
        assert np.abs(back - img).max() < 1e-4


def test_closed_form_equals_recursion():
    for N in range(2, 301):
        for level in range(0, wp.floor_log2(N) + 1):
            assert wp.nodes_closed_form(N, level) == wp.nodes_recursive(N, level), (N, level)


def test_every_split_node_has_two_samples():
    """levels <= floor(log2 N): the nodes of levels 0 .. levels-1 have 2 samples or more, the leaves 1 or more"""
    for N in range(2, 301):
        J = wp.floor_log2(N)
        assert min(n for _, n in wp.nodes_recursive(N, J - 1)) >= 2
        assert min(n for _, n in wp.nodes_recursive(N, J)) >= 1


def test_leaves_tile_the_line():
    for N in (2, 3, 5, 8, 63, 64, 100, 257, 300):
        for level in range(wp.floor_log2(N) + 1):
            pos = 0
            for s, n in wp.nodes_recursive(N, level):
                assert s == pos and n >= 1
                pos += n
            assert pos == N


def test_freq_order_is_the_gray_code():
    for level in range(0, 11):
        perm = wp.freq_order(level)
        assert sorted(perm) == list(range(1 << level))
        assert perm == [f ^ (f >> 1) for f in range(1 << level)]
        # neighbours in frequency differ in one split of the path
        assert all(bin(perm[f] ^ perm[f + 1]).count("1") == 1 for f in range(len(perm) - 1))


def test_freq_order_orders_the_bands():
    """a pure tone's energy lands in the node the Gray code names: the 9/7 packets of cos(pi (f + 1/2) t / 2^J)"""
    J, N = 3, 512
    t = np.arange(N)
    perm = wp.freq_order(J)
    for f in range(1 << J):
        x = np.cos(np.pi * (f + 0.5) / (1 << J) * (t + 0.5)).astype(np.float32)[None]
        y = wp.fwd1d("cdf97_s", x, J)[0]
        energy = [float((y[s:s + n].astype(np.float64) ** 2).sum()) for s, n in wp.nodes_recursive(N, J)]
        assert int(np.argmax(energy)) == perm[f], (f, energy)
