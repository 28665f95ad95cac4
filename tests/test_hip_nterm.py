"""GPU checks of the N-term approximation against the numpy model of tests/nterm_model.py and the fixture
tests/golden/nterm.npz, which tests/test_nterm.py pins to each other and to a literal restatement of the reference's flow.
Every comparison is exact: == on the uint32 image of thresholds, coefficients and magnitudes, == on the kept counts.

Groups are laid into a buffer whose every other word -- the padding behind each row, one row behind each frame, one spare
plane behind each group -- holds 3e38: a value that must come back with its bits, and whose square overflows, so that a
single padding word read for the decision would move the threshold to infinity."""
import numpy as np
import pytest

import nterm_model as nm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
HUGE = F32(3.0e38)
bits = nm.bits


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)


@pytest.fixture(scope="module")
def golden():
    return np.load(nm.GOLDEN)


def lay(groups, pad, step=1):
    """groups (n, C, h, w) -> (buffer [n, C + 1, h + 1, (w + pad) * step] of HUGE with the groups in it, mask of their words)"""
    groups = np.asarray(groups, F32)
    n, ch, h, w = groups.shape
    buf = np.full((n, ch + 1, h + 1, (w + pad) * step), HUGE, F32)
    mask = np.zeros(buf.shape, bool)
    buf[:, :ch, :h, :w * step:step] = groups
    mask[:, :ch, :h, :w * step:step] = True
    return buf, mask


def run(dwt, groups, keep, scope=nm.FRAME, j_max=-1, pad=3, device=True):
    """keep_largest_batch over the groups -> (groups after the call, thr, kept, launches); no word outside them changes"""
    groups = np.asarray(groups, F32)
    n, ch, h, w = groups.shape
    buf, mask = lay(groups, pad)
    bs, cs, sx = buf.strides[:3]
    res = []
    call = lambda p: res.append(dwt.keep_largest_batch(p, bs, n, ch, cs, sx, w, h, keep, j_max, scope))  # noqa: E731
    if device:
        d = Dev(dwt, buf)
        k = launches(dwt, lambda: call(d.ptr))
        out = d.get()
        d.free()
    else:
        out = buf.copy()
        k = launches(dwt, lambda: call(out))
    assert np.array_equal(bits(out)[~mask], bits(buf)[~mask]), "a word outside the frames was written"
    return out[:, :ch, :h, :w], res[0][0], res[0][1], k


def check(got, thr, kept, groups, keep, scope=nm.FRAME, j_max=-1, only=None):
    keeps = [keep] * len(groups) if np.isscalar(keep) else keep
    for g in range(len(groups)) if only is None else only:
        want, wthr, wkept = nm.keep_largest(groups[g], keeps[g], scope, j_max)
        assert bits(thr[g:g + 1])[0] == bits(wthr), (g, keeps[g], thr[g], wthr)
        assert kept[g] == wkept, (g, keeps[g], kept[g], wkept)
        assert np.array_equal(bits(got[g]), bits(want)), (g, keeps[g])


def keeps_small(M):
    return [1, 2, M - 1, M, 0, -1, M + 1]


# (size_x, size_y, pad): a pitch that is a multiple of 16 bytes takes 16-byte accesses, every other pitch single elements
SMALL_SHAPES = [(1, 1, 0), (1, 7, 0), (7, 1, 0), (7, 1, 1), (3, 5, 1), (3, 5, 0), (37, 53, 3), (37, 53, 4)]


@pytest.mark.parametrize("size_x,size_y,pad", SMALL_SHAPES)
@pytest.mark.parametrize("channels", [1, 2])
def test_small_shapes_every_rank(dwt, size_x, size_y, pad, channels):
    x = nm.make_input(size_x * 100 + size_y, "normal", channels, size_y, size_x)[None]
    for keep in keeps_small(size_x * size_y):
        got, thr, kept, k = run(dwt, x, keep, pad=pad)
        assert k <= 5
        check(got, thr, kept, x, keep)


@pytest.mark.parametrize("size_x,size_y,pad", [(300, 257, 0), (300, 257, 1), (1024, 1024, 0)])
def test_many_workgroups(dwt, size_x, size_y, pad):
    """several slabs and workgroups per group, merging into one histogram"""
    x = nm.make_input(size_x, "normal", 2, size_y, size_x)[None]
    M = size_x * size_y
    for keep in (M // 10,) if size_x == 1024 else (1, M // 10, M - 1):
        got, thr, kept, k = run(dwt, x, keep, pad=pad)
        assert k <= 5
        check(got, thr, kept, x, keep)


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_batch_of_five(dwt, channels):
    """five groups, five ranks, five scales; batch_stride and channel_stride larger than what they span"""
    w, h = 37, 29
    xs = np.stack([nm.make_input(40 + b, "normal", channels, h, w) * F32(10.0 ** (b - 2)) for b in range(5)])
    keep = [1, w * h // 2, w * h, 17, 0]
    for pad in (3, 0):
        got, thr, kept, k = run(dwt, xs, keep, pad=pad)
        assert k <= 5
        check(got, thr, kept, xs, keep)


def test_channel_major_layout(dwt):
    """every channel's frames one after the other: channel_stride spans the batch"""
    w, h, n = 24, 10, 3
    xs = np.stack([nm.make_input(70 + b, "normal", 2, h, w) for b in range(n)])
    d = Dev(dwt, np.ascontiguousarray(xs.transpose(1, 0, 2, 3)))
    keep = [5, 100, 239]
    thr, kept = dwt.keep_largest_batch(d.ptr, w * h * 4, n, 2, n * w * h * 4, w * 4, w, h, keep)
    check(d.get().transpose(1, 0, 2, 3), thr, kept, xs, keep)
    d.free()


def radix_cases():
    h, w = 16, 20
    rng = np.random.default_rng(3)
    one = np.ones((1, h, w), F32)
    low = (np.full((h, w), 0x3f800000, np.uint32) + rng.integers(0, 2, (h, w)).astype(np.uint32)).view(F32)[None]
    exps = (rng.integers(1, 255, (h, w)).astype(np.uint32) << 23).view(F32)[None]
    zeros = np.where(rng.random((1, h, w)) < 0.6, F32(0), rng.standard_normal((1, h, w)).astype(F32))
    zeros[0, 0, :4] = (F32(-0.0), F32(0.0), F32(-0.0), F32(1.0))
    top = np.full((1, h, w), 2.5, F32)
    top[0, 7, 9] = np.nextafter(F32(2.5), F32(3))
    mid = (np.full((h, w), 0x40000000, np.uint32) + (rng.integers(0, 1024, (h, w)).astype(np.uint32) << 10)).view(F32)[None]
    return {"equal": one, "lowest_bit": low, "exponent": exps, "zeros": zeros, "one_above": top, "middle_digit": mid}


@pytest.mark.parametrize("name", ["equal", "lowest_bit", "exponent", "zeros", "one_above", "middle_digit"])
def test_radix_digits(dwt, name):
    """data that one digit of the select alone decides"""
    x = radix_cases()[name][None]
    M = x[0, 0].size
    for keep in (1, 2, M // 2, M - 1, M):
        got, thr, kept, _ = run(dwt, x, keep, pad=0)
        check(got, thr, kept, x, keep)
        if name == "equal":
            assert kept[0] == M and np.array_equal(bits(got), bits(x))
        if name == "zeros" and keep >= M // 2:
            assert bits(thr)[0] == 0 and kept[0] == M and np.array_equal(bits(got), bits(x))  # (-0 stays -0)
        if name == "one_above" and keep == 1:
            assert kept[0] == 1 and np.count_nonzero(got) == 1
    if name == "one_above":
        two = np.concatenate([x, x * F32(0)], axis=1)
        got, thr, kept, _ = run(dwt, two, 1, pad=0)
        check(got, thr, kept, two, 1)


@pytest.mark.parametrize("kind", ["float_range", "underflow", "ties"])
def test_float_range(dwt, kind):
    """two channels: overflowing squares and infinities (ties at Inf), subnormals and vanishing squares, signed zeros"""
    w, h = 48, 33
    x = nm.make_input(900, kind, 2, h, w)[None]
    if kind == "float_range":
        x[0, :, 0, :4] = [[np.inf, -np.inf, 3e38, -0.0], [1.0, np.inf, 3e38, 0.0]]
    if kind == "underflow":
        assert (nm.magnitudes(x[0]) == 0).any() and ((x[0] != 0) & (np.abs(x[0]) < np.finfo(F32).tiny)).any()
    for keep in (1, w * h // 3, w * h // 2, w * h - 1, 0):
        got, thr, kept, _ = run(dwt, x, keep)
        check(got, thr, kept, x, keep)


@pytest.mark.parametrize("size_x,size_y", [(37, 53), (64, 64)])
@pytest.mark.parametrize("j_max", [1, 3, -1])
def test_details_scope(dwt, size_x, size_y, j_max):
    """the LL rectangle keeps its bits although it holds the largest values"""
    J = nm.band_levels(size_x, size_y, j_max)
    assert dwt.band_levels(size_x, size_y, j_max) == J
    lx, ly = -(-size_x // (1 << J)), -(-size_y // (1 << J))
    for channels in (1, 2):
        x = nm.make_input(31 + channels, "normal", channels, size_y, size_x)[None]
        x[0, :, :ly, :lx] *= F32(1000)
        M = size_x * size_y - lx * ly
        for keep in (1, M // 5, M, M + 1):
            got, thr, kept, k = run(dwt, x, keep, nm.DETAILS, j_max, pad=3 if size_x == 37 else 0)
            assert k <= 5
            check(got, thr, kept, x, keep, nm.DETAILS, j_max)
            assert np.array_equal(bits(got[0, :, :ly, :lx]), bits(x[0, :, :ly, :lx])) and thr[0] < 100


def test_empty_scope_launches_nothing(dwt):
    x = nm.make_input(1, "normal", 2, 12, 9)[None]
    for device in (True, False):
        got, thr, kept, k = run(dwt, x, 5, nm.DETAILS, 0, device=device)
        assert k == 0 and thr[0] == 0 and kept[0] == 0 and np.array_equal(bits(got), bits(x))
    d = Dev(dwt, x)
    thr, kept = dwt.keep_largest_batch(d.ptr, 0, 1, 2, 36 * 12, 36, 9, 0, 5)  # (no rows)
    assert thr[0] == 0 and kept[0] == 0
    assert dwt.keep_largest(d.ptr, 36, 4, 1, 1, 1, 0, nm.DETAILS) == (0.0, 0)
    d.free()


def test_nan_group_leaves_the_others_exact(dwt):
    w, h = 37, 21
    xs = np.stack([nm.make_input(60 + b, "normal", 2, h, w) for b in range(3)])
    xs[1, 0, 5, 5] = np.nan
    keep = [10, 10, 300]
    got, thr, kept, _ = run(dwt, xs, keep)
    check(got, thr, kept, xs, keep, only=(0, 2))


def test_host_frames_and_strided_single_frame(dwt):
    """the staged routes equal the dense device result; the words between strided elements keep their bits"""
    w, h = 37, 21
    xs = np.stack([nm.make_input(80 + b, "normal", 2, h, w) for b in range(2)])
    keep = [50, 400]
    dev = run(dwt, xs, keep)
    host = run(dwt, xs, keep, device=False)
    check(*dev[:3], xs, keep)
    assert np.array_equal(bits(host[0]), bits(dev[0])) and np.array_equal(bits(host[1]), bits(dev[1])) and np.array_equal(host[2], dev[2])
    x = xs[0, :1]
    want = nm.keep_largest(x, 50)
    for device in (True, False):
        for step in (1, 2):
            buf, mask = lay(x[None], 1, step)
            buf, mask = buf[0, 0], mask[0, 0]
            d = Dev(dwt, buf) if device else None
            out = buf.copy()
            thr, kept = dwt.keep_largest(d.ptr if device else out, buf.strides[0], 4 * step, w, h, 50)
            if device:
                out = d.get()
                d.free()
            assert np.array_equal(bits(out)[~mask], bits(buf)[~mask])
            assert np.array_equal(bits(out[:h, :w * step:step]), bits(want[0][0])) and bits(F32(thr)) == bits(want[1]) and kept == want[2]


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_magnitude_batch(dwt, channels):
    w, h, n = 37, 21, 3
    kinds = ("normal", "float_range", "underflow")
    xs = np.stack([nm.make_input(20 + b, kinds[b], channels, h, w) for b in range(n)])
    for pad, mpad in ((3, 7), (0, 1)):
        buf, _ = lay(xs, pad)
        mbuf, mmask = lay(np.zeros((n, 1, h, w), F32), mpad)
        mbuf, mmask = np.ascontiguousarray(mbuf[:, 0]), np.ascontiguousarray(mmask[:, 0])
        d, m = Dev(dwt, buf), Dev(dwt, mbuf)
        k = launches(dwt, lambda: dwt.magnitude_batch(d.ptr, buf.strides[0], n, channels, buf.strides[1], buf.strides[2], w, h,
                                                      m.ptr, mbuf.strides[0], mbuf.strides[1]))
        assert k == 1
        got = m.get()
        assert np.array_equal(bits(d.get()), bits(buf)), "the source changed"
        assert np.array_equal(bits(got)[~mmask], bits(mbuf)[~mmask])
        for b in range(n):
            assert np.array_equal(bits(got[b, :h, :w]), bits(nm.magnitudes(xs[b]))), b
        host = mbuf.copy()
        dwt.magnitude_batch(buf, buf.strides[0], n, channels, buf.strides[1], buf.strides[2], w, h, host, mbuf.strides[0], mbuf.strides[1])
        assert np.array_equal(bits(host), bits(got))
        d.free()
        m.free()


@pytest.mark.parametrize("name", ["flow97", "flow53"])
def test_flow(dwt, golden, name):
    """the flow of examples/displ-vectors: forward of both fields on the device, keep, inverse"""
    _, _, wavelet, h, w = nm.CASES[name]
    fwd, inv = getattr(dwt, "dwt_%s_2f_s" % wavelet), getattr(dwt, "dwt_%s_2i_s" % wavelet)
    fields = nm.flow_fields(h, w)
    M = w * h
    for i, keep in enumerate(nm.keeps_of(M)):
        if keep not in (M // 100, M // 10, 0):
            continue
        d = Dev(dwt, fields)
        j = [fwd(d.ptr + c * M * 4, w * 4, 4, w, h, w, h, -1, 0, 0) for c in range(2)]
        thr, kept = dwt.keep_largest_batch(d.ptr, 0, 1, 2, M * 4, w * 4, w, h, keep)
        want = nm.keep_largest(golden[name + ".coef"], keep)
        assert np.array_equal(bits(d.get()), bits(want[0]))
        assert bits(thr)[0] == bits(golden[name + ".thr"][i]) and kept[0] == golden[name + ".kept"][i] == want[2]
        for c in range(2):
            inv(d.ptr + c * M * 4, w * 4, 4, w, h, w, h, j[c], 0, 0)
        assert np.isfinite(d.get()).all()
        d.free()


def test_fixture_cases(dwt, golden):
    """every two-channel case of the fixture at every recorded rank: thresholds and kept counts as libc gave them"""
    for name in nm.CASES:
        planes = nm.case_planes(name, golden)
        for i, keep in enumerate(nm.keeps_of(planes[0].size)):
            got, thr, kept, _ = run(dwt, planes[None], keep, pad=0)
            assert bits(thr)[0] == bits(golden[name + ".thr"][i]) and kept[0] == golden[name + ".kept"][i], (name, keep)
            assert np.array_equal(bits(got[0]), bits(nm.keep_largest(planes, keep)[0])), (name, keep)


def test_two_calls_same_bits(dwt):
    x = nm.make_input(7, "ties", 2, 257, 300)[None]
    a, b = run(dwt, x, 20000, pad=0), run(dwt, x, 20000, pad=0)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def test_launch_counts(dwt):
    for n in (1, 5):
        for channels in (1, 2):
            xs = np.stack([nm.make_input(b, "normal", channels, 40, 64) for b in range(n)])
            assert 1 <= run(dwt, xs, 100, pad=0)[3] <= 5


def test_errors_launch_nothing(dwt):
    w, h, n, ch = 16, 8, 2, 2
    x = np.stack([nm.make_input(b, "normal", ch, h, w) for b in range(n)])
    d, m = Dev(dwt, x), Dev(dwt, np.zeros((n, h, w), F32))
    sx, cs, bs = 4 * w, 4 * w * h, 4 * w * h * ch
    keep = np.array([3, 4], np.int32)
    thr, kept = np.full(n, 7, F32), np.full(n, 7, np.int32)
    P = lambda a: a.ctypes.data  # noqa: E731
    L = dwt.lib

    def batch(ptr=d.ptr, bs=bs, n=n, ch=ch, cs=cs, sx=sx, w=w, h=h, j_max=-1, scope=0, keep=P(keep), thr=P(thr), kept=P(kept)):
        return L.dwt_hip_keep_largest_batch(ptr, bs, n, ch, cs, sx, w, h, j_max, scope, keep, thr, kept)

    def mag(ptr=d.ptr, bs=bs, n=n, ch=ch, cs=cs, sx=sx, w=w, h=h, mp=m.ptr, mbs=cs, msx=sx):
        return L.dwt_hip_magnitude_batch(ptr, bs, n, ch, cs, sx, w, h, mp, mbs, msx)

    k0 = dwt.get_option("stat_launches")
    bad = [
        batch(ptr=None), batch(ch=0), batch(ch=5), batch(scope=2), batch(scope=-1), batch(w=-1), batch(h=-1), batch(n=-1),
        batch(w=65536, h=32768, sx=4 * 65536), batch(sx=4 * w - 4), batch(cs=cs - 4), batch(bs=cs - 4), batch(bs=bs - 4),
        batch(keep=None), batch(thr=m.ptr), batch(kept=m.ptr), batch(ptr=d.ptr + 2), batch(sx=sx + 2, cs=cs * 2, bs=bs * 4),
        L.dwt_hip_keep_largest(None, sx, 4, w, h, -1, 0, 3, P(thr), P(kept)),
        L.dwt_hip_keep_largest(d.ptr, sx, 2, w, h, -1, 0, 3, P(thr), P(kept)),
        L.dwt_hip_keep_largest(d.ptr, sx, 4, w, h, -1, 5, 3, P(thr), P(kept)),
        L.dwt_hip_keep_largest(d.ptr, sx, 4, w, h, -1, 0, 3, m.ptr, P(kept)),
        L.dwt_hip_keep_largest(d.ptr, sx - 4, 4, w, h, -1, 0, 3, P(thr), P(kept)),
        mag(ptr=None), mag(mp=None), mag(ch=0), mag(ch=5), mag(w=-1), mag(n=-1), mag(sx=sx - 4), mag(msx=sx - 4), mag(cs=cs - 4),
        mag(bs=bs - 4), mag(mbs=cs - 4), mag(mp=d.ptr), mag(mp=d.ptr + bs * n - 4), mag(mp=m.ptr + 2), mag(ptr=d.ptr + 2),
        mag(mp=P(np.zeros((n, h, w), F32))),
    ]
    assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    assert len(dwt.last_error()) > 10
    assert dwt.get_option("stat_launches") == k0
    assert np.array_equal(bits(d.get()), bits(x)) and not m.get().any()
    assert (thr == 7).all() and (kept == 7).all()
    assert batch() == 0 and batch(thr=None, kept=None) == 0 and mag() == 0  # (the calls themselves are sound)
    d.free()
    m.free()


def test_example_nterm_approx(dwt, tmp_path):
    """examples/nterm_approx.c: two resident fields, forward, keep, inverse, each N against the program's host restatement"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = tmp_path / "nterm_approx", os.path.join(root, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "nterm_approx.c"),
                           "-o", str(exe), "-L" + libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "success" in out.stdout + out.stderr, out.stdout + out.stderr
