"""GPU checks of the per-band coefficient operators, the log / exp maps and the universal threshold
against the numpy model of tests/shape_model.py and the reference-generated fixture tests/golden/shape.npz, which
tests/test_shape.py pins to each other.

KEEP, ZERO, SCALE, HARD, SOFT, the threshold and the signs and zeros of COMPRESS are compared bit for bit (NaNs by
position: payloads are not pinned across architectures); COMPRESS magnitudes, LOG and EXP lie within 1 ulp of the float64
model rounded once.  The distance to the host libm's powf / logf / expf is printed by every test that meets it and
measured over the fixture by scripts/shape_timing.py; LIBM_ULPS is its expected maximum -- the device result and libm's
each lie within 1 ulp of the exact value, on either side of it at worst -- and a test fails only beyond LIBM_ULPS + 1.  Every word outside the selected
bands -- KEEP slots, the gap between inner and outer size, the pitch padding, neighbouring frames -- must come back with
the bits it had, checked against a background of NaNs."""
import numpy as np
import pytest

import shape_model as sm
from hipdev import Dev, launches

pytestmark = pytest.mark.gpu
F32 = np.float32
BACKGROUND = np.array([0x7fc0beef], np.uint32).view(F32)[0]
LIBM_ULPS = 1  # (see above; to be replaced by the measured maximum of profiles/shape_timing.json)


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)


@pytest.fixture(scope="module")
def golden():
    return np.load(sm.GOLDEN)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def frames(xs, pad, step=1):
    """frames laid into one buffer of NaNs: `pad` elements after every row, elements `step` floats apart, one row of
    background after every frame -> (buffer [n, h + 1, (w + pad) * step], mask of the frames' elements)"""
    n, (h, w) = len(xs), xs[0].shape
    buf = np.full((n, h + 1, (w + pad) * step), BACKGROUND, F32)
    mask = np.zeros(buf.shape, bool)
    for b, x in enumerate(xs):
        buf[b, :h, :w * step:step] = x
    mask[:, :h, :w * step:step] = True
    return buf, mask


def run(dwt, call, xs, pad=1, step=1, device=True):
    """call(ptr, batch_stride, stride_x, stride_y) over the frames -> (frames after the call, launches); every word
    outside the frames keeps its bits"""
    buf, mask = frames(xs, pad, step)
    sx, bs = buf.strides[1], buf.strides[0]
    if device:
        d = Dev(dwt, buf)
        k = launches(dwt, lambda: call(d.ptr, bs, sx, 4 * step))
        out = d.get()
        d.free()
    else:
        out = buf.copy()
        k = launches(dwt, lambda: call(out, bs, sx, 4 * step))
    assert np.array_equal(bits(out)[~mask], bits(buf)[~mask]), "a word outside the frames was written"
    h, w = xs[0].shape
    return [out[b, :h, :w * step:step] for b in range(len(xs))], k


def check_table(got, x, sizes, J, ops, params, want=None, libm=None):
    """one frame after a table against the model (or the fixture's copy of it) -> the largest distance to libm"""
    sox, soy, six, siy = sizes
    want = sm.apply_table(x, sox, soy, six, siy, J, ops, params) if want is None else want
    touched = np.zeros(x.shape, bool)
    worst = 0
    for (x0, y0, w, h), op in zip(sm.slots(sox, soy, six, siy, J), ops):
        g, t = got[y0:y0 + h, x0:x0 + w], want[y0:y0 + h, x0:x0 + w]
        if op == sm.KEEP or not (w and h):
            continue
        touched[y0:y0 + h, x0:x0 + w] = True
        if op != sm.COMPRESS:
            assert sm.same(g, t), "slot at (%d, %d), %s" % (x0, y0, sm.OP_NAMES[op])
            continue
        assert np.array_equal(np.signbit(g), np.signbit(t)) and np.array_equal(g == 0, t == 0), "compress: signs and zeros at (%d, %d)" % (x0, y0)
        d = int(sm.ulps(g, t).max())
        print("compress at (%d, %d): %d ulp from the float64 model" % (x0, y0, d))
        assert d <= 1
        if libm is not None:
            worst = max(worst, int(sm.ulps(g, libm[y0:y0 + h, x0:x0 + w]).max()))
    assert np.array_equal(bits(got)[~touched], bits(x)[~touched]), "a coefficient outside the selected bands changed"
    return worst


@pytest.mark.parametrize("name", list(sm.CASES))
def test_fixture_cases(dwt, golden, name):
    """every fixture case on a dense device frame with a pitch of (size_x + 1) * 4 bytes: one launch"""
    sox, soy, six, siy, j_max, _ = sm.CASES[name]
    x, J, ops, params = sm.case_arrays(name)
    (got,), k = run(dwt, lambda p, bs, sx, sy: dwt.bands_apply(p, sx, sy, sox, soy, six, siy, j_max, ops, params), [x])
    assert k == 1
    libm = golden[name + ".libm"] if name + ".libm" in golden else None
    worst = check_table(got, x, (sox, soy, six, siy), J, ops, params, golden[name + ".out"], libm)
    print("%s: %d ulp from libm" % (name, worst))
    assert worst <= LIBM_ULPS + 1


def test_mra_keeps_one_band(dwt):
    """examples/mra: every band of a transformed row but one zeroed"""
    x, J, ops, params = sm.case_arrays("row")
    (got,), _ = run(dwt, lambda p, bs, sx, sy: dwt.bands_apply(p, sx, sy, 130, 1, 130, 1, -1, ops, params), [x])
    x0, _, w, _ = sm.slots(130, 1, 130, 1, J)[3]
    assert w and np.array_equal(bits(got[0, x0:x0 + w]), bits(x[0, x0:x0 + w]))
    rest = np.ones(130, bool)
    rest[x0:x0 + w] = False
    assert np.array_equal(bits(got[0, rest]), np.zeros(130 - w, np.uint32))


def test_batch_with_per_image_tables(dwt):
    sox, soy, J = 37, 29, 3
    ns, ts = 3 * J + 1, 3 * J + 3
    xs = [sm.make_input(500 + b, soy, sox) for b in range(3)]
    ops, params = np.zeros((3, ts), np.int32), np.zeros((3, ts), F32)
    for b in range(3):
        ops[b, :ns], params[b, :ns] = sm.make_table("mixed", ns, shift=b + 1)
        params[b, :ns] *= F32(1 + b)  # per-image thresholds
    ops[:, ns:] = 77  # (behind a table: never read)
    got, k = run(dwt, lambda p, bs, sx, sy: dwt.bands_apply_batch(p, bs, 3, sx, sox, soy, J, ops, params, ts), xs)
    assert k == 1
    for b in range(3):
        check_table(got[b], xs[b], (sox, soy, sox, soy), J, ops[b, :ns], params[b, :ns])


def test_batch_with_one_table(dwt):
    sox, soy, J = 37, 29, 3
    xs = [sm.make_input(600 + b, soy, sox) for b in range(4)]
    ops, params = sm.make_table("soft", 3 * J + 1)
    got, k = run(dwt, lambda p, bs, sx, sy: dwt.bands_apply_batch(p, bs, 4, sx, sox, soy, J, ops, params), xs, pad=0)
    assert k == 1
    for b in range(4):
        check_table(got[b], xs[b], (sox, soy, sox, soy), J, ops, params)


@pytest.mark.parametrize("where", ["host", "strided"])
def test_staged_frames(dwt, golden, where):
    """a host-memory frame, and a device frame whose elements are 8 bytes apart: through the staging path, same results"""
    sox, soy, six, siy, j_max, _ = sm.CASES["inner"]
    x, J, ops, params = sm.case_arrays("inner")
    (got,), _ = run(dwt, lambda p, bs, sx, sy: dwt.bands_apply(p, sx, sy, sox, soy, six, siy, j_max, ops, params), [x],
                    device=where == "strided", step=2 if where == "strided" else 1)
    check_table(got, x, (sox, soy, six, siy), J, ops, params, golden["inner.out"])


def test_all_keep_launches_nothing(dwt):
    x = sm.make_input(3, 29, 37)
    ops, params = np.zeros(10, np.int32), np.ones(10, F32)
    for device in (True, False):
        (got,), k = run(dwt, lambda p, bs, sx, sy: dwt.bands_apply(p, sx, sy, 37, 29, 37, 29, 3, ops, params), [x], device=device)
        assert k == 0 and np.array_equal(bits(got), bits(x))


def test_multi_chunk_mapping(dwt):
    """1024 x 1024 at 5 levels: bands of many chunks beside bands of one, rows wider than a workgroup's reach"""
    sox, soy, six, siy, j_max, kind = sm.BIG
    x = sm.make_input(11, soy, sox)
    ops, params = sm.make_table(kind, 3 * j_max + 1, shift=2)
    (got,), k = run(dwt, lambda p, bs, sx, sy: dwt.bands_apply(p, sx, sy, sox, soy, six, siy, j_max, ops, params), [x])
    assert k == 1
    check_table(got, x, (sox, soy, six, siy), j_max, ops, params)


@pytest.mark.parametrize("op", [sm.LOG, sm.EXP])
def test_maps(dwt, golden, op):
    x = sm.make_input(99, 13, 21)
    f = dwt.map_log if op == sm.LOG else dwt.map_exp
    fb = dwt.map_log_batch if op == sm.LOG else dwt.map_exp_batch
    for device in (True, False):
        (got,), k = run(dwt, lambda p, bs, sx, sy: f(p, sx, sy, 21, 13, 1e-5), [x], device=device)
        d, dl = int(sm.ulps(got, golden["map." + op]).max()), int(sm.ulps(got, golden["map.%s.libm" % op]).max())
        print("%s: %d ulp from the float64 model, %d from libm" % (op, d, dl))
        assert d <= 1 and dl <= LIBM_ULPS + 1 and k == (1 if device else k)
    got, k = run(dwt, lambda p, bs, sx, sy: fb(p, bs, 3, sx, 21, 13, 1e-5), [x, x[::-1].copy(), x * F32(0.5)], pad=3)
    assert k == 1
    for g, src in zip(got, (x, x[::-1], x * F32(0.5))):
        assert sm.ulps(g, sm.apply_op(src, op, 1e-5)).max() <= 1


def test_threshold(dwt, golden):
    """bit-identical to the fixture; a batch in one call; the frames are only read"""
    for name in ("odd", "deep", "tiny", "inner", "hdr"):
        sox, soy = sm.CASES[name][:2]
        x = sm.threshold_input(sm.case_arrays(name)[0], sox, soy)
        d = Dev(dwt, x)
        lam = dwt.universal_threshold_batch(d.ptr, 0, 1, sox * 4, sox, soy)
        assert bits(lam)[0] == bits(golden[name + ".lambda"]), name
        assert np.array_equal(bits(d.get()), bits(x))
        d.free()
    xs = [sm.threshold_input(sm.make_input(40 + b, 200, 300) * F32(1 + b), 300, 200) for b in range(3)]
    buf, _ = frames(xs, 4)
    d = Dev(dwt, buf)
    lam = dwt.universal_threshold_batch(d.ptr, buf.strides[0], 3, buf.strides[1], 300, 200)
    assert np.array_equal(bits(lam), bits(np.array([sm.threshold(x, 300, 200) for x in xs], F32)))
    assert np.array_equal(bits(d.get()), bits(buf))
    host = dwt.universal_threshold_batch(buf, buf.strides[0], 3, buf.strides[1], 300, 200)
    assert np.array_equal(bits(host), bits(lam))
    d.free()


def test_existing_median_feature_keeps_its_bits(dwt):
    """the sign-blind key is a switch of the select: the MED feature still orders signed values"""
    import features_model as fm

    x = fm.make_input(5, "normal", 64, 48)
    fv = np.zeros(dwt.count_subbands(64, 48, 64, 48, 3), F32)
    dwt.features2d("med", x, 64 * 4, 4, 64, 48, 64, 48, 3, fv)
    assert np.array_equal(bits(fv), bits(fm.seq32(x, 64, 48, 64, 48, 3, 2.0)["med"]))


@pytest.mark.parametrize("wavelet", ["cdf97", "eaw53"])
def test_scale_by_one_round_trip(dwt, wavelet):
    """SCALE by 1 on every slot, then the inverse == the inverse alone, bit for bit"""
    w, h = 37, 29
    x = np.random.default_rng(8).standard_normal((h, w)).astype(F32)
    outs = []
    for scale in (False, True):
        d = Dev(dwt, x)
        if wavelet == "cdf97":
            j = dwt.dwt_cdf97_2f_s(d.ptr, w * 4, 4, w, h, w, h, -1, 0, 0)
        else:
            j, wH, wV = dwt.dwt_eaw53_2f_s(d.ptr, w * 4, 4, w, h, w, h, -1, 0, 0, alpha=1.0)
        assert j == dwt.band_levels(w, h, -1)
        if scale:
            n = dwt.band_slots(j)
            assert launches(dwt, lambda: dwt.bands_apply(d.ptr, w * 4, 4, w, h, w, h, j, ["scale"] * n, np.ones(n, F32))) == 1
        if wavelet == "cdf97":
            dwt.dwt_cdf97_2i_s(d.ptr, w * 4, 4, w, h, w, h, j, 0, 0)
        else:
            dwt.dwt_eaw53_2i_s(d.ptr, w * 4, 4, w, h, w, h, j, 0, 0, wH, wV)
        outs.append(d.get())
        d.free()
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    assert np.abs(outs[0] - x).max() < 1e-4


def test_hdr_flow(dwt, golden):
    """the flow of examples/hdr_tonemap.c on 64 x 48, step by step: each step of this feature within its tolerance of the
    model run over what the step read, and COMPRESS over the fixture's own EAW coefficients"""
    w, h, eps = 64, 48, 1e-5
    lum = sm.hdr_input(h, w)
    d = Dev(dwt, lum)
    dwt.map_log_batch(d.ptr, 0, 1, w * 4, w, h, eps)
    loglum = d.get()
    assert sm.ulps(loglum, golden["hdr.log"]).max() <= 1
    total, _, _ = dwt.eaw53_weights_layout(dwt.EAW_MALLAT, w, h, w, h, dwt.band_levels(w, h))
    wb = Dev(dwt, np.zeros(total, F32))
    j = dwt.eaw53_2d_batch(0, d.ptr, 0, 1, w * 4, w, h, wb.ptr, total, -1, alpha=0.8)
    assert j == dwt.band_levels(w, h)
    ops, params = sm.make_table("compress", dwt.band_slots(j))
    coef = d.get()
    dwt.bands_apply_batch(d.ptr, 0, 1, w * 4, w, h, j, ops, params)
    check_table(d.get(), coef, (w, h, w, h), j, ops, params)
    dwt.eaw53_2d_batch(1, d.ptr, 0, 1, w * 4, w, h, wb.ptr, total, j)
    back = d.get()
    dwt.map_exp_batch(d.ptr, 0, 1, w * 4, w, h, eps)
    out = d.get()
    assert sm.ulps(out, sm.apply_op(back, sm.EXP, eps)).max() <= 1
    assert np.isfinite(out).all()
    # the reference's own coefficients
    c = Dev(dwt, golden["hdr.eaw"])
    dwt.bands_apply(c.ptr, w * 4, 4, w, h, w, h, j, ops, params)
    worst = check_table(c.get(), golden["hdr.eaw"], (w, h, w, h), j, ops, params, golden["hdr.compressed"], golden["hdr.compressed.libm"])
    print("hdr coefficients: %d ulp from libm" % worst)
    assert worst <= LIBM_ULPS + 1
    for b in (d, wb, c):
        b.free()


def test_errors_launch_nothing(dwt):
    x = sm.make_input(1, 16, 16)
    d = Dev(dwt, x)
    n = dwt.band_slots(2)
    ops, params = np.full(n, sm.SCALE, np.int32), np.full(n, 2, F32)
    k0 = dwt.get_option("stat_launches")
    with pytest.raises(dwt.DwtError, match="null operator table"):
        dwt.bands_apply(d.ptr, 64, 4, 16, 16, 16, 16, 2, None, None)
    bad = ops.copy()
    bad[3] = 6
    with pytest.raises(dwt.DwtError, match="unknown operator"):
        dwt.bands_apply(d.ptr, 64, 4, 16, 16, 16, 16, 2, bad, params)
    bad[3] = -1
    with pytest.raises(dwt.DwtError, match="unknown operator"):
        dwt.bands_apply_batch(d.ptr, 0, 1, 64, 16, 16, 2, bad, params)
    with pytest.raises(dwt.DwtError, match="bad sizes"):
        dwt.bands_apply(d.ptr, 64, 4, -16, 16, -16, 16, 2, ops, params)
    with pytest.raises(dwt.DwtError, match="bad sizes"):
        dwt.bands_apply(d.ptr, 64, 4, 16, 16, 17, 16, 2, ops, params)
    with pytest.raises(dwt.DwtError, match="bad sizes"):
        dwt.bands_apply_batch(d.ptr, 1024, -1, 64, 16, 16, 2, ops, params)
    with pytest.raises(dwt.DwtError, match="bad strides"):
        dwt.bands_apply(d.ptr, 32, 4, 16, 16, 16, 16, 2, ops, params)
    with pytest.raises(dwt.DwtError, match="table stride"):
        dwt.bands_apply_batch(d.ptr, 512, 2, 64, 16, 8, 2, np.tile(ops, 2), np.tile(params, 2), n - 1)
    with pytest.raises(dwt.DwtError, match="unknown map"):
        dwt._check(dwt.lib.dwt_hip_map(2, d.ptr, 64, 4, 16, 16, 0.0), "dwt_hip_map")
    with pytest.raises(dwt.DwtError, match="bad sizes"):
        dwt.map_log(d.ptr, 64, 4, 16, -1, 0.0)
    with pytest.raises(dwt.DwtError, match="HH"):
        dwt.universal_threshold_batch(d.ptr, 0, 1, 64, 16, 1)
    with pytest.raises(dwt.DwtError, match="multiples of 4"):
        dwt.bands_apply(d.ptr + 2, 64, 4, 8, 8, 8, 8, 2, ops, params)
    assert dwt.get_option("stat_launches") == k0
    assert np.array_equal(bits(d.get()), bits(x))
    d.free()


def test_example_hdr_tonemap(dwt, tmp_path):
    """examples/hdr_tonemap.c: both flows on a resident batch, each against the program's own host restatement"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = tmp_path / "hdr_tonemap", os.path.join(root, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "hdr_tonemap.c"),
                           "-o", str(exe), "-L" + libdir, "-l:libdwt_hip.so", "-Wl,-rpath," + libdir, "-lm"])
    for mode in ("hdr", "denoise"):
        out = subprocess.run([str(exe), mode], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "success" in out.stdout + out.stderr, out.stdout + out.stderr
