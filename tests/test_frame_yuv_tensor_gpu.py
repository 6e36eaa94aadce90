"""The video-frame -> input-tensor plan through the C-ABI (include/snnhip.h, snnhip_yuv_tensor_plan_create / _planar_plan_create) against the float64
reference of tests/yuv_tensor_ref.py, into NaN-filled (fp32) or sentinel-filled (fp16) outputs.  Every output element is compared, nothing left out:
|got - want| <= |norms[c]| E(bits), plus half an fp16 ulp for fp16 output; E = 4 x the fp32-to-float64 distance of the reference on exactly these
frames (yuv_tensor_ref.E; tests/test_frame_yuv_tensor.py measures it on the CPU).  Alpha is exact."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import planar_ref
import yuv_rgb_ref
import yuv_tensor_ref as R
from test_frame_yuv_rgb_gpu import _capi_dtype, _download, _refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SENTINEL = -60000.0  # exact in fp16, outside every tensor of these tests


def run_plan(ctx, y, chroma, oh, ow, C, half=False, container="u8", maxval=255, shift=0, siting="left", rng="limited", kr=R.BT601[0], kb=R.BT601[1], flt="linear", means=(0, 0, 0),
             norms=(1, 1, 1), alpha=R.ALPHA, planar=False):
    """`chroma` is the tensor as the plan takes it: cbcr [N][H/2][W/2][2], or with planar=True [2N][H/2][W/2][1].  Returns the tensor as float32."""
    from shadernn_amd import capi

    n, h, w, _ = y.shape
    dt = _capi_dtype(container)
    odt = capi.F16 if half else capi.F32
    plan = capi.yuv_tensor_plan(ctx, n, h, w, oh, ow, C, dt, odt, maxval, shift, siting, rng, kr, kb, flt, means, norms, alpha, planar)
    desc = plan.describe()
    name = "yuv_tensor_planar" if planar else "yuv_tensor"
    assert desc.startswith("%s_%s c=%d %s %s siting=%s range=%s %dx%d->%dx%d tile=%d taps=" % (name, "u8" if container == "u8" else "u16", C, "f16" if half else "f32", flt, siting,
                                                                                             rng, h, w, oh, ow, R.TILE[(C, half)])), desc
    assert desc.endswith("kernel=%s_kernel" % name), desc
    assert plan.out_shape() == (n, oh, ow, C)
    assert plan.cost()[1] == (y.size + chroma.size) * y.dtype.itemsize + n * oh * ow * C * (2 if half else 4)  # both inputs once, the output once
    out = capi.Tensor.from_numpy(ctx, np.full((n, oh, ow, C), SENTINEL if half else np.nan, np.float32), dtype=odt)
    plan.run([capi.Tensor.from_numpy(ctx, y, dtype=dt), capi.Tensor.from_numpy(ctx, np.ascontiguousarray(chroma), dtype=dt)], out)
    got = out.numpy()
    plan.destroy()
    assert not (got == SENTINEL).any(), "%d output values were not written" % int((got == SENTINEL).sum())
    return got


def run_case(ctx, case, C, half, container, maxval, shift, planar=False):
    (n, h, w, oh, ow), flt, siting, rng, (kr, kb), whole, means, norms, seed = case
    y, cbcr = R.case_frames(case, container, maxval, shift)
    got = run_plan(ctx, y, planar_ref.deinterleave(cbcr) if planar else cbcr, oh, ow, C, half, container, maxval, shift, siting, rng, kr, kb, flt, means, norms, R.ALPHA, planar)
    return got, y, cbcr


def sweep(ctx, C, half, container, maxval, shift, planar=False, cases=None):
    """Every case of the sweep against the reference; returns the line to print."""
    worst, runs = 0.0, 0
    for case in cases or R.sweep_cases(C, half, container, maxval, shift):
        got, y, cbcr = run_case(ctx, case, C, half, container, maxval, shift, planar)
        worst = max(worst, R.compare(got, R.case_tensor(case, y, cbcr, C, maxval, shift), case[7], maxval, half))
        if C == 4:
            assert (got[..., 3] == np.float32(R.ALPHA)).all(), "alpha is not %g everywhere" % R.ALPHA
        runs += 1
    return "yuv_tensor%s %s maxval=%d shift=%d c=%d %s, %d runs: largest |got - want| is %.3f of the tolerance" % (" planar" if planar else "", container, maxval, shift, C,
                                                                                                                     "f16" if half else "f32", runs, worst)


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("c", [3, 4])
def test_plan_matches_the_reference(ctx, c, half, depth):
    container, maxval, shift = depth
    print(sweep(ctx, c, half, container, maxval, shift))


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_planar_plan_matches_the_reference(ctx, depth):
    container, maxval, shift = depth
    for c, half in ((3, True), (4, False)):
        print(sweep(ctx, c, half, container, maxval, shift, planar=True))


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_planar_and_interleaved_chroma_give_the_same_tensor(ctx, depth):
    container, maxval, shift = depth
    for c, half in ((3, False), (3, True), (4, True)):
        for case in R.sweep_cases(c, half, container, maxval, shift):
            a, _, _ = run_case(ctx, case, c, half, container, maxval, shift)
            b, _, _ = run_case(ctx, case, c, half, container, maxval, shift, planar=True)
            assert int((a != b).sum()) == 0, case[:4]


def test_the_reported_tile_is_the_references(ctx):
    from shadernn_amd import capi

    for (c, half), tile in R.TILE.items():
        plan = capi.yuv_tensor_plan(ctx, 1, 2, 2, 2, 2, c, capi.U8, capi.F16 if half else capi.F32)
        assert int(re.search(r"tile=(\d+) ", plan.describe()).group(1)) == tile
        assert "taps=single" in plan.describe()  # ratio 1: one source pixel per output pixel
        plan.destroy()
    for flt, taps in (("linear", "bilinear"), ("nearest", "single")):
        plan = capi.yuv_tensor_plan(ctx, 1, 1080, 1920, 224, 224, 4, filter=flt)
        assert "taps=" + taps in plan.describe(), plan.describe()
        assert plan.describe().startswith("yuv_tensor_u8 c=4 f32 %s siting=left range=limited 1080x1920->224x224 " % flt), plan.describe()
        plan.destroy()


def test_low_bits_of_a_high_aligned_frame_are_ignored(ctx):
    """P010 containers carry ten bits in the high end; whatever sits in the six bits below them must not reach the result."""
    g = np.random.default_rng(12)
    for n, h, w, oh, ow in [(2, 10, 12, 7, 9), (1, 6, 8, 6, 8)]:
        y, cbcr = R.frame(n, h, w, 1023, 6, np.uint16, seed=70 + h)
        dy = y | g.integers(1, 64, size=y.shape).astype(np.uint16)
        dc = cbcr | g.integers(1, 64, size=cbcr.shape).astype(np.uint16)
        for planar, conv in ((False, lambda a: a), (True, planar_ref.deinterleave)):
            np.testing.assert_array_equal(run_plan(ctx, dy, conv(dc), oh, ow, 4, False, "u16", 1023, 6, planar=planar),
                                          run_plan(ctx, y, conv(cbcr), oh, ow, 4, False, "u16", 1023, 6, planar=planar))


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_neutral_chroma_gives_equal_channels(ctx, depth):
    container, maxval, shift = depth
    k = (maxval + 1) // 256
    for n, h, w, oh, ow in R.shapes(3, True)[:5] + [(2, 10, 12, 9, 33)]:
        y, _ = R.frame(n, h, w, maxval, shift, planar_ref.np_dtype(container), seed=h + oh, whole_range=True)
        cbcr = np.full((n, h // 2, w // 2, 2), (128 * k) << shift, y.dtype)
        for flt in ("linear", "nearest"):
            for rng in R.RANGES:
                for half in (False, True):
                    got = run_plan(ctx, y, cbcr, oh, ow, 3, half, container, maxval, shift, "centre", rng, flt=flt)
                    np.testing.assert_array_equal(got[..., 0], got[..., 1])
                    np.testing.assert_array_equal(got[..., 0], got[..., 2])
                    R.compare(got, R.tensor(y, cbcr, oh, ow, 3, flt, "centre", rng, maxval, shift), (1, 1, 1), maxval, half)


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_ratio_one_against_the_yuv_rgb_plans_bytes(ctx, depth):
    """OH = H, OW = W, means 0, norms 1: rint(t) is yuv_rgb's value at r = 1 off the near ties (the rule and the cap of the CPU suite)."""
    from shadernn_amd import capi

    container, maxval, shift = depth
    dt = _capi_dtype(container)
    items = []
    for y, cbcr, siting, rng in R.ratio1_cases(container, maxval, shift):
        n, h, w, _ = y.shape
        plan = capi.yuv_rgb_plan(ctx, n, h // 2, w // 2, 3, 1, dt, maxval, shift, siting, rng)
        out = capi.Tensor.from_numpy(ctx, np.zeros((n, h, w, 3), y.dtype), dtype=dt)
        plan.run([capi.Tensor.from_numpy(ctx, y, dtype=dt), capi.Tensor.from_numpy(ctx, cbcr, dtype=dt)], out)
        fixed = _download(out, container).astype(np.int64) >> shift
        plan.destroy()
        got = run_plan(ctx, y, cbcr, h, w, 3, False, container, maxval, shift, siting, rng)
        items.append((np.rint(got.astype(np.float64)), fixed, R.source(y, cbcr, siting, rng, maxval, shift)))
    frac, ndiff = R.compare_ratio1(items, maxval)
    print("ratio 1 against yuv_rgb, %s maxval=%d shift=%d, %d frames: near ties %.3f %%, %d values differ" % (container, maxval, shift, len(items), 100 * frac, ndiff))


def test_the_three_launch_composition_of_existing_plans_is_within_half_a_code(ctx):
    """yuv_rgb at r = 1, image_u8, resize (8 bits only) round to a byte in the middle and blend the rounded bytes: every value lies within
    0.5 |norm| (a convex blend of rounding errors of at most half a code each) plus the tolerance.  A wrong phase or siting would not."""
    from shadernn_amd import capi

    worst = 0.0
    for k, (n, h, w, oh, ow) in enumerate([(1, 48, 64, 5, 7), (2, 10, 12, 9, 33), (1, 6, 8, 6, 8), (1, 16, 24, 40, 56)]):
        for si, siting in enumerate(R.SITINGS):
            for flt in ("linear", "nearest"):
                means, norms = R.normalisation(k + si, 255)
                y, cbcr = R.frame(n, h, w, 255, 0, np.uint8, seed=800 + k, whole_range=bool(k % 2))
                rgb = capi.Tensor(ctx, n, h, w, 4, dtype=capi.U8)
                f = capi.Tensor(ctx, n, h, w, 4)
                t = capi.Tensor.from_numpy(ctx, np.full((n, oh, ow, 4), np.nan, np.float32))
                p1 = capi.yuv_rgb_plan(ctx, n, h // 2, w // 2, 4, 1, capi.U8, 255, 0, siting)
                p2 = capi.image_u8_plan(ctx, n, h, w, 4)
                p3 = capi.resize_plan(ctx, n, h, w, 4, oh, ow, tuple(means) + (0.0,), tuple(norms) + (1.0,), linear=flt == "linear")
                p1.run([capi.Tensor.from_numpy(ctx, y, dtype=capi.U8), capi.Tensor.from_numpy(ctx, cbcr, dtype=capi.U8)], rgb)
                p2.run(rgb, f)
                p3.run(f, t)
                three = t.numpy()[..., :3].astype(np.float64)
                for p in (p1, p2, p3):
                    p.destroy()
                got = run_plan(ctx, y, cbcr, oh, ow, 3, False, siting=siting, flt=flt, means=means, norms=norms).astype(np.float64)
                bound = (0.5 + R.E[255]) * np.abs(np.asarray(norms, np.float32).astype(np.float64))
                err = np.abs(got - three)
                assert (err <= bound).all(), (n, h, w, oh, ow, siting, flt, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
    print("the three-launch composition: largest distance %.3f of 0.5 |norm| + tolerance" % worst)


def test_trace_report_names_the_kernel(ctx):
    from shadernn_amd import capi

    for planar, name in ((False, "yuv_tensor_kernel"), (True, "yuv_tensor_planar_kernel")):
        plan = capi.yuv_tensor_plan(ctx, 1, 6, 8, 5, 7, 3, planar=planar)
        y, cbcr = R.frame(1, 6, 8, 255, 0, np.uint8, seed=1)
        out = capi.Tensor(ctx, 1, 5, 7, 3)
        a, b = capi.Tensor.from_numpy(ctx, y, dtype=capi.U8), capi.Tensor.from_numpy(ctx, planar_ref.deinterleave(cbcr) if planar else cbcr, dtype=capi.U8)
        capi.trace_begin()
        plan.run([a, b], out)
        ctx.sync()
        text = str(capi.trace_end())
        assert name in text, text
        plan.destroy()


def test_a_recorded_graph_replays(ctx):
    from shadernn_amd import capi

    n, h, w, oh, ow = 2, 10, 12, 9, 33
    plan = capi.yuv_tensor_plan(ctx, n, h, w, oh, ow, 3, capi.U8, capi.F16)
    y, cbcr = R.frame(n, h, w, 255, 0, np.uint8, seed=3)
    a, b = capi.Tensor.from_numpy(ctx, y, dtype=capi.U8), capi.Tensor.from_numpy(ctx, cbcr, dtype=capi.U8)
    out = capi.Tensor.from_numpy(ctx, np.full((n, oh, ow, 3), SENTINEL, np.float32), dtype=capi.F16)
    with capi.Graph.capture(ctx) as g:
        plan.run([a, b], out)
    assert g.num_nodes() == 1
    for seed in (4, 5):  # replayed twice, on fresh inputs each time
        y, cbcr = R.frame(n, h, w, 255, 0, np.uint8, seed=seed)
        a.upload_u8(y)
        b.upload_u8(cbcr)
        out.upload(np.full((n, oh, ow, 3), SENTINEL, np.float32))
        g.launch()
        ctx.sync()
        R.compare(out.numpy(), R.tensor(y, cbcr, oh, ow, 3), (1, 1, 1), 255, True)
    g.destroy()
    plan.destroy()


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    mk = capi.yuv_tensor_plan
    for planar in (False, True):
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 2, planar=planar), "yuv_tensor desc", "2 channels")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 5, planar=planar), "yuv_tensor desc", "5 channels")
        _refused(lambda: mk(ctx, 1, 5, 4, 3, 3, 3, planar=planar), "yuv_tensor desc", "5x4", "even")
        _refused(lambda: mk(ctx, 1, 4, 7, 3, 3, 3, planar=planar), "yuv_tensor desc", "4x7", "even")
        _refused(lambda: mk(ctx, 1, 4, 4, 0, 3, 3, planar=planar), "yuv_tensor desc", "0x3 output")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, -1, 3, planar=planar), "yuv_tensor desc", "3x-1 output")
        _refused(lambda: mk(ctx, 0, 4, 4, 3, 3, 3, planar=planar), "yuv_tensor desc", "bad dims")
        _refused(lambda: mk(ctx, 1, 0, 4, 3, 3, 3, planar=planar), "yuv_tensor desc", "bad dims")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, filter=2, planar=planar), "yuv_tensor desc", "filter 2")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, filter=-1, planar=planar), "yuv_tensor desc", "filter -1")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.U8, capi.U8, planar=planar), "yuv_tensor desc", "out_dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.U8, capi.U16, planar=planar), "yuv_tensor desc", "out_dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.F32, planar=planar), "yuv_tensor desc", "dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.F16, planar=planar), "yuv_tensor desc", "dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.U8, capi.F32, 1023, 0, planar=planar), "yuv_tensor desc", "does not fit")   # above 255 in a byte
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.U16, capi.F32, 65535, 0, planar=planar), "yuv_tensor desc", "4095")          # above 12 bits
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.U16, capi.F32, 1023, 7, planar=planar), "yuv_tensor desc", "does not fit")   # 1023 << 7 needs 17 bits
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.U8, capi.F32, 255, 1, planar=planar), "yuv_tensor desc", "shift 1")          # 8-bit frames have no shift
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.U8, capi.F32, 127, 0, planar=planar), "yuv_tensor desc", "multiple of 256")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, capi.U16, capi.F32, 1000, 0, planar=planar), "yuv_tensor desc", "multiple of 256")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, siting=2, planar=planar), "yuv_tensor desc", "siting")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, range=2, planar=planar), "yuv_tensor desc", "range")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, kr=0.0, planar=planar), "yuv_tensor desc", "kr")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, kb=-0.1, planar=planar), "yuv_tensor desc", "kb")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, 3, 3, kr=0.7, kb=0.3, planar=planar), "yuv_tensor desc", "kr + kb < 1")
    n, h, w, oh, ow, C = 1, 4, 6, 5, 7, 3
    plan = mk(ctx, n, h, w, oh, ow, C)
    y, cbcr = R.frame(n, h, w, 255, 0, np.uint8, seed=1)
    a, b = capi.Tensor.from_numpy(ctx, y, dtype=capi.U8), capi.Tensor.from_numpy(ctx, cbcr, dtype=capi.U8)
    out = capi.Tensor.from_numpy(ctx, np.full((n, oh, ow, C), np.nan, np.float32))
    plan.run([a, b], out)  # the valid call
    for bad in ((n, oh + 1, ow, C), (n, oh, ow + 1, C), (n, oh, ow, 4), (n, oh, ow, 1), (2, oh, ow, C)):
        _refused(lambda: plan.run([a, b], capi.Tensor(ctx, *bad)), "yuv_tensor", "the output is")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, h, w + 2, 1, dtype=capi.U8), b], out), "yuv_tensor", "the luma plane is")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, h // 2, w // 2, 1, dtype=capi.U8), b], out), "yuv_tensor", "the luma plane is")
    _refused(lambda: plan.run([a, capi.Tensor(ctx, n, h, w, 2, dtype=capi.U8)], out), "yuv_tensor", "the chroma plane is")           # chroma at the luma size
    _refused(lambda: plan.run([a, capi.Tensor(ctx, 2 * n, h // 2, w // 2, 1, dtype=capi.U8)], out), "yuv_tensor", "the chroma plane is")  # planar planes into a CbCr plan
    _refused(lambda: plan.run([a], out), "yuv_tensor", "2 inputs")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, h, w, 1), b], out), "yuv_tensor", "both inputs must have dtype")                  # a float tensor as the luma plane
    _refused(lambda: plan.run([a, capi.Tensor(ctx, n, h // 2, w // 2, 2)], out), "yuv_tensor", "both inputs must have dtype")        # ... as the chroma plane
    _refused(lambda: plan.run([a, capi.Tensor(ctx, n, h // 2, w // 2, 2, dtype=capi.U16)], out), "plan_run", "16-bit")              # a 16-bit plane into an 8-bit plan
    _refused(lambda: plan.run([a, b], capi.Tensor(ctx, n, oh, ow, C, dtype=capi.F16)), "yuv_tensor", "the output must have dtype")   # a half tensor out of an fp32 plan
    _refused(lambda: plan.run([a, b], capi.Tensor(ctx, n, oh, ow, C, dtype=capi.U8)), "plan_run", "8-bit")                           # a byte tensor as the output
    wide = mk(ctx, n, h, w, oh, ow, C, capi.U16, capi.F32, 1023, 6)
    _refused(lambda: wide.run([a, b], out), "plan_run", "8-bit")                                                                      # 8-bit planes into a 16-bit plan
    planar = mk(ctx, n, h, w, oh, ow, C, planar=True)
    _refused(lambda: planar.run([a, b], out), "yuv_tensor_planar", "the chroma tensor is", "[2N][H/2][W/2][1]")                       # a CbCr plane into a planar plan
    R.compare(out.numpy(), R.tensor(y, cbcr, oh, ow, C), (1, 1, 1), 255, False)  # nothing above touched the valid result


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, checked by snnhip_sync) is fixed at the library's first allocation: a child
    process, started the way tests/test_frame_rgb_fit_gpu.py starts its own, runs every sweep once, interleaved and planar.  Valid shapes only: no
    SNNHIP_E_GUARD may come back."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_frame_yuv_tensor_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for c in (3, 4):
            for half in (False, True):
                for planar in (False, True):
                    for container, maxval, shift in T.R.DEPTHS:
                        T.sweep(ctx, c, half, container, maxval, shift, planar)
                        ctx.sync()                           # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]
