"""The two planar 4:2:0 plans through the C-ABI (include/snnhip.h, snnhip_yuv_rgb_planar_plan_create / snnhip_rgb_cbcr_planar_plan_create) against
the float64 references of the interleaved units (tests/planar_ref.py (de)interleaves and calls them), into sentinel-filled outputs.  The comparison
rule, EPS and the 3 % near-tie cap are yuv_rgb_ref's and rgb_cbcr_ref's own.  Each sweep also prints how many values differ from the INTERLEAVED plan
on the same samples (expected 0; printed, not asserted: another instantiation may contract differently at a near tie)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import planar_ref as P
import rgb_cbcr_ref as RC
import yuv_rgb_ref as RY
from test_frame_rgb_cbcr_gpu import tile_in as cbcr_tile_in
from test_frame_yuv_rgb_gpu import _capi_dtype, _download, _refused, tile_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FILL = 0xA5


def yuv_shapes(ctx, r, container, maxval, shift):
    """the shapes of planar_ref.yuv_shapes from the tile the PLANAR plan reports; the reference module's table (the CPU near-tie test's) must agree"""
    from shadernn_amd import capi

    probe = capi.yuv_rgb_planar_plan(ctx, 1, 1, 1, 3, r, _capi_dtype(container), maxval, shift)
    tile = tile_of(probe)
    probe.destroy()
    assert tile == P.YUV_TILE[container], (tile, P.YUV_TILE[container])
    return P.yuv_shapes(r, container, tile)


def run_yuv(ctx, yhi, planes, r, C, container, maxval, shift, siting, rng, kr=RY.BT601[0], kb=RY.BT601[1], interleaved=False):
    from shadernn_amd import capi

    n, h, w = planes.shape[0] // 2, planes.shape[1], planes.shape[2]
    dt = _capi_dtype(container)
    if interleaved:
        plan = capi.yuv_rgb_plan(ctx, n, h, w, C, r, dt, maxval, shift, siting, rng, kr, kb)
        chroma = P.interleave(planes)
    else:
        plan = capi.yuv_rgb_planar_plan(ctx, n, h, w, C, r, dt, maxval, shift, siting, rng, kr, kb)
        chroma = planes
        desc = plan.describe()
        assert "yuv_rgb_planar_%s r=%d c=%d siting=%s range=%s tile=" % ("u8" if container == "u8" else "u16", r, C, siting, rng) in desc, desc
        assert "kernel=yuv_rgb_planar_kernel" in desc, desc
        assert plan.out_shape() == (n, 2 * r * h, 2 * r * w, C)
        pixels = n * 2 * r * h * 2 * r * w
        assert plan.cost()[1] == (pixels + n * h * w * 2 + pixels * C) * planes.dtype.itemsize  # both inputs once, the output once
    fill = np.full((n, 2 * r * h, 2 * r * w, C), FILL if container == "u8" else FILL * 0x101, planes.dtype)
    out = capi.Tensor.from_numpy(ctx, fill, dtype=dt)
    plan.run([capi.Tensor.from_numpy(ctx, yhi, dtype=dt), capi.Tensor.from_numpy(ctx, chroma, dtype=dt)], out)
    got = _download(out, container)
    plan.destroy()
    return got


def sweep_yuv(ctx, r, C, container, maxval, shift, shapes, sitings=P.SITINGS, ranges=P.RANGES, whole_range=False, disjoint=False, against_interleaved=True):
    """Every shape, siting and range against the reference (the near-tie cap over the sweep's values together); returns the line to print.  An output
    byte the kernel left alone would still read 0xA5: with Y in [40k, 200k) and limited range that is outside what most pixels can be, and compare()
    holds every value against the reference anyway, so every byte of the frame is shown to be written."""
    items, other = [], 0
    for siting, rng, (n, h, w), seed in P.yuv_cases(r, container, maxval, shapes, sitings, ranges):
        yhi, planes = P.yuv_frame(n, h, w, r, maxval, shift, P.np_dtype(container), seed, whole_range=whole_range, disjoint=disjoint)
        got = run_yuv(ctx, yhi, planes, r, C, container, maxval, shift, siting, rng)
        items.append((got, P.yuv_values(yhi, planes, r, siting, rng, maxval, shift), maxval, shift))
        if against_interleaved:
            other += int((got != run_yuv(ctx, yhi, planes, r, C, container, maxval, shift, siting, rng, interleaved=True)).sum())
    frac, ndiff = RY.compare_all(items)
    return "yuv_rgb_planar %s maxval=%d shift=%d r=%d c=%d, %d runs: near ties %.3f %%, %d values differ from the reference, %d from the interleaved plan" % (
        container, maxval, shift, r, C, len(items), 100 * frac, ndiff, other)


@pytest.mark.parametrize("depth", P.DEPTHS, ids=P.DEPTH_IDS)
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_yuv_rgb_planar_matches_the_reference(ctx, r, C, depth):
    container, maxval, shift = depth
    print(sweep_yuv(ctx, r, C, container, maxval, shift, yuv_shapes(ctx, r, container, maxval, shift)))


@pytest.mark.parametrize("depth", P.DEPTHS, ids=P.DEPTH_IDS)
def test_yuv_rgb_planar_clamps_over_the_whole_code_range(ctx, depth):
    container, maxval, shift = depth
    for r in (1, 2, 3):
        print(sweep_yuv(ctx, r, 3, container, maxval, shift, [(1, 5, 7), (2, 9, 41)], whole_range=True))


@pytest.mark.parametrize("depth", P.DEPTHS, ids=P.DEPTH_IDS)
def test_yuv_rgb_planar_neutral_chroma_gives_grey_byte_for_byte(ctx, depth):
    container, maxval, shift = depth
    k = (maxval + 1) // 256
    for r in (1, 2, 3, 4):
        for rng in P.RANGES:
            for n, h, w in ((1, 2, 3), (2, 9, 71)):
                yhi, planes = P.yuv_frame(n, h, w, r, maxval, shift, P.np_dtype(container), seed=r, whole_range=True)
                planes[...] = (128 * k) << shift
                got = run_yuv(ctx, yhi, planes, r, 4, container, maxval, shift, "left", rng)
                c = RY.coefficients(maxval, rng)
                yl = c[2] * ((yhi.astype(np.int64) >> shift)[..., 0].astype(np.float32) - c[0])  # fp32, as the contract's yl
                want = RY.quantise(yl.astype(np.float64), maxval, shift, yhi.dtype)
                for ch in range(3):
                    np.testing.assert_array_equal(got[..., ch], want)  # no near-tie allowance
                np.testing.assert_array_equal(got[..., 3], np.full_like(want, maxval << shift))


@pytest.mark.parametrize("depth", P.DEPTHS, ids=P.DEPTH_IDS)
def test_yuv_rgb_planar_does_not_swap_or_mix_the_planes(ctx, depth):
    """Cb below and Cr above the neutral code, N = 2 with odd H * W: a swapped pair, a wrong plane stride or the second image's planes taken for the
    first's fail the comparison outright (B < yl < R everywhere)."""
    container, maxval, shift = depth
    for r in (1, 2):
        print(sweep_yuv(ctx, r, 3, container, maxval, shift, [(2, 5, 7), (2, 3, 131)], ranges=["full"], disjoint=True))
    yhi, planes = P.yuv_frame(2, 5, 7, 1, maxval, shift, P.np_dtype(container), seed=3, disjoint=True)
    got = run_yuv(ctx, yhi, planes, 1, 3, container, maxval, shift, "left", "full").astype(np.int64)
    assert (got[..., 2] < got[..., 0]).all()  # B = yl + cbu (Cb - Coff) < yl < R = yl + crv (Cr - Coff)


def run_cbcr(ctx, rgb, r, siting="left", rng="limited", kr=RC.BT601[0], kb=RC.BT601[1], interleaved=False):
    from shadernn_amd import capi

    n, h, w, C = rgb.shape
    oh, ow = r * h // 2, r * w // 2
    if interleaved:
        plan = capi.rgb_cbcr_plan(ctx, n, h, w, C, r, siting, rng, kr, kb)
        shape = (n, oh, ow, 2)
    else:
        plan = capi.rgb_cbcr_planar_plan(ctx, n, h, w, C, r, siting, rng, kr, kb)
        shape = (2 * n, oh, ow, 1)
        desc = plan.describe()
        assert "rgb_cbcr_planar_u8 r=%d c=%d siting=%s range=%s tile=" % (r, C, siting, rng) in desc and "kernel=rgb_cbcr_planar_kernel" in desc, desc
        assert plan.out_shape() == shape
        assert plan.cost()[1] == n * h * w * C + n * oh * ow * 2
    out = capi.Tensor.from_numpy(ctx, np.full(shape, FILL, np.uint8), dtype=capi.U8)
    plan.run([capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8)], out)
    got = out.numpy_u8()
    plan.destroy()
    return got if interleaved else P.interleave(got)


def sweep_cbcr(ctx, r, C, shapes, sitings=P.SITINGS, ranges=P.RANGES, primaries=False):
    """as sweep_yuv, on the interleaved view of the two planes: a byte of either plane that the kernel left at 0xA5 fails compare()"""
    items, other = [], 0
    for siting, rng, (n, h, w), seed in P.cbcr_cases(r, C, shapes, sitings, ranges):
        rgb = RC.frame(seed, n, h, w, C, primaries=primaries)
        got = run_cbcr(ctx, rgb, r, siting, rng)
        items.append((got, RC.values(rgb, r, siting, rng)))
        other += int((got != run_cbcr(ctx, rgb, r, siting, rng, interleaved=True)).sum())
    frac, ndiff = RC.compare_all(items)
    return "rgb_cbcr_planar r=%d c=%d, %d runs: near ties %.3f %%, %d bytes differ from the reference, %d from the interleaved plan" % (r, C, len(items), 100 * frac, ndiff, other)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_rgb_cbcr_planar_matches_the_reference(ctx, r, C):
    print(sweep_cbcr(ctx, r, C, RC.shapes_for(r, cbcr_tile_in(ctx, r))))


@pytest.mark.parametrize("r", [2, 3, 4])
def test_rgb_cbcr_planar_clamps_over_saturated_primaries(ctx, r):
    print(sweep_cbcr(ctx, r, 3, [(1, 6, 8), (2, 10, 42)], primaries=True))


def test_rgb_cbcr_planar_grey_gives_128_and_planes_are_not_swapped(ctx):
    for r in (2, 3, 4):
        grey = np.repeat(RC.frame(5, 2, 6, 10, 1), 3, axis=-1)
        assert (run_cbcr(ctx, grey, r) == 128).all()
        blue = np.zeros((2, 6, 10, 3), np.uint8)
        blue[..., 2] = 200  # Cb far above 128, Cr below it, in every pixel of both images
        got = run_cbcr(ctx, blue, r)
        assert (got[..., 0] > 160).all() and (got[..., 1] < 128).all()


def test_trace_report_names_the_kernels(ctx):
    from shadernn_amd import capi

    capi.trace_begin()
    yhi, planes = P.yuv_frame(1, 9, 13, 2, 255, 0, np.uint8, seed=1)
    run_yuv(ctx, yhi, planes, 2, 3, "u8", 255, 0, "left", "limited")
    run_cbcr(ctx, RC.frame(1, 1, 6, 10, 3), 2)
    ctx.sync()
    text = str(capi.trace_end())
    assert "yuv_rgb_planar_kernel" in text and "rgb_cbcr_planar_kernel" in text, text


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    mk = capi.yuv_rgb_planar_plan
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2), "yuv_rgb desc", "2 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 5), "yuv_rgb desc", "r = 5")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.F32), "yuv_rgb desc", "dtype")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U16, 8191, 0), "yuv_rgb desc", "4095")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U8, 127, 0), "yuv_rgb desc", "multiple of 256")
    n, h, w, C, r = 1, 4, 6, 3, 2
    plan = mk(ctx, n, h, w, C, r)
    yhi, planes = P.yuv_frame(n, h, w, r, 255, 0, np.uint8, seed=1)
    y = capi.Tensor.from_numpy(ctx, yhi, dtype=capi.U8)
    c = capi.Tensor.from_numpy(ctx, planes, dtype=capi.U8)
    out = capi.Tensor.from_numpy(ctx, np.full((n, 4 * h, 4 * w, C), FILL, np.uint8), dtype=capi.U8)
    plan.run([y, c], out)  # the valid call
    _refused(lambda: plan.run([y, capi.Tensor(ctx, n, h, w, 2, dtype=capi.U8)], out), "yuv_rgb_planar", "the chroma tensor is", "[2N][H][W][1]")  # the interleaved plane
    _refused(lambda: plan.run([y, capi.Tensor(ctx, n, h, w, 1, dtype=capi.U8)], out), "yuv_rgb_planar", "the chroma tensor is")                 # one plane only
    _refused(lambda: plan.run([y, capi.Tensor(ctx, 2 * n, h + 1, w, 1, dtype=capi.U8)], out), "yuv_rgb_planar", "the chroma tensor is")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, 2 * h, 2 * w, 1, dtype=capi.U8), c], out), "yuv_rgb_planar", "Yhi is")
    _refused(lambda: plan.run([y, c], capi.Tensor(ctx, n, 4 * h, 4 * w, 4, dtype=capi.U8)), "yuv_rgb_planar", "the output is")
    _refused(lambda: plan.run([y], out), "yuv_rgb_planar", "2 inputs")
    _refused(lambda: plan.run([y, capi.Tensor(ctx, 2 * n, h, w, 1, dtype=capi.U16)], out), "plan_run", "16-bit")  # a 16-bit tensor into an 8-bit plan
    _refused(lambda: plan.run([y, capi.Tensor(ctx, 2 * n, h, w, 1)], out), "plan_run: input 1 has dtype 0")
    wide = mk(ctx, n, h, w, C, r, capi.U16, 1023, 6)
    _refused(lambda: wide.run([y, c], capi.Tensor(ctx, n, 4 * h, 4 * w, C, dtype=capi.U16)), "plan_run", "8-bit")
    RY.compare(out.numpy_u8(), P.yuv_values(yhi, planes, r, "left", "limited", 255, 0), 255, 0)  # nothing above touched the valid result

    mk = capi.rgb_cbcr_planar_plan
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 1), "rgb_cbcr desc", "r = 1", "decimation")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 5), "rgb_cbcr desc", "r = 5")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2), "rgb_cbcr desc", "2 channels")
    _refused(lambda: mk(ctx, 1, 3, 4, 3, 3), "rgb_cbcr desc", "odd extent")
    plan = mk(ctx, 1, 4, 6, 3, 2)
    rgb = capi.Tensor.from_numpy(ctx, RC.frame(1, 1, 4, 6, 3), dtype=capi.U8)
    _refused(lambda: plan.run([rgb], capi.Tensor(ctx, 1, 4, 6, 2, dtype=capi.U8)), "rgb_cbcr_planar", "the output is", "[2N][rH/2][rW/2][1]")  # the interleaved plane
    _refused(lambda: plan.run([rgb], capi.Tensor(ctx, 1, 4, 6, 1, dtype=capi.U8)), "rgb_cbcr_planar", "the output is")
    _refused(lambda: plan.run([capi.Tensor(ctx, 1, 4, 6, 4, dtype=capi.U8)], capi.Tensor(ctx, 2, 4, 6, 1, dtype=capi.U8)), "rgb_cbcr_planar", "the input frame is")
    _refused(lambda: plan.run([rgb], capi.Tensor(ctx, 2, 4, 6, 1, dtype=capi.U16)), "plan_run")
    plan.run([rgb], capi.Tensor(ctx, 2, 4, 6, 1, dtype=capi.U8))  # the valid call


def test_the_plans_are_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, checked by snnhip_sync) is fixed at the library's first allocation: a child process,
    started the way tests/test_frame_yuv_rgb_gpu.py starts its own, runs one sweep of each plan -- every r, C and depth on every shape.  Valid shapes
    only: no SNNHIP_E_GUARD may come back."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import rgb_cbcr_ref as RC
        import test_frame_planar_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for r in (1, 2, 3, 4):
            for C in (3, 4):
                for container, maxval, shift in T.P.DEPTHS:
                    T.sweep_yuv(ctx, r, C, container, maxval, shift, T.yuv_shapes(ctx, r, container, maxval, shift), sitings=["left"], ranges=["limited"], against_interleaved=False)
                    ctx.sync()                               # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write
                if r >= 2:
                    T.sweep_cbcr(ctx, r, C, RC.shapes_for(r), sitings=["left"], ranges=["limited"])
                    ctx.sync()
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]
