"""The RGB -> 4:2:0 CbCr plan through the C-ABI (include/snnhip.h, snnhip_rgb_cbcr_plan_create) against the float64 reference of
tests/rgb_cbcr_ref.py, into sentinel-filled outputs.  The comparison rule (rgb_cbcr_ref.compare_all): a byte equals the reference's wherever the
reference's pre-rounding value is farther than eps = 1e-3 from a tie (40 times the measured fp32-to-float64 distance of the expression, 4 times its
worst case), is at most 1 off on near ties, and near ties are at most 3 % of a sweep's values taken together, asserted on the reference alone
(tests/test_frame_rgb_cbcr.py holds the share of these very frames to 0.5 %)."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import rgb_cbcr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

FILL = 0xA5


def tile_of(plan):
    m = re.search(r"tile=(\d+)x(\d+)", plan.describe())
    assert m, plan.describe()
    return int(m.group(1)), int(m.group(2))


def tile_in(ctx, r):
    """the tile the plan reports (output chroma pixels) in input pixels; the reference module's table, which the CPU near-tie test uses, must agree"""
    from shadernn_amd import capi

    probe = capi.rgb_cbcr_plan(ctx, 1, 2, 2, 3, r)
    th, tw = tile_of(probe)
    probe.destroy()
    assert (2 * th) % r == 0 and (2 * tw) % r == 0, (r, th, tw)
    t = (2 * th // r, 2 * tw // r)
    assert t == R.TILE_IN[r], (r, t, R.TILE_IN[r])
    return t


def run_plan(ctx, rgb, r, siting="left", rng="limited", kr=R.BT601[0], kb=R.BT601[1]):
    from shadernn_amd import capi

    n, h, w, C = rgb.shape
    plan = capi.rgb_cbcr_plan(ctx, n, h, w, C, r, siting, rng, kr, kb)
    desc = plan.describe()
    assert "rgb_cbcr_u8 r=%d c=%d siting=%s range=%s tile=" % (r, C, siting, rng) in desc and "kernel=rgb_cbcr_kernel" in desc, desc
    oh, ow = r * h // 2, r * w // 2
    assert plan.out_shape() == (n, oh, ow, 2)
    assert plan.cost()[1] == n * h * w * C + n * oh * ow * 2  # the input once, the output once
    out = capi.Tensor.from_numpy(ctx, np.full((n, oh, ow, 2), FILL, np.uint8), dtype=capi.U8)
    plan.run([capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8)], out)
    got = out.numpy_u8()
    plan.destroy()
    return got


def sweep(ctx, r, C, shapes, sitings=R.SITINGS, ranges=R.RANGE_NAMES, primaries=False):
    """Every shape, siting and range against the reference (the near-tie cap over the sweep's values together); returns the line to print."""
    items = []
    for siting, rng, (n, h, w), seed in R.sweep_cases(r, C, shapes, sitings, ranges):
        rgb = R.frame(seed, n, h, w, C, primaries=primaries)
        items.append((run_plan(ctx, rgb, r, siting, rng), R.values(rgb, r, siting, rng)))
    frac, ndiff = R.compare_all(items)
    return "rgb_cbcr r=%d c=%d, %d runs: near ties %.3f %%, %d bytes differ" % (r, C, len(items), 100 * frac, ndiff)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_plan_matches_the_reference(ctx, r, C):
    print(sweep(ctx, r, C, R.shapes_for(r, tile_in(ctx, r))))


@pytest.mark.parametrize("r", [2, 3, 4])
def test_the_clamps_over_saturated_primaries(ctx, r):
    """The whole code range, half the pixels saturated primaries (rgb_cbcr_ref.frame): the cubic overshoots between saturated colours, and in full
    range pure blue and pure red already sit at 255.5."""
    shapes = [(1, 6, 8), (1, 10, 40)]
    print(sweep(ctx, r, 3, shapes, primaries=True))
    assert R.clamp_fraction(R.values(R.frame(1, 1, 10, 40, 3, primaries=True), r, R.LEFT, R.FULL)) > 0.005  # the recipe does clamp


def test_grey_gives_128_byte_for_byte_and_a_constant_frame_a_constant_plane(ctx):
    for r in (2, 3, 4):
        for rng in R.RANGE_NAMES:
            for siting in R.SITINGS:
                for n, h, w in ((1, 2, 6), (2, 10, 70)):
                    grey = np.repeat(R.frame(r, n, h, w, 1), 3, axis=-1)
                    grey.reshape(-1, 3)[:min(256, n * h * w)] = np.arange(min(256, n * h * w), dtype=np.uint8)[:, None]  # every grey level
                    np.testing.assert_array_equal(run_plan(ctx, grey, r, siting, rng), np.full((n, r * h // 2, r * w // 2, 2), 128, np.uint8))  # no near-tie allowance
                const = np.empty((2, 6, 10, 4), np.uint8)
                const[...] = (200, 30, 90, 7)
                got = run_plan(ctx, const, r, siting, rng)
                assert (got == got[0, 0, 0]).all()
                np.testing.assert_array_equal(got[0, 0, 0], R.cbcr(const, r, siting, rng)[0, 0, 0])


def test_r2_centre_is_the_per_pixel_conversion(ctx):
    for C in (3, 4):
        for rng in R.RANGE_NAMES:
            rgb = R.frame(17 + C, 2, 9, 70, C)
            got = run_plan(ctx, rgb, 2, "centre", rng)
            assert got.shape == (2, 9, 70, 2)
            R.compare_all([(got, R.per_pixel(rgb, rng))])


def test_the_two_sitings_differ_on_a_horizontal_ramp(ctx):
    w = 24
    rgb = np.full((1, 4, w, 3), 60, np.uint8)
    rgb[..., 2] = (8 * np.arange(w) + 20).astype(np.uint8)[None, None, :]  # B rises: so does Cb
    for r in (2, 3, 4):
        left, centre = (run_plan(ctx, rgb, r, s, "full") for s in ("left", "centre"))
        assert not np.array_equal(left, centre)
        edge = 2 * r
        assert (centre[0, 0, edge:-edge, 0].astype(int) >= left[0, 0, edge:-edge, 0].astype(int)).all()  # centre sits half an output luma column further on
        assert (centre[0, 0, edge:-edge, 0].astype(int) > left[0, 0, edge:-edge, 0].astype(int)).any()


def test_another_matrix(ctx):
    rgb = R.frame(5, 1, 10, 70, 3)
    for r in (2, 3):
        got = run_plan(ctx, rgb, r, "left", "limited", *R.BT709)
        R.compare_all([(got, R.values(rgb, r, R.LEFT, R.LIMITED, *R.BT709))])
        assert not np.array_equal(got, run_plan(ctx, rgb, r, "left", "limited"))


def test_alpha_is_ignored(ctx):
    for r in (2, 3, 4):
        rgba = R.frame(30 + r, 2, 10, 70, 4)
        np.testing.assert_array_equal(run_plan(ctx, rgba, r), run_plan(ctx, np.ascontiguousarray(rgba[..., :3]), r))
        other = rgba.copy()
        other[..., 3] ^= 0xFF
        np.testing.assert_array_equal(run_plan(ctx, other, r), run_plan(ctx, rgba, r))


def test_trace_report_names_the_kernel(ctx):
    from shadernn_amd import capi

    plan = capi.rgb_cbcr_plan(ctx, 1, 9, 13, 3, 2)
    out = capi.Tensor.from_numpy(ctx, np.zeros((1, 9, 13, 2), np.uint8), dtype=capi.U8)
    ins = [capi.Tensor.from_numpy(ctx, R.frame(1, 1, 9, 13, 3), dtype=capi.U8)]
    capi.trace_begin()
    plan.run(ins, out)
    ctx.sync()
    text = str(capi.trace_end())
    assert "rgb_cbcr_kernel" in text, text


def _refused(fn, *needles):
    from shadernn_amd import capi

    with pytest.raises(capi.SnnHipError) as e:
        fn()
    assert e.value.code == capi.E_INVALID, str(e.value)
    msg = str(e.value)
    assert len(msg) > len("snnhip error -1: ") and all(s in msg for s in needles), msg


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    mk = capi.rgb_cbcr_plan
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2), "rgb_cbcr desc", "2 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 5, 2), "rgb_cbcr desc", "5 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 1), "rgb_cbcr desc", "r = 1", "decimation")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 0), "rgb_cbcr desc", "r = 0")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 5), "rgb_cbcr desc", "r = 5")
    _refused(lambda: mk(ctx, 1, 3, 4, 3, 3), "rgb_cbcr desc", "odd extent")
    _refused(lambda: mk(ctx, 1, 4, 5, 3, 3), "rgb_cbcr desc", "odd extent")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, 2), "rgb_cbcr desc", "siting")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, "left", 2), "rgb_cbcr desc", "range")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, kr=0.0), "rgb_cbcr desc", "kr")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, kb=-0.1), "rgb_cbcr desc", "kb")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, kr=0.7, kb=0.3), "rgb_cbcr desc", "kr + kb < 1")
    _refused(lambda: mk(ctx, 1, 0, 4, 3, 2), "rgb_cbcr desc", "bad dims")
    n, h, w, C, r = 1, 4, 6, 3, 3
    plan = mk(ctx, n, h, w, C, r)
    rgb = R.frame(1, n, h, w, C)
    x = capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8)
    out = capi.Tensor.from_numpy(ctx, np.full((n, 6, 9, 2), FILL, np.uint8), dtype=capi.U8)
    plan.run([x], out)  # the valid call
    for bad in ((n, 12, 18, 2), (n, 6, 9, 1), (n, 6, 9, 3), (n, 6, 10, 2), (n, 4, 6, 2), (2, 6, 9, 2)):
        _refused(lambda: plan.run([x], capi.Tensor(ctx, *bad, dtype=capi.U8)), "rgb_cbcr", "the output is")  # not [N][rH/2][rW/2][2]
    _refused(lambda: plan.run([capi.Tensor(ctx, n, h, w, 4, dtype=capi.U8)], out), "rgb_cbcr", "the input frame is")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, h + 2, w, C, dtype=capi.U8)], out), "rgb_cbcr", "the input frame is")
    _refused(lambda: plan.run([x, x], out), "rgb_cbcr", "1 input")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, h, w, C)], out), "plan_run", "dtype 0")                      # a float tensor as the frame
    _refused(lambda: plan.run([capi.Tensor(ctx, n, h, w, C, dtype=capi.U16)], out), "plan_run")                 # a 16-bit frame
    _refused(lambda: plan.run([x], capi.Tensor(ctx, n, 6, 9, 2)), "plan_run", "8-bit")                          # a float tensor as the output
    _refused(lambda: plan.run([x], capi.Tensor(ctx, n, 6, 9, 2, dtype=capi.U16)), "plan_run")                   # a 16-bit output
    R.compare(out.numpy_u8(), R.values(rgb, r))  # nothing above touched the valid result
    plan.destroy()


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, checked by snnhip_sync) is fixed at the library's first allocation: a child
    process, started the way tests/test_frame_yuv_rgb_gpu.py starts its own, runs the sweep once -- every r and C, both sitings, on every shape.
    Valid shapes only: no SNNHIP_E_GUARD may come back."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_frame_rgb_cbcr_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for r in (2, 3, 4):
            for C in (3, 4):
                T.sweep(ctx, r, C, T.R.shapes_for(r, T.tile_in(ctx, r)), ranges=["limited"])
                ctx.sync()                               # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]
