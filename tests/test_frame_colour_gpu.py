"""Colour frames through the C-ABI: the luma plan and the chroma-merge plan (include/snnhip.h, snnhip_rgb_luma_plan_create /
snnhip_ycc_merge_plan_create) against the float64 reference of tests/colour_ref.py.  The comparison rule (colour_ref.compare): bytes equal the
reference's wherever its pre-rounding value is no near tie (|v - floor(v) - 0.5| < 1e-3, about 20 times the fp32-vs-float64 distance of the
expression), differ by at most 1 on near ties, and near ties are at most 1 % of the values compared.  Outputs are pre-filled with 0xA5."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import colour_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 2, 3), (2, 5, 7), (1, 37, 29), (2, 19, 67)]  # (N, H, W); 5x7 RGB: pitch 45 at r = 3, 42 at r = 2 -- unaligned rows
FILL = 0xA5


def _frame(n, h, w, c, seed):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    k = min(4, u.size)
    u.reshape(-1)[:k] = (0, 255, 128, 1)[:k]
    return u


def _filled(ctx, n, h, w, c):
    from shadernn_amd import capi

    return capi.Tensor.from_numpy(ctx, np.full((n, h, w, c), FILL, np.uint8), dtype=capi.U8)


def tile_of(plan):
    m = re.search(r"tile=(\d+)x(\d+)", plan.describe())
    assert m, plan.describe()
    return int(m.group(1)), int(m.group(2))


def merge_shapes(ctx, r, c):
    """The fixed shapes plus two derived from the kernel's own tile: a tile seam with a batch boundary inside a block row, and exactly 2 x 2 tiles."""
    from shadernn_amd import capi

    probe = capi.ycc_merge_plan(ctx, 1, 1, 1, c, r)
    th, tw = tile_of(probe)
    probe.destroy()
    return SHAPES + [(2, th + 1, tw + 1), (1, 2 * th, 2 * tw)]


def run_merge(ctx, n, h, w, c, r, coeff, seed, rgb=None):
    from shadernn_amd import capi

    rgb = _frame(n, h, w, c, seed) if rgb is None else rgb
    yhi = _frame(n, r * h, r * w, 1, seed + 1000)
    plan = capi.ycc_merge_plan(ctx, n, h, w, c, r, *coeff)
    desc = plan.describe()
    assert "ycc_merge_u8 r=%d c=%d tile=" % (r, c) in desc, desc
    assert plan.out_shape() == (n, r * h, r * w, c)
    flops, nbytes = plan.cost()
    assert nbytes == n * r * h * r * w * c + n * r * h * r * w + n * h * w * c
    out = _filled(ctx, n, r * h, r * w, c)
    plan.run([capi.Tensor.from_numpy(ctx, yhi, dtype=capi.U8), capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8)], out)
    got = out.numpy_u8()
    plan.destroy()
    return rgb, yhi, got


def sweep_merge(ctx, r, c, shapes, coeff=R.BT601):
    """Every shape against the reference (the near-tie bound over the sweep's shapes together); returns the line to print."""
    pairs = []
    for k, (n, h, w) in enumerate(shapes):
        rgb, yhi, got = run_merge(ctx, n, h, w, c, r, coeff, seed=100 * r + 10 * c + k)
        pairs.append((got[..., :3], R.merge_values(yhi, rgb, r, *coeff)))
        if c == 4:  # the alpha plane: the low-resolution pixel's, exactly
            np.testing.assert_array_equal(got[..., 3], R.merge(yhi, rgb, r, *coeff)[..., 3])
    frac, ndiff = R.compare_all(pairs)
    return "merge r=%d c=%d, %d shapes: near ties %.3f %%, %d bytes differ" % (r, c, len(shapes), 100 * frac, ndiff)


def sweep_luma(ctx, c, shapes, coeff=R.BT601):
    from shadernn_amd import capi

    pairs = []
    for k, (n, h, w) in enumerate(shapes):
        rgb = _frame(n, h, w, c, seed=10 * c + k)
        plan = capi.rgb_luma_plan(ctx, n, h, w, c, *coeff)
        assert "rgb_luma_u8 c=%d" % c in plan.describe(), plan.describe()
        assert plan.out_shape() == (n, h, w, 1) and plan.cost()[1] == n * h * w * (c + 1)
        out = _filled(ctx, n, h, w, 1)
        plan.run(capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8), out)
        pairs.append((out.numpy_u8(), R.luma_values(rgb, *coeff)))
        plan.destroy()
    frac, ndiff = R.compare_all(pairs)
    return "luma c=%d, %d shapes: near ties %.3f %%, %d bytes differ" % (c, len(shapes), 100 * frac, ndiff)


@pytest.mark.parametrize("coeff", [R.BT601, R.BT709], ids=["bt601", "bt709"])
@pytest.mark.parametrize("c", [3, 4])
def test_luma_plan_matches_the_reference(ctx, c, coeff):
    from shadernn_amd import capi

    print(sweep_luma(ctx, c, SHAPES, coeff))


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_merge_plan_matches_the_reference(ctx, r, c):
    print(sweep_merge(ctx, r, c, merge_shapes(ctx, r, c)))


def test_merge_plan_bt709(ctx):
    print(sweep_merge(ctx, 2, 3, [(2, 5, 7), (1, 37, 29)], coeff=R.BT709))


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_grey_input_returns_yhi_byte_for_byte(ctx, r, c):
    for k, (n, h, w) in enumerate(merge_shapes(ctx, r, c)):
        g = _frame(n, h, w, 1, seed=7 + k)
        rgb = np.repeat(g, 3, axis=-1)
        if c == 4:
            rgb = np.concatenate([rgb, 255 - g], axis=-1)
        _, yhi, got = run_merge(ctx, n, h, w, c, r, R.BT601, seed=50 + k, rgb=rgb)
        np.testing.assert_array_equal(got[..., :3], np.repeat(yhi, 3, axis=-1))  # no near-tie allowance
        if c == 4:
            np.testing.assert_array_equal(got[..., 3:], np.repeat(np.repeat(255 - g, r, axis=1), r, axis=2))


def test_trace_report_names_both_kernels(ctx):
    from shadernn_amd import capi

    n, h, w, c, r = 1, 9, 13, 3, 2
    luma, merge = capi.rgb_luma_plan(ctx, n, h, w, c), capi.ycc_merge_plan(ctx, n, h, w, c, r)
    x = capi.Tensor.from_numpy(ctx, _frame(n, h, w, c, 1), dtype=capi.U8)
    y = _filled(ctx, n, h, w, 1)
    yhi = capi.Tensor.from_numpy(ctx, _frame(n, r * h, r * w, 1, 2), dtype=capi.U8)
    out = _filled(ctx, n, r * h, r * w, c)
    capi.trace_begin()
    luma.run(x, y)
    merge.run([yhi, x], out)
    ctx.sync()
    rep = capi.trace_end()
    text = str(rep)
    assert "rgb_luma_u8_kernel" in text and "ycc_merge_u8_kernel" in text, text


def _refused(fn, *needles):
    from shadernn_amd import capi

    with pytest.raises(capi.SnnHipError) as e:
        fn()
    assert e.value.code == capi.E_INVALID, str(e.value)
    msg = str(e.value)
    assert len(msg) > len("snnhip error -1: ") and all(s in msg for s in needles), msg


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    _refused(lambda: capi.rgb_luma_plan(ctx, 1, 4, 4, 2), "rgb_luma desc", "2 channels")
    _refused(lambda: capi.ycc_merge_plan(ctx, 1, 4, 4, 2, 2), "ycc_merge desc", "2 channels")
    _refused(lambda: capi.ycc_merge_plan(ctx, 1, 4, 4, 3, 5), "ycc_merge desc", "r = 5")
    _refused(lambda: capi.ycc_merge_plan(ctx, 1, 4, 4, 3, 0), "ycc_merge desc", "r = 0")
    _refused(lambda: capi.rgb_luma_plan(ctx, 1, 4, 4, 3, 0.6, 0.4), "kr", "kb")
    _refused(lambda: capi.ycc_merge_plan(ctx, 1, 4, 4, 3, 2, 0.7, 0.5), "kr", "kb")
    _refused(lambda: capi.ycc_merge_plan(ctx, 1, 4, 4, 3, 2, 0.0, 0.1), "kr", "kb")
    n, h, w, c, r = 1, 4, 6, 3, 2
    plan = capi.ycc_merge_plan(ctx, n, h, w, c, r)
    lo = capi.Tensor.from_numpy(ctx, _frame(n, h, w, c, 1), dtype=capi.U8)
    yhi = capi.Tensor.from_numpy(ctx, _frame(n, r * h, r * w, 1, 2), dtype=capi.U8)
    out = _filled(ctx, n, r * h, r * w, c)
    plan.run([yhi, lo], out)  # the valid call
    for bad in ((n, 3 * h, 3 * w, 1), (n, r * h, r * w + 1, 1), (n, r * h, 3 * w, 1), (n, h, w, 1)):  # Yhi of the wrong extent
        _refused(lambda: plan.run([capi.Tensor(ctx, *bad, dtype=capi.U8), lo], out), "ycc_merge", "Yhi")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, r * h, r * w, 1), lo], out), "plan_run: input 0 has dtype 0")      # a float tensor as Yhi
    _refused(lambda: plan.run([yhi, capi.Tensor(ctx, n, h, w, c)], out), "plan_run: input 1 has dtype 0")            # ... as the frame
    _refused(lambda: plan.run([yhi, lo], capi.Tensor(ctx, n, r * h, r * w, c)), "plan_run", "8-bit")                # ... as the output
    _refused(lambda: plan.run([yhi], out), "ycc_merge", "2 inputs")
    luma = capi.rgb_luma_plan(ctx, n, h, w, c)
    _refused(lambda: luma.run(capi.Tensor(ctx, n, h, w, c), _filled(ctx, n, h, w, 1)), "plan_run: input 0 has dtype 0")
    R.compare(out.numpy_u8(), R.merge_values(yhi.numpy_u8(), lo.numpy_u8(), r))  # nothing above touched the valid result


def test_both_plans_are_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, checked by snnhip_sync) is fixed at the library's first allocation: a child process,
    started the way tests/test_guard_gpu.py starts its own, re-runs the merge sweep's three smallest shapes and the two tile-derived ones, and the
    luma plan on the same shapes.  Valid shapes only: no SNNHIP_E_GUARD may come back."""
    code = """
        import numpy as np
        import shadernn_amd as snn
        from shadernn_amd import capi
        import colour_ref as R
        import test_frame_colour_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for r in (1, 2, 3, 4):
            for c in (3, 4):
                shapes = T.merge_shapes(ctx, r, c)
                T.sweep_merge(ctx, r, c, shapes[:3] + shapes[-2:])
                ctx.sync()                                   # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write
        for c in (3, 4):
            T.sweep_luma(ctx, c, T.SHAPES[:3] + [(2, 9, 65)])
            ctx.sync()
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]
