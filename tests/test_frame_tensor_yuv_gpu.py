"""The output-tensor -> video-frame plans through the C-ABI (include/snnhip.h, snnhip_tensor_yuv_plan_create / _planar_plan_create, run with
snnhip_plan_run_io) against the float64 reference of tests/tensor_yuv_ref.py, into 0xA5-filled planes.  Every element of both outputs is compared:
equal to the reference off the near ties (half-width tensor_yuv_ref.EPS, the family's), at most one code apart on them, and the near ties are at most
MAX_TIE_FRACTION of a sweep's values (asserted on the reference alone; tests/test_frame_tensor_yuv.py measures both on the CPU)."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import planar_ref
import rgb_cbcr_ref
import tensor_yuv_ref as R
from test_frame_yuv_rgb_gpu import _capi_dtype, _download, _refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FILL = 0xA5


def run_plan(ctx, x, container="u8", maxval=255, shift=0, siting="left", rng="limited", kr=R.BT601[0], kb=R.BT601[1], scale=(1, 1, 1), offset=(0, 0, 0), planar=False):
    """x: float32 or float16 [N][H][W][C].  Returns (luma [N][H][W][1], chroma as the plan writes it: [N][H/2][W/2][2] or, planar, [2N][H/2][W/2][1])."""
    from shadernn_amd import capi

    n, h, w, c = x.shape
    half = x.dtype == np.float16
    dt = _capi_dtype(container)
    npdt = planar_ref.np_dtype(container)
    plan = capi.tensor_yuv_plan(ctx, n, h, w, c, capi.F16 if half else capi.F32, dt, maxval, shift, siting, rng, kr, kb, scale, offset, planar)
    desc = plan.describe()
    name = "tensor_yuv_planar" if planar else "tensor_yuv"
    assert desc.startswith("%s_%s c=%d %s siting=%s range=%s %dx%d tile=%d " % (name, container, c, "f16" if half else "f32", siting, rng, h, w, R.TILE[(container, planar)])), desc
    assert desc.endswith("kernel=%s_kernel" % name), desc
    assert plan.out_shape() == (n, h, w, 1)
    assert plan.cost()[1] == x.size * x.dtype.itemsize + n * h * w * 3 // 2 * np.dtype(npdt).itemsize  # the input once, both outputs once
    fill = FILL if container == "u8" else FILL * 0x101
    cshape = (2 * n, h // 2, w // 2, 1) if planar else (n, h // 2, w // 2, 2)
    src = capi.Tensor.from_numpy(ctx, x.astype(np.float32), dtype=capi.F16 if half else capi.F32)  # (a float16 array widens and narrows back exactly)
    luma = capi.Tensor.from_numpy(ctx, np.full((n, h, w, 1), fill, npdt), dtype=dt)
    chroma = capi.Tensor.from_numpy(ctx, np.full(cshape, fill, npdt), dtype=dt)
    plan.run_io([src], [luma, chroma])
    got = _download(luma, container), _download(chroma, container)
    plan.destroy()
    for t in (src, luma, chroma):
        t.free()
    return got


def run_case(ctx, case, C, half, container, maxval, shift, planar=False):
    (n, h, w), siting, rng, (kr, kb), scale, offset, seed = case
    x = R.case_tensor(case, C, half, maxval)
    y, c = run_plan(ctx, x, container, maxval, shift, siting, rng, kr, kb, scale, offset, planar)
    return x, y, (planar_ref.interleave(c) if planar else c)


def sweep(ctx, C, half, container, maxval, shift, planar=False):
    """Every case of the sweep against the reference, every element of both planes; returns the line to print."""
    items, runs = [], 0
    for case in R.sweep_cases(C, half, container, maxval, shift, planar):
        x, y, c = run_case(ctx, case, C, half, container, maxval, shift, planar)
        yv, cv = R.case_values(case, x, maxval)
        items += [(y, yv, maxval, shift), (c, cv, maxval, shift)]
        runs += 1
    frac, ndiff = R.compare_all(items)
    return "tensor_yuv%s %s maxval=%d shift=%d c=%d %s, %d runs: near ties %.3f %%, %d values differ" % (" planar" if planar else "", container, maxval, shift, C,
                                                                                                        "f16" if half else "f32", runs, 100 * frac, ndiff)


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("c", [3, 4])
def test_plan_matches_the_reference(ctx, c, half, depth):
    container, maxval, shift = depth
    print(sweep(ctx, c, half, container, maxval, shift))


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("c", [3, 4])
def test_planar_plan_matches_the_reference(ctx, c, half, depth):
    container, maxval, shift = depth
    print(sweep(ctx, c, half, container, maxval, shift, planar=True))


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_planar_and_interleaved_chroma_give_the_same_frame(ctx, depth):
    """the same tensor through both plans (the planar sweep's shapes: the two tiles differ): 0 values differ"""
    container, maxval, shift = depth
    for c, half in ((3, False), (4, True)):
        for case in R.sweep_cases(c, half, container, maxval, shift, True):
            _, y0, c0 = run_case(ctx, case, c, half, container, maxval, shift, planar=False)
            _, y1, c1 = run_case(ctx, case, c, half, container, maxval, shift, planar=True)
            assert int((y0 != y1).sum()) + int((c0 != c1).sum()) == 0, case[:3]


def test_the_reported_tile_is_the_references(ctx):
    from shadernn_amd import capi

    for (container, planar), tile in R.TILE.items():
        plan = capi.tensor_yuv_plan(ctx, 1, 2, 2, 3, capi.F32, _capi_dtype(container), 255 if container == "u8" else 1023, planar=planar)
        assert int(re.search(r"tile=(\d+) ", plan.describe()).group(1)) == tile, plan.describe()
        plan.destroy()
    plan = capi.tensor_yuv_plan(ctx, 1, 720, 1280, 3, capi.F16)
    assert plan.describe().startswith("tensor_yuv_u8 c=3 f16 siting=left range=limited 720x1280 tile=2048 "), plan.describe()
    assert plan.describe().endswith("kernel=tensor_yuv_kernel")
    plan.destroy()


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_grey_gives_neutral_chroma_and_a_constant_gives_constant_planes(ctx, depth):
    container, maxval, shift = depth
    k = (maxval + 1) // 256
    g = np.random.default_rng(5)
    for n, h, w in [(1, 2, 2), (1, 6, 18), (2, 4, 70)]:
        grey = np.repeat(g.uniform(-0.1 * maxval, 1.1 * maxval, size=(n, h, w, 1)), 3, axis=3).astype(np.float32)
        const = np.broadcast_to(g.uniform(0, maxval, size=(1, 1, 1, 3)), (n, h, w, 3)).astype(np.float32)
        for siting in R.SITINGS:
            for rng in R.RANGE_NAMES:
                for planar in (False, True):
                    _, c = run_plan(ctx, grey, container, maxval, shift, siting, rng, planar=planar)
                    assert (c == ((128 * k) << shift)).all(), (n, h, w, siting, rng, planar)
                    y, c = run_plan(ctx, const, container, maxval, shift, siting, rng, planar=planar)
                    c = planar_ref.interleave(c) if planar else c
                    assert (y == y.flat[0]).all() and (c[..., 0] == c[0, 0, 0, 0]).all() and (c[..., 1] == c[0, 0, 0, 1]).all()


def test_integer_luma_is_the_rgb_luma_plans_byte_for_byte(ctx):
    """8 bits, full range, an integer-valued tensor: ys = 1 and Yoff = 0, so the luma plane is rgb_luma's of the same pixels, the one device function"""
    from shadernn_amd import capi

    for (n, h, w), matrix in (((1, 6, 18), R.BT601), ((2, 4, 70), R.BT709), ((1, 2, 1026), R.BT601)):
        rgb = rgb_cbcr_ref.frame(40 + w, n, h, w, 3, primaries=True)
        lp = capi.rgb_luma_plan(ctx, n, h, w, 3, *matrix)
        out = capi.Tensor.from_numpy(ctx, np.zeros((n, h, w, 1), np.uint8), dtype=capi.U8)
        lp.run(capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8), out)
        want = out.numpy_u8()
        lp.destroy()
        for half in (False, True):
            y, _ = run_plan(ctx, rgb.astype(np.float16 if half else np.float32), rng="full", kr=matrix[0], kb=matrix[1])
            assert int((y != want).sum()) == 0, (n, h, w, half)


def test_replicated_tensor_centre_against_the_rgb_cbcr_plan(ctx):
    """A 2 x 2-replicated integer tensor, centred: the decimation returns each block's own pixel, so the chroma is rgb_cbcr's at r = 2, centre (the
    identity resampling) of the unreplicated frame -- another kernel, another summation: equal off the near ties of the shared float64 value."""
    from shadernn_amd import capi

    items = []
    for k, (n, h, w) in enumerate([(1, 3, 9), (2, 5, 35), (1, 2, 515)]):
        for rng in R.RANGE_NAMES:
            rgb = rgb_cbcr_ref.frame(60 + k, n, h, w, 3)
            plan = capi.rgb_cbcr_plan(ctx, n, h, w, 3, 2, "centre", rng)
            out = capi.Tensor.from_numpy(ctx, np.zeros((n, h, w, 2), np.uint8), dtype=capi.U8)
            plan.run(capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8), out)
            theirs = out.numpy_u8()
            plan.destroy()
            x = np.repeat(np.repeat(rgb, 2, axis=1), 2, axis=2).astype(np.float32)
            _, c = run_plan(ctx, x, siting="centre", rng=rng)
            want = rgb_cbcr_ref.values(rgb, 2, "centre", rng)
            assert np.abs(R.values(x, siting="centre", rng=rng)[1] - want).max() < 1e-9  # the two references state the same value
            tie = R.near_tie(want, R.EPS[255])
            assert not ((c != theirs) & ~tie).any(), (n, h, w, rng)
            items.append((c, want, 255, 0))
    frac, ndiff = R.compare_all(items)
    print("replicated tensor against rgb_cbcr r=2 centre: near ties %.3f %%, %d values differ from the reference" % (100 * frac, ndiff))


def test_the_sitings_differ_as_the_filter_predicts(ctx):
    """A horizontal ramp in B alone, constant down the columns, full range: dB is linear in the column, so centred sample I reads position 2I + 1/2 and
    the left-sited one position 2I -- half a column's step apart -- except I = 0, where the clamp makes the left one read (3 d0 + d1) / 4.  On a
    2 x 2-replicated tensor both sitings give the same plane except in column 0."""
    n, h, w = 1, 4, 40
    x = np.zeros((n, h, w, 3), np.float32)
    x[..., 2] = 4.0 * np.arange(w, dtype=np.float32)  # B = 4 X: 0 .. 156
    kb = R.BT601[1]
    coff, cbs = float(R.coefficients(255, "full")[2]), float(R.coefficients(255, "full")[3])
    step = cbs * (1.0 - float(np.float32(kb))) * 4.0  # Cb per column
    values = {}
    for siting in R.SITINGS:
        _, c = run_plan(ctx, x, rng="full", siting=siting)
        values[siting] = R.values(x, siting=siting, rng="full")[1]
        R.compare(c, values[siting], 255, 0)
        assert (c == c[:, :1]).all()  # every chroma row alike
    d = values["centre"][0, 0, :, 0] - values["left"][0, 0, :, 0]
    assert np.abs(d[1:] - 0.5 * step).max() < 1e-4 and abs(d[0] - 0.25 * step) < 1e-4, d[:4]
    assert abs(values["centre"][0, 0, 3, 0] - (coff + step * 6.5)) < 1e-3
    rep = np.repeat(np.repeat(R.tensor(1, 3, 20, 3, False, 255, (1, 1, 1), (0, 0, 0), 9), 2, axis=1), 2, axis=2)
    a = run_plan(ctx, rep, siting="centre")[1].astype(np.int64)
    b = run_plan(ctx, rep, siting="left")[1].astype(np.int64)
    va, vb = R.values(rep, siting="centre")[1], R.values(rep, siting="left")[1]
    assert np.abs(va[:, :, 0] - vb[:, :, 0]).max() < 1e-9  # column 0: (d0 + d0) / 2 = (d0 + 2 d0 + d0) / 4
    assert np.abs(a - b)[:, :, 0].max() <= 1 and (a != b)[:, :, 1:].any()  # ... and the planes differ further right, where the left one reads column 2I - 1


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_saturated_primaries(ctx, depth):
    """Every channel 0 or maxval in 2 x 2 blocks, centred: each chroma sample is its block's own colour.  Limited range keeps every code inside
    [16k, 240k]; full range puts pure blue's Cb and pure red's Cr on maxval + 1/2, a tie that the clamp resolves to maxval either way."""
    container, maxval, shift = depth
    k = (maxval + 1) // 256
    x = R.saturated(2, 6, 22, 3, maxval, seed=3)
    for rng in R.RANGE_NAMES:
        for planar in (False, True):
            y, c = run_plan(ctx, x, container, maxval, shift, "centre", rng, planar=planar)
            c = planar_ref.interleave(c) if planar else c
            yv, cv = R.values(x, siting="centre", rng=rng, maxval=maxval)
            R.compare(y, yv, maxval, shift)  # off the near ties equal, on them (yellow's Cb = 1/2 in full range is one) at most one code apart
            R.compare(c, cv, maxval, shift)
            top = cv > maxval + 0.25  # the tie above the clamp: maxval from either side
            assert (c[top] >> shift == maxval).all(), rng
            if rng == "limited":
                assert (y >> shift).min() >= 16 * k and (y >> shift).max() <= 235 * k and (c >> shift).min() >= 16 * k and (c >> shift).max() <= 240 * k


def test_trace_report_names_the_kernel(ctx):
    from shadernn_amd import capi

    for planar, name in ((False, "tensor_yuv_kernel"), (True, "tensor_yuv_planar_kernel")):
        plan = capi.tensor_yuv_plan(ctx, 1, 6, 8, 3, planar=planar)
        src = capi.Tensor.from_numpy(ctx, R.tensor(1, 6, 8, 3, False, 255, (1, 1, 1), (0, 0, 0), 1))
        y = capi.Tensor(ctx, 1, 6, 8, 1, dtype=capi.U8)
        c = capi.Tensor(ctx, 2, 3, 4, 1, dtype=capi.U8) if planar else capi.Tensor(ctx, 1, 3, 4, 2, dtype=capi.U8)
        capi.trace_begin()
        plan.run_io([src], [y, c])
        ctx.sync()
        text = str(capi.trace_end())
        assert name in text, text
        plan.destroy()


def test_a_recorded_graph_replays_bit_identically(ctx):
    from shadernn_amd import capi

    n, h, w = 2, 6, 70
    plan = capi.tensor_yuv_plan(ctx, n, h, w, 3, capi.F16)
    x = R.tensor(n, h, w, 3, True, 255, (1, 1, 1), (0, 0, 0), 3)
    src = capi.Tensor.from_numpy(ctx, x.astype(np.float32), dtype=capi.F16)
    y = capi.Tensor.from_numpy(ctx, np.full((n, h, w, 1), FILL, np.uint8), dtype=capi.U8)
    c = capi.Tensor.from_numpy(ctx, np.full((n, h // 2, w // 2, 2), FILL, np.uint8), dtype=capi.U8)
    with capi.Graph.capture(ctx) as g:
        plan.run_io([src], [y, c])
    assert g.num_nodes() == 1
    want = run_plan(ctx, x)
    for _ in range(2):  # replayed twice into freshly filled planes
        y.upload_u8(np.full((n, h, w, 1), FILL, np.uint8))
        c.upload_u8(np.full((n, h // 2, w // 2, 2), FILL, np.uint8))
        g.launch()
        ctx.sync()
        assert np.array_equal(y.numpy_u8(), want[0]) and np.array_equal(c.numpy_u8(), want[1])
    g.destroy()
    plan.destroy()


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    mk = capi.tensor_yuv_plan
    for planar in (False, True):
        _refused(lambda: mk(ctx, 1, 4, 4, 2, planar=planar), "tensor_yuv desc", "2 channels")
        _refused(lambda: mk(ctx, 1, 4, 4, 5, planar=planar), "tensor_yuv desc", "5 channels")
        _refused(lambda: mk(ctx, 1, 5, 4, 3, planar=planar), "tensor_yuv desc", "5x4", "even")
        _refused(lambda: mk(ctx, 1, 4, 7, 3, planar=planar), "tensor_yuv desc", "4x7", "even")
        _refused(lambda: mk(ctx, 0, 4, 4, 3, planar=planar), "tensor_yuv desc", "bad dims")
        _refused(lambda: mk(ctx, 1, 0, 4, 3, planar=planar), "tensor_yuv desc", "bad dims")
        _refused(lambda: mk(ctx, 1, 4, -2, 3, planar=planar), "tensor_yuv desc", "bad dims")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.U8, planar=planar), "tensor_yuv desc", "in_dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.U16, planar=planar), "tensor_yuv desc", "in_dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.F32, capi.F32, planar=planar), "tensor_yuv desc", "dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.F32, capi.F16, planar=planar), "tensor_yuv desc", "dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.F32, capi.U8, 1023, 0, planar=planar), "tensor_yuv desc", "does not fit")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.F32, capi.U16, 65535, 0, planar=planar), "tensor_yuv desc", "4095")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.F32, capi.U16, 1023, 7, planar=planar), "tensor_yuv desc", "does not fit")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.F32, capi.U8, 255, 1, planar=planar), "tensor_yuv desc", "shift 1")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.F32, capi.U8, 127, 0, planar=planar), "tensor_yuv desc", "multiple of 256")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, capi.F32, capi.U16, 1000, 0, planar=planar), "tensor_yuv desc", "multiple of 256")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, siting=2, planar=planar), "tensor_yuv desc", "siting")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, range=2, planar=planar), "tensor_yuv desc", "range")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, kr=0.0, planar=planar), "tensor_yuv desc", "kr")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, kb=-0.1, planar=planar), "tensor_yuv desc", "kb")
        _refused(lambda: mk(ctx, 1, 4, 4, 3, kr=0.7, kb=0.3, planar=planar), "tensor_yuv desc", "kr + kb < 1")
    n, h, w, C = 1, 4, 6, 3
    x = R.tensor(n, h, w, C, False, 255, (1, 1, 1), (0, 0, 0), 1)
    plan = mk(ctx, n, h, w, C)
    src = capi.Tensor.from_numpy(ctx, x)
    y = capi.Tensor.from_numpy(ctx, np.full((n, h, w, 1), FILL, np.uint8), dtype=capi.U8)
    c = capi.Tensor.from_numpy(ctx, np.full((n, h // 2, w // 2, 2), FILL, np.uint8), dtype=capi.U8)
    plan.run_io([src], [y, c])  # the valid call
    u8 = lambda *s: capi.Tensor(ctx, *s, dtype=capi.U8)  # noqa: E731
    _refused(lambda: plan.run(src, y), "tensor_yuv", "snnhip_plan_run_io")          # snnhip_plan_run
    _refused(lambda: plan.run([src], y), "tensor_yuv", "snnhip_plan_run_io")        # snnhip_plan_run_n
    _refused(lambda: plan.run([src, src], y), "tensor_yuv", "snnhip_plan_run_io")
    _refused(lambda: plan.run_io([src, src], [y, c]), "tensor_yuv", "1 input")
    _refused(lambda: plan.run_io([src], [y]), "tensor_yuv", "2 outputs")
    _refused(lambda: plan.run_io([src], [y, c, c]), "tensor_yuv", "2 outputs")
    _refused(lambda: plan.run_io([capi.Tensor(ctx, n, h, w, C, dtype=capi.F16)], [y, c]), "tensor_yuv", "the input must have dtype")
    _refused(lambda: plan.run_io([y], [y, c]), "tensor_yuv", "the input must have dtype")                                   # a byte plane as the input
    _refused(lambda: plan.run_io([src], [capi.Tensor(ctx, n, h, w, 1, dtype=capi.U16), c]), "tensor_yuv", "both outputs must have dtype")
    _refused(lambda: plan.run_io([src], [y, capi.Tensor(ctx, n, h // 2, w // 2, 2)]), "tensor_yuv", "both outputs must have dtype")  # a float tensor as the chroma
    for bad in ((n, h, w, 4), (n, h + 2, w, C), (n, h, w - 2, C), (2, h, w, C)):
        _refused(lambda: plan.run_io([capi.Tensor(ctx, *bad)], [y, c]), "tensor_yuv", "the input is")
    _refused(lambda: plan.run_io([src], [u8(n, h, w + 2, 1), c]), "tensor_yuv", "the luma plane is")
    _refused(lambda: plan.run_io([src], [u8(n, h // 2, w // 2, 1), c]), "tensor_yuv", "the luma plane is")
    _refused(lambda: plan.run_io([src], [y, u8(n, h, w, 2)]), "tensor_yuv", "the chroma plane is")                           # chroma at the luma size
    _refused(lambda: plan.run_io([src], [y, u8(2 * n, h // 2, w // 2, 1)]), "tensor_yuv", "the chroma plane is")             # planar planes out of a CbCr plan
    planar = mk(ctx, n, h, w, C, planar=True)
    _refused(lambda: planar.run_io([src], [y, c]), "tensor_yuv_planar", "the chroma tensor is", "[2N][H/2][W/2][1]")         # a CbCr plane out of a planar plan
    _refused(lambda: planar.run(src, y), "tensor_yuv_planar", "snnhip_plan_run_io")
    other = capi.rgb_luma_plan(ctx, n, h, w, 3)
    _refused(lambda: other.run_io([u8(n, h, w, 3)], [y, c]), "plan_run_io", "tensor_yuv", "rgb_luma")                         # snnhip_plan_run_io on another plan
    _refused(lambda: other.run_io([u8(n, h, w, 3)], [y]), "plan_run_io", "tensor_yuv")
    yv, cv = R.values(x)
    R.compare(y.numpy_u8(), yv, 255, 0)  # nothing above touched the valid result
    R.compare(c.numpy_u8(), cv, 255, 0)


def test_the_plans_are_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, checked by snnhip_sync) is fixed at the library's first allocation: a fresh child
    process runs one sweep of every layout and container, the ragged shapes included.  Valid shapes only: no SNNHIP_E_GUARD may come back."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_frame_tensor_yuv_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for planar in (False, True):
            for k, (container, maxval, shift) in enumerate(T.R.DEPTHS):
                T.sweep(ctx, 3 + k % 2, bool((k + planar) % 2), container, maxval, shift, planar)
                ctx.sync()                           # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]
