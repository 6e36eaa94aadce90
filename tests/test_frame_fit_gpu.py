"""The plane-fit plan through the C-ABI (include/snnhip.h, snnhip_plane_fit_plan_create) against the float64 reference of tests/fit_ref.py, into
0xA5-filled outputs.  The comparison rule (fit_ref.compare_all): a value equals the reference's wherever the reference's pre-rounding value is
farther than eps from a tie (1e-3 at 8 bits, 3e-3 at 10, 8e-3 at 12: 22 / 14 / 11 times the fp32-to-float64 distance of the expression), is at
most 1 off (in units of 1 << shift) on near ties, and near ties are at most 2.5 % of a sweep's values taken together, asserted on the reference
alone."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import fit_ref as R
from test_frame_chroma_gpu import DEPTHS, DEPTH_IDS, FILL, SITINGS, _capi_dtype, _download, _np_dtype, _plane, _refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
assert DEPTHS == R.DEPTHS


def tile_of(plan):
    m = re.search(r"tile=(\d+)x(\d+)", plan.describe())
    assert m, plan.describe()
    return int(m.group(1)), int(m.group(2))


def shapes_for(ctx, c, container, maxval, shift):
    """The fixed shapes plus two derived from the tile the kernel reports for a shrinking plan: a tile seam on both axes with ragged edges at 3/4,
    and N = 2 at exactly 1/2 with one pixel more than a tile each way -- all eight taps live and the input span at its largest."""
    from shadernn_amd import capi

    probe = capi.plane_fit_plan(ctx, 1, 2, 2, c, 1, 1, _capi_dtype(container), maxval, shift, "left")
    th, tw = tile_of(probe)
    probe.destroy()
    oh, ow = 2 * th - 3, 2 * tw - 5
    return R.SHAPES + [(1, -(-4 * oh // 3), -(-4 * ow // 3), oh, ow), (2, 2 * (th + 1), 2 * (tw + 1), th + 1, tw + 1)]


def run_plan(ctx, u, oh, ow, container, maxval, shift, siting):
    from shadernn_amd import capi

    n, h, w, c = u.shape
    dt = _capi_dtype(container)
    plan = capi.plane_fit_plan(ctx, n, h, w, c, oh, ow, dt, maxval, shift, siting)
    desc = plan.describe()
    assert "plane_fit_%s c=%d %dx%d->%dx%d siting=%s tile=" % ("u8" if container == "u8" else "u16", c, h, w, oh, ow, siting) in desc, desc
    assert plan.out_shape() == (n, oh, ow, c)
    assert plan.cost()[1] == (n * h * w * c + n * oh * ow * c) * u.dtype.itemsize  # the input once, the output once
    fill = np.full((n, oh, ow, c), FILL if container == "u8" else FILL * 0x101, u.dtype)
    out = capi.Tensor.from_numpy(ctx, fill, dtype=dt)
    plan.run(capi.Tensor.from_numpy(ctx, u, dtype=dt), out)
    got = _download(out, container)
    plan.destroy()
    return got


def sweep(ctx, c, container, maxval, shift, shapes, sitings=SITINGS):
    """Every shape and siting against the reference (the near-tie cap over the sweep's values together); returns the line to print."""
    items = []
    for si, siting in enumerate(sitings):
        for k, (n, h, w, oh, ow) in enumerate(shapes):
            u = _plane(n, h, w, c, maxval, shift, container, seed=100 * c + 10 * k + si + maxval)
            got = run_plan(ctx, u, oh, ow, container, maxval, shift, siting)
            items.append((got, R.fit_values(u, oh, ow, siting, shift), maxval, shift))
    frac, ndiff = R.compare_all(items)
    return "plane_fit %s maxval=%d shift=%d c=%d, %d runs: near ties %.3f %%, %d values differ" % (container, maxval, shift, c, len(items), 100 * frac, ndiff)


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("c", [1, 2])
def test_plan_matches_the_reference(ctx, c, depth):
    container, maxval, shift = depth
    print(sweep(ctx, c, container, maxval, shift, shapes_for(ctx, c, container, maxval, shift)))


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("c", [1, 2])
def test_ratio_one_is_the_input_byte_for_byte_with_the_low_bits_cleared(ctx, c, depth):
    container, maxval, shift = depth
    rng = np.random.default_rng(11)
    shapes = shapes_for(ctx, c, container, maxval, shift)
    for siting in SITINGS:
        for k, (n, _, _, h, w) in enumerate(shapes):  # every output extent of the sweep, the tile-derived ones included, as a copy
            u = _plane(n, h, w, c, maxval, shift, container, seed=60 + k)
            dirty = u | rng.integers(0, 1 << shift, size=u.shape).astype(u.dtype)
            np.testing.assert_array_equal(run_plan(ctx, dirty, h, w, container, maxval, shift, siting), u)  # no near-tie allowance


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
def test_a_constant_plane_stays_constant(ctx, depth):
    container, maxval, shift = depth
    for n, h, w, oh, ow in R.SHAPES:
        for value in (0, maxval, maxval // 3):
            k = np.full((n, h, w, 2), value << shift, _np_dtype(container))
            got = run_plan(ctx, k, oh, ow, container, maxval, shift, "left")
            np.testing.assert_array_equal(got, np.full_like(got, value << shift))


def test_low_bits_of_a_high_aligned_plane_are_ignored(ctx):
    """P010 containers carry ten bits in the high end; whatever sits in the six bits below them must not reach the result."""
    container, maxval, shift = "u16", 1023, 6
    rng = np.random.default_rng(12)
    for n, h, w, oh, ow in [(2, 13, 21, 7, 11), (1, 19, 67, 27, 100), (1, 37, 29, 19, 15)]:
        u = _plane(n, h, w, 2, maxval, shift, container, seed=70 + h)
        dirty = u | rng.integers(1, 1 << shift, size=u.shape).astype(u.dtype)
        np.testing.assert_array_equal(run_plan(ctx, dirty, oh, ow, container, maxval, shift, "left"), run_plan(ctx, u, oh, ow, container, maxval, shift, "left"))


def test_the_two_sitings_differ_except_on_an_axis_that_copies(ctx):
    u = _plane(1, 12, 33, 2, 255, 0, "u8", seed=3)
    for oh, ow in ((9, 25), (12, 50), (24, 22)):
        assert not np.array_equal(run_plan(ctx, u, oh, ow, "u8", 255, 0, "left"), run_plan(ctx, u, oh, ow, "u8", 255, 0, "centre")), (oh, ow)
    for oh in (6, 12, 17):  # the horizontal axis copies: the siting has nothing to act on
        np.testing.assert_array_equal(run_plan(ctx, u, oh, 33, "u8", 255, 0, "left"), run_plan(ctx, u, oh, 33, "u8", 255, 0, "centre"))


def test_trace_report_names_the_kernel(ctx):
    from shadernn_amd import capi

    plan = capi.plane_fit_plan(ctx, 1, 9, 13, 2, 7, 10)
    x = capi.Tensor.from_numpy(ctx, _plane(1, 9, 13, 2, 255, 0, "u8", 1), dtype=capi.U8)
    y = capi.Tensor.from_numpy(ctx, np.zeros((1, 7, 10, 2), np.uint8), dtype=capi.U8)
    capi.trace_begin()
    plan.run(x, y)
    ctx.sync()
    text = str(capi.trace_end())
    assert "plane_fit_kernel" in text, text


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    mk = capi.plane_fit_plan
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 4, 4), "plane_fit desc", "3 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 0, 4, 4), "plane_fit desc", "0 channels")
    _refused(lambda: mk(ctx, 1, 5, 4, 2, 2, 4), "plane_fit desc", "vertical", "from 5 to 2")         # below 1/2
    _refused(lambda: mk(ctx, 1, 4, 5, 2, 4, 2), "plane_fit desc", "horizontal", "from 5 to 2")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 17, 4), "plane_fit desc", "vertical", "from 4 to 17")       # above 4
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 4, 17), "plane_fit desc", "horizontal", "from 4 to 17")
    _refused(lambda: mk(ctx, 1, 0, 4, 2, 4, 4), "plane_fit desc", "bad dims")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 4, 0), "plane_fit desc", "bad dims")
    _refused(lambda: mk(ctx, 0, 4, 4, 2, 4, 4), "plane_fit desc", "bad dims")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 6, 6, capi.F32), "plane_fit desc", "dtype")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 6, 6, capi.F16), "plane_fit desc", "dtype")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 6, 6, capi.U8, 255, 0, 2), "plane_fit desc", "siting")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 6, 6, capi.U8, 256, 0), "plane_fit desc", "maxval 256")      # does not fit a byte
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 6, 6, capi.U8, 127, 1), "plane_fit desc", "shift 1")          # 8-bit planes have no shift
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 6, 6, capi.U16, 1023, 7), "plane_fit desc", "does not fit")    # 1023 << 7 needs 17 bits
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 6, 6, capi.U16, 1023, 16), "plane_fit desc", "shift 16")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 6, 6, capi.U16, 0, 0), "plane_fit desc", "maxval 0")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 6, 6, capi.U16, 65535, 0), "plane_fit desc", "4095")
    n, h, w, c, oh, ow = 1, 4, 6, 2, 6, 5
    plan = mk(ctx, n, h, w, c, oh, ow)
    u = _plane(n, h, w, c, 255, 0, "u8", 1)
    x = capi.Tensor.from_numpy(ctx, u, dtype=capi.U8)
    out = capi.Tensor.from_numpy(ctx, np.full((n, oh, ow, c), FILL, np.uint8), dtype=capi.U8)
    plan.run(x, out)  # the valid call
    for bad in ((n, oh + 1, ow, c), (n, oh, ow + 1, c), (n, h, w, c), (n, oh, ow, 1), (2, oh, ow, c)):
        _refused(lambda: plan.run(x, capi.Tensor(ctx, *bad, dtype=capi.U8)), "plane_fit", "the output is")
    _refused(lambda: plan.run(capi.Tensor(ctx, n, h + 1, w, c, dtype=capi.U8), out), "plane_fit", "the input plane is")
    _refused(lambda: plan.run(capi.Tensor(ctx, n, h, w, c), out), "plan_run: input 0 has dtype 0")               # a float tensor as the input
    _refused(lambda: plan.run(capi.Tensor(ctx, n, h, w, c, dtype=capi.U16), out), "plan_run", "16-bit")         # a 16-bit plane into an 8-bit plan
    _refused(lambda: plan.run(x, capi.Tensor(ctx, n, oh, ow, c)), "plan_run", "8-bit")                           # a float tensor as the output
    _refused(lambda: plan.run(x, capi.Tensor(ctx, n, oh, ow, c, dtype=capi.U16)), "plan_run")                   # a 16-bit output
    wide = mk(ctx, n, h, w, c, oh, ow, capi.U16, 1023, 6)
    _refused(lambda: wide.run(x, capi.Tensor(ctx, n, oh, ow, c, dtype=capi.U16)), "plan_run", "8-bit")           # an 8-bit plane into a 16-bit plan
    R.compare(out.numpy_u8(), R.fit_values(u, oh, ow, "left"), 255, 0)  # nothing above touched the valid result


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, checked by snnhip_sync) is fixed at the library's first allocation: a child
    process, started the way tests/test_frame_chroma_gpu.py starts its own, runs the sweep once -- every C, depth and siting on the three smallest
    shapes and the two tile-derived ones.  Valid shapes only: no SNNHIP_E_GUARD may come back."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_frame_fit_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for c in (1, 2):
            for container, maxval, shift in T.DEPTHS:
                shapes = T.shapes_for(ctx, c, container, maxval, shift)
                T.sweep(ctx, c, container, maxval, shift, shapes[:3] + shapes[-2:])
                ctx.sync()                               # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]


def test_rows_dealt_to_lane_sets_meet_at_the_chunk_boundaries(ctx):
    """Pass 1 deals a tile's rows to lane sets when the tile's column span has fewer strips than the block has lanes: sets >= 2, chunks of
    ceil(rows / sets).  One row less and one row more than a tile of an enlarging plan (tests/test_frame_fit.py::lane_set_frames, whose near ties are
    counted there): chunks of one row with sets to spare, a short last chunk, a second tile of a single row."""
    from shadernn_amd import capi
    from test_frame_fit import lane_set_frames

    probe = capi.plane_fit_plan(ctx, 1, 11, 20, 1, 12, 30, capi.U8, 255, 0, "left")  # enlarging: the four-tap instance
    th, _ = tile_of(probe)
    probe.destroy()
    items = [(run_plan(ctx, u, oh, ow, "u8", 255, 0, "left"), R.fit_values(u, oh, ow, "left"), 255, 0) for u, oh, ow in lane_set_frames(th)]
    frac, ndiff = R.compare_all(items)
    print("plane_fit lane sets, tile of %d rows, %d runs: near ties %.3f %%, %d values differ" % (th, len(items), 100 * frac, ndiff))
