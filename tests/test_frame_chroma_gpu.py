"""The chroma-plane upsampler through the C-ABI (include/snnhip.h, snnhip_chroma_up_plan_create) against the float64 reference of
tests/chroma_ref.py, into 0xA5-filled outputs.  The comparison rule (chroma_ref.compare_all): a value equals the reference's wherever the
reference's pre-rounding value is farther than eps from a tie (1e-3 at 8 bits, 2e-3 at 10, 6e-3 at 12: six to seventeen times the fp32-to-float64
distance of the expression), is at most 1 off (in units of 1 << shift) on near ties, and near ties are at most 2.5 % of a sweep's values taken
together, asserted on the reference alone."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import chroma_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 2, 3), (2, 5, 7), (1, 37, 29), (2, 19, 67)]  # (N, H, W) of the chroma plane; 5x7 and 19x67: odd rows, U8 rows not dword-aligned
DEPTHS = [("u8", 255, 0), ("u16", 1023, 0), ("u16", 1023, 6), ("u16", 4095, 0)]  # (container, maxval, shift)
DEPTH_IDS = ["u8", "u10", "p010", "u12"]
SITINGS = ["centre", "left"]
FILL = 0xA5


def _np_dtype(container):
    return np.uint8 if container == "u8" else np.uint16


def _capi_dtype(container):
    from shadernn_amd import capi

    return capi.U8 if container == "u8" else capi.U16


def _plane(n, h, w, c, maxval, shift, container, seed):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, maxval + 1, size=(n, h, w, c))
    k = min(4, u.size)
    u.reshape(-1)[:k] = (0, maxval, maxval // 2 + 1, 1)[:k]
    return (u << shift).astype(_np_dtype(container))


def _download(t, container):
    return t.numpy_u8() if container == "u8" else t.numpy_u16()


def tile_of(plan):
    m = re.search(r"tile=(\d+)x(\d+)", plan.describe())
    assert m, plan.describe()
    return int(m.group(1)), int(m.group(2))


def shapes_for(ctx, r, c, container, maxval, shift):
    """The fixed shapes plus two derived from the kernel's own tile: 2 x 2 tiles with a ragged right and bottom edge, and a tile seam in both
    directions with a batch boundary (N = 2)."""
    from shadernn_amd import capi

    probe = capi.chroma_up_plan(ctx, 1, 1, 1, c, r, _capi_dtype(container), maxval, shift, "left")
    th, tw = tile_of(probe)
    probe.destroy()
    return SHAPES + [(1, 2 * th - 3, 2 * tw - 5), (2, th + 1, tw + 1)]


def run_plan(ctx, u, r, container, maxval, shift, siting):
    from shadernn_amd import capi

    n, h, w, c = u.shape
    dt = _capi_dtype(container)
    plan = capi.chroma_up_plan(ctx, n, h, w, c, r, dt, maxval, shift, siting)
    desc = plan.describe()
    assert "chroma_up_%s r=%d c=%d siting=%s tile=" % ("u8" if container == "u8" else "u16", r, c, siting) in desc, desc
    assert plan.out_shape() == (n, r * h, r * w, c)
    assert plan.cost()[1] == (n * h * w * c + n * r * h * r * w * c) * u.dtype.itemsize  # the input once, the output once
    fill = np.full((n, r * h, r * w, c), FILL if container == "u8" else FILL * 0x101, u.dtype)
    out = capi.Tensor.from_numpy(ctx, fill, dtype=dt)
    plan.run(capi.Tensor.from_numpy(ctx, u, dtype=dt), out)
    got = _download(out, container)
    plan.destroy()
    return got


def sweep(ctx, r, c, container, maxval, shift, shapes, sitings=SITINGS):
    """Every shape and siting against the reference (the near-tie cap over the sweep's values together); returns the line to print."""
    items = []
    for si, siting in enumerate(sitings):
        for k, (n, h, w) in enumerate(shapes):
            u = _plane(n, h, w, c, maxval, shift, container, seed=1000 * r + 100 * c + 10 * k + si + maxval)
            got = run_plan(ctx, u, r, container, maxval, shift, siting)
            items.append((got, R.up_values(u, r, siting, shift), maxval, shift))
    frac, ndiff = R.compare_all(items)
    return "chroma_up %s maxval=%d shift=%d r=%d c=%d, %d runs: near ties %.3f %%, %d values differ" % (container, maxval, shift, r, c, len(items), 100 * frac, ndiff)


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_plan_matches_the_reference(ctx, r, c, depth):
    container, maxval, shift = depth
    print(sweep(ctx, r, c, container, maxval, shift, shapes_for(ctx, r, c, container, maxval, shift)))


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("c", [1, 2])
def test_r1_is_the_input_byte_for_byte_with_the_low_bits_cleared(ctx, c, depth):
    container, maxval, shift = depth
    rng = np.random.default_rng(11)
    for siting in SITINGS:
        for k, (n, h, w) in enumerate(shapes_for(ctx, 1, c, container, maxval, shift)):
            u = _plane(n, h, w, c, maxval, shift, container, seed=60 + k)
            dirty = u | rng.integers(0, 1 << shift, size=u.shape).astype(u.dtype)
            np.testing.assert_array_equal(run_plan(ctx, dirty, 1, container, maxval, shift, siting), u)  # no near-tie allowance


@pytest.mark.parametrize("r", [2, 3])
def test_low_bits_of_a_high_aligned_plane_are_ignored(ctx, r):
    """P010 containers carry ten bits in the high end; whatever sits in the six bits below them must not reach the result."""
    container, maxval, shift = "u16", 1023, 6
    rng = np.random.default_rng(12)
    for n, h, w in [(2, 5, 7), (1, 37, 29)]:
        u = _plane(n, h, w, 2, maxval, shift, container, seed=70 + r)
        dirty = u | rng.integers(1, 1 << shift, size=u.shape).astype(u.dtype)
        np.testing.assert_array_equal(run_plan(ctx, dirty, r, container, maxval, shift, "left"), run_plan(ctx, u, r, container, maxval, shift, "left"))


def test_the_two_sitings_differ_and_a_constant_plane_stays_constant(ctx):
    u = _plane(1, 9, 33, 2, 255, 0, "u8", seed=3)
    assert not np.array_equal(run_plan(ctx, u, 2, "u8", 255, 0, "left"), run_plan(ctx, u, 2, "u8", 255, 0, "centre"))
    for r in (1, 2, 3, 4):
        for container, maxval, shift in DEPTHS:
            for value in (0, maxval, maxval // 3):
                k = np.full((2, 5, 7, 2), value << shift, _np_dtype(container))
                got = run_plan(ctx, k, r, container, maxval, shift, "left")
                np.testing.assert_array_equal(got, np.full_like(got, value << shift))


def test_trace_report_names_the_kernel(ctx):
    from shadernn_amd import capi

    plan = capi.chroma_up_plan(ctx, 1, 9, 13, 2, 2)
    x = capi.Tensor.from_numpy(ctx, _plane(1, 9, 13, 2, 255, 0, "u8", 1), dtype=capi.U8)
    y = capi.Tensor.from_numpy(ctx, np.zeros((1, 18, 26, 2), np.uint8), dtype=capi.U8)
    capi.trace_begin()
    plan.run(x, y)
    ctx.sync()
    text = str(capi.trace_end())
    assert "chroma_up_kernel" in text, text


def _refused(fn, *needles):
    from shadernn_amd import capi

    with pytest.raises(capi.SnnHipError) as e:
        fn()
    assert e.value.code == capi.E_INVALID, str(e.value)
    msg = str(e.value)
    assert len(msg) > len("snnhip error -1: ") and all(s in msg for s in needles), msg


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    mk = capi.chroma_up_plan
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2), "chroma_up desc", "3 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 0, 2), "chroma_up desc", "0 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 0), "chroma_up desc", "r = 0")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 5), "chroma_up desc", "r = 5")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.F32), "chroma_up desc", "dtype")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.F16), "chroma_up desc", "dtype")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.U8, 255, 0, 2), "chroma_up desc", "siting")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.U8, 256, 0), "chroma_up desc", "maxval 256")        # does not fit a byte
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.U8, 127, 1), "chroma_up desc", "shift 1")            # 8-bit planes have no shift
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.U16, 1023, 7), "chroma_up desc", "does not fit")      # 1023 << 7 needs 17 bits
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.U16, 1023, 16), "chroma_up desc", "shift 16")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.U16, 0, 0), "chroma_up desc", "maxval 0")
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.U16, 65535, 0), "chroma_up desc", "4095")             # P016 chroma is not built
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2, capi.U16, 4096, 0), "chroma_up desc", "4095")
    _refused(lambda: mk(ctx, 1, 0, 4, 2, 2), "chroma_up desc", "bad dims")
    n, h, w, c, r = 1, 4, 6, 2, 2
    plan = mk(ctx, n, h, w, c, r)
    u = _plane(n, h, w, c, 255, 0, "u8", 1)
    x = capi.Tensor.from_numpy(ctx, u, dtype=capi.U8)
    out = capi.Tensor.from_numpy(ctx, np.full((n, r * h, r * w, c), FILL, np.uint8), dtype=capi.U8)
    plan.run(x, out)  # the valid call
    for bad in ((n, 3 * h, 3 * w, c), (n, r * h, r * w + 1, c), (n, r * h, 3 * w, c), (n, h, w, c), (n, r * h, r * w, 1), (2, r * h, r * w, c)):
        _refused(lambda: plan.run(x, capi.Tensor(ctx, *bad, dtype=capi.U8)), "chroma_up", "the output is")  # not r times the input
    _refused(lambda: plan.run(capi.Tensor(ctx, n, h + 1, w, c, dtype=capi.U8), out), "chroma_up", "the input plane is")
    _refused(lambda: plan.run(capi.Tensor(ctx, n, h, w, c), out), "plan_run: input 0 has dtype 0")               # a float tensor as the input
    _refused(lambda: plan.run(capi.Tensor(ctx, n, h, w, c, dtype=capi.U16), out), "plan_run", "16-bit")         # a 16-bit plane into an 8-bit plan
    _refused(lambda: plan.run(x, capi.Tensor(ctx, n, r * h, r * w, c)), "plan_run", "8-bit")                     # a float tensor as the output
    _refused(lambda: plan.run(x, capi.Tensor(ctx, n, r * h, r * w, c, dtype=capi.U16)), "plan_run")             # a 16-bit output
    wide = mk(ctx, n, h, w, c, r, capi.U16, 1023, 6)
    _refused(lambda: wide.run(x, capi.Tensor(ctx, n, r * h, r * w, c, dtype=capi.U16)), "plan_run", "8-bit")     # an 8-bit plane into a 16-bit plan
    R.compare(out.numpy_u8(), R.up_values(u, r, "left"), 255, 0)  # nothing above touched the valid result


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, checked by snnhip_sync) is fixed at the library's first allocation: a child
    process, started the way tests/test_frame_colour_gpu.py starts its own, runs the same sweep once -- every r, C, depth and siting on the three
    smallest shapes and the two tile-derived ones.  Valid shapes only: no SNNHIP_E_GUARD may come back."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_frame_chroma_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for r in (1, 2, 3, 4):
            for c in (1, 2):
                for container, maxval, shift in T.DEPTHS:
                    shapes = T.shapes_for(ctx, r, c, container, maxval, shift)
                    T.sweep(ctx, r, c, container, maxval, shift, shapes[:3] + shapes[-2:])
                    ctx.sync()                               # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]
