"""The NV12 / P010 -> RGB plan through the C-ABI (include/snnhip.h, snnhip_yuv_rgb_plan_create) against the float64 reference of
tests/yuv_rgb_ref.py, into sentinel-filled outputs.  The comparison rule (yuv_rgb_ref.compare_all): a value equals the reference's wherever the
reference's pre-rounding value is farther than eps from a tie (1e-3 at 8 bits, 3e-3 at 10, 8e-3 at 12: 15 to 34 times the measured fp32-to-float64
distance of the expression), is at most 1 off (in units of 1 << shift) on near ties, and near ties are at most 3 % of a sweep's values taken together,
asserted on the reference alone."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import yuv_rgb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

DEPTHS = [("u8", 255, 0), ("u16", 1023, 6), ("u16", 1023, 0), ("u16", 4095, 0)]  # (container, maxval, shift)
DEPTH_IDS = ["u8", "p010", "u10", "u12"]
SITINGS = ["centre", "left"]
RANGES = ["limited", "full"]
FILL = 0xA5


def _np_dtype(container):
    return np.uint8 if container == "u8" else np.uint16


def _capi_dtype(container):
    from shadernn_amd import capi

    return capi.U8 if container == "u8" else capi.U16


def _download(t, container):
    return t.numpy_u8() if container == "u8" else t.numpy_u16()


def tile_of(plan):
    m = re.search(r"tile=(\d+)x(\d+)", plan.describe())
    assert m, plan.describe()
    return int(m.group(1)), int(m.group(2))


def shapes_for(ctx, r, container, maxval, shift):
    """(N, H, W) of the chroma plane, the smallest where the kernel can go wrong, from the tile (TH, TW) the plan reports: one pixel; 2 x 3 (odd
    width: the last lane of an 8-bit row owns one pixel); one short of a tile, a tile, one past it (a second block in both directions); three rows
    of two tiles and five pixels; for odd r an odd width once more, where the RGB8 and 8-bit Yhi rows are not dword-aligned; N = 2 on the tile seam
    for the batch stride."""
    from shadernn_amd import capi

    probe = capi.yuv_rgb_plan(ctx, 1, 1, 1, 3, r, _capi_dtype(container), maxval, shift)
    th, tw = tile_of(probe)
    probe.destroy()
    shapes = [(1, 1, 1), (1, 2, 3), (1, th - 1, tw - 1), (1, th, tw), (2, th + 1, tw + 1), (1, 3, 2 * tw + 5)]
    if r % 2:
        shapes.append((1, 5, 7))
    return shapes


def run_plan(ctx, yhi, cbcr, r, C, container, maxval, shift, siting, rng, kr=R.BT601[0], kb=R.BT601[1]):
    from shadernn_amd import capi

    n, h, w, _ = cbcr.shape
    dt = _capi_dtype(container)
    plan = capi.yuv_rgb_plan(ctx, n, h, w, C, r, dt, maxval, shift, siting, rng, kr, kb)
    desc = plan.describe()
    assert "yuv_rgb_%s r=%d c=%d siting=%s range=%s tile=" % ("u8" if container == "u8" else "u16", r, C, siting, rng) in desc and "kernel=yuv_rgb_kernel" in desc, desc
    assert plan.out_shape() == (n, 2 * r * h, 2 * r * w, C)
    pixels = n * 2 * r * h * 2 * r * w
    assert plan.cost()[1] == (pixels + n * h * w * 2 + pixels * C) * cbcr.dtype.itemsize  # both inputs once, the output once
    fill = np.full((n, 2 * r * h, 2 * r * w, C), FILL if container == "u8" else FILL * 0x101, cbcr.dtype)
    out = capi.Tensor.from_numpy(ctx, fill, dtype=dt)
    plan.run([capi.Tensor.from_numpy(ctx, yhi, dtype=dt), capi.Tensor.from_numpy(ctx, cbcr, dtype=dt)], out)
    got = _download(out, container)
    plan.destroy()
    return got


def sweep(ctx, r, C, container, maxval, shift, shapes, sitings=SITINGS, ranges=RANGES, whole_range=False):
    """Every shape, siting and range against the reference (the near-tie cap over the sweep's values together); returns the line to print."""
    items = []
    for si, siting in enumerate(sitings):
        for ri, rng in enumerate(ranges):
            for k, (n, h, w) in enumerate(shapes):
                yhi, cbcr = R.frame(n, h, w, r, maxval, shift, _np_dtype(container), seed=1000 * r + 100 * C + 10 * k + 2 * si + ri + maxval, whole_range=whole_range)
                got = run_plan(ctx, yhi, cbcr, r, C, container, maxval, shift, siting, rng)
                items.append((got, R.values(yhi, cbcr, r, siting, rng, maxval, shift), maxval, shift))
    frac, ndiff = R.compare_all(items)
    return "yuv_rgb %s maxval=%d shift=%d r=%d c=%d, %d runs: near ties %.3f %%, %d values differ" % (container, maxval, shift, r, C, len(items), 100 * frac, ndiff)


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_plan_matches_the_reference(ctx, r, C, depth):
    container, maxval, shift = depth
    print(sweep(ctx, r, C, container, maxval, shift, shapes_for(ctx, r, container, maxval, shift)))


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
def test_the_clamps_over_the_whole_code_range(ctx, depth):
    """Y and chroma over 0 .. maxval: a large share of the values leaves [0, maxval] in front of the rounding."""
    container, maxval, shift = depth
    for r in (1, 2, 3):
        print(sweep(ctx, r, 3, container, maxval, shift, [(1, 5, 7), (1, 9, 40)], whole_range=True))


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
def test_neutral_chroma_gives_grey_byte_for_byte_and_alpha_is_maxval(ctx, depth):
    container, maxval, shift = depth
    k = (maxval + 1) // 256
    for r in (1, 2, 3, 4):
        for rng in RANGES:
            for n, h, w in ((1, 2, 3), (2, 9, 70)):
                yhi, cbcr = R.frame(n, h, w, r, maxval, shift, _np_dtype(container), seed=r, whole_range=True)
                if n == 2:  # every luma code (10 bits: 146 above Yoff is an exact tie of the limited-range yl)
                    yhi.reshape(-1)[:min(maxval + 1, yhi.size)] = (np.arange(min(maxval + 1, yhi.size)) << shift).astype(yhi.dtype)
                cbcr[...] = (128 * k) << shift
                got = run_plan(ctx, yhi, cbcr, r, 4, container, maxval, shift, "left", rng)
                c = R.coefficients(maxval, rng)
                yl = c[2] * ((yhi.astype(np.int64) >> shift)[..., 0].astype(np.float32) - c[0])  # fp32, as the contract's yl
                want = R.quantise(yl.astype(np.float64), maxval, shift, yhi.dtype)
                for ch in range(3):
                    np.testing.assert_array_equal(got[..., ch], want)  # no near-tie allowance
                np.testing.assert_array_equal(got[..., 3], np.full_like(want, maxval << shift))


@pytest.mark.parametrize("r", [1, 2, 3])
def test_low_bits_of_a_high_aligned_input_are_ignored(ctx, r):
    container, maxval, shift = "u16", 1023, 6
    rng = np.random.default_rng(12)
    for n, h, w in [(2, 5, 7), (1, 9, 70)]:
        yhi, cbcr = R.frame(n, h, w, r, maxval, shift, np.uint16, seed=70 + r)
        dy = yhi | rng.integers(1, 1 << shift, size=yhi.shape).astype(np.uint16)
        dc = cbcr | rng.integers(1, 1 << shift, size=cbcr.shape).astype(np.uint16)
        np.testing.assert_array_equal(run_plan(ctx, dy, dc, r, 3, container, maxval, shift, "left", "limited"), run_plan(ctx, yhi, cbcr, r, 3, container, maxval, shift, "left", "limited"))


def test_the_two_sitings_differ_on_a_ramp_and_constant_planes_stay_constant(ctx):
    w = 24
    ramp = (8 * np.arange(w) + 20).astype(np.uint8)
    cbcr = np.empty((1, 4, w, 2), np.uint8)
    cbcr[..., 0] = ramp[None, None, :]
    cbcr[..., 1] = ramp[None, None, ::-1]
    for r in (1, 2):
        yhi = np.full((1, 2 * r * 4, 2 * r * w, 1), 120, np.uint8)
        left, centre = (run_plan(ctx, yhi, cbcr, r, 3, "u8", 255, 0, s, "limited") for s in ("left", "centre"))
        assert not np.array_equal(left, centre)
        edge = 4 * r
        assert (left[0, 0, edge:-edge, 2].astype(int) >= centre[0, 0, edge:-edge, 2].astype(int)).all()  # a rising Cb ramp: left reads a quarter sample further on
        assert (left[0, 0, edge:-edge, 2].astype(int) > centre[0, 0, edge:-edge, 2].astype(int)).any()
    for r in (1, 2, 3, 4):
        for container, maxval, shift in DEPTHS:
            k = (maxval + 1) // 256
            yhi = np.full((2, 2 * r * 5, 2 * r * 7, 1), (100 * k) << shift, _np_dtype(container))
            c = np.empty((2, 5, 7, 2), _np_dtype(container))
            c[..., 0], c[..., 1] = (90 * k) << shift, (200 * k) << shift
            got = run_plan(ctx, yhi, c, r, 3, container, maxval, shift, "left", "limited")
            assert (got == got[0, 0, 0]).all()
            np.testing.assert_array_equal(got[0, 0, 0], R.rgb(yhi, c, r, 3, R.LEFT, R.LIMITED, maxval, shift)[0, 0, 0])


def test_another_matrix(ctx):
    yhi, cbcr = R.frame(1, 9, 70, 2, 255, 0, np.uint8, seed=5)
    got = run_plan(ctx, yhi, cbcr, 2, 3, "u8", 255, 0, "left", "limited", *R.BT709)
    R.compare_all([(got, R.values(yhi, cbcr, 2, R.LEFT, R.LIMITED, 255, 0, *R.BT709), 255, 0)])
    assert not np.array_equal(got, run_plan(ctx, yhi, cbcr, 2, 3, "u8", 255, 0, "left", "limited"))


def test_trace_report_names_the_kernel(ctx):
    from shadernn_amd import capi

    plan = capi.yuv_rgb_plan(ctx, 1, 9, 13, 3, 2)
    yhi, cbcr = R.frame(1, 9, 13, 2, 255, 0, np.uint8, seed=1)
    out = capi.Tensor.from_numpy(ctx, np.zeros((1, 36, 52, 3), np.uint8), dtype=capi.U8)
    ins = [capi.Tensor.from_numpy(ctx, yhi, dtype=capi.U8), capi.Tensor.from_numpy(ctx, cbcr, dtype=capi.U8)]
    capi.trace_begin()
    plan.run(ins, out)
    ctx.sync()
    text = str(capi.trace_end())
    assert "yuv_rgb_kernel" in text, text


def _refused(fn, *needles):
    from shadernn_amd import capi

    with pytest.raises(capi.SnnHipError) as e:
        fn()
    assert e.value.code == capi.E_INVALID, str(e.value)
    msg = str(e.value)
    assert len(msg) > len("snnhip error -1: ") and all(s in msg for s in needles), msg


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    mk = capi.yuv_rgb_plan
    _refused(lambda: mk(ctx, 1, 4, 4, 2, 2), "yuv_rgb desc", "2 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 5, 2), "yuv_rgb desc", "5 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 0), "yuv_rgb desc", "r = 0")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 5), "yuv_rgb desc", "r = 5")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.F32), "yuv_rgb desc", "dtype")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.F16), "yuv_rgb desc", "dtype")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U8, 1023, 0), "yuv_rgb desc", "does not fit")          # above 255 in a byte
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U16, 65535, 0), "yuv_rgb desc", "4095")                 # above 12 bits
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U16, 8191, 0), "yuv_rgb desc", "4095")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U16, 1023, 7), "yuv_rgb desc", "does not fit")          # 1023 << 7 needs 17 bits
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U8, 255, 1), "yuv_rgb desc", "shift 1")                 # 8-bit frames have no shift
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U8, 127, 0), "yuv_rgb desc", "multiple of 256")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U16, 1000, 0), "yuv_rgb desc", "multiple of 256")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U8, 255, 0, 2), "yuv_rgb desc", "siting")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, capi.U8, 255, 0, "left", 2), "yuv_rgb desc", "range")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, kr=0.0), "yuv_rgb desc", "kr")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, kb=-0.1), "yuv_rgb desc", "kb")
    _refused(lambda: mk(ctx, 1, 4, 4, 3, 2, kr=0.7, kb=0.3), "yuv_rgb desc", "kr + kb < 1")
    _refused(lambda: mk(ctx, 1, 0, 4, 3, 2), "yuv_rgb desc", "bad dims")
    n, h, w, C, r = 1, 4, 6, 3, 2
    plan = mk(ctx, n, h, w, C, r)
    yhi, cbcr = R.frame(n, h, w, r, 255, 0, np.uint8, seed=1)
    y = capi.Tensor.from_numpy(ctx, yhi, dtype=capi.U8)
    c = capi.Tensor.from_numpy(ctx, cbcr, dtype=capi.U8)
    out = capi.Tensor.from_numpy(ctx, np.full((n, 4 * h, 4 * w, C), FILL, np.uint8), dtype=capi.U8)
    plan.run([y, c], out)  # the valid call
    for bad in ((n, 2 * h, 2 * w, C), (n, 4 * h, 4 * w + 1, C), (n, 6 * h, 6 * w, C), (n, 4 * h, 4 * w, 4), (2, 4 * h, 4 * w, C)):
        _refused(lambda: plan.run([y, c], capi.Tensor(ctx, *bad, dtype=capi.U8)), "yuv_rgb", "the output is")  # not 2r times the chroma plane
    _refused(lambda: plan.run([capi.Tensor(ctx, n, 2 * h, 2 * w, 1, dtype=capi.U8), c], out), "yuv_rgb", "Yhi is")  # Yhi at the input resolution
    _refused(lambda: plan.run([y, capi.Tensor(ctx, n, h + 1, w, 2, dtype=capi.U8)], out), "yuv_rgb", "the chroma plane is")
    _refused(lambda: plan.run([y, capi.Tensor(ctx, n, h, w, 1, dtype=capi.U8)], out), "yuv_rgb", "the chroma plane is")
    _refused(lambda: plan.run([y], out), "yuv_rgb", "2 inputs")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, 4 * h, 4 * w, 1), c], out), "plan_run: input 0 has dtype 0")          # a float tensor as Yhi
    _refused(lambda: plan.run([y, capi.Tensor(ctx, n, h, w, 2)], out), "plan_run: input 1 has dtype 0")                   # ... as the chroma plane
    _refused(lambda: plan.run([y, capi.Tensor(ctx, n, h, w, 2, dtype=capi.U16)], out), "plan_run", "16-bit")            # a 16-bit plane into an 8-bit plan
    _refused(lambda: plan.run([y, c], capi.Tensor(ctx, n, 4 * h, 4 * w, C)), "plan_run", "8-bit")                         # a float tensor as the output
    _refused(lambda: plan.run([y, c], capi.Tensor(ctx, n, 4 * h, 4 * w, C, dtype=capi.U16)), "plan_run")                 # a 16-bit output
    wide = mk(ctx, n, h, w, C, r, capi.U16, 1023, 6)
    _refused(lambda: wide.run([y, c], capi.Tensor(ctx, n, 4 * h, 4 * w, C, dtype=capi.U16)), "plan_run", "8-bit")       # 8-bit planes into a 16-bit plan
    R.compare(out.numpy_u8(), R.values(yhi, cbcr, r), 255, 0)  # nothing above touched the valid result


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, checked by snnhip_sync) is fixed at the library's first allocation: a child
    process, started the way tests/test_frame_chroma_gpu.py starts its own, runs the sweep once -- every r, C and depth, both sitings, on every
    shape.  Valid shapes only: no SNNHIP_E_GUARD may come back."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_frame_yuv_rgb_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for r in (1, 2, 3, 4):
            for C in (3, 4):
                for container, maxval, shift in T.DEPTHS:
                    T.sweep(ctx, r, C, container, maxval, shift, T.shapes_for(ctx, r, container, maxval, shift), ranges=["limited"])
                    ctx.sync()                               # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]
