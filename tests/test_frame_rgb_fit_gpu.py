"""The fitted-RGB plan through the C-ABI (include/snnhip.h, snnhip_rgb_fit_plan_create) against the float64 reference of tests/rgb_fit_ref.py, into
0xA5-filled outputs.  The comparison rule (rgb_fit_ref.compare_all): a value equals the reference's wherever the reference's pre-rounding value is
farther than eps from a tie (1e-3 at 8 bits, 3e-3 at 10, 8e-3 at 12: the family's values, 16 to 37 times the fp32-to-float64 distance of these
expressions), is at most 1 off (in units of 1 << shift) on near ties, and near ties are at most 3 % (video sources) or 1 % (the RGB source) of a
sweep's values taken together, asserted on the reference alone.  Alpha is exact."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import colour_ref
import rgb_fit_ref as R
import yuv_rgb_ref
from test_frame_chroma_gpu import DEPTHS, DEPTH_IDS, FILL, SITINGS, _capi_dtype, _download, _np_dtype
from test_frame_yuv_rgb_gpu import _refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RANGES = ["limited", "full"]
SHAPES = R.SHAPES[:-2]  # all but the two largest (those serve the CPU measurements)


def tile_of(plan):
    m = re.search(r"tile=(\d+)x(\d+)", plan.describe())
    assert m, plan.describe()
    return int(m.group(1)), int(m.group(2))


def shapes_for(ctx, source, c, container, maxval, shift):
    """The fixed shapes plus two derived from the tile the kernel reports: a tile seam on both axes with ragged edges at ratio 3/2, and N = 2 at
    ratio exactly 1 with one pixel more than a tile each way -- the source span and the LDS rows at their largest."""
    from shadernn_amd import capi

    probe = capi.rgb_fit_plan(ctx, 1, 2, 2, 2, 2, c, source, _capi_dtype(container), maxval, shift)
    th, tw = tile_of(probe)
    probe.destroy()
    oh, ow = 2 * th - 3, 2 * tw - 5
    return SHAPES + [(1, -(-2 * oh // 3), -(-2 * ow // 3), oh, ow), (2, th + 1, tw + 1, th + 1, tw + 1)]


def run_plan(ctx, yfit, chroma, source, c, container="u8", maxval=255, shift=0, siting="left", rng="limited", kr=R.BT601[0], kb=R.BT601[1]):
    """`chroma` is the source tensor as the plan takes it (cbcr [N][H][W][2], planar [2N][H][W][1] or the colour frame)."""
    from shadernn_amd import capi

    n, oh, ow, _ = yfit.shape
    h, w = chroma.shape[1:3]
    dt = _capi_dtype(container)
    plan = capi.rgb_fit_plan(ctx, n, h, w, oh, ow, c, source, dt, maxval, shift, siting, rng, kr, kb)
    desc = plan.describe()
    assert "rgb_fit_%s src=%s c=%d %dx%d->%dx%d siting=" % ("u8" if container == "u8" else "u16", source, c, h, w, oh, ow) in desc and "taps=4 lds=49152" in desc, desc
    assert desc.endswith("kernel=rgb_fit_kernel"), desc
    assert plan.out_shape() == (n, oh, ow, c)
    assert plan.cost()[1] == (yfit.size + chroma.size + n * oh * ow * c) * yfit.dtype.itemsize  # both inputs once, the output once
    fill = np.full((n, oh, ow, c), FILL if container == "u8" else FILL * 0x101, yfit.dtype)
    out = capi.Tensor.from_numpy(ctx, fill, dtype=dt)
    plan.run([capi.Tensor.from_numpy(ctx, yfit, dtype=dt), capi.Tensor.from_numpy(ctx, np.ascontiguousarray(chroma), dtype=dt)], out)
    got = _download(out, container)
    plan.destroy()
    return got


def video_sweep(ctx, source, c, container, maxval, shift, shapes):
    """Every shape, siting and range against the reference (the near-tie cap over the sweep's values together); returns the line to print."""
    items = []
    for si, siting in enumerate(SITINGS):
        for ri, rng in enumerate(RANGES):
            for k, (n, h, w, oh, ow) in enumerate(shapes):
                yfit, cbcr = R.video_frame(n, h, w, oh, ow, maxval, shift, _np_dtype(container), seed=1000 * c + 100 * k + 10 * si + ri + maxval)
                src = R.to_planar(cbcr) if source == "planar" else cbcr
                got = run_plan(ctx, yfit, src, source, c, container, maxval, shift, siting, rng)
                items.append((got, R.video_values(yfit, cbcr, siting, rng, maxval, shift), maxval, shift))
    frac, ndiff = R.compare_all(items, "video")
    return "rgb_fit %s %s maxval=%d shift=%d c=%d, %d runs: near ties %.3f %%, %d values differ" % (source, container, maxval, shift, c, len(items), 100 * frac, ndiff)


def rgb_sweep(ctx, c, shapes):
    items = []
    for k, (n, h, w, oh, ow) in enumerate(shapes):
        yfit, frame = R.rgb_frame(n, h, w, oh, ow, c, seed=300 + 10 * k + c)
        got = run_plan(ctx, yfit, frame, "rgb", c)
        items.append((got, R.rgb_values(yfit, frame), 255, 0, R.alpha_of(frame, oh, ow) if c == 4 else None))
    frac, ndiff = R.compare_all(items, "rgb")
    return "rgb_fit rgb u8 c=%d, %d runs: near ties %.3f %%, %d values differ" % (c, len(items), 100 * frac, ndiff)


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("source", ["cbcr", "planar"])
def test_video_plan_matches_the_reference(ctx, source, c, depth):
    container, maxval, shift = depth
    print(video_sweep(ctx, source, c, container, maxval, shift, shapes_for(ctx, source, c, container, maxval, shift)))


@pytest.mark.parametrize("c", [3, 4])
def test_rgb_plan_matches_the_reference(ctx, c):
    print(rgb_sweep(ctx, c, shapes_for(ctx, "rgb", c, "u8", 255, 0)))


def test_rows_dealt_to_lane_sets_meet_at_the_chunk_boundaries(ctx):
    """Pass 1 deals a tile's rows to lane sets when the tile's column span has fewer strips than the block has lanes: sets >= 2, chunks of
    ceil(rows / sets).  One row less and one row more than a tile (tests/test_frame_rgb_fit.py::lane_set_frames, whose near ties are counted
    there): chunks of one and two rows, two sets with a short second chunk, a second tile of a single row."""
    from shadernn_amd import capi
    from test_frame_rgb_fit import lane_set_frames

    probe = capi.rgb_fit_plan(ctx, 1, 11, 20, 12, 30, 3, "cbcr", capi.U8, 255, 0)
    th, _ = tile_of(probe)
    probe.destroy()
    items = [(run_plan(ctx, yfit, cbcr, "cbcr", 3), R.video_values(yfit, cbcr), 255, 0) for yfit, cbcr in lane_set_frames(th)]
    frac, ndiff = R.compare_all(items, "video")
    print("rgb_fit lane sets, tile of %d rows, %d runs: near ties %.3f %%, %d values differ" % (th, len(items), 100 * frac, ndiff))


def test_odd_widths_unaligned_rows_and_ratio_eight(ctx):
    """Odd OW: the RGB8 pitch 3 OW and the 8-bit Yfit pitch are no multiples of 4, so rows start off a dword; an odd source width does the same to the
    source rows of every layout.  Ratio 8 on both axes is the far end of the range."""
    items = []
    for k, (n, h, w, oh, ow) in enumerate([(1, 3, 5, 9, 13), (2, 3, 3, 24, 24), (1, 7, 33, 56, 263), (1, 2, 1, 16, 8)]):
        for source in ("cbcr", "planar"):
            yfit, cbcr = R.video_frame(n, h, w, oh, ow, 255, 0, np.uint8, seed=40 + k)
            got = run_plan(ctx, yfit, R.to_planar(cbcr) if source == "planar" else cbcr, source, 3)
            items.append((got, R.video_values(yfit, cbcr), 255, 0))
        yfit, cbcr = R.video_frame(n, h, w, oh, ow, 1023, 6, np.uint16, seed=50 + k)
        items.append((run_plan(ctx, yfit, cbcr, "cbcr", 3, "u16", 1023, 6), R.video_values(yfit, cbcr, maxval=1023, shift=6), 1023, 6))
    frac, ndiff = R.compare_all(items, "video")
    print("odd widths and ratio 8, video: near ties %.3f %%, %d values differ" % (100 * frac, ndiff))
    items = []
    for k, (n, h, w, oh, ow) in enumerate([(1, 3, 5, 9, 13), (2, 3, 3, 24, 24), (1, 7, 33, 56, 263)]):
        for c in (3, 4):
            yfit, frame = R.rgb_frame(n, h, w, oh, ow, c, seed=60 + k)
            items.append((run_plan(ctx, yfit, frame, "rgb", c), R.rgb_values(yfit, frame), 255, 0, R.alpha_of(frame, oh, ow) if c == 4 else None))
    frac, ndiff = R.compare_all(items, "rgb")
    print("odd widths and ratio 8, rgb: near ties %.3f %%, %d values differ" % (100 * frac, ndiff))


def test_low_bits_of_a_high_aligned_frame_are_ignored(ctx):
    """P010 containers carry ten bits in the high end; whatever sits in the six bits below them must not reach the result."""
    rng = np.random.default_rng(12)
    for n, h, w, oh, ow in [(2, 9, 11, 23, 30), (1, 19, 35, 27, 100)]:
        yfit, cbcr = R.video_frame(n, h, w, oh, ow, 1023, 6, np.uint16, seed=70 + h)
        dy = yfit | rng.integers(1, 64, size=yfit.shape).astype(np.uint16)
        dc = cbcr | rng.integers(1, 64, size=cbcr.shape).astype(np.uint16)
        for source, conv in (("cbcr", lambda a: a), ("planar", R.to_planar)):
            np.testing.assert_array_equal(run_plan(ctx, dy, conv(dc), source, 4, "u16", 1023, 6), run_plan(ctx, yfit, conv(cbcr), source, 4, "u16", 1023, 6))


def test_another_matrix(ctx):
    kr, kb = R.BT709
    n, h, w, oh, ow = 1, 12, 16, 36, 48
    yfit, cbcr = R.video_frame(n, h, w, oh, ow, 255, 0, np.uint8, seed=5)
    a = run_plan(ctx, yfit, cbcr, "cbcr", 3, kr=kr, kb=kb)
    R.compare_all([(a, R.video_values(yfit, cbcr, kr=kr, kb=kb), 255, 0)], "video")
    assert not np.array_equal(a, run_plan(ctx, yfit, cbcr, "cbcr", 3))
    yfit, frame = R.rgb_frame(n, h, w, oh, ow, 3, seed=6)
    b = run_plan(ctx, yfit, frame, "rgb", 3, kr=kr, kb=kb)
    R.compare_all([(b, R.rgb_values(yfit, frame, kr, kb), 255, 0)], "rgb")
    assert not np.array_equal(b, run_plan(ctx, yfit, frame, "rgb", 3))


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
def test_neutral_chroma_gives_the_quantised_luma_term_byte_for_byte(ctx, depth):
    container, maxval, shift = depth
    dt = _np_dtype(container)
    k = (maxval + 1) // 256
    for i, (n, h, w, oh, ow) in enumerate(SHAPES):
        yfit, _ = R.video_frame(n, h, w, oh, ow, maxval, shift, dt, seed=i, whole_range=True)
        cbcr = np.full((n, h, w, 2), (128 * k) << shift, dt)
        for rng in RANGES:
            c = yuv_rgb_ref.coefficients(maxval, rng)  # float32, as the device sees them: cy (Y - Yoff) is an exact difference and one product
            yl32 = c[2] * ((yfit.astype(np.int64) >> shift).astype(np.float32) - c[0])
            for source, conv in (("cbcr", lambda a: a), ("planar", R.to_planar)):
                got = run_plan(ctx, yfit, conv(cbcr), source, 4, container, maxval, shift, "left", rng)
                np.testing.assert_array_equal(got[..., 0], got[..., 1])
                np.testing.assert_array_equal(got[..., 0], got[..., 2])
                np.testing.assert_array_equal(got[..., :1], R.quantise(yl32, maxval, shift, dt))  # the quantised luma term, as fp32 forms it
                R.compare(got, R.video_values(yfit, cbcr, "left", rng, maxval, shift), maxval, shift)


def test_a_grey_source_frame_gives_the_luma_frame_byte_for_byte(ctx):
    for i, (n, h, w, oh, ow) in enumerate(SHAPES):
        yfit, frame = R.rgb_frame(n, h, w, oh, ow, 4, seed=i)
        frame[..., :3] = frame[..., :1]
        got = run_plan(ctx, yfit, frame, "rgb", 4)
        np.testing.assert_array_equal(got[..., :3], np.repeat(yfit, 3, axis=-1))
        np.testing.assert_array_equal(got[..., 3:], R.alpha_of(frame, oh, ow))


def test_constant_chroma_planes_give_constant_chroma_terms(ctx):
    for n, h, w, oh, ow in SHAPES:
        yfit = np.full((n, oh, ow, 1), 100, np.uint8)
        cbcr = np.zeros((n, h, w, 2), np.uint8)
        cbcr[..., 0], cbcr[..., 1] = 90, 170
        got = run_plan(ctx, yfit, cbcr, "cbcr", 3)
        np.testing.assert_array_equal(got, np.broadcast_to(got[:1, :1, :1], got.shape))


def test_alpha_is_the_source_pixel_underneath(ctx):
    for n, h, w, oh, ow in [(2, 3, 5, 4, 7), (1, 5, 7, 40, 56), (1, 19, 35, 27, 100), (1, 12, 16, 12, 16)]:
        yfit, frame = R.rgb_frame(n, h, w, oh, ow, 4, seed=h)
        frame[..., 3] = (np.arange(n * h * w) % 251).reshape(n, h, w)
        got = run_plan(ctx, yfit, frame, "rgb", 4)
        np.testing.assert_array_equal(got[..., 3:], R.alpha_of(frame, oh, ow))


@pytest.mark.parametrize("depth", DEPTHS, ids=DEPTH_IDS)
def test_planar_and_interleaved_chroma_give_the_same_frame(ctx, depth):
    container, maxval, shift = depth
    for c in (3, 4):
        for k, (n, h, w, oh, ow) in enumerate(shapes_for(ctx, "planar", c, container, maxval, shift)):
            yfit, cbcr = R.video_frame(n, h, w, oh, ow, maxval, shift, _np_dtype(container), seed=80 + k, whole_range=True)
            a = run_plan(ctx, yfit, cbcr, "cbcr", c, container, maxval, shift)
            b = run_plan(ctx, yfit, R.to_planar(cbcr), "planar", c, container, maxval, shift)
            assert int((a != b).sum()) == 0, (n, h, w, oh, ow)


def test_an_integer_factor_against_the_fixed_phase_plans(ctx):
    """O = 2r I against yuv_rgb and O = r I against ycc_merge on the same inputs: the tables agree to one float ulp and the passes run in the other
    order, so the frames may differ -- only where the reference's value is a near tie."""
    from shadernn_amd import capi

    for r in (1, 2, 3, 4):
        n, h, w = 1, 9, 13
        for siting in SITINGS:
            yhi, cbcr = yuv_rgb_ref.frame(n, h, w, r, 255, 0, np.uint8, seed=90 + r)
            plan = capi.yuv_rgb_plan(ctx, n, h, w, 3, r, capi.U8, 255, 0, siting)
            out = capi.Tensor.from_numpy(ctx, np.zeros((n, 2 * r * h, 2 * r * w, 3), np.uint8), dtype=capi.U8)
            plan.run([capi.Tensor.from_numpy(ctx, yhi, dtype=capi.U8), capi.Tensor.from_numpy(ctx, cbcr, dtype=capi.U8)], out)
            fixed = out.numpy_u8()
            plan.destroy()
            got = run_plan(ctx, yhi, cbcr, "cbcr", 3, siting=siting)
            diff = got != fixed
            tie = R.near_tie(R.video_values(yhi, cbcr, siting), R.EPS[255])
            print("r = %d %s: rgb_fit against yuv_rgb, %d of %d values differ" % (r, siting, int(diff.sum()), diff.size))
            assert not (diff & ~tie).any()
        yhi = np.random.default_rng(r).integers(0, 256, size=(n, r * h, r * w, 1)).astype(np.uint8)
        frame = np.random.default_rng(10 + r).integers(0, 256, size=(n, h, w, 4)).astype(np.uint8)
        plan = capi.ycc_merge_plan(ctx, n, h, w, 4, r)
        out = capi.Tensor.from_numpy(ctx, np.zeros((n, r * h, r * w, 4), np.uint8), dtype=capi.U8)
        plan.run([capi.Tensor.from_numpy(ctx, yhi, dtype=capi.U8), capi.Tensor.from_numpy(ctx, frame, dtype=capi.U8)], out)
        fixed = out.numpy_u8()
        plan.destroy()
        got = run_plan(ctx, yhi, frame, "rgb", 4)
        diff = got != fixed
        tie = R.near_tie(R.rgb_values(yhi, frame), R.EPS[255])
        print("r = %d: rgb_fit against ycc_merge, %d of %d values differ" % (r, int(diff.sum()), diff.size))
        assert not diff[..., 3].any() and not (diff[..., :3] & ~tie).any()
        colour_ref.compare(fixed[..., :3], colour_ref.merge_values(yhi, frame, r), None)  # (the fixed-phase frame is itself within its own contract)


def test_trace_report_names_the_kernel(ctx):
    from shadernn_amd import capi

    plan = capi.rgb_fit_plan(ctx, 1, 5, 7, 13, 19, 3)
    yfit, cbcr = R.video_frame(1, 5, 7, 13, 19, 255, 0, np.uint8, seed=1)
    out = capi.Tensor.from_numpy(ctx, np.zeros((1, 13, 19, 3), np.uint8), dtype=capi.U8)
    y, c = capi.Tensor.from_numpy(ctx, yfit, dtype=capi.U8), capi.Tensor.from_numpy(ctx, cbcr, dtype=capi.U8)
    capi.trace_begin()
    plan.run([y, c], out)
    ctx.sync()
    text = str(capi.trace_end())
    assert "rgb_fit_kernel" in text, text


def test_a_recorded_graph_replays(ctx):
    from shadernn_amd import capi

    n, h, w, oh, ow = 2, 9, 11, 23, 30
    plan = capi.rgb_fit_plan(ctx, n, h, w, oh, ow, 4, "planar")
    yfit, cbcr = R.video_frame(n, h, w, oh, ow, 255, 0, np.uint8, seed=3)
    y, c = capi.Tensor.from_numpy(ctx, yfit, dtype=capi.U8), capi.Tensor.from_numpy(ctx, R.to_planar(cbcr), dtype=capi.U8)
    out = capi.Tensor.from_numpy(ctx, np.full((n, oh, ow, 4), FILL, np.uint8), dtype=capi.U8)
    with capi.Graph.capture(ctx) as g:
        plan.run([y, c], out)
    assert g.num_nodes() == 1
    for seed in (4, 5):  # replayed twice, on fresh inputs each time
        yfit, cbcr = R.video_frame(n, h, w, oh, ow, 255, 0, np.uint8, seed=seed)
        y.upload_u8(yfit)
        c.upload_u8(R.to_planar(cbcr))
        out.upload_u8(np.full((n, oh, ow, 4), FILL, np.uint8))
        g.launch()
        ctx.sync()
        R.compare(out.numpy_u8(), R.video_values(yfit, cbcr), 255, 0)
    g.destroy()
    plan.destroy()


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    mk = capi.rgb_fit_plan
    _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 2), "rgb_fit desc", "2 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 5), "rgb_fit desc", "5 channels")
    _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, 3), "rgb_fit desc", "source 3")
    _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, -1), "rgb_fit desc", "source -1")
    _refused(lambda: mk(ctx, 1, 5, 4, 4, 8, 3), "rgb_fit desc", "vertical", "from 5 to 4")          # below 1
    _refused(lambda: mk(ctx, 1, 4, 5, 8, 4, 3), "rgb_fit desc", "horizontal", "from 5 to 4")
    _refused(lambda: mk(ctx, 1, 4, 4, 33, 8, 3), "rgb_fit desc", "vertical", "from 4 to 33")        # above 8
    _refused(lambda: mk(ctx, 1, 4, 4, 8, 33, 3), "rgb_fit desc", "horizontal", "from 4 to 33")
    _refused(lambda: mk(ctx, 1, 0, 4, 8, 8, 3), "rgb_fit desc", "bad dims")
    _refused(lambda: mk(ctx, 1, 4, 4, 8, 0, 3), "rgb_fit desc", "bad dims")
    _refused(lambda: mk(ctx, 0, 4, 4, 8, 8, 3), "rgb_fit desc", "bad dims")
    _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, "rgb", capi.U16, 1023), "rgb_fit desc", "RGB source")
    _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, "rgb", capi.F32), "rgb_fit desc", "RGB source")
    for source in ("cbcr", "planar"):
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.F32), "rgb_fit desc", "dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.F16), "rgb_fit desc", "dtype")
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.U8, 1023, 0), "rgb_fit desc", "does not fit")   # above 255 in a byte
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.U16, 65535, 0), "rgb_fit desc", "4095")          # above 12 bits
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.U16, 1023, 7), "rgb_fit desc", "does not fit")   # 1023 << 7 needs 17 bits
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.U8, 255, 1), "rgb_fit desc", "shift 1")          # 8-bit frames have no shift
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.U8, 127, 0), "rgb_fit desc", "multiple of 256")
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.U16, 1000, 0), "rgb_fit desc", "multiple of 256")
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.U8, 255, 0, 2), "rgb_fit desc", "siting")
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, capi.U8, 255, 0, "left", 2), "rgb_fit desc", "range")
    for source in ("cbcr", "planar", "rgb"):
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, kr=0.0), "rgb_fit desc", "kr")
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, kb=-0.1), "rgb_fit desc", "kb")
        _refused(lambda: mk(ctx, 1, 4, 4, 8, 8, 3, source, kr=0.7, kb=0.3), "rgb_fit desc", "kr + kb < 1")
    n, h, w, oh, ow, C = 1, 4, 6, 6, 9, 3
    plan = mk(ctx, n, h, w, oh, ow, C)
    yfit, cbcr = R.video_frame(n, h, w, oh, ow, 255, 0, np.uint8, seed=1)
    y, c = capi.Tensor.from_numpy(ctx, yfit, dtype=capi.U8), capi.Tensor.from_numpy(ctx, cbcr, dtype=capi.U8)
    out = capi.Tensor.from_numpy(ctx, np.full((n, oh, ow, C), FILL, np.uint8), dtype=capi.U8)
    plan.run([y, c], out)  # the valid call
    for bad in ((n, oh + 1, ow, C), (n, oh, ow + 1, C), (n, oh, ow, 4), (n, oh, ow, 1), (2, oh, ow, C)):
        _refused(lambda: plan.run([y, c], capi.Tensor(ctx, *bad, dtype=capi.U8)), "rgb_fit", "the output is")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, oh, ow + 1, 1, dtype=capi.U8), c], out), "rgb_fit", "Yfit is")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, h, w, 1, dtype=capi.U8), c], out), "rgb_fit", "Yfit is")            # the luma frame at the source's size
    _refused(lambda: plan.run([y, capi.Tensor(ctx, n, h + 1, w, 2, dtype=capi.U8)], out), "rgb_fit", "the chroma source is")
    _refused(lambda: plan.run([y, capi.Tensor(ctx, 2 * n, h, w, 1, dtype=capi.U8)], out), "rgb_fit", "the chroma source is")  # planar planes into a CbCr plan
    _refused(lambda: plan.run([y], out), "rgb_fit", "2 inputs")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, oh, ow, 1), c], out), "plan_run: input 0 has dtype 0")                # a float tensor as Yfit
    _refused(lambda: plan.run([y, capi.Tensor(ctx, n, h, w, 2)], out), "plan_run: input 1 has dtype 0")                   # ... as the chroma source
    _refused(lambda: plan.run([y, capi.Tensor(ctx, n, h, w, 2, dtype=capi.U16)], out), "plan_run", "16-bit")            # a 16-bit plane into an 8-bit plan
    _refused(lambda: plan.run([y, c], capi.Tensor(ctx, n, oh, ow, C)), "plan_run", "8-bit")                               # a float tensor as the output
    _refused(lambda: plan.run([y, c], capi.Tensor(ctx, n, oh, ow, C, dtype=capi.U16)), "plan_run")                       # a 16-bit output
    wide = mk(ctx, n, h, w, oh, ow, C, "cbcr", capi.U16, 1023, 6)
    _refused(lambda: wide.run([y, c], capi.Tensor(ctx, n, oh, ow, C, dtype=capi.U16)), "plan_run", "8-bit")              # 8-bit planes into a 16-bit plan
    planar = mk(ctx, n, h, w, oh, ow, C, "planar")
    _refused(lambda: planar.run([y, c], out), "rgb_fit", "the chroma source is", "src=planar")                            # a CbCr plane into a planar plan
    R.compare(out.numpy_u8(), R.video_values(yfit, cbcr), 255, 0)  # nothing above touched the valid result


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, checked by snnhip_sync) is fixed at the library's first allocation: a child
    process, started the way tests/test_frame_fit_gpu.py starts its own, runs the sweep once -- every source, C, depth, siting and range on the three
    smallest shapes and the two tile-derived ones.  Valid shapes only: no SNNHIP_E_GUARD may come back."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_frame_rgb_fit_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for c in (3, 4):
            for source in ("cbcr", "planar"):
                for container, maxval, shift in T.DEPTHS:
                    shapes = T.shapes_for(ctx, source, c, container, maxval, shift)
                    T.video_sweep(ctx, source, c, container, maxval, shift, shapes[:3] + shapes[-2:])
                    ctx.sync()                           # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write
            shapes = T.shapes_for(ctx, "rgb", c, "u8", 255, 0)
            T.rgb_sweep(ctx, c, shapes[:3] + shapes[-2:])
            ctx.sync()
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]
