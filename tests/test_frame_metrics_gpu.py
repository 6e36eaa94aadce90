"""The frame-metrics plan through the C-ABI (include/snnhip.h, snnhip_frame_metrics_plan_create / _read) against tests/metrics_ref.py.

What is asserted, for every case: sse, pixels and windows equal the reference EXACTLY (they are integers); |ssim - ssim_ref| <= 1e-9 -- the terms lie
in [-1, 1], adding at most 10^4 of them in any order differs by at most about n * 2^-52 = 2e-12, plus a few ulps per term: 1e-9 sits three orders above
that and six below any error of meaning; the fp32 output tensor equals float32 of the double results of the rows (inf allowed).

Shapes, with T the tile of the tile kernel (capi.FRAME_METRICS_TILE): 8x8 (one window), 9x11 (a ragged tail that counts in SSE only), 37x53,
(T_h + 4) x (T_w + 4) (one window past the tile on each axis), (2 T_h + 5) x (2 T_w + 7) with two different images (image mixing, windows that
straddle four tiles), and (2 T_h + 8) x (2 T_w + 8) with two images: the same seams with every row aligned, so that the wide-load path crosses them
too (the odd widths above take the element path)."""
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SHAPE_IDS = ["8x8", "9x11", "37x53", "tile+4", "2tile+5x7", "2tile+8"]
FORMATS = [("u8", 255, 0), ("u16", 1023, 0), ("u16", 1023, 6), ("u16", 4095, 4), ("u16", 65535, 0)]
FORMAT_IDS = ["u8", "u16-1023", "u16-1023<<6", "u16-4095<<4", "u16-65535"]
SENTINEL = -7.25


def shape(label):
    """(N, H, W) of a shape label"""
    from shadernn_amd import capi

    th, tw = capi.FRAME_METRICS_TILE
    return {"8x8": (1, 8, 8), "9x11": (1, 9, 11), "37x53": (1, 37, 53), "tile+4": (1, th + 4, tw + 4), "2tile+5x7": (2, 2 * th + 5, 2 * tw + 7),
            "2tile+8": (2, 2 * th + 8, 2 * tw + 8)}[label]


def frames(n, h, w, c, container, maxval, shift, seed):
    """(test, reference) containers [N][H][W][C]: a smooth-plus-noise reference, the test frame a different distortion of it per channel and image
    (noise of growing strength, a gain on odd channels, an offset on the second image); random bits below `shift` in BOTH frames."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ref = np.empty((n, h, w, c), np.float64)
    test = np.empty_like(ref)
    for i in range(n):
        for k in range(c):
            base = 0.5 + 0.3 * np.sin(0.11 * (k + 1) * xx + i) * np.cos(0.07 * yy + k) + 0.15 * rng.standard_normal((h, w))
            ref[i, :, :, k] = base
            gain = 0.9 if k % 2 else 1.0
            test[i, :, :, k] = gain * base + 0.02 * (k + 1) * rng.standard_normal((h, w)) + 0.03 * i
    dt = np.uint8 if container == "u8" else np.uint16
    out = []
    for v in (test, ref):
        q = np.clip(np.rint(v * maxval), 0, maxval).astype(np.int64) << shift
        if shift:
            q |= rng.integers(0, 1 << shift, q.shape)
        out.append(q.astype(dt))
    return out[0], out[1]


def dtype_of(a):
    from shadernn_amd import capi

    return capi.U8 if a.dtype == np.uint8 else capi.U16


def run_plan(ctx, plan, a, b, out=None):
    """runs `plan` on the containers a, b into a sentinel-filled output; returns (rows, the fp32 output [N][1][C][2], the output tensor)"""
    from shadernn_amd import capi

    n, _, _, c = a.shape
    ta, tb = capi.Tensor.from_numpy(ctx, a, dtype=dtype_of(a)), capi.Tensor.from_numpy(ctx, b, dtype=dtype_of(b))
    if out is None:
        out = capi.Tensor(ctx, n, 1, c, 2)
    out.upload(np.full((n, 1, c, 2), SENTINEL, np.float32))
    plan.run([ta, tb], out)
    rows = capi.frame_metrics_read(plan)
    got = out.numpy()
    ta.free()
    tb.free()
    return rows, got, out


def check(rows, got, a, b, maxval, shift, label=""):
    """the device's rows and fp32 output against the reference; prints each figure before it asserts"""
    from shadernn_amd import capi

    n, _, _, c = a.shape
    ref = R.frame_metrics(a, b, maxval, shift)
    assert len(rows) == len(ref) == n * c
    for i, (r, e) in enumerate(zip(rows, ref)):
        img, ch = divmod(i, c)
        print("%s n=%d c=%d: sse %d (ref %d) windows %d ssim %.15f (ref %.15f, diff %.2e) psnr %.6f" %
              (label, img, ch, r["sse"], e["sse"], r["windows"], r["ssim"], e["ssim"], abs(r["ssim"] - e["ssim"]), e["psnr_db"]))
        assert r["sse"] == e["sse"] and r["pixels"] == e["pixels"] and r["windows"] == e["windows"], (label, i, r, e)
        assert abs(r["ssim"] - e["ssim"]) <= 1e-9, (label, i, r["ssim"], e["ssim"])
        psnr = capi.frame_metrics_psnr(r["sse"], r["pixels"], maxval)
        assert psnr == e["psnr_db"] or abs(psnr - e["psnr_db"]) <= 1e-12 * abs(e["psnr_db"]), (psnr, e["psnr_db"])
        assert got[img, 0, ch, 0] == np.float32(psnr), (label, i, got[img, 0, ch, 0], psnr)
        assert got[img, 0, ch, 1] == np.float32(r["ssim_sum"] / r["windows"]), (label, i, got[img, 0, ch, 1], r["ssim"])
    assert not np.any(got == np.float32(SENTINEL)), got
    return ref


def measure(ctx, a, b, maxval, shift, label=""):
    from shadernn_amd import capi

    n, h, w, c = a.shape
    plan = capi.frame_metrics_plan(ctx, n, h, w, c, dtype_of(a), maxval, shift)
    rows, got, out = run_plan(ctx, plan, a, b)
    out.free()
    plan.destroy()
    return check(rows, got, a, b, maxval, shift, label)


@pytest.mark.parametrize("label", SHAPE_IDS)
def test_u8_luma_matches_the_reference(ctx, label):
    n, h, w = shape(label)
    a, b = frames(n, h, w, 1, "u8", 255, 0, seed=h * 1000 + w)
    ref = measure(ctx, a, b, 255, 0, label)
    assert ref[0]["windows"] == ((h >> 2) - 1) * ((w >> 2) - 1) and ref[0]["pixels"] == h * w
    assert all(0 < r["sse"] and r["ssim"] < 1.0 for r in ref)
    if n == 2:
        assert ref[0]["sse"] != ref[1]["sse"]  # the two images differ: mixing them would show


@pytest.mark.parametrize("c", [2, 3, 4])
@pytest.mark.parametrize("label", ["9x11", "37x53", "tile+4", "2tile+5x7", "2tile+8"])
def test_interleaved_channels_stay_apart(ctx, label, c):
    n, h, w = shape(label)
    a, b = frames(n, h, w, c, "u8", 255, 0, seed=h * 100 + w + c)
    ref = measure(ctx, a, b, 255, 0, "%s c=%d" % (label, c))
    assert len({r["sse"] for r in ref}) == len(ref)  # a different distortion per channel and image: every row is its own


@pytest.mark.parametrize("fmt", FORMATS[1:], ids=FORMAT_IDS[1:])
@pytest.mark.parametrize("label", ["8x8", "9x11", "37x53", "tile+4", "2tile+5x7", "2tile+8"])
def test_16_bit_containers(ctx, label, fmt):
    container, maxval, shift = fmt
    n, h, w = shape(label)
    for c in ((1, 2, 3, 4) if label in ("9x11", "2tile+5x7", "2tile+8") else (1, 3)):
        a, b = frames(n, h, w, c, container, maxval, shift, seed=h + w + c + maxval)
        measure(ctx, a, b, maxval, shift, "%s %s c=%d" % (label, FORMAT_IDS[FORMATS.index(fmt)], c))


def test_bits_below_the_shift_are_ignored(ctx):
    n, h, w = shape("37x53")
    a, b = frames(n, h, w, 2, "u16", 1023, 6, seed=5)
    assert np.any(a & 63) and np.any(b & 63)
    ref = measure(ctx, a, b, 1023, 6, "low bits")
    clean = R.frame_metrics(a & 0xFFC0, b & 0xFFC0, 1023, 6)
    assert [r["sse"] for r in ref] == [r["sse"] for r in clean] and [r["ssim"] for r in ref] == [r["ssim"] for r in clean]


@pytest.mark.parametrize("label", ["9x11", "2tile+5x7", "2tile+8"])
def test_all_zero_against_all_maxval_at_16_bits(ctx, label):
    """every moment at its largest: 32-bit block moments or a 32-bit SSE would wrap (16 * 65535^2 > 2^32)"""
    n, h, w = shape(label)
    for c in (1, 4):
        a = np.zeros((n, h, w, c), np.uint16)
        b = np.full((n, h, w, c), 65535, np.uint16)
        ref = measure(ctx, a, b, 65535, 0, "zero/max " + label)
        assert ref[0]["sse"] == 65535 * 65535 * h * w and ref[0]["sse"] > 1 << 32
        ref = measure(ctx, b, b, 65535, 0, "max/max " + label)
        assert ref[0]["sse"] == 0 and ref[0]["ssim"] == 1.0


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_identical_frames_give_zero_inf_and_exactly_one(ctx, fmt):
    from shadernn_amd import capi

    container, maxval, shift = fmt
    for label in ("9x11", "2tile+5x7", "2tile+8"):
        n, h, w = shape(label)
        _, b = frames(n, h, w, 3, container, maxval, shift, seed=11)
        plan = capi.frame_metrics_plan(ctx, n, h, w, 3, dtype_of(b), maxval, shift)
        rows, got, out = run_plan(ctx, plan, b, b)
        for r in rows:
            assert r["sse"] == 0 and r["ssim_sum"] == float(r["windows"]) and r["ssim"] == 1.0, r
        assert np.all(np.isposinf(got[:, 0, :, 0])) and np.all(got[:, 0, :, 1] == np.float32(1.0)), got
        out.free()
        plan.destroy()


def test_a_second_run_carries_nothing_of_the_first_and_repeats_bit_for_bit(ctx):
    from shadernn_amd import capi

    n, h, w = shape("2tile+5x7")
    c = 3
    plan = capi.frame_metrics_plan(ctx, n, h, w, c)
    a1, b1 = frames(n, h, w, c, "u8", 255, 0, seed=1)
    a2, b2 = frames(n, h, w, c, "u8", 255, 0, seed=2)
    rows1, got1, out = run_plan(ctx, plan, a1, b1)
    check(rows1, got1, a1, b1, 255, 0, "first")
    rows2, got2, _ = run_plan(ctx, plan, a2, b2, out)  # the same plan and output tensor, sentinel-filled again
    check(rows2, got2, a2, b2, 255, 0, "second")
    assert [r["sse"] for r in rows1] != [r["sse"] for r in rows2]
    rows3, got3, _ = run_plan(ctx, plan, a2, b2, out)
    assert rows3 == rows2 and got3.tobytes() == got2.tobytes()  # no atomics, a fixed order: bit-identical from run to run
    out.free()
    plan.destroy()


def test_the_plan_replays_from_a_recorded_graph_behind_another_plan(ctx):
    """chroma_up at r = 1 (a copy that clears nothing at 8 bits) produces the test frame, the metrics plan reads it: both recorded, replayed twice
    with different sources"""
    from shadernn_amd import capi

    n, h, w = shape("tile+4")
    c = 2
    a1, b = frames(n, h, w, c, "u8", 255, 0, seed=21)
    a2, _ = frames(n, h, w, c, "u8", 255, 0, seed=22)
    copy = capi.chroma_up_plan(ctx, n, h, w, c, 1)
    plan = capi.frame_metrics_plan(ctx, n, h, w, c)
    src = capi.Tensor.from_numpy(ctx, a1, dtype=capi.U8)
    mid = capi.Tensor(ctx, n, h, w, c, dtype=capi.U8)
    tb = capi.Tensor.from_numpy(ctx, b, dtype=capi.U8)
    out = capi.Tensor(ctx, n, 1, c, 2)
    with capi.Graph.capture(ctx) as g:
        copy.run(src, mid)
        plan.run([mid, tb], out)
    assert g.num_nodes() >= 3, g.num_nodes()  # the copy and the two metrics launches
    for a in (a1, a2):
        src.upload_u8(a)
        out.upload(np.full((n, 1, c, 2), SENTINEL, np.float32))
        g.launch()
        rows = capi.frame_metrics_read(plan)
        check(rows, out.numpy(), a, b, 255, 0, "replay")
    g.destroy()
    for t in (src, mid, tb, out):
        t.free()
    copy.destroy()
    plan.destroy()


def test_describe_cost_and_trace_name_both_kernels(ctx):
    from shadernn_amd import capi

    th, tw = capi.FRAME_METRICS_TILE
    n, h, w = shape("2tile+5x7")
    plan = capi.frame_metrics_plan(ctx, n, h, w, 3)
    desc = plan.describe()
    assert desc.startswith("frame_metrics_u8 c=3 tile=%dx%d " % (th, tw)) and "frame_metrics_tile_kernel" in desc and "frame_metrics_fold_kernel" in desc, desc
    assert plan.out_shape() == (n, 1, 3, 2)
    tiles = -(-h // th) * -(-w // tw)
    assert plan.cost()[1] == 2 * n * h * w * 3 + 2 * n * 3 * tiles * 16  # both frames once, the partials written and read
    a, b = frames(n, h, w, 3, "u8", 255, 0, seed=3)
    capi.trace_begin()
    rows, got, out = run_plan(ctx, plan, a, b)
    text = str(capi.trace_end())
    assert "frame_metrics_tile_kernel" in text and "frame_metrics_fold_kernel" in text, text
    check(rows, got, a, b, 255, 0, "traced")
    out.free()
    plan.destroy()


def _refused(fn, *needles):
    from shadernn_amd import capi

    with pytest.raises(capi.SnnHipError) as e:
        fn()
    assert e.value.code == capi.E_INVALID, str(e.value)
    msg = str(e.value)
    assert all(s in msg for s in needles), msg


def test_refusals_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    mk = capi.frame_metrics_plan
    start = "snnhip error -1: frame_metrics"
    _refused(lambda: mk(ctx, 1, 16, 16, 0), start, "0 channels")
    _refused(lambda: mk(ctx, 1, 16, 16, 5), start, "5 channels")
    _refused(lambda: mk(ctx, 1, 16, 16, 1, capi.F32), start, "dtype 0")
    _refused(lambda: mk(ctx, 1, 16, 16, 1, capi.F16), start, "dtype 1")
    _refused(lambda: mk(ctx, 1, 7, 16, 1), start, "7x16")
    _refused(lambda: mk(ctx, 1, 16, 7, 1), start, "16x7")
    _refused(lambda: mk(ctx, 0, 16, 16, 1), start, "batch")
    _refused(lambda: mk(ctx, 1, 16, 16, 1, capi.U8, 256, 0), start, "maxval 256")
    _refused(lambda: mk(ctx, 1, 16, 16, 1, capi.U8, 127, 1), start, "shift 1")
    _refused(lambda: mk(ctx, 1, 16, 16, 1, capi.U16, 1023, 7), start, "does not fit")
    _refused(lambda: mk(ctx, 1, 16, 16, 1, capi.U16, 1023, 16), start, "shift 16")
    _refused(lambda: mk(ctx, 1, 16, 16, 1, capi.U16, 0, 0), start, "maxval 0")
    _refused(lambda: mk(ctx, 1, 16, 16, 1, capi.U16, 65536, 0), start, "does not fit")
    mk(ctx, 1, 16, 16, 1, capi.U16, 65535, 0).destroy()  # the extension past chroma_up's 4095

    n, h, w, c = 1, 12, 20, 2
    plan = mk(ctx, n, h, w, c)
    a, b = frames(n, h, w, c, "u8", 255, 0, seed=9)
    ta, tb = capi.Tensor.from_numpy(ctx, a, dtype=capi.U8), capi.Tensor.from_numpy(ctx, b, dtype=capi.U8)
    out = capi.Tensor(ctx, n, 1, c, 2)
    out.upload(np.full((n, 1, c, 2), SENTINEL, np.float32))
    plan.run([ta, tb], out)  # the valid call
    for bad in ((n, h + 1, w, c), (n, h, w + 1, c), (n, h, w, 1), (2, h, w, c)):
        _refused(lambda: plan.run([capi.Tensor(ctx, *bad, dtype=capi.U8), tb], out), "frame_metrics: input 0 is")
        _refused(lambda: plan.run([ta, capi.Tensor(ctx, *bad, dtype=capi.U8)], out), "frame_metrics: input 1 is")
    _refused(lambda: plan.run([capi.Tensor(ctx, n, h, w, c), tb], out), "frame_metrics: input 0 has dtype 0")
    _refused(lambda: plan.run([ta, capi.Tensor(ctx, n, h, w, c, dtype=capi.F16)], out), "frame_metrics: input 1 has dtype 1")
    _refused(lambda: plan.run([ta, capi.Tensor(ctx, n, h, w, c, dtype=capi.U16)], out), "plan_run", "16-bit")  # a 16-bit frame into an 8-bit plan
    _refused(lambda: plan.run(ta, out), "frame_metrics: expects 2 inputs")
    for bad in ((n, 1, c, 1), (n, 2, c, 2), (n, 1, c + 1, 2), (2, 1, c, 2)):
        _refused(lambda: plan.run([ta, tb], capi.Tensor(ctx, *bad)), "frame_metrics: the output is")
    _refused(lambda: plan.run([ta, tb], capi.Tensor(ctx, n, 1, c, 2, dtype=capi.F16)), "frame_metrics: the output is")
    _refused(lambda: plan.run([ta, tb], capi.Tensor(ctx, n, 1, c, 2, dtype=capi.U8)), "plan_run", "8-bit")
    with pytest.raises(capi.SnnHipError) as e:
        capi.frame_metrics_read(plan, max_rows=n * c - 1)
    assert "frame_metrics_read" in str(e.value) and e.value.code == capi.E_INVALID
    with pytest.raises(capi.SnnHipError) as e:
        capi.frame_metrics_read(capi.chroma_up_plan(ctx, 1, 8, 8, 1, 1))
    assert "not a frame_metrics plan" in str(e.value)
    check(capi.frame_metrics_read(plan), out.numpy(), a, b, 255, 0, "after refusals")  # nothing above touched the valid result


def guard_sweep(ctx):
    """what the guard child runs: every container and channel count on the ragged, the seam and the aligned seam shape"""
    for container, maxval, shift in FORMATS:
        for label in ("9x11", "tile+4", "2tile+5x7", "2tile+8"):
            n, h, w = shape(label)
            for c in (1, 2, 3, 4):
                a, b = frames(n, h, w, c, container, maxval, shift, seed=c)
                measure(ctx, a, b, maxval, shift, "guard")
        ctx.sync()  # verifies every red zone: raises SnnHipError(E_GUARD) on a stray write


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 (red zones around every device allocation, fresh scratch poisoned with 0xFF, checked by snnhip_sync) is fixed at the library's
    first allocation: a child process, started the way tests/test_frame_fit_gpu.py starts its own.  Poisoned partials that a block failed to write
    would show in the sums."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_frame_metrics_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        T.guard_sweep(ctx)
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]


def test_psnr_of_the_output_is_finite_and_sane(ctx):
    """a frame one grey level off everywhere: sse = pixels, psnr = 20 log10(255) = 48.13 dB"""
    n, h, w = shape("37x53")
    b = np.full((n, h, w, 1), 100, np.uint8)
    ref = measure(ctx, b + 1, b, 255, 0, "one off")
    assert ref[0]["sse"] == h * w and abs(ref[0]["psnr_db"] - 20 * math.log10(255)) < 1e-12
