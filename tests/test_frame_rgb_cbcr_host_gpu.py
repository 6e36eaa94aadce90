"""RGB8 / RGBA8 frames in, NV12 frames out through the C++ host mirror (snn_model_create10, host.Model(colour=..., video_out="NV12")): ESPCN at x2 /
x3 on a 32 x 48 frame.  The luma plane that comes back is byte for byte what the same model built with R8 frames at both ends and the range's maps
makes of the frame's rgb_luma plane; the chroma plane is byte for byte what the C-ABI plan (snnhip_rgb_cbcr_plan_create) makes of the same frame: the
same kernels on the same bytes.  The plan itself is held to the float64 reference in tests/test_frame_rgb_cbcr_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import rgb_cbcr_ref as R

pytestmark = pytest.mark.gpu
H, W = 32, 48


def _luma_maps(rng):
    """the model's maps as include/snn_c.h states them for snn_model_create10"""
    scale, off = (219.0, 16.0) if rng == "limited" else (255.0, 0.0)
    return dict(in_means=(0.0,) * 4, in_norms=(1.0 / 255.0,) * 4, out_scale=(scale,) * 4, out_offset=(off,) * 4)


def _json(tmp_path, r):
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r)
    return models.write_json(net, W, H, str(tmp_path / (net["name"] + ".json")))


def _plan_luma(ctx, rgb, kr, kb):
    from shadernn_amd import capi

    n, h, w, c = rgb.shape
    plan = capi.rgb_luma_plan(ctx, n, h, w, c, kr, kb)
    out = capi.Tensor(ctx, n, h, w, 1, dtype=capi.U8)
    plan.run([capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8)], out)
    got = out.numpy_u8()
    plan.destroy()
    return got


def _plan_cbcr(ctx, rgb, r, siting, rng, kr, kb):
    from shadernn_amd import capi

    n, h, w, c = rgb.shape
    plan = capi.rgb_cbcr_plan(ctx, n, h, w, c, r, siting, rng, kr, kb)
    out = capi.Tensor(ctx, n, r * h // 2, r * w // 2, 2, dtype=capi.U8)
    plan.run([capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8)], out)
    got = out.numpy_u8()
    plan.destroy()
    return got


def _run(m, frame, batch):
    m.upload_frame(frame if batch > 1 else frame[0])
    m.run()
    return m.download_frame()


def _check(ctx, path, colour, r, rng, batch=1, siting="left", kr=0.299, kb=0.114, seeds=(1,), **kw):
    from shadernn_amd import host

    channels = 4 if colour == "RGBA8" else 3
    m = host.Model(path, W, H, 1, batch=batch, colour=colour, video_out="NV12", video_range=rng, siting=siting, kr=kr, kb=kb, **kw)
    ref = host.Model(path, W, H, 1, batch=batch, input_format="R8", output_format="R8", **_luma_maps(rng), **kw)
    desc = m.describe()
    # four launches in all: rgb_luma, the two fused ESPCN kernels with the R8 ends folded in, exactly as the R8 model runs them, and rgb_cbcr
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert steps == [d for _, _, d, _, _ in ref.plan_steps()] and len(steps) == 2, steps
    first = [line for line in desc.split("\n") if line.startswith("[colour in]")]
    last = [line for line in desc.split("\n") if line.startswith("[chroma out]")]
    assert len(first) == 1 and len(last) == 1 and len(steps) + len(first) + len(last) == 4, desc
    assert "rgb_luma_u8 c=%d" % channels in first[0], desc
    assert "rgb_cbcr_u8 r=%d c=%d siting=%s range=%s" % (r, channels, siting, rng) in last[0] and "rgb_cbcr_kernel" in last[0], desc
    assert "ycc_merge" not in desc and "[colour out]" not in desc and "chroma_up" not in desc, desc
    outs = []
    for seed in seeds:
        frame = R.frame(seed, batch, H, W, channels)
        y, cbcr = _run(m, frame, batch)
        y, cbcr = y.reshape(batch, r * H, r * W), cbcr.reshape(batch, r * H // 2, r * W // 2, 2)
        assert y.dtype == np.uint8 and cbcr.dtype == np.uint8
        luma = _plan_luma(ctx, frame, kr, kb)
        ref.upload_frame(luma if batch > 1 else luma[0])
        ref.run()
        np.testing.assert_array_equal(y, ref.download_frame().reshape(batch, r * H, r * W))  # byte for byte
        np.testing.assert_array_equal(cbcr, _plan_cbcr(ctx, frame, r, siting, rng, kr, kb))
        outs.append((y, cbcr))
    m.close()
    ref.close()
    return outs


@pytest.mark.parametrize("rng", ["limited", "full"])
@pytest.mark.parametrize("colour", ["RGB8", "RGBA8"])
@pytest.mark.parametrize("r", [2, 3])
def test_rgb_in_nv12_out_around_espcn(ctx, tmp_path, r, colour, rng):
    path = _json(tmp_path, r)
    _check(ctx, path, colour, r, rng, seeds=(10 * r,))
    _check(ctx, path, colour, r, rng, siting="centre", kr=0.2126, kb=0.0722, seeds=(3,))


def test_the_two_ranges_differ_in_both_planes(ctx, tmp_path):
    path = _json(tmp_path, 2)
    (yl, cl), = _check(ctx, path, "RGB8", 2, "limited", seeds=(4,))
    (yf, cf), = _check(ctx, path, "RGB8", 2, "full", seeds=(4,))
    assert not np.array_equal(yl, yf) and not np.array_equal(cl, cf)
    assert yl.max() <= 235  # ESPCN ends in tanh: its output is at most 1, which the limited-range map sends to 16 + 219


def test_batch_2(ctx, tmp_path):
    for r in (2, 3):
        (y, cbcr), = _check(ctx, _json(tmp_path, r), "RGB8", r, "limited", batch=2, seeds=(7,))
        assert not np.array_equal(y[0], y[1]) and not np.array_equal(cbcr[0], cbcr[1])


def test_a_captured_graph_holds_four_launches_and_reads_each_new_frame(ctx, tmp_path, monkeypatch):
    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "4")  # the four launches are just enough to record / replay
    from shadernn_amd import host

    r = 2
    path = _json(tmp_path, r)
    # the first run records, the others replay: each is compared with the plans on its own frame
    outs = _check(ctx, path, "RGBA8", r, "limited", seeds=(1, 2, 3), capture_graph=True)
    assert not np.array_equal(outs[0][1], outs[1][1]) and not np.array_equal(outs[1][0], outs[2][0])
    m = host.Model(path, W, H, 1, colour="RGB8", video_out="NV12", capture_graph=True)
    frame = R.frame(5, 1, H, W, 3)
    y0, c0 = _run(m, frame, 1)
    for _ in range(2):  # the replayed graph gives the bytes of the first run
        y, c = _run(m, frame, 1)
        np.testing.assert_array_equal(y, y0)
        np.testing.assert_array_equal(c, c0)
    m.close()
    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "5")  # one more than the inference has: launched directly, same bytes
    m = host.Model(path, W, H, 1, colour="RGB8", video_out="NV12", capture_graph=True)
    y, c = _run(m, frame, 1)
    np.testing.assert_array_equal(y, y0)
    np.testing.assert_array_equal(c, c0)
    m.close()


@pytest.fixture
def f16_rules():
    from shadernn_amd import capi

    capi.set_option("SNNHIP_ESPCN_F16", "1")
    yield
    capi.set_option("SNNHIP_ESPCN_F16", None)


def test_the_fp16_opt_in_works_too(ctx, tmp_path, f16_rules):
    """prefer_half with SNNHIP_ESPCN_F16=1: the fused fp16 chain between the same two extra launches"""
    path = _json(tmp_path, 2)
    (y, cbcr), = _check(ctx, path, "RGB8", 2, "limited", seeds=(8,), prefer_half=True)
    assert y.shape == (1, 2 * H, 2 * W)


def test_what_is_refused_with_a_device(ctx, tmp_path):
    from shadernn_amd import host, models

    path = _json(tmp_path, 2)
    h = C.c_void_p()

    def create10(p, in_c=1, fmt=3, out=0x201, w=W, hh=H):
        io = host.EncodeIO(fmt, out, 1, 0, 0.299, 0.114)
        return host.lib().snn_model_create10(p.encode(), 0, w, hh, in_c, 0, 1, 0, 0, 0, 1, C.byref(io), C.byref(h))

    three = models.write_json(models.single_conv(seed=1, ic=3, oc=3), W, H, str(tmp_path / "three.json"))
    assert create10(three, 3) == -1                                 # a three-channel model
    wide = models.write_json(models.single_conv(seed=1, ic=1, oc=16), W, H, str(tmp_path / "wide.json"))
    assert create10(wide, 1) == -1                                  # one channel in, sixteen out
    one = models.write_json(models.single_conv(seed=1, ic=1, oc=1), W, H, str(tmp_path / "one.json"))
    assert create10(one, 1) == -1                                   # r = 1: the chroma grid would be decimated
    x3 = models.write_json(models.espcn_weights(seed=1, scale=3), 47, H, str(tmp_path / "x3odd.json"))
    assert create10(x3, w=47) == -1                                 # r * in_w is odd: no 4:2:0 plane
    x3h = models.write_json(models.espcn_weights(seed=1, scale=3), W, 31, str(tmp_path / "x3oddh.json"))
    assert create10(x3h, hh=31) == -1
    assert create10(path, out=3) == -1                              # an RGB8 output is snn_model_create7's
    assert h.value is None
    assert create10(path) == 0                                      # the process and the device are fine
    frame = R.frame(2, 1, H, W, 3)
    assert host.lib().snn_model_upload_frame_nv12(h, frame.ctypes.data_as(C.c_void_p)) == -1  # no NV12 frame at this model's input
    assert host.lib().snn_model_upload_frame_u8(h, frame.ctypes.data_as(C.c_void_p)) == 0
    assert host.lib().snn_model_run(h) == 0
    big = np.zeros(4 * H * W * 3, np.uint8)
    assert host.lib().snn_model_download_frame_u8(h, big.ctypes.data_as(C.c_void_p)) == -1   # the output is an NV12 frame
    assert host.lib().snn_model_download_frame_u16(h, big.ctypes.data_as(C.c_void_p)) == -1
    assert not big.any()
    assert host.lib().snn_model_download_frame_nv12(h, big.ctypes.data_as(C.c_void_p)) == 0
    assert big[:2 * H * 2 * W * 3 // 2].any() and not big[2 * H * 2 * W * 3 // 2:].any()      # rH*rW + (rH/2)*rW bytes, no more
    assert host.lib().snn_model_destroy(h) == 0
    with pytest.raises(AssertionError):                             # the same through host.Model
        host.Model(one, W, H, 1, colour="RGB8", video_out="NV12")
