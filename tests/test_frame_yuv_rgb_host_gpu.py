"""NV12 / P010 frames in, RGB frames out through the C++ host mirror (snn_model_create9, host.Model(video=..., video_out=...)): ESPCN at x2 / x3 on
a 32 x 48 luma frame.  The RGB frame that comes back is byte for byte what the C-ABI plan (snnhip_yuv_rgb_plan_create) makes of the luma plane
returned by the same model built with video= alone (snn_model_create8, the range's luma maps passed by hand) and the original chroma plane: the
same kernels on the same bytes.  The plan itself is held to the float64 reference in tests/test_frame_yuv_rgb_gpu.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
H, W = 32, 48  # the luma plane; the chroma plane is 16 x 24

VIDEO = {
    "NV12": dict(maxval=255, shift=0, dtype=np.uint8, outs=("RGB8", "RGBA8")),
    "P010": dict(maxval=1023, shift=6, dtype=np.uint16, outs=("RGB16", "RGBA16")),
}


def _luma_maps(maxval, rng):
    """the luma plane's maps as include/snn_c.h states them for snn_model_create9"""
    k = (maxval + 1) / 256.0
    off, span = (16.0 * k, 219.0 * k) if rng == "limited" else (0.0, float(maxval))
    return dict(in_means=(off,) * 4, in_norms=(1.0 / span,) * 4, out_scale=(span,) * 4, out_offset=(off,) * 4)


def _json(tmp_path, r):
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r)
    return models.write_json(net, W, H, str(tmp_path / (net["name"] + ".json")))


def _frame(video, batch, seed):
    v = VIDEO[video]
    k = (v["maxval"] + 1) // 256
    rng = np.random.default_rng(seed)
    y = (rng.integers(16 * k, 236 * k, size=(batch, H, W)) << v["shift"]).astype(v["dtype"])
    cbcr = (rng.integers(16 * k, 241 * k, size=(batch, H // 2, W // 2, 2)) << v["shift"]).astype(v["dtype"])
    return y, cbcr


def _plan_rgb(ctx, yhi, cbcr, r, channels, video, siting, rng, kr, kb):
    """the C-ABI plan on a luma plane [n][rH][rW] and the original chroma plane"""
    from shadernn_amd import capi

    v = VIDEO[video]
    dt = capi.U8 if video == "NV12" else capi.U16
    n = yhi.shape[0]
    plan = capi.yuv_rgb_plan(ctx, n, H // 2, W // 2, channels, r, dt, v["maxval"], v["shift"], siting, rng, kr, kb)
    out = capi.Tensor(ctx, n, r * H, r * W, channels, dtype=dt)
    plan.run([capi.Tensor.from_numpy(ctx, np.ascontiguousarray(yhi[..., None]), dtype=dt), capi.Tensor.from_numpy(ctx, cbcr, dtype=dt)], out)
    got = out.numpy_u8() if video == "NV12" else out.numpy_u16()
    plan.destroy()
    return got


def _run(m, frame, batch):
    y, cbcr = frame
    m.upload_frame((y, cbcr) if batch > 1 else (y[0], cbcr[0]))
    m.run()
    return m.download_frame()


def _check(ctx, path, video, video_out, r, rng, batch=1, siting="left", kr=0.299, kb=0.114, seeds=(1,), **kw):
    from shadernn_amd import host

    v = VIDEO[video]
    channels = 4 if "A" in video_out else 3
    m = host.Model(path, W, H, 1, batch=batch, video=video, video_out=video_out, video_range=rng, siting=siting, kr=kr, kb=kb, **kw)
    ref = host.Model(path, W, H, 1, batch=batch, video=video, siting=siting, **_luma_maps(v["maxval"], rng))
    desc = m.describe()
    # three launches in all: the two fused ESPCN kernels with the frame ends folded in, exactly as the NV12 -> NV12 model runs them, and the RGB launch
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert steps == [d for _, _, d, _, _ in ref.plan_steps()] and len(steps) == 2, steps
    extra = [line for line in desc.split("\n") if line.startswith("[rgb out]")]
    assert len(extra) == 1 and len(steps) + len(extra) == 3, desc
    assert "yuv_rgb_%s r=%d c=%d siting=%s range=%s" % ("u8" if video == "NV12" else "u16", r, channels, siting, rng) in extra[0] and "yuv_rgb_kernel" in extra[0], desc
    assert "chroma_up" not in desc and "[chroma out]" not in desc, desc
    outs = []
    for seed in seeds:
        frame = _frame(video, batch, seed)
        got = _run(m, frame, batch).reshape(batch, r * H, r * W, channels)
        assert got.dtype == v["dtype"]
        yhi = _run(ref, frame, batch)[0].reshape(batch, r * H, r * W)
        want = _plan_rgb(ctx, yhi, frame[1], r, channels, video, siting, rng, kr, kb)
        np.testing.assert_array_equal(got, want)  # byte for byte
        if channels == 4:
            assert (got[..., 3] == v["maxval"] << v["shift"]).all()
        outs.append(got)
    m.close()
    ref.close()
    return outs


@pytest.mark.parametrize("rng", ["limited", "full"])
@pytest.mark.parametrize("video", ["NV12", "P010"])
@pytest.mark.parametrize("r", [2, 3])
def test_video_in_rgb_out_around_espcn(ctx, tmp_path, r, video, rng):
    path = _json(tmp_path, r)
    for video_out in VIDEO[video]["outs"]:
        _check(ctx, path, video, video_out, r, rng, seeds=(10 * r,))
    _check(ctx, path, video, VIDEO[video]["outs"][0], r, rng, siting="centre", kr=0.2126, kb=0.0722, seeds=(3,))


@pytest.mark.parametrize("video", ["NV12", "P010"])
def test_batch_2(ctx, tmp_path, video):
    for r in (2, 3):
        _check(ctx, _json(tmp_path, r), video, VIDEO[video]["outs"][0], r, "limited", batch=2, seeds=(7,))


@pytest.mark.parametrize("video", ["NV12", "P010"])
def test_a_captured_graph_replays_the_same_bytes_and_reads_each_new_frame(ctx, tmp_path, monkeypatch, video):
    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the three-launch inference
    from shadernn_amd import host

    r = 2
    path = _json(tmp_path, r)
    # the first run records, the others replay: each is compared with the plan on its own frame
    outs = _check(ctx, path, video, VIDEO[video]["outs"][1], r, "limited", seeds=(1, 2, 3), capture_graph=True)
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    m = host.Model(path, W, H, 1, video=video, video_out=VIDEO[video]["outs"][0], capture_graph=True)
    frame = _frame(video, 1, 5)
    first = _run(m, frame, 1)
    for _ in range(2):  # the replayed graph gives the bytes of the first run
        np.testing.assert_array_equal(_run(m, frame, 1), first)
    m.close()


@pytest.fixture
def f16_rules():
    from shadernn_amd import capi

    capi.set_option("SNNHIP_ESPCN_F16", "1")
    yield
    capi.set_option("SNNHIP_ESPCN_F16", None)


def test_the_fp16_opt_in_folds_the_ends_too(ctx, tmp_path, f16_rules):
    """prefer_half with SNNHIP_ESPCN_F16=1: the fused fp16 chain, still two launches with the frame ends folded in, and the RGB launch behind them"""
    from shadernn_amd import host

    path = _json(tmp_path, 2)
    m = host.Model(path, W, H, 1, video="NV12", video_out="RGB8", prefer_half=True)
    ref = host.Model(path, W, H, 1, video="NV12", prefer_half=True, **_luma_maps(255, "limited"))
    assert len(m.plan_steps()) == 2 and [d for _, _, d, _, _ in m.plan_steps()] == [d for _, _, d, _, _ in ref.plan_steps()], m.plan_steps()
    assert "[rgb out] yuv_rgb_u8" in m.describe() and "chroma_up" not in m.describe()
    frame = _frame("NV12", 1, 8)
    got = _run(m, frame, 1).reshape(1, 2 * H, 2 * W, 3)
    yhi = _run(ref, frame, 1)[0].reshape(1, 2 * H, 2 * W)
    np.testing.assert_array_equal(got, _plan_rgb(ctx, yhi, frame[1], 2, 3, "NV12", "left", "limited", 0.299, 0.114))
    m.close()
    ref.close()


def test_what_is_refused_with_a_device(ctx, tmp_path):
    from shadernn_amd import host, models

    path = _json(tmp_path, 2)
    h = C.c_void_p()

    def create9(p, in_c=1, fmt=0x201, out=3, w=W, hh=H):
        io = host.VideoRgbIO(fmt, out, 255, 0, 1, 0, 0.299, 0.114)
        return host.lib().snn_model_create9(p.encode(), 0, w, hh, in_c, 0, 1, 0, 0, 0, 1, C.byref(io), C.byref(h))

    three = models.write_json(models.single_conv(seed=1, ic=3, oc=3), W, H, str(tmp_path / "three.json"))
    assert create9(three, 3) == -1                                  # a three-channel model
    wide = models.write_json(models.single_conv(seed=1, ic=1, oc=16), W, H, str(tmp_path / "wide.json"))
    assert create9(wide, 1) == -1                                   # one channel in, sixteen out
    assert create9(path, out=0x103) == -1                           # an 8-bit input with a 16-bit output
    assert create9(path) == 0                                       # the process and the device are fine
    frame = np.zeros(H * W * 3 // 2, np.uint8)
    assert host.lib().snn_model_upload_frame_nv12(h, frame.ctypes.data_as(C.c_void_p)) == 0
    big = np.zeros(4 * H * W * 3, np.uint8)
    assert host.lib().snn_model_download_frame_nv12(h, big.ctypes.data_as(C.c_void_p)) == -1  # no NV12 frame at this model's output
    assert host.lib().snn_model_download_frame_u16(h, big.ctypes.data_as(C.c_void_p)) == -1   # ... and its RGB frame is 8-bit
    assert host.lib().snn_model_download_frame_u8(h, big.ctypes.data_as(C.c_void_p)) == 0
    assert host.lib().snn_model_destroy(h) == 0
