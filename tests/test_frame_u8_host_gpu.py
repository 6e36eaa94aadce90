"""8-bit frames through the C++ host mirror (snn_model_create5 / host.Model(input_format=, output_format=)): the conversions join the stage
graph, fold into the fused ESPCN kernels, and the frames equal the float model's output quantised by the u8_out contract."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEMO = dict(in_means=(127.5, 127.5, 127.5, 0), in_norms=(1 / 127.5, 1 / 127.5, 1 / 127.5, 1), out_scale=(127.5, 127.5, 127.5, 1), out_offset=(127.5, 127.5, 127.5, 0))


def _json(tmp_path, net, w, h):
    from shadernn_amd import models

    return models.write_json(net, w, h, str(tmp_path / (net["name"] + ".json")))


def _q(x, scale, offset):
    C = x.shape[-1]
    s = np.asarray(scale[:C], np.float32).astype(np.float64)
    o = np.asarray(offset[:C], np.float32).astype(np.float64)
    y = np.rint((x.astype(np.float64) * s + o).astype(np.float32))  # (powers of two times small floats: the float64 sum is exact)
    return np.where(np.isnan(y), 0.0, np.clip(y, 0.0, 255.0)).astype(np.uint8)


def _expected(float_model, u, io):
    C = u.shape[-1]
    x = (u.astype(np.float32) - np.float32(io["in_means"][:C])) * np.float32(io["in_norms"][:C])
    return _q(float_model(x), io["out_scale"], io["out_offset"])


@pytest.mark.parametrize("capture", [False, True])
def test_espcn_r8_frames_in_and_out(ctx, tmp_path, monkeypatch, capture):
    from shadernn_amd import host, models

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the two-launch ESPCN inference
    H, W = 45, 67
    path = _json(tmp_path, models.espcn_weights(seed=1), W, H)
    m = host.Model(path, W, H, 1, capture_graph=capture, input_format="R8", output_format="R8", **DEMO)
    ref = host.Model(path, W, H, 1)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert len(steps) == 2, steps
    assert "conv_kxk_c1o16_wino3x3_c16o16_u8_kernel" in steps[0] and "conv3x3_c16o4_d2s_tanh_u8_kernel" in steps[1], steps
    rng = np.random.default_rng(3)
    for _ in range(4):  # several frames in a row: a replayed graph must read the new frame
        u = rng.integers(0, 256, size=(H, W, 1), dtype=np.uint8)
        m.upload_frame(u)
        m.run()
        got = m.output_frame()
        assert got.dtype == np.uint8 and got.shape == (2 * H, 2 * W, 1)
        np.testing.assert_array_equal(got, _expected(ref, u, DEMO))


def test_espcn_r8_batch4(ctx, tmp_path):
    from shadernn_amd import host, models

    H, W, B = 19, 33, 4
    path = _json(tmp_path, models.espcn_weights(seed=2), W, H)
    io = dict(in_means=(0, 0, 0, 0), in_norms=(1 / 255.0, 1, 1, 1), out_scale=(255.0, 1, 1, 1), out_offset=(0, 0, 0, 0))
    m = host.Model(path, W, H, 1, batch=B, input_format="R8", output_format="R8", **io)
    ref = host.Model(path, W, H, 1, batch=B)
    u = np.random.default_rng(4).integers(0, 256, size=(B, H, W, 1), dtype=np.uint8)
    m.upload_frame(u)
    m.run()
    np.testing.assert_array_equal(m.output_frame(), _expected(ref, u, io))


def test_espcn_r8_prefer_half_runs_the_conversions_unfused(ctx, tmp_path):
    from shadernn_amd import host, models

    H, W = 24, 40
    path = _json(tmp_path, models.espcn_weights(seed=1), W, H)
    m = host.Model(path, W, H, 1, prefer_half=True, input_format="R8", output_format="R8", **DEMO)
    ref = host.Model(path, W, H, 1, prefer_half=True)
    assert not any("u8_kernel" in d for _, _, d, _, _ in m.plan_steps())
    u = np.random.default_rng(5).integers(0, 256, size=(H, W, 1), dtype=np.uint8)
    m.upload_frame(u)
    m.run()
    np.testing.assert_array_equal(m.output_frame(), _expected(ref, u, DEMO))


@pytest.mark.parametrize("fuse", [True, False])
def test_rgb8_single_conv(ctx, tmp_path, fuse):
    from shadernn_amd import host, models

    H, W = 17, 29
    net = models.single_conv(seed=3, ic=3, oc=3, k=3, act="tanh")
    path = _json(tmp_path, net, W, H)
    m = host.Model(path, W, H, 3, fuse_chains=fuse, input_format="RGB8", output_format="RGB8", **DEMO)
    ref = host.Model(path, W, H, 3, fuse_chains=fuse)
    u = np.random.default_rng(6).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    m.upload_frame(u)
    m.run()
    np.testing.assert_array_equal(m.output_frame(), _expected(ref, u, DEMO))


def test_frame_format_must_match_the_channel_count(ctx, tmp_path):
    from shadernn_amd import host, models

    path = _json(tmp_path, models.espcn_weights(seed=1), 16, 16)
    with pytest.raises(AssertionError):
        host.Model(path, 16, 16, 1, input_format="RGB8")
