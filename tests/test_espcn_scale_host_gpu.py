"""ESPCN at upscale factors 3 and 4 through the C++ host mirror: JSON ("upscale" on the Subpixel lambda) -> host.Model, fp32 and 8-bit frames,
fused (two launches) and per-layer, prefer_half on the per-layer path, and the models the loader refuses."""
import copy
import json

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
DEMO = dict(in_means=(127.5, 127.5, 127.5, 0), in_norms=(1 / 127.5, 1 / 127.5, 1 / 127.5, 1), out_scale=(127.5, 127.5, 127.5, 1), out_offset=(127.5, 127.5, 127.5, 0))


def _json(tmp_path, net, w, h):
    from shadernn_amd import models

    return models.write_json(net, w, h, str(tmp_path / (net["name"] + ".json")))


def _oracle(net, x, **kw):
    r = int(net["layers"][-1].get("upscale", 2))
    return O.subpixel(O.forward(dict(net, layers=net["layers"][:-1]), x, **kw), r, 0)


def _q(x, scale, offset):  # the u8_out contract in numpy (tests/test_frame_u8_host_gpu.py)
    C = x.shape[-1]
    s = np.asarray(scale[:C], np.float32).astype(np.float64)
    o = np.asarray(offset[:C], np.float32).astype(np.float64)
    y = np.rint((x.astype(np.float64) * s + o).astype(np.float32))
    return np.where(np.isnan(y), 0.0, np.clip(y, 0.0, 255.0)).astype(np.uint8)


def _expected(float_model, u, io):
    C = u.shape[-1]
    x = (u.astype(np.float32) - np.float32(io["in_means"][:C])) * np.float32(io["in_norms"][:C])
    return _q(float_model(x), io["out_scale"], io["out_offset"])


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("r", [3, 4])
def test_json_model_fp32(ctx, tmp_path, r, fuse):
    from shadernn_amd import host, models

    H, W = 37, 70
    net = models.espcn_weights(seed=1, scale=r)
    m = host.Model(_json(tmp_path, net, W, H), W, H, 1, fuse_chains=fuse)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    if fuse:
        assert len(steps) == 2 and "conv3x3_c16oR_d2s_tanh_kernel<%d>" % r in steps[1] and "depth_to_space(%d)" % r in steps[1], steps
    else:
        assert len(steps) == 4 and "subpixel f=%d" % r in steps[3], steps
    x = np.random.default_rng(2).random((1, H, W, 1), dtype=np.float32)
    y = m(x)
    assert y.shape == (r * H, r * W, 1)
    np.testing.assert_allclose(y.reshape(-1), _oracle(net, x).reshape(-1), err_msg="; ".join(steps), **TOL)
    m.close()


@pytest.mark.parametrize("capture", [False, True])
@pytest.mark.parametrize("r,H,W", [(3, 45, 67), (3, 30, 68), (4, 45, 67)])  # (x3: a row pitch 3W that is not / is a multiple of 4 bytes)
def test_r8_frames_in_and_out(ctx, tmp_path, monkeypatch, r, H, W, capture):
    from shadernn_amd import host, models

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the two-launch inference
    path = _json(tmp_path, models.espcn_weights(seed=1, scale=r), W, H)
    m = host.Model(path, W, H, 1, capture_graph=capture, input_format="R8", output_format="R8", **DEMO)
    ref = host.Model(path, W, H, 1)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert len(steps) == 2, steps
    assert "conv_kxk_c1o16_wino3x3_c16o16_u8_kernel" in steps[0] and "conv3x3_c16oR_d2s_tanh_u8_kernel<%d>" % r in steps[1], steps
    rng = np.random.default_rng(3)
    for _ in range(4):  # several frames in a row: a replayed graph must read the new frame
        u = rng.integers(0, 256, size=(H, W, 1), dtype=np.uint8)
        m.upload_frame(u)
        m.run()
        got = m.output_frame()
        assert got.dtype == np.uint8 and got.shape == (r * H, r * W, 1)
        np.testing.assert_array_equal(got, _expected(ref, u, DEMO))


@pytest.mark.parametrize("r,W", [(3, 33), (3, 36), (4, 33)])
def test_r8_batch4(ctx, tmp_path, r, W):
    from shadernn_amd import host, models

    H, B = 19, 4
    path = _json(tmp_path, models.espcn_weights(seed=2, scale=r), W, H)
    io = dict(in_means=(0, 0, 0, 0), in_norms=(1 / 255.0, 1, 1, 1), out_scale=(255.0, 1, 1, 1), out_offset=(0, 0, 0, 0))
    m = host.Model(path, W, H, 1, batch=B, input_format="R8", output_format="R8", **io)
    ref = host.Model(path, W, H, 1, batch=B)
    u = np.random.default_rng(4).integers(0, 256, size=(B, H, W, 1), dtype=np.uint8)
    m.upload_frame(u)
    m.run()
    got = m.output_frame()
    assert got.shape == (B, r * H, r * W, 1)
    np.testing.assert_array_equal(got, _expected(ref, u, io))


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("r", [3, 4])
def test_prefer_half_runs_per_layer(ctx, tmp_path, r, fuse):
    """preferHp: half tensors end to end, the fp32-only fused rules step aside; the bounds of tests/test_fp16_gpu.py's x2 case."""
    from shadernn_amd import host, models

    net = models.espcn_weights(seed=1, scale=r)
    w, h = 48, 40
    m = host.Model(_json(tmp_path, net, w, h), w, h, 1, fuse_chains=fuse, prefer_half=True)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert not any("fused[" in d for d in steps) and any("subpixel f=%d" % r in d for d in steps), steps
    x = np.random.default_rng(8).random((1, h, w, 1), dtype=np.float32)
    y = m(x)
    assert y.shape == (r * h, r * w, 1)
    q = copy.deepcopy(net)
    trunc = np.vectorize(O.to_medium_precision, otypes=[np.float32])  # the parser truncates weights / bias to half
    for l in q["layers"]:
        for k in ("w", "b"):
            if l.get(k) is not None:
                l[k] = trunc(np.asarray(l[k], np.float32))
    want = O._h(O.subpixel(O.forward(dict(q, layers=q["layers"][:-1]), x, fp16=True), r, 0))
    np.testing.assert_allclose(y.reshape(-1), want.reshape(-1), rtol=4e-3, atol=4e-3)
    np.testing.assert_allclose(y.reshape(-1), _oracle(net, x).reshape(-1), atol=0.02)
    m.close()


@pytest.mark.parametrize("r", [3, 4])
def test_r8_prefer_half_keeps_the_conversions_separate(ctx, tmp_path, r):
    from shadernn_amd import host, models

    H, W = 24, 40
    path = _json(tmp_path, models.espcn_weights(seed=1, scale=r), W, H)
    m = host.Model(path, W, H, 1, prefer_half=True, input_format="R8", output_format="R8", **DEMO)
    ref = host.Model(path, W, H, 1, prefer_half=True)
    assert not any("u8_kernel" in d for _, _, d, _, _ in m.plan_steps())
    u = np.random.default_rng(5).integers(0, 256, size=(H, W, 1), dtype=np.uint8)
    m.upload_frame(u)
    m.run()
    got = m.output_frame()
    assert got.shape == (r * H, r * W, 1)
    np.testing.assert_array_equal(got, _expected(ref, u, DEMO))


@pytest.mark.parametrize("bad", ["channels", "zero"])
def test_a_bad_model_is_refused(ctx, tmp_path, bad):
    from shadernn_amd import host, models

    path = _json(tmp_path, models.espcn_weights(seed=1, scale=3), 16, 16)
    d = json.load(open(path))
    d["Layer_4"]["upscale"] = 4 if bad == "channels" else 0
    json.dump(d, open(path, "w"))
    with pytest.raises(AssertionError):
        host.Model(path, 16, 16, 1)
    good = _json(tmp_path, models.espcn_weights(seed=1, scale=4), 16, 16)  # the process and the context are fine
    assert host.Model(good, 16, 16, 1)(np.zeros((1, 16, 16, 1), np.float32)).shape == (64, 64, 1)
