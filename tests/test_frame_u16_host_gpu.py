"""16-bit frames through the C++ host mirror (snn_model_create6 / host.Model(input_format="R16", output_format="R16", ...)): the conversions join
the stage graph, fold into the fused fp32 ESPCN kernels, and the frames equal the float model's output quantised by the u16_out contract."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SYM10 = dict(in_means=(511.5, 511.5, 511.5, 0), in_norms=(1 / 511.5, 1 / 511.5, 1 / 511.5, 1), out_scale=(511.5, 511.5, 511.5, 1), out_offset=(511.5, 511.5, 511.5, 0),
             frame_out_maxval=1023)


def _json(tmp_path, net, w, h):
    from shadernn_amd import models

    return models.write_json(net, w, h, str(tmp_path / (net["name"] + ".json")))


def _q(x, io):
    C_ = x.shape[-1]
    s = np.asarray(io["out_scale"][:C_], np.float32).astype(np.float64)
    o = np.asarray(io["out_offset"][:C_], np.float32).astype(np.float64)
    # |x| <= 1 (tanh), scale = offset = 511.5: the float64 product is exact (24 + 10 bits) and so is its sum with the offset whenever |x * s| >= 2^-10
    # (below that the float32 result is 511.5 +- a few ulp either way), so rounding the sum to float32 once is fmaf
    y = np.rint((x.astype(np.float64) * s + o).astype(np.float32))
    y = np.where(np.isnan(y), 0.0, np.clip(y, 0.0, float(io.get("frame_out_maxval", 65535))))
    return (y.astype(np.uint32) << io.get("frame_out_shift", 0)).astype(np.uint16)


def _expected(float_model, u, io):
    C_ = u.shape[-1]
    x = ((u >> io.get("frame_in_shift", 0)).astype(np.float32) - np.float32(io["in_means"][:C_])) * np.float32(io["in_norms"][:C_])
    return _q(float_model(x), io)


def _frames(rng, shape, shift):
    return (rng.integers(0, 1024, size=shape).astype(np.uint16) << shift).astype(np.uint16)


@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("capture", [False, True])
def test_espcn_r16_frames_in_and_out(ctx, tmp_path, monkeypatch, capture, shift):
    from shadernn_amd import capi, host, models
    from shadernn_amd.runner import _layer_plan

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the two-launch ESPCN inference
    H, W = 45, 67
    net = models.espcn_weights(seed=1)
    path = _json(tmp_path, net, W, H)
    io = dict(SYM10, frame_in_shift=shift, frame_out_shift=shift)
    m = host.Model(path, W, H, 1, capture_graph=capture, input_format="R16", output_format="R16", **io)
    ref = host.Model(path, W, H, 1)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert len(steps) == 2, steps
    assert "conv_kxk_c1o16_wino3x3_c16o16_u16_kernel" in steps[0] and "conv3x3_c16o4_d2s_tanh_u16_kernel" in steps[1], steps
    # the same chain through the C-ABI
    plans, shape = [capi.u16_in_plan(ctx, 1, H, W, 1, io["in_means"], io["in_norms"], shift=shift)], (1, H, W, 1)
    for layer in net["layers"]:
        plans.append(_layer_plan(ctx, layer, shape))
        shape = plans[-1].out_shape()
    plans.append(capi.u16_out_plan(ctx, *shape, io["out_scale"], io["out_offset"], maxval=1023, shift=shift))
    chain = capi.chain_plan(ctx, plans)
    y = capi.Tensor(ctx, *shape, dtype=capi.U16)
    rng = np.random.default_rng(3)
    for _ in range(4):  # several frames in a row: a replayed graph must read the new frame
        u = _frames(rng, (H, W, 1), shift)
        m.upload_frame(u)
        m.run()
        got = m.output_frame()
        assert got.dtype == np.uint16 and got.shape == (2 * H, 2 * W, 1)
        np.testing.assert_array_equal(got, _expected(ref, u, io))
        chain.run(capi.Tensor.from_numpy(ctx, u[None]), y)
        np.testing.assert_array_equal(got, y.numpy_u16()[0])


def test_espcn_r16_batch4(ctx, tmp_path):
    from shadernn_amd import host, models

    H, W, B = 19, 33, 4
    path = _json(tmp_path, models.espcn_weights(seed=2), W, H)
    m = host.Model(path, W, H, 1, batch=B, input_format="R16", output_format="R16", **SYM10)
    ref = host.Model(path, W, H, 1, batch=B)
    u = _frames(np.random.default_rng(4), (B, H, W, 1), 0)
    m.upload_frame(u)
    m.run()
    np.testing.assert_array_equal(m.output_frame(), _expected(ref, u, SYM10))


def test_espcn_r16_prefer_half_runs_the_conversions_unfused(ctx, tmp_path):
    """prefer_half without SNNHIP_ESPCN_F16: one fp16 plan per layer, the conversions (the C-ABI's own u16 plans in fp16) as launches of their own.
    The float prefer_half host model is the one-by-one reference: the host parser truncates weights and bias to half, which plans built from the
    fp32 weights through the C-ABI would not reproduce bit for bit."""
    from shadernn_amd import host, models

    H, W = 24, 40
    net = models.espcn_weights(seed=1)
    path = _json(tmp_path, net, W, H)
    m = host.Model(path, W, H, 1, prefer_half=True, input_format="R16", output_format="R16", **SYM10)
    ref = host.Model(path, W, H, 1, prefer_half=True)
    assert not any("_u16_kernel" in d for _, _, d, _, _ in m.plan_steps())
    u = _frames(np.random.default_rng(5), (H, W, 1), 0)
    m.upload_frame(u)
    m.run()
    np.testing.assert_array_equal(m.output_frame(), _expected(ref, u, SYM10))


@pytest.mark.parametrize("fuse", [True, False])
def test_rgb16_single_conv(ctx, tmp_path, fuse):
    from shadernn_amd import host, models

    H, W = 17, 29
    net = models.single_conv(seed=3, ic=3, oc=3, k=3, act="tanh")
    path = _json(tmp_path, net, W, H)
    m = host.Model(path, W, H, 3, fuse_chains=fuse, input_format="RGB16", output_format="RGB16", **SYM10)
    ref = host.Model(path, W, H, 3, fuse_chains=fuse)
    u = _frames(np.random.default_rng(6), (H, W, 3), 0)
    m.upload_frame(u)
    m.run()
    np.testing.assert_array_equal(m.output_frame(), _expected(ref, u, SYM10))


def test_formats_layouts_and_the_older_entry_points(ctx, tmp_path):
    from shadernn_amd import host, models

    path = _json(tmp_path, models.espcn_weights(seed=1), 16, 16)
    with pytest.raises(AssertionError):  # channel count
        host.Model(path, 16, 16, 1, input_format="RGB16")
    with pytest.raises(AssertionError):  # 1023 << 7 does not fit
        host.Model(path, 16, 16, 1, output_format="R16", frame_out_maxval=1023, frame_out_shift=7)
    lib = host.lib()
    # snn_model_create5 knows the 8-bit formats only, and its struct keeps its layout
    assert C.sizeof(host.FrameIO) == 18 * 4 and C.sizeof(host.FrameIO2) == 21 * 4
    io = host.FrameIO(host.FRAME_FORMATS["R16"], 0, (C.c_float * 4)(0, 0, 0, 0), (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0))
    h = host._P()
    assert lib.snn_model_create5(path.encode(), 0, 16, 16, 1, 0, 1, 0, 0, 0, 1, C.byref(io), C.byref(h)) == -1
    # an 8-bit model (snn_model_create5) is unaffected: the 16-bit calls return -1 on it, and the 8-bit calls on a 16-bit model
    m8 = host.Model(path, 16, 16, 1, input_format="R8", output_format="R8")
    m16 = host.Model(path, 16, 16, 1, input_format="R16", output_format="R16", **SYM10)
    buf = np.zeros((32, 32, 1), np.uint16)
    assert lib.snn_model_upload_frame_u16(m8.h, buf.ctypes.data_as(host._P)) == -1
    assert lib.snn_model_download_frame_u16(m8.h, buf.ctypes.data_as(host._P)) == -1
    assert lib.snn_model_upload_frame_u8(m16.h, buf.ctypes.data_as(host._P)) == -1
    assert lib.snn_model_download_frame_u8(m16.h, buf.ctypes.data_as(host._P)) == -1
    mf = host.Model(path, 16, 16, 1)
    assert lib.snn_model_upload_frame_u16(mf.h, buf.ctypes.data_as(host._P)) == -1
