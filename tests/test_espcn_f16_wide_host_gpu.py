"""The fused fp16 ESPCN chain at the published widths (1 -> 64 -> 32 -> r*r, SNNHIP_ESPCN_F16=1) through the C++ host mirror: a (64, 32) model file
through host.Model(prefer_half=True) reaches the two launches of espcn_f16_wide.hip with no code of its own, launched directly and as a recorded
graph; R8 frames at both ends give the bytes of the C-ABI chain; an NV12 frame runs in three launches and its luma plane is the R8 model's."""
import copy

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
WIDE = (64, 32)
DEMO = dict(in_means=(127.5, 127.5, 127.5, 0), in_norms=(1 / 127.5, 1 / 127.5, 1 / 127.5, 1), out_scale=(127.5, 127.5, 127.5, 1), out_offset=(127.5, 127.5, 127.5, 0))


@pytest.fixture
def f16_rules(monkeypatch):
    from shadernn_amd import capi

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even a two-launch inference
    capi.set_option("SNNHIP_ESPCN_F16", "1")
    yield
    capi.set_option("SNNHIP_ESPCN_F16", None)


def _json(tmp_path, net, w, h):
    from shadernn_amd import models

    return models.write_json(net, w, h, str(tmp_path / (net["name"] + "_wide.json")))


def _as_the_host_parser_reads_it(net):
    """The host parser truncates weights and bias to half (tests/test_espcn_scale_host_gpu.py): the net the C-ABI chain must be given to compute the same."""
    q = copy.deepcopy(net)
    trunc = np.vectorize(O.to_medium_precision, otypes=[np.float32])
    for l in q["layers"]:
        for k in ("w", "b"):
            if l.get(k) is not None:
                l[k] = trunc(np.asarray(l[k], np.float32))
    return q


@pytest.mark.parametrize("capture", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("r,H,W", [(2, 24, 40), (3, 19, 33), (4, 24, 40)])
def test_r8_frames_through_the_host_mirror_are_the_c_abi_chains_bytes(ctx, tmp_path, f16_rules, r, H, W, capture):
    from shadernn_amd import capi, host, models
    from shadernn_amd.runner import _layer_plan

    net = models.espcn_weights(seed=1, scale=r, widths=WIDE)
    m = host.Model(_json(tmp_path, net, W, H), W, H, 1, prefer_half=True, capture_graph=capture, input_format="R8", output_format="R8", **DEMO)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert len(steps) == 2 and "u8_in(1ch)" in steps[0] and "u8_out(1ch)" in steps[1], steps
    assert "espcn_f16_wide_conv_pair_kernel<u8>" in steps[0] and "espcn_f16_wide_d2s_kernel<%d,u8>" % r in steps[1], steps
    assert m.describe().count("(fused into a later stage's plan)") == 3, m.describe()  # four layers, one stage left: the chain of the two launches
    u = np.random.default_rng(5).integers(0, 256, size=(H, W, 1), dtype=np.uint8)
    m.upload_frame(u)
    m.run()  # (with capture: records, then launches the recording)
    got = m.output_frame()
    m.upload_frame(u)
    m.run()  # (with capture: a replay)
    np.testing.assert_array_equal(m.output_frame(), got)
    assert got.shape == (r * H, r * W, 1)
    m.close()

    plans, shape = [capi.u8_in_plan(ctx, 1, H, W, 1, DEMO["in_means"], DEMO["in_norms"], dtype=capi.F16)], (1, H, W, 1)
    for layer in _as_the_host_parser_reads_it(net)["layers"]:
        plans.append(_layer_plan(ctx, layer, shape, capi.F16))
        shape = plans[-1].out_shape()
    plans.append(capi.u8_out_plan(ctx, 1, r * H, r * W, 1, DEMO["out_scale"], DEMO["out_offset"], dtype=capi.F16))
    chain = capi.chain_plan(ctx, plans)
    assert chain.num_steps() == 2, chain.describe()
    xt = capi.Tensor.from_numpy(ctx, u[None], dtype=capi.U8)
    yt = capi.Tensor(ctx, 1, r * H, r * W, 1, dtype=capi.U8)
    chain.run(xt, yt)
    np.testing.assert_array_equal(got.reshape(-1), yt.numpy_u8().reshape(-1), err_msg="; ".join(steps))


def test_nv12_frames_run_in_three_launches_and_the_luma_is_the_r8_models(ctx, tmp_path, f16_rules):
    from shadernn_amd import capi, host, models

    r, H, W, N = 2, 16, 36, 2
    maps = dict(in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4)
    path = _json(tmp_path, models.espcn_weights(seed=1, scale=r, widths=WIDE), W, H)
    rng = np.random.default_rng(5)
    y = rng.integers(16, 236, size=(N, H, W)).astype(np.uint8)
    cbcr = rng.integers(16, 241, size=(N, H // 2, W // 2, 2)).astype(np.uint8)
    m = host.Model(path, W, H, 1, batch=N, prefer_half=True, video="NV12", **maps)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert len(steps) == 2 and "espcn_f16_wide_conv_pair_kernel<u8>" in steps[0] and "espcn_f16_wide_d2s_kernel<2,u8>" in steps[1], steps
    m.upload_frame((y, cbcr))
    m.run()
    y2, cbcr2 = m.download_frame()
    assert y2.shape == (N, r * H, r * W) and cbcr2.shape == (N, r * H // 2, r * W // 2, 2)
    capi.trace_begin()
    m.run()
    trace = capi.trace_end()
    assert trace["launches"] == 3, trace
    m.close()
    luma = host.Model(path, W, H, 1, batch=N, prefer_half=True, input_format="R8", output_format="R8", **maps)
    luma.upload_frame(y[..., None])
    luma.run()
    np.testing.assert_array_equal(y2, luma.download_frame().reshape(y2.shape))
    luma.close()
