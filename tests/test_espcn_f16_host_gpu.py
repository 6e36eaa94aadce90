"""The fused fp16 ESPCN chain (SNNHIP_ESPCN_F16=1) through the C++ host mirror: host.Model(prefer_half=True) reaches chain rules A16 / B16 through
HipBackend::finalizeStages -> snnhip_graph_fuse with no code of its own, for upscale 2, 3, 4 and with 8-bit frames at both ends."""
import copy

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
TOLH = dict(rtol=4e-3, atol=4e-3)
DEMO = dict(in_means=(127.5, 127.5, 127.5, 0), in_norms=(1 / 127.5, 1 / 127.5, 1 / 127.5, 1), out_scale=(127.5, 127.5, 127.5, 1), out_offset=(127.5, 127.5, 127.5, 0))


@pytest.fixture
def f16_rules():
    from shadernn_amd import capi

    capi.set_option("SNNHIP_ESPCN_F16", "1")
    yield
    capi.set_option("SNNHIP_ESPCN_F16", None)


def _json(tmp_path, net, w, h):
    from shadernn_amd import models

    return models.write_json(net, w, h, str(tmp_path / (net["name"] + ".json")))


def _quantised_oracle(net, x):
    """forward(quantised net, x, fp16=True) for any upscale factor; the host parser truncates weights and bias to half (tests/test_espcn_scale_host_gpu.py)."""
    r = int(net["layers"][-1].get("upscale", 2))
    q = copy.deepcopy(net)
    trunc = np.vectorize(O.to_medium_precision, otypes=[np.float32])
    for l in q["layers"]:
        for k in ("w", "b"):
            if l.get(k) is not None:
                l[k] = trunc(np.asarray(l[k], np.float32))
    return O._h(O.subpixel(O.forward(dict(q, layers=q["layers"][:-1]), x, fp16=True), r, 0))


def _fp32_oracle(net, x):
    r = int(net["layers"][-1].get("upscale", 2))
    return O.subpixel(O.forward(dict(net, layers=net["layers"][:-1]), x), r, 0)


@pytest.mark.parametrize("r", [2, 3, 4])
def test_prefer_half_model_runs_the_two_f16_launches(ctx, tmp_path, f16_rules, r):
    from shadernn_amd import host, models

    net = models.espcn_weights(seed=1, scale=r)
    w, h = 48, 40
    path = _json(tmp_path, net, w, h)
    m = host.Model(path, w, h, 1, prefer_half=True)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert len(steps) == 2 and all(d.startswith("fused[") and "f16" in d for d in steps), steps
    assert "espcn_f16_conv_pair_kernel" in steps[0] and "espcn_f16_d2s_kernel<%d>" % r in steps[1], steps
    per_layer = host.Model(path, w, h, 1, prefer_half=True, fuse_chains=False)
    lsteps = [d for _, _, d, _, _ in per_layer.plan_steps()]
    assert len(lsteps) == 4 and not any("fused[" in d for d in lsteps), lsteps
    x = np.random.default_rng(8).random((1, h, w, 1), dtype=np.float32)
    y = m(x)
    assert y.shape == (r * h, r * w, 1)
    np.testing.assert_allclose(y.reshape(-1), _quantised_oracle(net, x).reshape(-1), err_msg="; ".join(steps), **TOLH)
    np.testing.assert_allclose(y.reshape(-1), per_layer(x).reshape(-1), **TOLH)
    np.testing.assert_allclose(y.reshape(-1), _fp32_oracle(net, x).reshape(-1), atol=0.02)
    m.close()
    per_layer.close()


@pytest.mark.parametrize("r,H,W", [(2, 24, 40), (3, 19, 33), (4, 24, 40)])
def test_prefer_half_r8_frames_fold_into_the_two_launches(ctx, tmp_path, f16_rules, r, H, W):
    from shadernn_amd import host, models

    net = models.espcn_weights(seed=1, scale=r)
    path = _json(tmp_path, net, W, H)
    m = host.Model(path, W, H, 1, prefer_half=True, input_format="R8", output_format="R8", **DEMO)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert len(steps) == 2 and all("fused[" in d and "f16" in d for d in steps), steps
    assert "u8_in(1ch)" in steps[0] and "u8_out(1ch)" in steps[1], steps
    per_layer = host.Model(path, W, H, 1, prefer_half=True, fuse_chains=False, input_format="R8", output_format="R8", **DEMO)
    assert not any("fused[" in d for _, _, d, _, _ in per_layer.plan_steps())
    u = np.random.default_rng(5).integers(0, 256, size=(H, W, 1), dtype=np.uint8)
    got = []
    for model in (m, per_layer):
        model.upload_frame(u)
        model.run()
        got.append(model.output_frame().astype(np.int32))
    assert got[0].shape == (r * H, r * W, 1)
    # one level: the fp16 bound 4e-3 (1 + |y|) at 127.5 levels per unit (tests/test_espcn_f16_gpu.py)
    assert np.abs(got[0] - got[1]).max() <= 1
    xin = O._h((u.astype(np.float32)[None] - np.float32(127.5)) * np.float32(1 / 127.5))
    pre = _quantised_oracle(net, xin).astype(np.float64) * 127.5 + 127.5
    want = np.clip(np.rint(pre), 0, 255).astype(np.int32)
    assert np.abs(got[0].reshape(-1) - want.reshape(-1)).max() <= 1


def test_fuse_chains_off_stays_per_layer(ctx, tmp_path, f16_rules):
    from shadernn_amd import host, models

    net = models.espcn_weights(seed=1, scale=3)
    w, h = 48, 40
    m = host.Model(_json(tmp_path, net, w, h), w, h, 1, prefer_half=True, fuse_chains=False)
    steps = [d for _, _, d, _, _ in m.plan_steps()]
    assert len(steps) == 4 and not any("fused[" in d for d in steps) and any("subpixel f=3" in d for d in steps), steps
    x = np.random.default_rng(8).random((1, h, w, 1), dtype=np.float32)
    np.testing.assert_allclose(m(x).reshape(-1), _quantised_oracle(net, x).reshape(-1), **TOLH)
    m.close()


def test_snn_run_half_reaches_the_rules_through_the_environment(ctx, tmp_path):
    """lib/snn_run --half has no code of its own for the rules either: with SNNHIP_ESPCN_F16=1 in its environment (the registry's fallback, a fresh
    process) it runs, prints the same stage table (one row per layer, fused or not) and its output checksum stays within the fp16 bound, summed over
    the elements, of the per-layer run's."""
    import os
    import subprocess

    from shadernn_amd import models

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "shadernn_amd", "lib", "snn_run")
    assert os.path.exists(cli), "build() did not produce lib/snn_run"
    r, H, W = 3, 24, 32
    path = _json(tmp_path, models.espcn_weights(seed=1, scale=r), W, H)
    env = {k: v for k, v in os.environ.items() if k != "SNNHIP_ESPCN_F16"}
    runs = []
    for extra in ({}, {"SNNHIP_ESPCN_F16": "1"}):
        p = subprocess.run([cli, path, "--w", str(W), "--h", str(H), "--c", "1", "--loops", "1", "--half"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=300, env=dict(env, **extra))
        assert p.returncode == 0, p.stderr[-2000:]
        lines = p.stdout.strip().split("\n")
        assert lines[0].startswith("id") and lines[-1].startswith("output 1x%dx%dx1" % (r * H, r * W)), p.stdout
        runs.append((len(lines), float(lines[-1].split("checksum")[1].split()[0])))
    (rows_layers, sum_layers), (rows_fused, sum_fused) = runs
    assert rows_fused == rows_layers, runs
    assert abs(sum_fused - sum_layers) <= 8e-3 * (r * H) * (r * W), runs  # 4e-3 (1 + |y|), |y| <= 1 behind tanh, per element
