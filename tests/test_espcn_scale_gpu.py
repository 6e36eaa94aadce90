"""ESPCN at upscale factors 3 and 4 through the C-ABI (EspcnRunner): per-layer plans and the fused chain (rule A + rule B's matrix-core kernel for
r = 3, 4) against the CPU oracle.  tests/oracle_lib.forward knows factor 2 only, so the expectation is forward(net without its Subpixel layer)
followed by subpixel(., r, 0)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
SHAPES = [(1, 32, 32), (1, 72, 96), (2, 19, 71), (1, 8, 64), (1, 9, 130), (3, 5, 7)]


def _oracle(net, x, return_layers=False):
    r = int(net["layers"][-1].get("upscale", 2))
    head = dict(net, layers=net["layers"][:-1])
    y, layers = O.forward(head, x, return_layers=True)
    out = O.subpixel(y, r, 0)
    return (out, layers + [out]) if return_layers else out


@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("r", [3, 4])
def test_espcn_scale_matches_oracle(ctx, r, n, h, w, fused):
    import shadernn_amd as snn
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r)
    x = np.random.default_rng(7767517).random((n, h, w, 1), dtype=np.float32)
    runner = snn.EspcnRunner(ctx, net, n, h, w, fused=fused)
    y = runner(x)
    want, layers = _oracle(net, x, return_layers=True)
    assert y.shape == (n, r * h, r * w, 1)
    np.testing.assert_allclose(y, want, err_msg="; ".join(runner.describe()), **TOL)
    if not fused:
        assert len(runner.layer_outputs()) == len(layers) == 4
        for got, exp in zip(runner.layer_outputs(), layers):
            np.testing.assert_allclose(got, exp, **TOL)
    else:
        desc = runner.describe()
        assert len(desc) == 1
        steps = desc[0][len("chain{"):-1].split(" -> ")
        assert len(steps) == 2, desc
        assert "fused[conv5x5" in steps[0], desc
        assert "depth_to_space(%d)" % r in steps[1] and "conv3x3(16->%d)" % (r * r) in steps[1], desc
        assert "conv3x3_c16oR_d2s_tanh_kernel<%d>" % r in steps[1], desc


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("f", [3, 4, 5])
def test_subpixel_plan_general_factor(ctx, f, mode, dtype):
    """The stand-alone Subpixel plan (the unfused path of any integer factor), depth-to-space and the reference's Vulkan quirk mode."""
    import shadernn_amd as snn

    x = np.random.default_rng(10 * f + mode).standard_normal((2, 9, 7, f * f)).astype(np.float32)
    plan = snn.subpixel_plan(ctx, 2, 9, 7, f * f, f, mode)
    if dtype == "f32":
        y = plan(snn.Tensor.from_numpy(ctx, x)).numpy()
        assert y.shape == (2, 9 * f, 7 * f, 1)
        np.testing.assert_allclose(y, O.subpixel(x, f, mode), **TOL)
    else:  # half storage, tanh in fp32, one rounding on the way out (the bound tests/test_fp16_gpu.py uses for x2)
        y = plan(snn.Tensor.from_numpy(ctx, x, dtype=snn.F16)).numpy()
        assert y.shape == (2, 9 * f, 7 * f, 1)
        np.testing.assert_allclose(y, O._h(O.subpixel(O._h(x), f, mode)), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("r", [3, 4])
def test_espcn_scale_fused_with_bn_and_other_activations(ctx, r):
    """Rule B for r = 3, 4 carries the full epilogue (bias, BN, any plain activation), as the x2 rule does."""
    import shadernn_amd as snn
    from shadernn_amd import models

    net = models.espcn_weights(seed=3, scale=r)
    rng = np.random.default_rng(5)
    for i, act in enumerate(["leakyRelu", "sigmoid", "tanh"]):
        l = net["layers"][i]
        l["activation"] = act
        l["alpha"] = 0.2
        c = l["oc"]
        l["bn"] = {"beta": rng.uniform(-0.1, 0.1, c).astype(np.float32), "gamma": rng.uniform(0.5, 1.5, c).astype(np.float32),
                   "mean": rng.uniform(-0.1, 0.1, c).astype(np.float32), "var": rng.uniform(0.5, 1.5, c).astype(np.float32)}
    x = rng.random((1, 21, 67, 1), dtype=np.float32)
    runner = snn.EspcnRunner(ctx, net, 1, 21, 67, fused=True)
    assert "depth_to_space(%d)" % r in runner.describe()[0]
    np.testing.assert_allclose(runner(x), _oracle(net, x), err_msg=runner.describe()[0], **TOL)


@pytest.mark.parametrize("r,h,w", [(3, 720, 1280), (4, 540, 960)])
def test_espcn_scale_full_size_properties(ctx, r, h, w):
    """720p x3 and 540p x4 (both -> 3840 x 2160): fused and per-layer paths agree everywhere; windows of the image equal the oracle run on
    window + halo (the net's receptive field reaches 4 pixels: 2 + 1 + 1)."""
    import shadernn_amd as snn
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r)
    x = np.random.default_rng(1).random((1, h, w, 1), dtype=np.float32)
    y_f = snn.EspcnRunner(ctx, net, 1, h, w, fused=True)(x)
    y_u = snn.EspcnRunner(ctx, net, 1, h, w, fused=False)(x)
    assert y_f.shape == (1, 2160, 3840, 1)
    np.testing.assert_allclose(y_f, y_u, rtol=1e-5, atol=1e-5)
    assert np.isfinite(y_f).all() and np.abs(y_f).max() <= 1.0
    crop = _oracle(net, x[:, :40, :48, :])  # top-left corner (true borders)
    np.testing.assert_allclose(y_f[:, : r * 36, : r * 44, :], crop[:, : r * 36, : r * 44, :], **TOL)
    y0, x0 = 300, 500  # an interior window, halo 4 discarded
    crop = _oracle(net, x[:, y0 - 4 : y0 + 36, x0 - 4 : x0 + 44, :])
    np.testing.assert_allclose(y_f[:, r * y0 : r * (y0 + 32), r * x0 : r * (x0 + 40), :], crop[:, 4 * r : 4 * r + 32 * r, 4 * r : 4 * r + 40 * r, :], **TOL)
    crop = _oracle(net, x[:, h - 40 :, w - 48 :, :])  # bottom-right corner
    np.testing.assert_allclose(y_f[:, r * (h - 36) :, r * (w - 44) :, :], crop[:, 4 * r :, 4 * r :, :], **TOL)


@pytest.mark.parametrize("switch,value", [("SNNHIP_ESPCN_B", "wino"), ("SNNHIP_ESPCN_FUSION", "stream")])
def test_x2_only_switches_leave_scale_3_working(ctx, monkeypatch, switch, value):
    import shadernn_amd as snn
    from shadernn_amd import models

    monkeypatch.setenv(switch, value)
    net = models.espcn_weights(seed=4, scale=3)
    n, h, w = 2, 19, 71
    x = np.random.default_rng(11).random((n, h, w, 1), dtype=np.float32)
    runner = snn.EspcnRunner(ctx, net, n, h, w, fused=True)
    np.testing.assert_allclose(runner(x), _oracle(net, x), err_msg=runner.describe()[0], **TOL)
