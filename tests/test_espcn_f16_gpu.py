"""The fused fp16 ESPCN chain (chain rules A16 / B16, espcn_f16.hip, SNNHIP_ESPCN_F16=1) through the C-ABI: two launches on the f16 matrix cores for
upscale 2, 3 and 4, the 8-bit ends folded in, against the oracle with the same quantisation points, the per-layer fp16 plans of the same build and
the fp32 oracle; the option unset leaves the per-layer path as it was; everything once more between red zones (SNNHIP_GUARD=1)."""
import functools
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TOLH = dict(rtol=4e-3, atol=4e-3)  # tests/test_fp16_gpu.py: the project's bound for a four-layer fp16 chain


def _tiles():
    txt = open(os.path.join(ROOT, "shadernn_amd", "csrc", "espcn_f16.h")).read()
    return {k: int(re.search(r"\b%s = (\d+)" % k, txt).group(1)) for k in ("kEspcnF16TW_A", "kEspcnF16TH_A", "kEspcnF16TW_B", "kEspcnF16TH_B")}


T = _tiles()
# smaller than any tile with an odd width; batch, ragged in both axes, odd width (the x3 store alignment); the existing fp16 host test's shape; one row
# and one column past a tile edge of each kernel
SHAPES = [(1, 5, 7), (2, 19, 33), (1, 40, 48), (1, T["kEspcnF16TH_A"] + 1, T["kEspcnF16TW_A"] + 1), (1, T["kEspcnF16TH_B"] + 1, T["kEspcnF16TW_B"] + 1)]
DEMO = ((127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1), (127.5, 0, 0, 0), (127.5, 0, 0, 0))  # means, norms, scale, offset (tests/test_frame_u8_gpu.py)


@pytest.fixture
def f16_rules():
    from shadernn_amd import capi

    capi.set_option("SNNHIP_ESPCN_F16", "1")
    yield
    capi.set_option("SNNHIP_ESPCN_F16", None)


@functools.lru_cache(maxsize=None)
def _net(r, variant="plain"):
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r)
    if variant == "acts":  # activations other than relu, BN on conv2 and conv3
        rng = np.random.default_rng(5)
        for i, act in enumerate(["tanh", "leakyRelu", "sigmoid"]):
            l = net["layers"][i]
            l["activation"] = act
            l["alpha"] = 0.2
            if i:
                c = l["oc"]
                l["bn"] = {"beta": rng.uniform(-0.1, 0.1, c).astype(np.float32), "gamma": rng.uniform(0.5, 1.5, c).astype(np.float32),
                           "mean": rng.uniform(-0.1, 0.1, c).astype(np.float32), "var": rng.uniform(0.5, 1.5, c).astype(np.float32)}
    return net


@functools.lru_cache(maxsize=None)
def _case(r, n, h, w, variant="plain"):
    """(input, quantised oracle, fp32 oracle) of one case, computed once and shared (read-only)."""
    net = _net(r, variant)
    x = np.random.default_rng(8).random((n, h, w, 1), dtype=np.float32)
    head = dict(net, layers=net["layers"][:-1])
    want16 = O._h(O.subpixel(O.forward(head, x, fp16=True), r, 0))
    want32 = O.subpixel(O.forward(head, x), r, 0)
    for a in (x, want16, want32):
        a.setflags(write=False)
    return x, want16, want32


def _layer_plans(ctx, net, n, h, w):
    from shadernn_amd import capi
    from shadernn_amd.runner import _layer_plan

    plans, shape = [], (n, h, w, 1)
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape, capi.F16)
        plans.append(p)
        shape = p.out_shape()
    return plans


def _one_by_one(ctx, plans, src, last_u8=False):
    from shadernn_amd import capi

    for k, p in enumerate(plans):
        u8 = last_u8 and k == len(plans) - 1
        dst = capi.Tensor(ctx, *p.out_shape(), dtype=capi.U8 if u8 else capi.F16)
        p.run(src, dst)
        src = dst
    return src


def _steps(chain):
    return [chain.step_describe(i) for i in range(chain.num_steps())]


@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("r", [2, 3, 4])
def test_fused_f16_chain_is_two_f16_launches_within_the_fp16_bounds(ctx, f16_rules, r, n, h, w):
    from shadernn_amd import capi

    net = _net(r)
    x, want16, want32 = _case(r, n, h, w)
    plans = _layer_plans(ctx, net, n, h, w)
    chain = capi.chain_plan(ctx, plans)
    steps = _steps(chain)
    assert len(steps) == 2 and all(s.startswith("fused[") and "f16" in s for s in steps), steps
    assert "espcn_f16_conv_pair_kernel" in steps[0] and "espcn_f16_d2s_kernel<%d>" % r in steps[1], steps
    xt = capi.Tensor.from_numpy(ctx, x, dtype=capi.F16)
    yt = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=capi.F16)
    chain.run(xt, yt)
    y = yt.numpy()
    per_layer = _one_by_one(ctx, plans, xt).numpy()
    print("r=%d %dx%dx%d: max |fused - quantised oracle| %.3e, |fused - per layer| %.3e, |fused - fp32 oracle| %.3e"
          % (r, n, h, w, np.abs(y - want16).max(), np.abs(y - per_layer).max(), np.abs(y - want32).max()))
    np.testing.assert_allclose(y, want16, err_msg="; ".join(steps), **TOLH)
    np.testing.assert_allclose(y, per_layer, err_msg="; ".join(steps), **TOLH)
    assert np.abs(y - want32).max() < 0.02, steps
    # the plans are priced on their own bytes: fp16 = 2 B
    px, taps = n * h * w, net["layers"][0]["kernel"] ** 2
    assert chain.step_cost(0)[1] == pytest.approx(2.0 * (px * 17 + 16 * taps + 16 * 16 * 9))
    assert chain.step_cost(1)[1] == pytest.approx(2.0 * (px * (16 + r * r) + r * r * 16 * 9))


@pytest.mark.parametrize("r", [2, 3])
def test_fused_f16_chain_with_bn_and_other_activations(ctx, f16_rules, r):
    from shadernn_amd import capi

    n, h, w = 1, 21, 35
    net = _net(r, "acts")
    x, want16, want32 = _case(r, n, h, w, "acts")
    plans = _layer_plans(ctx, net, n, h, w)
    chain = capi.chain_plan(ctx, plans)
    steps = _steps(chain)
    assert len(steps) == 2 and all(s.startswith("fused[") and "f16" in s for s in steps), steps
    xt = capi.Tensor.from_numpy(ctx, x, dtype=capi.F16)
    yt = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=capi.F16)
    chain.run(xt, yt)
    y = yt.numpy()
    np.testing.assert_allclose(y, want16, **TOLH)
    np.testing.assert_allclose(y, _one_by_one(ctx, plans, xt).numpy(), **TOLH)
    assert np.abs(y - want32).max() < 0.02


def test_a_3x3_first_convolution_takes_the_rule_too(ctx, f16_rules):
    """Rule A accepts k = 3 and 5 for the first convolution; so does A16 (nine taps of the 32-tap K-step carry weights)."""
    import copy

    from shadernn_amd import capi

    n, h, w, r = 1, 18, 37, 2
    net = copy.deepcopy(_net(r))
    l0 = net["layers"][0]
    l0["w"] = np.ascontiguousarray(l0["w"][:, :, 1:4, 1:4])
    l0["kernel"] = 3
    x = np.random.default_rng(9).random((n, h, w, 1), dtype=np.float32)
    plans = _layer_plans(ctx, net, n, h, w)
    chain = capi.chain_plan(ctx, plans)
    steps = _steps(chain)
    assert len(steps) == 2 and "fused[conv3x3(1->16)" in steps[0] and "f16" in steps[0], steps
    xt = capi.Tensor.from_numpy(ctx, x, dtype=capi.F16)
    yt = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=capi.F16)
    chain.run(xt, yt)
    np.testing.assert_allclose(yt.numpy(), O.forward(net, x, fp16=True), **TOLH)
    np.testing.assert_allclose(yt.numpy(), _one_by_one(ctx, plans, xt).numpy(), **TOLH)


def _frame(n, h, w, seed):
    u = np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 1), dtype=np.uint8)
    u.reshape(-1)[:4] = (0, 255, 128, 1)
    return u


# x3 with W = 33: a row pitch that is no multiple of 4 bytes (single-byte stores); W = 48: the 4-byte stores
@pytest.mark.parametrize("n,h,w", [(2, 19, 33), (1, 40, 48)])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_8bit_ends_fold_into_the_two_launches(ctx, f16_rules, r, n, h, w):
    from shadernn_amd import capi

    means, norms, scale, offset = DEMO
    net = _net(r)
    body = _layer_plans(ctx, net, n, h, w)
    head = capi.u8_in_plan(ctx, n, h, w, 1, means, norms, dtype=capi.F16)
    tail = capi.u8_out_plan(ctx, n, r * h, r * w, 1, scale, offset, dtype=capi.F16)
    chain = capi.chain_plan(ctx, [head] + body + [tail])
    steps = _steps(chain)
    assert len(steps) == 2 and all("fused[" in s and "f16" in s for s in steps), steps
    assert "u8_in(1ch)" in steps[0] and "u8_out(1ch)" in steps[1], steps
    px = n * h * w
    assert chain.step_cost(0)[1] == pytest.approx(2.0 * (px * 17 + 16 * 25 + 16 * 16 * 9) - px)
    assert chain.step_cost(1)[1] == pytest.approx(2.0 * (px * (16 + r * r) + r * r * 16 * 9) - r * r * px)
    u = _frame(n, h, w, 7)
    xt = capi.Tensor.from_numpy(ctx, u, dtype=capi.U8)
    yt = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=capi.U8)
    chain.run(xt, yt)
    got = yt.numpy_u8()
    # bit-identical to the u8_in plan, the fused fp16 chain and the u8_out plan run one by one
    fused_body = capi.chain_plan(ctx, body)
    assert fused_body.num_steps() == 2
    want = _one_by_one(ctx, [head, fused_body, tail], xt, last_u8=True).numpy_u8()
    np.testing.assert_array_equal(got, want, err_msg="; ".join(steps))
    # The quantised oracle.  The fp16 chain is held to |y - oracle| <= 4e-3 (1 + |oracle|) (TOLH); at 127.5 levels per unit that is up to one level,
    # so "equal away from the rounding boundaries" (the fp32 test's second assertion, boundary distance 0.02 = 1e-4 * 127.5 rounded up) has no
    # pixels left to hold on: the assertion is the one-level bound on every pixel.
    xin = O._h((u.astype(np.float32) - np.float32(means[0])) * np.float32(norms[0]))
    y16 = O._h(O.subpixel(O.forward(dict(net, layers=net["layers"][:-1]), xin, fp16=True), r, 0))
    pre = y16.astype(np.float64) * scale[0] + offset[0]
    want_q = np.clip(np.rint(pre), 0, 255).astype(np.int32)
    print("r=%d %dx%dx%d: %d of %d bytes differ from the quantised oracle" % (r, n, h, w, int((got.astype(np.int32) != want_q).sum()), got.size))
    assert np.max(np.abs(got.astype(np.int32) - want_q)) <= 1


def test_with_the_option_unset_the_fp16_chain_is_what_it_was(ctx):
    """No rule for fp16 ESPCN layers without the switch: the chain planner reports that nothing matches (callers keep the per-layer plans), and the
    graph runner's output is the per-layer plans' run one by one, bit for bit."""
    import shadernn_amd as snn
    from shadernn_amd import capi

    assert capi.get_option("SNNHIP_ESPCN_F16") is None
    r, n, h, w = 3, 2, 19, 33
    net = _net(r)
    x, want16, _ = _case(r, n, h, w)
    plans = _layer_plans(ctx, net, n, h, w)
    try:
        chain = capi.chain_plan(ctx, plans)
    except capi.SnnHipError as e:
        assert e.code == capi.E_UNSUPPORTED, str(e)
    else:
        assert not any("fused[" in s for s in _steps(chain)), _steps(chain)
    runner = snn.GraphRunner(ctx, net, n, h, w, dtype=snn.F16)
    assert not any("fused[" in d for d in runner.describe()), runner.describe()
    y = runner(x)
    xt = capi.Tensor.from_numpy(ctx, x, dtype=capi.F16)
    np.testing.assert_array_equal(y, _one_by_one(ctx, plans, xt).numpy())
    np.testing.assert_allclose(y, want16, **TOLH)


@pytest.mark.parametrize("switch", [("SNNHIP_ESPCN_FUSION", "stream"), ("SNNHIP_ESPCN_A", "direct"), ("SNNHIP_ESPCN_B", "wino")])
def test_the_fp32_only_alternatives_keep_the_fp16_chain_per_layer(ctx, f16_rules, monkeypatch, switch):
    import shadernn_amd as snn

    monkeypatch.setenv(*switch)
    r, n, h, w = 2, 1, 40, 48
    runner = snn.GraphRunner(ctx, _net(r), n, h, w, dtype=snn.F16)
    assert not any("fused[" in d for d in runner.describe()), runner.describe()
    x, want16, _ = _case(r, n, h, w)
    np.testing.assert_allclose(runner(x), want16, **TOLH)


def test_graph_fuse_and_the_graph_runner_reach_the_rules(ctx, f16_rules):
    """snnhip_graph_fuse (what HipBackend::finalizeStages and GraphRunner call) needs no code of its own: it goes through the chain planner."""
    import shadernn_amd as snn

    r, n, h, w = 4, 1, 40, 48
    runner = snn.GraphRunner(ctx, _net(r), n, h, w, dtype=snn.F16)
    assert len(runner.steps) == 1, runner.describe()
    plan = runner.steps[0][0]
    steps = _steps(plan)
    assert len(steps) == 2 and all(s.startswith("fused[") and "f16" in s for s in steps), steps
    x, want16, want32 = _case(r, n, h, w)
    y = runner(x)
    np.testing.assert_allclose(y, want16, **TOLH)
    assert np.abs(y - want32).max() < 0.02


def test_captured_graph_replays_fresh_frames(ctx, f16_rules):
    from shadernn_amd import capi

    means, norms, scale, offset = DEMO
    r, n, h, w = 3, 2, 19, 33
    body = _layer_plans(ctx, _net(r), n, h, w)
    head = capi.u8_in_plan(ctx, n, h, w, 1, means, norms, dtype=capi.F16)
    tail = capi.u8_out_plan(ctx, n, r * h, r * w, 1, scale, offset, dtype=capi.F16)
    chain = capi.chain_plan(ctx, [head] + body + [tail])
    x = capi.Tensor(ctx, n, h, w, 1, dtype=capi.U8)
    y = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=capi.U8)
    x.upload_u8(_frame(n, h, w, 0))
    with capi.Graph.capture(ctx) as g:
        chain.run(x, y)
    for seed in (1, 2):
        x.upload_u8(_frame(n, h, w, seed))
        g.launch()
        got = y.numpy_u8()
        direct = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=capi.U8)
        chain.run(x, direct)
        np.testing.assert_array_equal(got, direct.numpy_u8())
    g.destroy()


def test_the_shape_sweep_is_clean_under_the_guard(ctx):
    """Every shape, every factor, fp16 and 8-bit ends, with each allocation between red zones: a fresh process (the mode is fixed at the library's
    first allocation), ending in a clean snnhip_guard_check."""
    code = """
        import numpy as np
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_espcn_f16_gpu as t
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        capi.set_option("SNNHIP_ESPCN_F16", "1")
        means, norms, scale, offset = t.DEMO
        for r in (2, 3, 4):
            for (n, h, w) in t.SHAPES:
                net = t._net(r)
                x = np.random.default_rng(8).random((n, h, w, 1), dtype=np.float32)
                plans = t._layer_plans(ctx, net, n, h, w)
                chain = capi.chain_plan(ctx, plans)
                assert chain.num_steps() == 2 and "espcn_f16" in chain.describe(), chain.describe()
                xt = capi.Tensor.from_numpy(ctx, x, dtype=capi.F16)
                yt = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=capi.F16)
                chain.run(xt, yt)
                y = yt.numpy()
                assert np.isfinite(y).all()
                np.testing.assert_allclose(y, t._one_by_one(ctx, plans, xt).numpy(), **t.TOLH)
                head = capi.u8_in_plan(ctx, n, h, w, 1, means, norms, dtype=capi.F16)
                tail = capi.u8_out_plan(ctx, n, r * h, r * w, 1, scale, offset, dtype=capi.F16)
                chain8 = capi.chain_plan(ctx, [head] + plans + [tail])
                assert chain8.num_steps() == 2
                ut = capi.Tensor.from_numpy(ctx, t._frame(n, h, w, 3), dtype=capi.U8)
                qt = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=capi.U8)
                chain8.run(ut, qt)
                np.testing.assert_array_equal(qt.numpy_u8(), t._one_by_one(ctx, [head, chain, tail], ut, last_u8=True).numpy_u8())
                ctx.sync()
        capi.check(capi.lib().snnhip_guard_check(ctx.h))
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0 and "GUARD-OK" in p.stdout, p.stdout[-3000:]
