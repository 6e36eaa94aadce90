"""irb_f16.hip (chain rule G on half tensors, SNNHIP_IRB_F16=1): Conv2D 1x1 -> DepthwiseConv2D 3x3 -> Conv2D 1x1 [-> Add with the block input] as one
f16-MFMA launch, against the quantised oracle run layer by layer (every stored tensor rounded to half) and against the three / four per-layer fp16 plans."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle_lib as O
from test_fp16_gpu import TOLH
from test_ops_gpu import _bn, _rand

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME = O.padding_offsets("same", 3)
R6 = ("relu6", "relu6", "")

# N, H, W, C, Ch, Co, stride, residual, (act1, act2, act3)
CASES = {"one_pixel": (1, 1, 1, 16, 32, 16, 1, False, R6),          # every halo position but one is masked
         "one_tile": (1, 8, 8, 16, 32, 16, 1, True, R6),
         "tile_plus_1": (1, 9, 9, 16, 32, 16, 1, False, R6),       # four tiles, three of them ragged
         "odd_below_tile": (1, 5, 7, 16, 32, 16, 1, True, R6),
         "two_images_res": (2, 9, 9, 16, 32, 16, 1, True, R6),
         "s2_8x8": (1, 8, 8, 16, 32, 16, 2, False, R6),            # "same" at stride 2 on even extents: pads 0 before, 1 after
         "s2_16x16": (1, 16, 16, 16, 32, 16, 2, False, R6),
         "s2_odd_9x11": (2, 9, 11, 16, 32, 24, 2, False, R6),
         "C8": (1, 9, 9, 8, 32, 8, 1, True, R6),                   # below one K-step; Co = 8
         "C24": (1, 9, 9, 24, 32, 16, 1, False, R6),               # 16 + 8 tail
         "C40": (1, 9, 9, 40, 32, 16, 1, False, R6),               # 32 + 8 tail: two K-steps
         "Ch16": (1, 9, 9, 16, 16, 16, 1, True, R6),               # a single short slice
         "Ch48": (1, 9, 9, 16, 48, 16, 1, False, R6),              # 32 + 16 tail
         "b02": (1, 9, 9, 24, 144, 24, 1, True, R6),               # MobileNetV2 b02; Co % 16 == 8
         "b16_widest": (1, 7, 7, 160, 960, 320, 1, False, R6),     # twenty accumulator tiles, thirty slices
         "acts_none_leaky_relu": (1, 9, 9, 16, 32, 16, 1, True, ("", "leakyRelu", "relu")),
         "acts_relu_none_relu6": (1, 9, 9, 16, 32, 16, 2, False, ("relu", "", "relu6"))}


def _nbn(c, seed):
    bn = _bn(c, seed)
    bn["gamma"][::3] *= -1.0  # negative gammas: the masked halo positions would otherwise hide behind a ReLU
    return bn


def _block(ctx, case, seed, env=None):
    """The three per-layer fp16 plans [+ Add], the input, and the quantised oracle's result."""
    import shadernn_amd as snn

    N, H, W, C, Ch, Co, s, res, acts = case
    x = _rand((N, H, W, C), seed)
    we, be, bne = _rand((Ch, C, 1, 1), seed + 1, 1.0 / np.sqrt(C)), _rand((Ch,), seed + 2, 0.1), _nbn(Ch, seed + 3)
    wd, bd, bnd = _rand((Ch, 3, 3), seed + 4, 1.0 / 3.0), _rand((Ch,), seed + 5, 0.1), _nbn(Ch, seed + 6)
    wp, bp, bnp = _rand((Co, Ch, 1, 1), seed + 7, 1.0 / np.sqrt(Ch)), _rand((Co,), seed + 8, 0.1), _nbn(Co, seed + 9)
    pe = snn.conv2d_plan(ctx, N, H, W, we, be, act=acts[0], leaky=0.1, bn=bne, dtype=snn.F16)
    pd = snn.conv2d_plan(ctx, N, H, W, wd, bd, stride=s, pads=SAME, act=acts[1], leaky=0.1, bn=bnd, depthwise=True, dtype=snn.F16)
    _, OH, OW, _ = pd.out_shape()
    pp = snn.conv2d_plan(ctx, N, OH, OW, wp, bp, act=acts[2], leaky=0.1, bn=bnp, dtype=snn.F16)
    pa = snn.add_plan(ctx, N, OH, OW, Co, act="relu" if acts[2] == "relu" else "") if res else None
    h = O._h(O.conv2d(O._h(x), O._h(we), be, 1, (0, 0, 0, 0), "constant", acts[0], 0.1, bne))
    d = O._h(O.depthwise(h, O._h(wd), bd, s, SAME, acts[1], 0.1, bnd))
    want = O._h(O.conv2d(d, O._h(wp), bp, 1, (0, 0, 0, 0), "constant", acts[2], 0.1, bnp))
    if res:
        want = O._h(O.add_act(want, O._h(x), "relu" if acts[2] == "relu" else "", 0.0))
    return (pe, pd, pp, pa), x, want


def _fuse(ctx, plans):
    import shadernn_amd as snn

    pe, pd, pp, pa = plans
    if pa is None:
        return snn.chain_plan(ctx, [pe, pd, pp])
    fused = snn.graph_fuse(ctx, [(pe, [-1], False), (pd, [0], False), (pp, [1], False), (pa, [2, -1], True)])
    assert [f[0] is None for f in fused] == [True, True, True, False] and fused[3][1] == [-1], [f[0] and f[0].describe() for f in fused]
    return fused[3][0]


def _nan_out(ctx, shape):
    import shadernn_amd as snn

    return snn.Tensor.from_numpy(ctx, np.full(shape, np.nan, np.float32), dtype=snn.F16)


@pytest.mark.parametrize("name", sorted(CASES))
def test_irb_f16_matches_quantised_oracle_and_per_layer_plans(ctx, name, monkeypatch):
    import shadernn_amd as snn

    case = CASES[name]
    N, H, W, C, Ch, Co, s, res, acts = case
    plans, x, want = _block(ctx, case, 500)
    monkeypatch.setenv("SNNHIP_IRB_F16", "1")
    plan = _fuse(ctx, plans)
    d = plan.describe()
    assert plan.num_steps() == 1 and "irb_f16" in d and "16x16x32_f16" in d and ("+ add" in d) == res, d
    assert "C=%d Ch=%d Co=%d stride=%d" % (C, Ch, Co, s) in d, d
    xt = snn.Tensor.from_numpy(ctx, x, dtype=snn.F16)
    yt = _nan_out(ctx, want.shape)
    plan.run(xt, yt)
    got = yt.numpy()
    pe, pd, pp, pa = plans
    sep = pp(pd(pe(xt)))
    sep = (pa([sep, xt]) if pa else sep).numpy()
    print("%s: max |fused - oracle| %.3e, max |per-layer - oracle| %.3e, max |fused - per-layer| %.3e" %
          (name, np.abs(got - want).max(), np.abs(sep - want).max(), np.abs(got - sep).max()))
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, err_msg=d, **TOLH)
    np.testing.assert_allclose(got, sep, err_msg=d, **TOLH)
    f, b = plan.cost()
    assert f > 0 and b > 0


def test_padded_hidden_positions_are_zero_not_the_expand_bias(ctx, monkeypatch):
    """x = 0, expand bias 1 (no activation, no BN), depthwise weights all 1, project = identity: the output counts the in-image taps, exactly."""
    import shadernn_amd as snn

    monkeypatch.setenv("SNNHIP_IRB_F16", "1")
    n = 16
    pe = snn.conv2d_plan(ctx, 1, 9, 9, _rand((n, n, 1, 1), 1), np.ones(n, np.float32), dtype=snn.F16)
    pd = snn.conv2d_plan(ctx, 1, 9, 9, np.ones((n, 3, 3), np.float32), None, pads=SAME, depthwise=True, dtype=snn.F16)
    pp = snn.conv2d_plan(ctx, 1, 9, 9, np.eye(n, dtype=np.float32).reshape(n, n, 1, 1), None, dtype=snn.F16)
    plan = snn.chain_plan(ctx, [pe, pd, pp])
    assert "irb_f16" in plan.describe(), plan.describe()
    yt = _nan_out(ctx, (1, 9, 9, n))
    plan.run(snn.Tensor.from_numpy(ctx, np.zeros((1, 9, 9, n), np.float32), dtype=snn.F16), yt)
    edge = np.array([2] + [3] * 7 + [2], np.float32)
    np.testing.assert_array_equal(yt.numpy(), np.broadcast_to(np.outer(edge, edge)[None, :, :, None], (1, 9, 9, n)))


def test_irb_f16_is_opt_in_and_declines_what_it_cannot_run(ctx, monkeypatch):
    import shadernn_amd as snn

    monkeypatch.delenv("SNNHIP_IRB_F16", raising=False)
    plans, _, _ = _block(ctx, CASES["tile_plus_1"], 7)
    with pytest.raises(snn.SnnHipError) as e:  # as before this kernel existed: no rule takes three fp16 layers
        snn.chain_plan(ctx, list(plans[:3]))
    assert e.value.code == snn.E_UNSUPPORTED
    resplans, _, _ = _block(ctx, CASES["one_tile"], 7)
    nodes = [(resplans[0], [-1], False), (resplans[1], [0], False), (resplans[2], [1], False), (resplans[3], [2, -1], True)]
    assert not any("irb" in f[0].describe() for f in snn.graph_fuse(ctx, nodes) if f[0] is not None)
    monkeypatch.setenv("SNNHIP_IRB_F16", "1")
    assert "irb_f16" in snn.chain_plan(ctx, list(plans[:3])).describe()
    monkeypatch.setenv("SNNHIP_NO_IRB_FUSION", "1")  # rule G's own switch wins
    with pytest.raises(snn.SnnHipError):
        snn.chain_plan(ctx, list(plans[:3]))
    monkeypatch.delenv("SNNHIP_NO_IRB_FUSION")
    odd, _, _ = _block(ctx, (1, 9, 9, 12, 32, 16, 1, False, R6), 7)  # C = 12: no 16-byte input loads
    with pytest.raises(snn.SnnHipError):
        snn.chain_plan(ctx, list(odd[:3]))


def test_replays_of_a_recorded_graph_are_bit_identical(ctx, monkeypatch):
    import shadernn_amd as snn

    monkeypatch.setenv("SNNHIP_IRB_F16", "1")
    plans, x, want = _block(ctx, CASES["two_images_res"], 500)
    plan = _fuse(ctx, plans)
    xt, yt = snn.Tensor.from_numpy(ctx, x, dtype=snn.F16), _nan_out(ctx, want.shape)
    plan.run(xt, yt)
    eager = yt.numpy()
    with snn.Graph.capture(ctx) as g:
        plan.run(xt, yt)
    for _ in range(2):
        yt.upload(np.full(want.shape, np.nan, np.float32))
        g.launch()
        np.testing.assert_array_equal(yt.numpy(), eager)
    g.destroy()


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 is fixed at the library's first allocation: a child process runs a ragged stride-2 block between red zones; ctx.sync() verifies them."""
    code = """
        import numpy as np
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_irb_f16_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        plans, x, want = T._block(ctx, T.CASES["s2_odd_9x11"], 500)
        plan = T._fuse(ctx, plans)
        assert "irb_f16" in plan.describe(), plan.describe()
        yt = T._nan_out(ctx, want.shape)
        plan.run(snn.Tensor.from_numpy(ctx, x, dtype=snn.F16), yt)
        np.testing.assert_allclose(yt.numpy(), want, **T.TOLH)
        ctx.sync()
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", SNNHIP_IRB_F16="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]


def test_mobilenetv2_fp16_runs_its_blocks_on_the_fused_kernel(ctx, tmp_path, monkeypatch):
    """GraphRunner(dtype=F16) and host.Model(prefer_half=True) with the switch: the quantised oracle's result to the fp16 classifier test's tolerances, in
    fewer launches than without the switch (both counted by the launch trace)."""
    import shadernn_amd as snn
    from shadernn_amd import capi, host, models

    net = models.mobilenetv2(seed=3, num_classes=10, width_mult=0.5)
    x = np.random.default_rng(7).random((2, 64, 64, 3), dtype=np.float32)
    want = O.forward(net, x, fp16=True).reshape(2, -1)
    path = models.write_json(net, 64, 64, str(tmp_path / "mbv2.json"))

    def traced(run):
        capi.trace_begin()
        y = run(x)
        kernels = capi.trace_end()["kernels"]
        return np.asarray(y).reshape(2, -1), sum(k["launches"] for k in kernels), sum(k["launches"] for k in kernels if "irb_f16_kernel" in k["function"])

    counts = {}
    for on in (False, True):
        with monkeypatch.context() as mp:
            if on:
                mp.setenv("SNNHIP_IRB_F16", "1")
            else:
                mp.delenv("SNNHIP_IRB_F16", raising=False)
            r = snn.GraphRunner(ctx, net, 2, 64, 64, dtype=snn.F16)
            m = host.Model(path, 64, 64, 3, batch=2, prefer_half=True)
            for what, run in (("graph", r), ("host", m)):
                y, launches, fused = traced(run)
                np.testing.assert_allclose(y, want, rtol=2e-2, atol=4e-3, err_msg=what)
                counts[what, on] = launches
                assert (fused > 0) == on, (what, on, fused)
            assert any("irb_f16" in d for d in r.describe()) == on, r.describe()
            m.close()
    assert counts["graph", True] < counts["graph", False] and counts["host", True] < counts["host", False], counts
