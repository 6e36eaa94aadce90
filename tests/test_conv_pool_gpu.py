"""Chain rule L (Conv2D -> MaxPooling2D 2x2 stride 2 as ONE launch: the POOL instances of conv2d_mfma_kernel.h) through snn.chain_plan under
SNNHIP_POOL_FUSE=1, into NaN-filled outputs, against float64: ref64.maxpool(ref64.conv_layer_general(...), 2, 2, out_hw); the unit is
ref64.maxpool(ref64.conv_layer_pairwise32(...), 2, 2, out_hw).  fp32 within ref64.M_CONV (budget_pairwise), fp16 within ref64.M_F16 (budget_half):
the maximum is 1-Lipschitz, so a kernel inside the full-resolution budget is inside the pooled one up to the smaller sample."""
import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import ref64
from test_ops_gpu import _bn, _rand

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = {False: 16, True: 32}  # channels per K chunk of conv2d_mfma
TH, TW, LEAKY, ON = 8, 16, 0.1, {"SNNHIP_POOL_FUSE": "1"}


def case(n, h, w, ic=0, oc=32, k=3, mode="constant", epi=False, f16=False, same=True):
    ic = ic or CH[f16]
    return pytest.param((n, h, w, ic, oc, k, mode, epi, f16, same), id="%dx%dx%d_%d-%d_k%d_%s%s%s%s" % (n, h, w, ic, oc, k, mode, "_bn_leaky" * epi, "" if same else "_valid", "_f16" * f16))


CASES = [c for f in (False, True) for C in (CH[f],) for c in (
    [case(1, 2, 2, f16=f), case(1, TH, TW, f16=f), case(1, TH + 2, TW + 2, f16=f), case(1, 5, 7, f16=f), case(1, 5, 7, f16=f, same=False), case(2, 6, 6, f16=f)]  # one window; tile edges; clipped windows; the batch seam
    + [case(1, 9, 13, 3, 16, f16=f), case(1, 5, 7, 2 * C, f16=f), case(1, 5, 7, k=1, f16=f), case(1, 5, 7, mode="replicate", f16=f), case(1, 5, 7, mode="reflect", f16=f)]  # tap pairs; two chunks; pointwise; padding modes
    + [case(1, 5, 7, epi=True, f16=f), case(1, 5, 7, oc=64, f16=f), case(1, 5, 7, oc=128, f16=f), case(1, 4, 4, 128, f16=f)]  # negative gamma; the other block widths; K = 1152
    + ([case(1, 5, 7, oc=20, f16=True)] if f else []))]  # no whole 8-channel vectors: direct 2-byte stores


def _pooled(h, w, same):
    return ((h + 1) // 2, (w + 1) // 2) if same else (h // 2, w // 2)


@functools.lru_cache(maxsize=None)
def _refs(layer):
    n, h, w, ic, oc, k, mode, epi, f16, same = layer
    q = (lambda v: v.astype(np.float16).astype(np.float32)) if f16 else (lambda v: v)
    x = q(_rand((n, h, w, ic), 71))
    wt, bias = q(_rand((oc, ic, k, k), 72, 1.0 / np.sqrt(k * k * ic))), _rand((oc,), 73, 0.1)
    bn, act = (_bn(oc, 74), "leakyRelu") if epi else (None, "")
    if bn:
        bn["gamma"][::2] *= -1.0  # a negative scale on half the channels: the maximum cannot move in front of the BN
    args = (x, wt, bias, 1, (k // 2,) * 4, mode, (h, w), bn, act, LEAKY)
    out = (x, wt, bias, bn, act, ref64.maxpool(ref64.conv_layer_general(*args), 2, 2, _pooled(h, w, same)), ref64.maxpool(ref64.conv_layer_pairwise32(*args), 2, 2, _pooled(h, w, same)))
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _plans(ctx, layer, x=None, wt=None, bias=None, pool=(2, 2, "max"), stride=1, act=None):
    """the per-layer plans conv, pool and the tensors x, y (NaN-filled, of the pooling plan's extent)"""
    import shadernn_amd as snn

    n, h, w, ic, oc, k, mode, epi, f16, same = layer
    x0, w0, b0, bn, act0 = _refs(layer)[:5]
    dt = snn.F16 if f16 else snn.F32
    conv = snn.conv2d_plan(ctx, n, h, w, w0 if wt is None else wt, b0 if bias is None else bias, stride=stride, pads=(k // 2,) * 4, pad_mode=mode, act=act0 if act is None else act, leaky=LEAKY, bn=bn, dtype=dt)
    ch, cw = conv.out_shape()[1:3]
    plans = [conv, snn.pool2d_plan(ctx, n, ch, cw, oc, pool[0], pool[1], kind=pool[2], same=same)]
    return plans, [snn.Tensor.from_numpy(ctx, x0 if x is None else x, dtype=dt), snn.Tensor.from_numpy(ctx, np.full(plans[1].out_shape(), np.nan, np.float32), dtype=dt)]


def _fused(ctx, layer, env=ON, **kw):
    import shadernn_amd as snn

    plans, ts = _plans(ctx, layer, **kw)
    with pytest.MonkeyPatch.context() as m:
        for key, v in env.items():
            m.setenv(key, v)
        return snn.chain_plan(ctx, plans), ts


def _run(ctx, layer, env=ON, **kw):
    plan, (xt, yt) = _fused(ctx, layer, env, **kw)
    plan.run(xt, yt)
    desc = plan.describe()
    assert plan.num_steps() == 1 and "+maxpool(2x2)" in desc and "splitK=1" in desc, desc
    return yt.numpy(), desc


@pytest.mark.parametrize("layer", CASES)
def test_conv_maxpool_within_the_float64_budget(ctx, request, layer):
    got, desc = _run(ctx, layer)
    assert ("tap-pairs" in desc) == (layer[3] == 3), desc
    budget, m = (ref64.budget_half, ref64.M_F16) if layer[8] else (ref64.budget_pairwise, ref64.M_CONV)
    print("BUDGET pool | %s | %.2f %.2f %.2f" % ((request.node.callspec.id,) + tuple(budget(got, *_refs(layer)[5:], m, what=desc, tile=(TH // 2, TW // 2)))))


@pytest.mark.parametrize("f16", [False, True])
def test_a_wrong_window_shows_exactly(ctx, f16):
    """pointwise identity weights, no bias, small integers: the output is NumPy's 2x2 maximum of the input bit for bit (a swapped dx / dy, a shifted
    window or a mixed image changes it)"""
    layer = case(2, 10, 18, 32, 32, k=1, f16=f16).values[0]
    n, y, x, c = np.meshgrid(np.arange(2), np.arange(10), np.arange(18), np.arange(32), indexing="ij")
    xin = (1 + (7 * y + 3 * x + c + 5 * n) % 61).astype(np.float32)
    got, desc = _run(ctx, layer, x=xin, wt=np.eye(32, dtype=np.float32).reshape(32, 32, 1, 1), bias=np.zeros(32, np.float32))
    np.testing.assert_array_equal(got, ref64.maxpool(xin, 2, 2, (5, 9)), err_msg=desc)


def test_the_floor_is_the_pooling_plans_own(ctx):
    layer = case(1, 5, 7).values[0]
    got, desc = _run(ctx, layer, wt=np.zeros((32, 16, 3, 3), np.float32), bias=np.full(32, -2e5, np.float32))
    assert (got == np.float32(-100000.0)).all(), desc


def test_off_by_default_and_every_decline_keeps_the_separate_plans(ctx):
    """without the switch, and for what the rule declines (YOLO's stride-1 pool, average pooling, a stride-2 convolution, the SiLU quirk, K > 1152), the
    chain planner has nothing to fuse and snnhip_graph_fuse hands both plans back; the two launches are the reference of the fused one"""
    import shadernn_amd as snn
    from shadernn_amd import capi

    base = case(1, 13, 13).values[0]
    for layer, env, kw in ((base, {}, {}), (base, {"SNNHIP_POOL_FUSE": "0"}, {}), (base, ON, {"pool": (2, 1, "max")}), (base, ON, {"pool": (2, 2, "avg")}), (base, ON, {"stride": 2}),
                           (base, ON, {"act": "SiLU_quirk"}),(case(1, 4, 4, 160).values[0], ON, {})):
        with pytest.raises(snn.SnnHipError) as e:
            _fused(ctx, layer, env, **kw)
        assert e.value.code == capi.E_UNSUPPORTED
        plans, (xt, yt) = _plans(ctx, layer, **kw)
        with pytest.MonkeyPatch.context() as m:
            for key, v in env.items():
                m.setenv(key, v)
            kept = capi.graph_fuse(ctx, [(plans[0], [-1], False), (plans[1], [0], True)])
        assert [f[0] for f in kept] == plans, (env, kw)


def test_replays_of_a_recorded_graph_are_bit_identical(ctx):
    import shadernn_amd as snn

    layer = case(2, TH + 1, TW + 1, mode="reflect", epi=True).values[0]
    eager = _run(ctx, layer)[0]
    plan, (xt, yt) = _fused(ctx, layer)
    with snn.Graph.capture(ctx) as g:
        plan.run(xt, yt)
    for _ in range(2):
        yt.upload(np.full(eager.shape, np.nan, np.float32))
        g.launch()
        np.testing.assert_array_equal(yt.numpy(), eager)
    g.destroy()


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 is fixed at the library's first allocation: a child process runs the ragged, tap-pair and K = 1152 cases between red zones; ctx.sync() verifies them."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_conv_pool_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for c in (T.case(1, 5, 7), T.case(1, 5, 7, oc=20, f16=True, same=False), T.case(1, 9, 13, 3, 16), T.case(1, 9, 13, 3, 16, f16=True), T.case(1, 4, 4, 128), T.case(1, 4, 4, 128, f16=True)):
            got, desc = T._run(ctx, c.values[0])
            assert (got == got).all(), desc
            ctx.sync()
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]


def test_zoo_yolov3_tiny_runs_four_pools_inside_the_convolutions(ctx, tmp_path, monkeypatch, size=64):
    """host.Model and GraphRunner at 64 x 64, batch 2, with the switch on and off: the four pooling launches gone (conv2d .. conv2d_3; conv2d_4's tensor has a second
    reader, the 13 x 13 pool has stride 1), outputs within the host tests' tolerance"""
    import shadernn_amd as snn
    from shadernn_amd import capi, host, models
    from test_host import TOL

    net = models.zoo("yolov3-tiny", (size, size, 3))
    path = models.write_json(net, size, size, str(tmp_path / "net.json"), bin_weights=True)
    x = np.random.default_rng(3).random((2, size, size, 3), dtype=np.float32)
    out, launches = {}, {}
    for key in ("on", "off"):
        with monkeypatch.context() as mp:
            if key == "on":
                mp.setenv("SNNHIP_POOL_FUSE", "1")
            m = host.Model(path, size, size, 3, batch=2)
            r = snn.GraphRunner(ctx, net, 2, size, size)
        out[key], launches[key] = [], []
        for run in (lambda: [np.asarray(m(x)).copy()], lambda: [r(x)] and r.outputs()):
            capi.trace_begin()
            out[key] += run()
            ks = capi.trace_end()["kernels"]
            launches[key].append((sum(k["launches"] for k in ks if k["function"] == "pool2d_kernel"), sum(k["launches"] for k in ks if k["function"] != "pool2d_kernel")))
        m.close()
    # exactly the four pooling launches go and nothing is added (a folded convolution whose own plan was two launches, conv2d_wino + its split-K reduce at
    # this size, becomes one: the total falls by five here)
    assert [(off[0] - on[0], on[1] <= off[1]) for off, on in zip(launches["off"], launches["on"])] == [(4, True), (4, True)], launches
    for got, want in zip(out["on"], out["off"]):
        np.testing.assert_allclose(got, want, **TOL)
