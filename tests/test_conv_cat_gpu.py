"""Chain rule K (Concatenate -> Conv2D, optionally a nearest x2 UpSampling2D on the concat's input 0, as ONE convolution over two source tensors: the
CAT instances of conv2d_mfma_kernel.h) through snn.chain_plan under SNNHIP_CONV=cat and through snnhip_graph_fuse, into NaN-filled outputs, against
float64: ref64.conv_layer_general of np.concatenate([a, b], -1) (np.repeat x2 on a for the upsample case); the unit is ref64.conv_layer_pairwise32 on the
same tensor.  fp32 within ref64.M_CONV (budget_pairwise), fp16 within ref64.M_F16 (budget_half).  Input 0 lies in [1, 2] and input 1 in [-2, -1]."""
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
CH = {False: 16, True: 32}  # channels per K chunk of conv2d_mfma (a halo tile of these layers never makes the planner halve it)
TH, TW, LEAKY, CAT = 8, 16, 0.1, {"SNNHIP_CONV": "cat"}


def case(n, h, w, c0=0, c1=0, k=3, mode="constant", epi=False, f16=False, up=False, oc=32):
    c0, c1 = c0 or CH[f16], c1 or CH[f16]
    return pytest.param((n, h, w, c0, c1, oc, k, mode, epi, f16, up), id="%dx%dx%d_%d+%d_k%d_%s%s%s%s" % (n, h, w, c0, c1, k, mode, "_bn_leaky" * epi, "_up" * up, "_f16" * f16))


CASES = [c for f in (False, True) for C in (CH[f],) for c in (
    [case(1, 1, 1, f16=f), case(1, TH, TW, f16=f), case(1, TH + 1, TW + 1, f16=f), case(1, 5, 7, f16=f), case(2, 5, 7, C, 2 * C, f16=f)]  # tile edges; the batch seam with two pitches
    + [case(1, 5, 7, 2 * C, C, f16=f), case(1, 5, 7, C, C + 8, f16=f), case(1, 5, 7, C, C + 6, f16=f)]       # pitch / offset of input 1; its last chunk ragged, its pixels no whole slots
    + [case(1, 5, 7, C, 2 * C, k=1, f16=f), case(1, 5, 7, mode="replicate", f16=f), case(1, 5, 7, mode="reflect", f16=f), case(1, 5, 7, C, 2 * C, epi=True, f16=f)]
    + [case(1, 4, 4, 512, 512, oc=128, f16=f)]                                                                # IC = 1024 on a small map: split over K, a split starts inside input 1
    + [case(1, 6, 8, C, 2 * C, up=True, f16=f), case(2, 6, 8, 2 * C, C, mode="replicate", epi=True, up=True, f16=f)])]  # input 0 at 3 x 4 behind the upsampling, input 1 at 6 x 8


@functools.lru_cache(maxsize=None)
def _refs(layer):
    n, h, w, c0, c1, oc, k, mode, epi, f16, up = layer
    q = (lambda v: v.astype(np.float16).astype(np.float32)) if f16 else (lambda v: v)
    rng = np.random.default_rng(61)
    a = q(rng.uniform(1.0, 2.0, (n, h // 2, w // 2, c0) if up else (n, h, w, c0)).astype(np.float32))
    b = q(rng.uniform(-2.0, -1.0, (n, h, w, c1)).astype(np.float32))
    wt, bias = q(_rand((oc, c0 + c1, k, k), 62, 1.0 / np.sqrt(k * k * (c0 + c1)))), _rand((oc,), 63, 0.1)
    bn, act = (_bn(oc, 64), "leakyRelu") if epi else (None, "")
    x = np.concatenate([np.repeat(np.repeat(a, 2, axis=1), 2, axis=2) if up else a, b], -1)
    args = (x, wt, bias, 1, (k // 2,) * 4, mode, (h, w), bn, act, LEAKY)
    out = (a, b, wt, bias, bn, act, ref64.conv_layer_general(*args), ref64.conv_layer_pairwise32(*args))
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _plans(ctx, layer, wt=None):
    """the per-layer plans [upsample,] concat, conv and the tensors a, b, y (NaN-filled)"""
    import shadernn_amd as snn

    n, h, w, c0, c1, oc, k, mode, epi, f16, up = layer
    a, b, w0, bias, bn, act = _refs(layer)[:6]
    dt = snn.F16 if f16 else snn.F32
    plans = [snn.upsample_plan(ctx, n, h // 2, w // 2, c0, 2.0, "nearest")] if up else []
    plans += [snn.concat_plan(ctx, n, h, w, c0, c1), snn.conv2d_plan(ctx, n, h, w, w0 if wt is None else wt, bias, pads=(k // 2,) * 4, pad_mode=mode, act=act, leaky=LEAKY, bn=bn, dtype=dt)]
    return plans, [snn.Tensor.from_numpy(ctx, v, dtype=dt) for v in (a, b, np.full((n, h, w, oc), np.nan, np.float32))]


def _fused(ctx, layer, env=CAT, wt=None):
    import shadernn_amd as snn

    plans, ts = _plans(ctx, layer, wt)
    with pytest.MonkeyPatch.context() as m:
        for key, v in env.items():
            m.setenv(key, v)
        return snn.chain_plan(ctx, plans), ts


def _run(ctx, layer, env=CAT, wt=None):
    plan, (at, bt, yt) = _fused(ctx, layer, env, wt)
    plan.run([at, bt], yt)
    return yt.numpy(), plan.describe(), plan.num_steps()


def _check(got, layer, desc):
    budget, m = (ref64.budget_half, ref64.M_F16) if layer[9] else (ref64.budget_pairwise, ref64.M_CONV)
    return budget(got, *_refs(layer)[6:], m, what=desc, tile=(TH, TW))


@pytest.mark.parametrize("layer", CASES)
def test_concat_conv_within_the_float64_budget(ctx, request, layer):
    got, desc, steps = _run(ctx, layer)
    c0, c1, up = layer[3], layer[4], layer[10]
    assert steps == 1 and "+concat(%d+%d)" % (c0, c1) in desc and ("+upsample(x2 on input 0)" in desc) == up and ("splitK=1" not in desc) == (c0 + c1 == 1024), desc
    print("BUDGET cat | %s | %.2f %.2f %.2f" % ((request.node.callspec.id,) + tuple(_check(got, layer, desc))))


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("live", [0, 1])
def test_a_swapped_or_shifted_source_would_show_as_a_wrong_sign(ctx, f16, live):
    """weights positive on input `live`'s channels and zero on the other's, no bias: input 0 in [1, 2] gives y > 0, input 1 in [-2, -1] gives y < 0"""
    layer = case(2, TH + 1, TW + 1, CH[f16], 2 * CH[f16], f16=f16).values[0]
    c0 = layer[3]
    wt = np.abs(_refs(layer)[2])
    wt[:, c0:] *= live
    wt[:, :c0] *= 1 - live
    got, desc, _ = _run(ctx, layer, wt=wt)
    y = got - _refs(layer)[3]  # (the bias)
    assert np.isfinite(got).all() and ((y < 0).all() if live else (y > 0).all()), desc


def test_the_rule_declines_what_it_cannot_keep_and_the_switch_restores_the_separate_plans(ctx):
    import shadernn_amd as snn
    from shadernn_amd import capi

    for layer, env in ((case(1, 5, 7, 6, 18).values[0], CAT), (case(1, 5, 7, 4, 28).values[0], CAT), (case(1, 5, 7).values[0], {"SNNHIP_CONV": "cat", "SNNHIP_CAT": "0"})):
        with pytest.raises(snn.SnnHipError) as e:  # C0 % 4 != 0 (quirk Q21), C0 no multiple of the chunk, SNNHIP_CAT=0: the caller keeps its plans
            _fused(ctx, layer, env)
        assert e.value.code == capi.E_UNSUPPORTED
        (cat, conv), (at, bt, yt) = _plans(ctx, layer)
        mid = snn.Tensor(ctx, *yt.shape[:3], layer[3] + layer[4])
        cat.run([at, bt], mid)
        conv.run(mid, yt)
        a, b, wt, bias = _refs(layer)[:4]  # the Concatenate's own result: texel planes, a gap behind a C0 that is no multiple of 4 (quirk Q21)
        x = np.concatenate([a, np.zeros(a.shape[:3] + (-a.shape[3] % 4,), np.float32), b], -1)[..., :a.shape[3] + b.shape[3]]
        args = (x, wt, bias, 1, (1, 1, 1, 1), "constant", x.shape[1:3])
        ref64.budget_pairwise(yt.numpy(), ref64.conv_layer_general(*args), ref64.conv_layer_pairwise32(*args), ref64.M_CONV, what="separate plans")


@pytest.mark.parametrize("hold", ["", "keep", "second consumer"])
def test_graph_fuse_folds_a_concat_only_a_convolution_reads(ctx, monkeypatch, hold):
    import shadernn_amd as snn
    from shadernn_amd import capi

    monkeypatch.setenv("SNNHIP_CONV", "cat")
    layer = case(1, 6, 8, 16, 32, up=True).values[0]
    n, h, w, c0, c1, oc = layer[:6]
    (up, cat, conv), (at, bt, yt) = _plans(ctx, layer)
    ident = [snn.activation_plan(ctx, n, h // 2, w // 2, c0, ""), snn.activation_plan(ctx, n, h, w, c1, ""), snn.activation_plan(ctx, n, h, w, c0 + c1, "")]
    nodes = [(ident[0], [-1], False), (ident[1], [-2], False), (up, [0], False), (cat, [2, 1], hold == "keep"), (conv, [3], True)]
    nodes += [(ident[2], [3], True)] if hold == "second consumer" else []
    fused = capi.graph_fuse(ctx, nodes)
    if hold:
        assert [p is q[0] for p, q in zip((f[0] for f in fused), nodes)] == [True] * len(nodes)
        return
    assert fused[2][0] is None and fused[3][0] is None and fused[4][1] == [0, 1] and "+concat" in fused[4][0].describe(), [f[0] and f[0].describe() for f in fused]
    a2, b2 = snn.Tensor(ctx, *at.shape), snn.Tensor(ctx, *bt.shape)
    ident[0].run(at, a2)
    ident[1].run(bt, b2)
    fused[4][0].run([a2, b2], yt)
    _check(yt.numpy(), layer, fused[4][0].describe())


def test_replays_of_a_recorded_graph_are_bit_identical(ctx):
    import shadernn_amd as snn

    layer = case(2, TH + 1, TW + 1, 16, 32, mode="reflect", epi=True).values[0]
    eager = _run(ctx, layer)[0]
    plan, (at, bt, yt) = _fused(ctx, layer)
    with snn.Graph.capture(ctx) as g:
        plan.run([at, bt], yt)
    for _ in range(2):
        yt.upload(np.full(eager.shape, np.nan, np.float32))
        g.launch()
        np.testing.assert_array_equal(yt.numpy(), eager)
    g.destroy()


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 is fixed at the library's first allocation: a child process runs ragged, split-K and upsampled cases between red zones; ctx.sync() verifies them."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_conv_cat_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for c in (T.case(1, 1, 1), T.case(2, 5, 7, 32, 32 + 6, f16=True), T.case(1, 4, 4, 512, 512, oc=128), T.case(2, 6, 8, 64, 32, mode="replicate", epi=True, up=True, f16=True)):
            got, desc, _ = T._run(ctx, c.values[0])
            assert "+concat" in desc and (got == got).all(), desc
            ctx.sync()
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize("name,ch,folded", [("unet", 1, 4), ("yolov3-tiny", 3, 2)])
def test_zoo_graphs_run_their_concats_inside_the_convolutions(ctx, tmp_path, monkeypatch, name, ch, folded, size=32):
    """host.Model and GraphRunner at 32 x 32, batch 2: the rule against SNNHIP_CAT=0 with every other layer on the same kernel; one launch fewer per folded
    Concatenate (and YOLOv3-tiny's UpSampling2D)"""
    import shadernn_amd as snn
    from shadernn_amd import capi, host, models
    from test_host import TOL

    net = models.zoo(name, (size, size, ch))
    path = models.write_json(net, size, size, str(tmp_path / "net.json"), bin_weights=True)
    x = np.random.default_rng(3).random((2, size, size, ch), dtype=np.float32)
    out, launches = {}, {}
    for key, env in (("cat", CAT), ("off", dict(CAT, SNNHIP_CAT="0"))):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m = host.Model(path, size, size, ch, batch=2)
            r = snn.GraphRunner(ctx, net, 2, size, size)
        out[key], launches[key] = [], []
        for run in (lambda: [np.asarray(m(x)).copy()], lambda: [r(x)] and r.outputs()):
            capi.trace_begin()
            out[key] += run()
            launches[key].append(sum(k["launches"] for k in capi.trace_end()["kernels"]))
        m.close()
    assert [off - cat for off, cat in zip(launches["off"], launches["cat"])] == [folded, folded], launches
    for got, want in zip(out["cat"], out["off"]):
        np.testing.assert_allclose(got, want, **TOL)

