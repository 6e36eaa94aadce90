"""Chain rule K on the layer's own kernel (SNNHIP_CAT_KERNEL): [UpSampling2D x2 ->] Concatenate -> Conv2D as ONE launch of conv2d_wino's two-source
instances (conv2d_wino_cat_kernel, fp32) or conv2d_wide_f16's (conv2d_wide_cat_kernel, fp16, plain concats), into NaN-filled outputs.  Each case is held (a) to
one step whose description names the kernel and the fold, (b) to the float64 budget of test_conv_cat_gpu (ref64 on np.concatenate, budget_pairwise / M_CONV in
fp32, budget_half / M_F16 in fp16) and (c) to the separate launches -- [upsample,] concat, then the convolution plan built under SNNHIP_CONV=wino / wide with the
same other switches -- BIT FOR BIT: same kernel, same chunk order, same split."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import ref64
from test_conv_cat_gpu import _check, _fused, _plans, _refs, _run, case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINO, SEP, NAME = {"SNNHIP_CAT_KERNEL": "wino"}, {"SNNHIP_CONV": "wino"}, "conv2d_mfma_wino_f32"
WIDE, WSEP, WNAME = {"SNNHIP_CAT_KERNEL": "wide"}, {"SNNHIP_CONV": "wide"}, "conv2d_mfma_wide_f16"
KERNELS = {"wino": (WINO, SEP, NAME), "wide": (WIDE, WSEP, WNAME)}
KG2, SK2, OPB2 = {"SNNHIP_WINO_KGROUPS": "2"}, {"SNNHIP_CONV_SPLITK": "2"}, {"SNNHIP_WINO_OPB": "2"}

# chunk 8; a block tile is 64 Winograd tiles = 16 x 16 output pixels of one image at the least
CASES = [(case(1, 1, 1, 8, 8), {}), (case(1, 16, 16, 8, 8), {}), (case(1, 17, 17, 8, 8), {}), (case(1, 5, 7, 8, 8), {}),
         (case(2, 5, 7, 8, 16), {}),                                          # the batch seam with two pitches
         (case(1, 5, 7, 16, 8), {}), (case(1, 5, 7, 8, 24), {}),              # input 1's pitch and origin
         (case(1, 5, 7, 8, 8, mode="none"), {}),                              # the pad-free form
         (case(1, 5, 7, 8, 16, epi=True), {}),                                # bias + BN + leakyRelu
         (case(2, 5, 7, 8, 24), KG2), (case(2, 5, 7, 16, 16), KG2),           # KS = 2, two chunks per K group: the boundary inside group 0's range / at the seam
         (case(1, 5, 7, 8, 24), SK2),                                         # slice 1 begins inside input 1
         (case(1, 4, 4, 64, 64, oc=128), {}),                                 # the planner splits K on its own
         (case(1, 5, 7, 8, 8), OPB2),
         (case(1, 6, 8, 8, 16, up=True), {}), (case(2, 6, 8, 16, 8, epi=True, up=True), {})]  # input 0 at 3 x 4 behind the upsampling
# conv2d_wide_f16: chunk 16 / 32; tiles 16 x 32 px for OC 32 / 64, 8 x 32 px for OC 128 (expected chunk beside the case)
WIDE_CASES = [(case(1, 1, 1, 16, 16, f16=True), 16), (case(1, 16, 32, 16, 16, f16=True), 16), (case(1, 17, 33, 16, 16, f16=True), 16), (case(1, 5, 7, 16, 16, f16=True), 16),
              (case(2, 5, 7, 16, 32, f16=True), 16),                             # the batch seam with two pitches
              (case(1, 5, 7, 32, 16, f16=True), 16),                             # input 1's pitch and origin
              (case(1, 9, 33, 32, 64, oc=128, f16=True), 32),                    # C8 = 2, the 8-row tile and one row more
              (case(1, 5, 7, 16, 32, oc=128, f16=True), 16),                     # the 16-channel chunk under the 128-wide block (C0 % 32 != 0)
              (case(1, 5, 7, 16, 16, mode="replicate", f16=True), 16), (case(1, 5, 7, 16, 16, mode="reflect", f16=True), 16),
              (case(1, 5, 7, 16, 16, epi=True, f16=True), 16)]


def _separate(ctx, layer, env, wt=None):
    """[upsample,] concat, convolution as three (two) launches, the convolution plan built under env"""
    import shadernn_amd as snn

    n, h, w, c0, c1 = layer[:5]
    with pytest.MonkeyPatch.context() as m:
        for key, v in env.items():
            m.setenv(key, v)
        plans, (at, bt, yt) = _plans(ctx, layer, wt)
    dt = snn.F16 if layer[9] else snn.F32
    if layer[10]:
        a2 = snn.Tensor(ctx, n, h, w, c0, dtype=dt)
        plans[0].run(at, a2)
        at = a2
    mid = snn.Tensor(ctx, n, h, w, c0 + c1, dtype=dt)
    plans[-2].run([at, bt], mid)
    plans[-1].run(mid, yt)
    return yt.numpy(), plans[-1].describe()


@pytest.mark.parametrize("layer,extra", [pytest.param(c.values[0], e, id=c.id + "".join("_%s%s" % (k[7:].lower(), v) for k, v in e.items())) for c, e in CASES])
def test_wino_concat_conv_is_the_separate_launches_bit_for_bit(ctx, request, layer, extra):
    got, desc, steps = _run(ctx, layer, dict(WINO, **extra))
    c0, c1, up = layer[3], layer[4], layer[10]
    assert steps == 1 and desc.startswith(NAME) and "+concat(%d+%d)" % (c0, c1) in desc and ("+upsample(x2 on input 0)" in desc) == up, desc
    split, kgroups = (int(re.search(key + r"=(\d+)", desc).group(1)) for key in ("splitK", "kgroups"))
    assert (kgroups == 2 or extra is not KG2) and (split == 2 or extra is not SK2) and ("x 64oc" in desc) == (extra is OPB2), desc
    assert split * kgroups > 1 or c0 + c1 != 128, desc  # (the planner splits the sixteen chunks of the 4 x 4 map on its own)
    print("BUDGET cat-wino | %s | %.2f %.2f %.2f" % ((request.node.callspec.id,) + tuple(_check(got, layer, desc))))
    want, sdesc = _separate(ctx, layer, dict(SEP, **extra))
    assert sdesc.startswith(NAME) and "+concat" not in sdesc, sdesc
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("layer,chunk", [pytest.param(c.values[0], k, id=c.id) for c, k in WIDE_CASES])
def test_wide_concat_conv_is_the_separate_launches_bit_for_bit(ctx, request, layer, chunk):
    got, desc, steps = _run(ctx, layer, WIDE)
    assert steps == 1 and desc.startswith(WNAME) and "+concat(%d+%d)" % layer[3:5] in desc and "+upsample" not in desc, desc
    assert "chunk=%d " % chunk in desc and ("x 128oc" in desc) == (layer[5] == 128), desc
    print("BUDGET cat-wide | %s | %.2f %.2f %.2f" % ((request.node.callspec.id,) + tuple(_check(got, layer, desc))))
    want, sdesc = _separate(ctx, layer, WSEP)
    assert sdesc.startswith(WNAME) and "+concat" not in sdesc, sdesc
    np.testing.assert_array_equal(got, want)


def test_auto_takes_the_wide_kernel_where_its_own_gate_holds(ctx):
    """fp16, nothing forced, 208 blocks of 512 pixels (the blocks-per-CU gate of make_conv2d_wide_plan passes): the layer's own plan and the two-source plan under
    SNNHIP_CAT_KERNEL=auto are both conv2d_wide_f16, and agree bit for bit"""
    import shadernn_amd as snn

    n, h, w, c = 2, 208, 256, 16
    rng = np.random.default_rng(71)
    a, b = rng.uniform(1.0, 2.0, (n, h, w, c)).astype(np.float32), rng.uniform(-2.0, -1.0, (n, h, w, c)).astype(np.float32)
    wt, bias = rng.normal(0.0, 1.0 / np.sqrt(18 * c), (32, 2 * c, 3, 3)).astype(np.float32), rng.normal(0.0, 0.1, 32).astype(np.float32)
    plans = [snn.concat_plan(ctx, n, h, w, c, c), snn.conv2d_plan(ctx, n, h, w, wt, bias, pads=(1,) * 4, act="relu", dtype=snn.F16)]
    at, bt, mid, yt, zt = [snn.Tensor.from_numpy(ctx, v, dtype=snn.F16) for v in (a, b, np.zeros((n, h, w, 2 * c), np.float32))] + [snn.Tensor(ctx, n, h, w, 32, dtype=snn.F16) for _ in "yz"]
    with pytest.MonkeyPatch.context() as m:
        m.setenv("SNNHIP_CAT_KERNEL", "auto")
        fused = snn.chain_plan(ctx, plans)
    assert fused.num_steps() == 1 and fused.describe().startswith(WNAME) and "+concat(16+16)" in fused.describe() and plans[1].describe().startswith(WNAME), fused.describe()
    fused.run([at, bt], yt)
    plans[0].run([at, bt], mid)
    plans[1].run(mid, zt)
    got = yt.numpy()
    assert np.isfinite(got).all() and (got != 0).any()
    np.testing.assert_array_equal(got, zt.numpy())


def test_wino_general_epilogue_behind_two_sources(ctx):
    """an activation outside the simple set (tanh): the SIMPLE = false instances"""
    import shadernn_amd as snn

    layer = case(1, 5, 7, 8, 16).values[0]
    n, h, w, c0, c1, oc = layer[:6]
    a, b, wt, bias = _refs(layer)[:4]

    def build():
        plans, ts = _plans(ctx, layer)
        return plans[:1] + [snn.conv2d_plan(ctx, n, h, w, wt, bias, pads=(1,) * 4, act="tanh")], ts

    with pytest.MonkeyPatch.context() as m:
        m.setenv("SNNHIP_CAT_KERNEL", "wino")
        plans, (at, bt, yt) = build()
        fused = snn.chain_plan(ctx, plans)
    fused.run([at, bt], yt)
    got, desc = yt.numpy(), fused.describe()
    assert fused.num_steps() == 1 and desc.startswith(NAME) and "+concat(8+16)" in desc, desc
    args = (np.concatenate([a, b], -1), wt, bias, 1, (1,) * 4, "constant", (h, w), None, "tanh", 0.0)
    print("BUDGET cat-wino | tanh | %.2f %.2f %.2f" % ref64.budget_pairwise(got, ref64.conv_layer_general(*args), ref64.conv_layer_pairwise32(*args), ref64.M_CONV, what=desc))
    with pytest.MonkeyPatch.context() as m:
        m.setenv("SNNHIP_CONV", "wino")
        (cat, conv), (at, bt, yt) = build()
    mid = snn.Tensor(ctx, n, h, w, c0 + c1)
    cat.run([at, bt], mid)
    conv.run(mid, yt)
    np.testing.assert_array_equal(got, yt.numpy())


@pytest.mark.parametrize("live", [0, 1])
@pytest.mark.parametrize("kern,layer", [("wino", case(2, 17, 17, 8, 16)), ("wide", case(2, 17, 33, 16, 32, f16=True))], ids=["wino", "wide"])
def test_a_swapped_or_shifted_source_would_show_as_a_wrong_sign(ctx, kern, layer, live):
    """weights positive on input `live`'s channels and zero on the other's, no bias: input 0 in [1, 2] gives y > 0, input 1 in [-2, -1] gives y < 0"""
    layer, (env, _, name) = layer.values[0], KERNELS[kern]
    c0 = layer[3]
    wt = np.abs(_refs(layer)[2])
    wt[:, c0:] *= live
    wt[:, :c0] *= 1 - live
    got, desc, _ = _run(ctx, layer, env, wt=wt)
    y = got - _refs(layer)[3]  # (the bias)
    assert desc.startswith(name) and np.isfinite(got).all() and ((y < 0).all() if live else (y > 0).all()), desc


@pytest.mark.parametrize("layer,env", [(case(1, 5, 7, 4, 12), WINO), (case(1, 5, 7, 8, 24, f16=True), WIDE), (case(1, 6, 8, 16, 16, up=True, f16=True), WIDE),
                                       (case(1, 5, 7, 8, 8), dict(WINO, SNNHIP_CAT="0")), (case(1, 5, 7, 16, 16, f16=True), dict(WIDE, SNNHIP_CAT="0"))],
                         ids=["wino_C0=4", "wide_C0=8", "wide_up", "wino_SNNHIP_CAT=0", "wide_SNNHIP_CAT=0"])
def test_the_kernel_declines_and_the_separate_plans_stay_correct(ctx, layer, env):
    import shadernn_amd as snn
    from shadernn_amd import capi

    layer = layer.values[0]
    with pytest.raises(snn.SnnHipError) as e:
        _fused(ctx, layer, env)
    assert e.value.code == capi.E_UNSUPPORTED
    _check(_separate(ctx, layer, WSEP if layer[9] else SEP)[0], layer, "separate plans")


@pytest.mark.parametrize("kern", ["wino", "wide"])
def test_a_convolution_with_a_fused_add_behind_the_concat_is_declined(ctx, kern):
    """rule E's plan (Conv2D + Add, a residual as its second input) has no two-source form: the chain stays unsupported and the caller keeps its plans"""
    import shadernn_amd as snn
    from shadernn_amd import capi

    layer = case(1, 5, 7, 16, 16, f16=kern == "wide").values[0]
    n, h, w, _, _, oc = layer[:6]
    (cat, conv), _ = _plans(ctx, layer)
    with_add = snn.chain_plan(ctx, [conv, snn.add_plan(ctx, n, h, w, oc)])
    assert "+add" in with_add.describe(), with_add.describe()
    with pytest.MonkeyPatch.context() as m, pytest.raises(snn.SnnHipError) as e:
        m.setenv("SNNHIP_CAT_KERNEL", KERNELS[kern][0]["SNNHIP_CAT_KERNEL"])
        snn.chain_plan(ctx, [cat, with_add])
    assert e.value.code == capi.E_UNSUPPORTED


def test_with_the_option_unset_the_rule_is_conv2d_mfma_as_before(ctx):
    for f16, env in ((True, {}), (True, {"SNNHIP_CONV": "cat"}), (False, {"SNNHIP_CONV": "cat"})):  # (fp32 is opt-in today: cat_default)
        layer = case(1, 6, 8, up=True, f16=f16).values[0]
        desc = _fused(ctx, layer, env)[0].describe()
        assert desc.startswith("conv2d_mfma_f16_" if f16 else "conv2d_mfma_f32_") and "+concat" in desc, desc


@pytest.mark.parametrize("kern,layer", [("wino", case(2, 17, 17, 8, 16, epi=True)), ("wide", case(2, 17, 33, 16, 32, epi=True, f16=True))], ids=["wino", "wide"])
def test_replays_of_a_recorded_graph_are_bit_identical(ctx, kern, layer):
    import shadernn_amd as snn

    layer, env = layer.values[0], KERNELS[kern][0]
    eager = _run(ctx, layer, env)[0]
    plan, (at, bt, yt) = _fused(ctx, layer, env)
    with snn.Graph.capture(ctx) as g:
        plan.run([at, bt], yt)
    for _ in range(2):
        yt.upload(np.full(eager.shape, np.nan, np.float32))
        g.launch()
        np.testing.assert_array_equal(yt.numpy(), eager)
    g.destroy()


GUARD_CASES = {"wino": """((T.case(1, 1, 1, 8, 8), ""), (T.case(2, 5, 7, 8, 16), ""), (T.case(1, 5, 7, 8, 24), "2"), (T.case(2, 6, 8, 16, 8, epi=True, up=True), ""))""",
               # (the wide kernel has no split-K and declines the upsampling: the smallest, a two-image and the 32-channel-chunk case)
               "wide": """((T.case(1, 1, 1, 16, 16, f16=True), ""), (T.case(2, 5, 7, 16, 32, f16=True), ""), (T.case(1, 9, 33, 32, 64, oc=128, f16=True), ""))"""}


@pytest.mark.parametrize("kern", ["wino", "wide"])
def test_the_plan_is_clean_under_the_guard(kern):
    """SNNHIP_GUARD=1 is fixed at the library's first allocation: a child process runs the smallest, a two-image, a split-K and an upsampled case between red zones"""
    code = """
        import os
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_conv_cat_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for c, sk in %s:
            got, desc, _ = T._run(ctx, c.values[0], dict({"SNNHIP_CAT_KERNEL": "%s"}, **({"SNNHIP_CONV_SPLITK": sk} if sk else {})))
            assert desc.startswith("%s") and "+concat" in desc and (got == got).all(), desc
            ctx.sync()
        print("GUARD-OK")
    """ % (GUARD_CASES[kern], kern, KERNELS[kern][2])
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize("name,ch", [("unet", 1), ("yolov3-tiny", 3)])
def test_zoo_graphs_fold_their_concats_under_auto(ctx, tmp_path, monkeypatch, name, ch, size=32):
    """host.Model and GraphRunner at 32 x 32, batch 2, fp32, nothing forced: SNNHIP_CAT_KERNEL=auto against SNNHIP_CAT=0.  One launch fewer per folded
    Concatenate (and per UpSampling2D folded with it), no concat_kernel launch for those, the outputs within test_host.TOL."""
    import shadernn_amd as snn
    from shadernn_amd import capi, host, models
    from test_host import TOL

    net = models.zoo(name, (size, size, ch))
    path = models.write_json(net, size, size, str(tmp_path / "net.json"), bin_weights=True)
    x = np.random.default_rng(3).random((2, size, size, ch), dtype=np.float32)
    out, launches, concats, folds = {}, {}, {}, []
    for key, env in (("auto", {"SNNHIP_CAT_KERNEL": "auto"}), ("off", {"SNNHIP_CAT_KERNEL": "auto", "SNNHIP_CAT": "0"})):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m = host.Model(path, size, size, ch, batch=2)
            r = snn.GraphRunner(ctx, net, 2, size, size)
        if key == "auto":
            lines = [d for d in r.describe() if "+concat(" in d]  # (host.Model plans through the same snnhip_graph_fuse: the launch counts below hold it to these)
            assert lines and all(NAME in d for d in lines), r.describe()
            folds = [(len(lines), sum("+upsample(x2 on input 0)" in d for d in lines))] * 2
        out[key], launches[key], concats[key] = [], [], []
        for run in (lambda: [np.asarray(m(x)).copy()], lambda: [r(x)] and r.outputs()):
            capi.trace_begin()
            out[key] += run()
            kernels = capi.trace_end()["kernels"]
            launches[key].append(sum(k["launches"] for k in kernels))
            concats[key].append(sum(k["launches"] for k in kernels if "concat_kernel" in k["function"]))
        m.close()
    assert [off - on for off, on in zip(launches["off"], launches["auto"])] == [f + u for f, u in folds], (launches, folds)
    assert [off - on for off, on in zip(concats["off"], concats["auto"])] == [f for f, _ in folds], (concats, folds)
    for got, want in zip(out["auto"], out["off"]):
        np.testing.assert_allclose(got, want, **TOL)
