"""conv2d_upconv2.hip (nearest UpSampling2D x2 -> Conv2D 2x2 "same" as nine pre-summed GEMMs on the low-resolution tensor) through
snn.chain_plan([upsample_plan, conv2d_plan]) under SNNHIP_CONV=upconv2, into NaN-filled outputs, against float64: np.repeat twice, then
ref64.conv_layer_general; the unit is ref64.conv_layer_pairwise32 on the same upsampled input.  fp32 within ref64.M_CONV (budget_pairwise); fp16 with weights
on a grid where every sum of up to four taps is exact in half within ref64.M_F16 (budget_half), with ordinary weights within the rounding of the pre-summed
weights.  The tile numbers come from conv2d_upconv2.h."""
import functools
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import ref64
from test_ops_gpu import _bn, _rand
from test_upconv2 import PADS, ROOT, axis_entries

pytestmark = pytest.mark.gpu

_K = {k: int(v) for k, v in re.findall(r"constexpr int (kUpconv2\w+) = (\d+);", open(os.path.join(ROOT, "shadernn_amd", "csrc", "conv2d_upconv2.h")).read())}
TH, TW, OC0, CHAIN = _K["kUpconv2TH"], _K["kUpconv2TW"], _K["kUpconv2OC"], _K["kUpconv2Chain"]
IC0 = {False: _K["kUpconv2ICBytes"] // 4, True: _K["kUpconv2ICBytes"] // 2}
SAME, LEAKY = PADS[0], 0.1


def case(n, h, w, oc=OC0, ic=None, pads=SAME, epi=False, f16=False):
    ic = ic or IC0[f16]
    return pytest.param((n, h, w, ic, oc, pads, epi, f16, True), id="%dx%dx%dx%dx%d_p%d%d%d%d%s%s" % ((n, h, w, ic, oc) + pads + ("_bn_leaky" if epi else "", "_f16" if f16 else "")))


CASES = [c for f16 in (False, True) for c in (
    [case(1, 1, 1, f16=f16), case(1, TH, TW, f16=f16), case(1, TH + 1, TW + 1, f16=f16), case(1, 5, 7, f16=f16), case(2, 5, 7, f16=f16)]  # tile edges, batch seam
    + [case(1, 5, 7, pads=p, f16=f16) for p in PADS[1:]] + [case(1, 5, 7, epi=True, f16=f16)]
    + [case(1, TH + 1, TW + 1, oc=2 * OC0, pads=PADS[2], f16=f16)]       # 64 channels: the instance with four row blocks per wave
    + [case(1, 4, 4, ic=1024, f16=f16)])]                                # 4 IC > the chain limit: the flushing instance
assert 4 * 1024 > CHAIN >= 4 * IC0[True]


@functools.lru_cache(maxsize=None)
def _refs(layer):
    n, h, w, ic, oc, pads, epi, f16, grid = layer
    q = (lambda a: a.astype(np.float16).astype(np.float32)) if f16 else (lambda a: a)
    x, b = q(_rand((n, h, w, ic), 51)), _rand((oc,), 53, 0.1)
    wt = _rand((oc, ic, 2, 2), 52, 1.0 / np.sqrt(4 * ic))
    if f16 and grid:  # multiples of 2^-6 s, |k| <= 64, s a power of two: every sum of up to four taps is exact in half
        s = 2.0 ** -int(np.ceil(np.log2(np.sqrt(4 * ic))))
        wt = (np.random.default_rng(52).integers(-64, 65, wt.shape) * (s / 64)).astype(np.float32)
    wt = q(wt)
    bn, act = (_bn(oc, 54), "leakyRelu") if epi else (None, "")
    xu = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    args = (xu, wt, b, 1, pads, "constant", (2 * h, 2 * w), bn, act, LEAKY)
    y64, y32 = ref64.conv_layer_general(*args), ref64.conv_layer_pairwise32(*args)
    for a in (x, wt, b, y64, y32):
        a.setflags(write=False)
    return x, wt, b, bn, act, y64, y32


def _chain(ctx, layer, env, k3=False):
    import shadernn_amd as snn

    n, h, w, ic, oc, pads, epi, f16, _ = layer
    x, wt, b, bn, act = _refs(layer)[:5]
    if k3:
        wt, pads = np.zeros((oc, ic, 3, 3), np.float32), (1, 1, 1, 1)
    dt = snn.F16 if f16 else snn.F32
    plans = [snn.upsample_plan(ctx, n, h, w, ic, 2.0, "nearest"), snn.conv2d_plan(ctx, n, 2 * h, 2 * w, wt, b, stride=1, pads=pads, act=act, leaky=LEAKY, bn=bn, dtype=dt)]
    with pytest.MonkeyPatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        chain = snn.chain_plan(ctx, plans)
    xt = snn.Tensor.from_numpy(ctx, x, dtype=dt)
    yt = snn.Tensor.from_numpy(ctx, np.full((n, 2 * h, 2 * w, oc), np.nan, np.float32), dtype=dt)
    return chain, xt, yt


def _run(ctx, layer, env={"SNNHIP_CONV": "upconv2"}):
    chain, xt, yt = _chain(ctx, layer, env)
    chain.run(xt, yt)
    return yt.numpy(), chain.describe(), chain.num_steps()


@pytest.mark.parametrize("layer", CASES)
def test_upconv2_within_the_float64_budget(ctx, request, layer):
    got, desc, steps = _run(ctx, layer)
    f16 = layer[7]
    assert steps == 1 and "conv2d_mfma_upconv2_" + ("f16" if f16 else "f32") in desc and "+upsample(x2)" in desc, desc
    y64, y32 = _refs(layer)[5:]
    budget, m = (ref64.budget_half, ref64.M_F16) if f16 else (ref64.budget_pairwise, ref64.M_CONV)
    print("BUDGET upconv2 | %s | %.2f %.2f %.2f" % ((request.node.callspec.id,) + tuple(budget(got, y64, y32, m, what=desc, tile=(2 * TH, 2 * TW)))))


def test_fp16_ordinary_weights_stay_within_the_rounding_of_the_presummed_weights(ctx):
    """|y - y64| <= 2^-11 sum |w_presummed| |x| + half an ulp16 + M_F16 E32p: a pre-summed weight is rounded to half once more than its taps were."""
    from shadernn_amd import capi

    layer = (1, TH + 1, TW + 1, IC0[True], OC0, PADS[2], False, True, False)
    got, desc, _ = _run(ctx, layer)
    x, wt, _, _, _, y64, y32 = _refs(layer)
    n, h, w, ic, oc, pads = layer[:6]
    m9 = np.abs(capi.upconv2_presum_weights(wt, pads).astype(np.float64))
    xp = np.zeros((n, h + 2, w + 2, ic))
    xp[:, 1:-1, 1:-1] = np.abs(x)
    mag = np.zeros(y64.shape)
    for ey, (py, ay, _) in enumerate(axis_entries(pads[2])):
        for ex, (px, ax, _) in enumerate(axis_entries(pads[0])):
            mag[:, py::2, px::2] += xp[:, 1 - pads[2] + ay:1 - pads[2] + ay + h, 1 - pads[0] + ax:1 - pads[0] + ax + w] @ m9[3 * ey + ex].T
    bound = 2.0 ** -11 * mag + 0.5 * ref64.ulp16(y64) + ref64.M_F16 * np.abs(y32 - y64).max()
    err = np.abs(got.astype(np.float64) - y64)
    assert np.isfinite(got).all() and (err <= bound).all(), "%s: max excess %.3e at %s" % (desc, (err - bound).max(), np.unravel_index(int((err - bound).argmax()), err.shape))


def test_other_layers_and_the_switch_keep_the_direct_kernel(ctx):
    base = (1, 5, 7, IC0[False], OC0, SAME, False, False, True)
    for layer, env, k3 in ((base, {"SNNHIP_CONV": "upconv2"}, True), (base[:3] + (IC0[False] // 2,) + base[4:], {"SNNHIP_CONV": "upconv2"}, False), (base, {"SNNHIP_UPCONV2": "0"}, False)):
        d = _chain(ctx, layer, env, k3)[0].describe()
        assert "upconv2" not in d and "conv2d_mfma_f32_32x32x2" in d and "+upsample(x2)" in d, d
    got, d, _ = _run(ctx, base, {"SNNHIP_UPCONV2": "0"})
    ref64.budget_pairwise(got, *_refs(base)[5:], ref64.M_CONV, what=d)


def test_replays_of_a_recorded_graph_are_bit_identical(ctx):
    import shadernn_amd as snn

    layer = (2, TH + 1, TW + 1, IC0[False], OC0, PADS[2], True, False, True)
    eager = _run(ctx, layer)[0]
    chain, xt, yt = _chain(ctx, layer, {"SNNHIP_CONV": "upconv2"})
    with snn.Graph.capture(ctx) as g:
        chain.run(xt, yt)
    for _ in range(2):
        yt.upload(np.full(eager.shape, np.nan, np.float32))
        g.launch()
        np.testing.assert_array_equal(yt.numpy(), eager)
    g.destroy()


def test_the_plan_is_clean_under_the_guard(ctx):
    """SNNHIP_GUARD=1 is fixed at the library's first allocation: a child process runs three ragged cases between red zones; ctx.sync() verifies them."""
    code = """
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_upconv2_gpu as T
        snn.load_library()
        assert capi.lib().snnhip_guard_active() == 1
        ctx = snn.Context(0)
        for layer in ((1, 1, 1, T.IC0[False], T.OC0, T.PADS[1], False, False, True), (2, T.TH + 1, T.TW + 1, T.IC0[True], 2 * T.OC0, T.PADS[2], True, True, True),
                      (1, 4, 4, 1024, T.OC0, T.SAME, False, False, True)):
            got, desc, _ = T._run(ctx, layer)
            assert "upconv2" in desc and (got == got).all(), desc
            ctx.sync()
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "GUARD-OK" in r.stdout, r.stdout[-3000:]


def test_zoo_unet_runs_its_four_up_convolutions_on_the_new_kernel(ctx, tmp_path, monkeypatch):
    from shadernn_amd import capi, host, models
    from test_host import TOL

    net = models.zoo("unet", (16, 16, 1))  # four poolings: 16 x 16 is the smallest input
    path = models.write_json(net, 16, 16, str(tmp_path / "unet.json"), bin_weights=True)
    x = np.random.default_rng(3).random((1, 16, 16, 1), dtype=np.float32)
    out = {}
    for env in ({"SNNHIP_CONV": "upconv2"}, {"SNNHIP_UPCONV2": "0"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m = host.Model(path, 16, 16, 1)
            capi.trace_begin()
            out[tuple(env)] = m(x)
            launches = {k["function"]: k["launches"] for k in capi.trace_end()["kernels"]}
            m.close()
        assert launches.get("conv2d_upconv2_kernel", 0) == (4 if "SNNHIP_CONV" in env else 0), launches
    np.testing.assert_allclose(out[("SNNHIP_CONV",)], out[("SNNHIP_UPCONV2",)], **TOL)
