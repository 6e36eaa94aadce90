"""Chain rule L on the layer's own kernel (SNNHIP_POOL_FUSE=1 + SNNHIP_POOL_KERNEL): Conv2D -> MaxPooling2D 2x2 stride 2 as ONE launch of conv2d_wino's pooling
instances (conv2d_wino_pool_kernel, fp32; a split over blockIdx.z ends in splitk_reduce_pool_kernel) or conv2d_wide_f16's (conv2d_wide_pool_kernel, fp16), through
snn.chain_plan into NaN-filled outputs.  Each case is held to one step whose description names the kernel and the fold, to the block tiles its comment counts
(from the tile in the plan's description) and to the float64 budget of test_conv_pool_gpu (ref64.maxpool of ref64.conv_layer_general; budget_pairwise / M_CONV
in fp32, budget_half / M_F16 in fp16); the BITWISE ones also to the separate launches -- the convolution plan built under SNNHIP_CONV=wino / wide with the same
other switches, then the pooling plan -- bit for bit."""
import re

import numpy as np
import pytest

import ref64
from test_conv_pool_gpu import LEAKY, ON, _fused, _plans, _refs, case

pytestmark = pytest.mark.gpu
WINO, WIDE, AUTO = (dict(ON, SNNHIP_POOL_KERNEL=k) for k in ("wino", "wide", "auto"))
NAMES = {False: "conv2d_mfma_wino_f32", True: "conv2d_mfma_wide_f16"}
OPB2, KG2, SK2, SK4 = {"SNNHIP_WINO_OPB": "2"}, {"SNNHIP_WINO_KGROUPS": "2"}, {"SNNHIP_CONV_SPLITK": "2"}, {"SNNHIP_CONV_SPLITK": "4"}
BN32, BN64, BN128 = ({"SNNHIP_WIDE_BN": v} for v in ("32", "64", "128"))
h = lambda *a, **kw: case(*a, f16=True, **kw)

# (case, switches, block tiles, (splitK, kgroups)).  fp32: chunk 8, channel block 16 -- IC = 8, OC = 16 is one chunk and one block; a block tile is 64 Winograd
# tiles, 16 x 16 output pixels of one image at 16 x 16 (the planner picks the shape per layer)
CASES = [(case(1, 2, 2, 8, 16), {}, 1, (1, 1)), (case(1, 5, 7, 8, 16), {}, 1, (1, 1)), (case(1, 5, 7, 8, 16, same=False), {}, 1, (1, 1)),  # one window; clipped windows, both extents
         (case(2, 6, 6, 8, 16), {}, 1, (1, 1)), (case(1, 16, 16, 8, 16), {}, 1, (1, 1)), (case(1, 18, 18, 8, 16), {}, 3, (1, 1)),    # the batch seam in a tile; one tile; one more
         (case(1, 5, 7, 16, 16), {}, 1, (1, 1)), (case(1, 5, 7, 8, 48), {}, 1, (1, 1)),                    # two chunks; a ragged channel block (oc >= OC skipped)
         (case(1, 5, 7, 8, 16, epi=True), {}, 1, (1, 1)), (case(1, 5, 7, 8, 16, mode="none"), {}, 1, (1, 1)),  # negative gamma + leakyRelu; the pad-free form
         (case(1, 5, 7, 8, 64), OPB2, 1, (1, 1)), (case(1, 5, 7, 16, 16, same=False), KG2, 1, (1, 2)),     # 64-channel blocks; the exchange of the two K groups
         (case(1, 5, 7, 32, 16), SK2, 1, (2, 1)), (case(2, 6, 6, 32, 16, epi=True), SK2, 1, (2, 1)),       # the pooled reduce
         (case(1, 5, 7, 32, 16, same=False), SK4, 1, (4, 1)), (case(2, 6, 6, 32, 16), SK4, 1, (4, 1)),
         (case(1, 4, 4, 128, 16), {}, 1, (8, 1)),                                                          # K = 1152: the planner splits the sixteen chunks on its own
         # fp16: chunk 16 (32 under the 128-wide block); tiles 16 x 32 px for OC 32 / 64, 8 x 32 px for OC 128
         (h(1, 2, 2, 16, 32), {}, 1, None), (h(1, 5, 7, 16, 32), {}, 1, None), (h(1, 5, 7, 16, 32, same=False), {}, 1, None), (h(2, 6, 6, 16, 32), {}, 2, None),
         (h(1, 16, 32, 16, 32), {}, 1, None), (h(1, 17, 33, 16, 32), {}, 4, None), (h(1, 5, 33, 16, 32, same=False), {}, 2, None),  # one tile; a row and a column more; a tile of one column
         (h(1, 5, 7, 32, 32), {}, 1, None), (h(1, 5, 7, 16, 32, epi=True), {}, 1, None),                   # two chunks; negative gamma + leakyRelu
         (h(1, 5, 7, 16, 64), BN32, 1, None), (h(1, 17, 7, 16, 64), BN64, 2, None), (h(1, 9, 33, 32, 128, epi=True), BN128, 4, None)]  # the three block widths (128: 8-row tiles, chunk 32)
BITWISE = [CASES[i] for i in (5, 7, 11, 13, 14, 22, 23, 25, 28)]  # one tile more, the ragged block, KS = 2, split 2 and 4; fp16: tile edges, negative gamma, the 128-wide block
IDS = lambda cases: [pytest.param(c.values[0], *rest, id=c.id + "".join("_%s%s" % (k[7:].lower(), v) for k, v in rest[0].items())) for c, *rest in cases]


def _run(ctx, layer, env, **kw):
    plan, (xt, yt) = _fused(ctx, layer, env, **kw)
    plan.run(xt, yt)
    return yt.numpy(), plan.describe(), plan.num_steps()


@pytest.mark.parametrize("layer,extra,tiles,split", IDS(CASES))
def test_conv_maxpool_on_the_layers_own_kernel_within_the_float64_budget(ctx, request, layer, extra, tiles, split):
    n, hh, ww, f16 = layer[0], layer[1], layer[2], layer[8]
    got, desc, steps = _run(ctx, layer, dict(WIDE if f16 else WINO, **extra))
    assert steps == 1 and NAMES[f16] in desc and "+maxpool(2x2)" in desc, desc
    tb, th, tw = (int(v) for v in re.search(r"tile=(?:(\d+)x)?(\d+)x(\d+)px", desc).groups(default="1"))
    assert -(-n // tb) * -(-hh // th) * -(-ww // tw) == tiles, desc
    if f16:
        bn = int(extra.get("SNNHIP_WIDE_BN", 32))
        assert "x %doc" % bn in desc and "chunk=%d " % (32 if bn == 128 else 16) in desc, desc
    else:
        assert tuple(int(re.search(key + r"=(\d+)", desc).group(1)) for key in ("splitK", "kgroups")) == split and ("x 64oc" in desc) == (extra == OPB2), desc
    budget, m = (ref64.budget_half, ref64.M_F16) if f16 else (ref64.budget_pairwise, ref64.M_CONV)
    print("BUDGET pool-kernel | %s | %.2f %.2f %.2f" % ((request.node.callspec.id,) + tuple(budget(got, *_refs(layer)[5:], m, what=desc, tile=(th // 2, tw // 2)))))


@pytest.mark.parametrize("layer,extra,tiles,split", IDS(BITWISE))
def test_conv_maxpool_is_the_separate_launches_bit_for_bit(ctx, layer, extra, tiles, split):
    import shadernn_amd as snn

    f16 = layer[8]
    got, desc, _ = _run(ctx, layer, dict(WIDE if f16 else WINO, **extra))
    with pytest.MonkeyPatch.context() as m:
        for key, v in dict(extra, SNNHIP_CONV="wide" if f16 else "wino").items():
            m.setenv(key, v)
        (conv, pool), (xt, yt) = _plans(ctx, layer)
    mid = snn.Tensor(ctx, *conv.out_shape(), dtype=snn.F16 if f16 else snn.F32)
    conv.run(xt, mid)
    pool.run(mid, yt)
    same = lambda d: re.search(r"tile=\S+ x \d+oc.* chunk=\d+", d).group(0) + (re.search(r"kgroups=\d+ splitK=\d+", d).group(0) if not f16 else "")  # tile, block, chunk, split
    assert NAMES[f16] in conv.describe() and "+maxpool" not in conv.describe() and same(conv.describe()) == same(desc), (conv.describe(), desc)
    np.testing.assert_array_equal(got, yt.numpy())


def test_routing_follows_the_option(ctx):
    """unset, and the other precision's word: today's conv2d_mfma plan; auto: each kernel under its own default gate only (fp32 IC, OC >= 32; fp16 the wide kernel's
    blocks-per-CU gate; no SNNHIP_CONV= word); OC % 8 != 0 falls through; an unknown word is an error whatever the chain; without SNNHIP_POOL_FUSE, and for what
    the rule declines, nothing fuses"""
    import shadernn_amd as snn
    from shadernn_amd import capi

    small, big, half = case(1, 5, 7, 16, 32).values[0], case(1, 5, 7, 32, 32).values[0], h(1, 5, 7, 16, 32).values[0]
    for layer, env, own in ((big, ON, False), (big, WIDE, False), (half, WINO, False), (half, ON, False), (small, WINO, True), (half, WIDE, True), (big, AUTO, True), (small, AUTO, False),
                            (half, AUTO, False), (h(1, 5, 7, 16, 20).values[0], WIDE, False), (big, {"SNNHIP_CONV": "pool", "SNNHIP_POOL_KERNEL": "auto"}, False)):
        plan = _fused(ctx, layer, env)[0]
        desc = plan.describe()
        assert plan.num_steps() == 1 and "+maxpool(2x2)" in desc and "conv2d_mfma" in desc and (NAMES[layer[8]] in desc) == own, (env, desc)
    with pytest.MonkeyPatch.context() as m:  # 208 blocks of 512 pixels: the wide kernel's own gate passes under auto
        for key, v in AUTO.items():
            m.setenv(key, v)
        desc = snn.chain_plan(ctx, [snn.conv2d_plan(ctx, 2, 208, 256, _refs(half)[1], None, pads=(1,) * 4, dtype=snn.F16), snn.pool2d_plan(ctx, 2, 208, 256, 32, 2, 2)]).describe()
    assert NAMES[True] in desc and "+maxpool(2x2)" in desc, desc
    for env, kw, code in ((dict(ON, SNNHIP_POOL_KERNEL="winograd"), {}, capi.E_INVALID), ({"SNNHIP_POOL_KERNEL": "winograd"}, {"stride": 2}, capi.E_INVALID),
                          ({"SNNHIP_POOL_KERNEL": "wino"}, {}, capi.E_UNSUPPORTED), (WINO, {"stride": 2}, capi.E_UNSUPPORTED), (WINO, {"pool": (2, 2, "avg")}, capi.E_UNSUPPORTED),
                          (WINO, {"pool": (2, 1, "max")}, capi.E_UNSUPPORTED)):
        with pytest.raises(snn.SnnHipError, match="SNNHIP_POOL_KERNEL=winograd" if code == capi.E_INVALID else None) as e:
            _fused(ctx, big, env, **kw)
        assert e.value.code == code, (env, kw)
    # an Add behind the convolution (rule E's two-input plan in front of the pooling): no chain, as today
    for layer, env in ((big, WINO), (half, WIDE)):
        (conv, pool), _ = _plans(ctx, layer)
        with pytest.MonkeyPatch.context() as m:
            m.setenv("SNNHIP_CONV", "mfma")
            (direct, _), _ = _plans(ctx, layer)
        added = snn.chain_plan(ctx, [direct, snn.add_plan(ctx, *direct.out_shape(), act="relu", leaky=LEAKY)])
        assert "+add" in added.describe(), added.describe()
        for e2 in (ON, env):
            with pytest.MonkeyPatch.context() as m, pytest.raises(snn.SnnHipError) as e:
                for key, v in e2.items():
                    m.setenv(key, v)
                snn.chain_plan(ctx, [added, pool])
            assert e.value.code == capi.E_UNSUPPORTED, e2


def test_zoo_yolov3_tiny_pools_inside_the_winograd_launches(ctx, tmp_path, monkeypatch, size=64):
    import shadernn_amd as snn  # noqa: F401
    from shadernn_amd import capi, host, models
    from test_host import TOL

    net = models.zoo("yolov3-tiny", (size, size, 3))
    path = models.write_json(net, size, size, str(tmp_path / "net.json"), bin_weights=True)
    x = np.random.default_rng(3).random((2, size, size, 3), dtype=np.float32)
    out, launches = {}, {}
    for key, env in (("off", {}), ("on", WINO)):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m = host.Model(path, size, size, 3, batch=2)
        capi.trace_begin()
        out[key] = np.asarray(m(x)).copy()
        launches[key] = {k["function"]: k["launches"] for k in capi.trace_end()["kernels"]}
        m.close()
    # conv2d (IC = 3) stays on conv2d_mfma's form; conv2d_1 .. conv2d_3 run the Winograd pooling instances, split over K at this size
    assert launches["off"].get("pool2d_kernel", 0) - launches["on"].get("pool2d_kernel", 0) == 4 and launches["on"].get("conv2d_wino_pool_kernel", 0) == 3, launches
    assert "conv2d_wino_pool_kernel" not in launches["off"] and "splitk_reduce_pool_kernel" not in launches["off"], launches
    np.testing.assert_allclose(out["on"], out["off"], **TOL)
