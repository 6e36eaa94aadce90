"""deconv2d_mfma (Conv2DTranspose on the matrix cores, shadernn_amd/csrc/deconv2d_mfma.hip) through snn.deconv2d_plan under SNNHIP_DECONV=mfma, against
the float64 statement of tests/deconv_ref.py into output tensors that start as NaN: fp32 within ref64.M_CONV of the pairwise fp32 evaluation
(budget_pairwise), fp16 on half-rounded inputs and weights within ref64.M_F16 beyond half an ulp (budget_half).  The kernel's tile is TH x 16
low-resolution positions, TH = 16 / 8 / 4 / 2 at stride 1 / 2 / 3 / 4; an IC chunk is 16 channels in fp32, 32 in fp16."""
import functools

import numpy as np
import pytest

import deconv_ref
import ref64
from test_ops_gpu import _bn, _rand

pytestmark = pytest.mark.gpu

TH, TW, LEAKY = {1: 16, 2: 8, 3: 4, 4: 2}, 16, 0.1


def case(shape, k, s, same=True, act="", bn=False, f16=False, env="mfma", expect="deconv2d_mfma_"):
    ident = "x".join(map(str, shape)) + "_k%ds%d%s" % (k, s, "" if same else "_valid") + "".join("_" + t for t in (act, "bn" if bn else "", "f16" if f16 else "") if t)
    return pytest.param((tuple(shape), k, s, same, act, bn, f16), env, expect, id=ident + ("" if env == "mfma" else "_" + env))


EDGES = [(4, 2, True), (2, 2, True), (4, 2, False), (3, 1, True), (5, 2, True), (6, 3, True), (8, 4, True)]
# 72: two 32-channel chunks + 8 (fp16), four 16-channel chunks + 8 (fp32); 17 -> 18: pixels that are no whole 16-byte vectors (element loads and stores)
RAGGED = [(24, 20), (48, 40), (72, 24), (17, 18)]
CASES = (
    [case((2, TH[s] + 1, TW + 1, 16, 16), k, s, same) for k, s, same in EDGES]             # the tile edge, the second tile and the image seam
    + [case((2, TH[s] + 1, TW + 1, 16, 16), k, s, f16=True) for k, s in ((4, 2), (5, 2), (3, 1))]
    + [case((1, 3, 5, 16, 16), 4, 2), case((1, TH[2], TW, 16, 16), 4, 2, same=False)]       # below a tile; "valid": the position grid one past the tile
    + [case((1, 5, 7, 16, 16), 1, 2, same=False)]                                           # k < s: a phase no kernel row meets writes the bias alone
    + [case((1, 5, 7, ic, oc), 4, 2, f16=f16) for ic, oc in RAGGED for f16 in (False, True)]
    + [case((1, 5, 7, 16, 16), 4, 2, act="leakyRelu", bn=True), case((1, 5, 7, 16, 16), 4, 2, act="tanh"), case((1, 5, 7, 16, 16), 4, 2, act="sigmoid")]
    + [case((2, TH[2] + 1, TW + 1, 16, 16), 4, 2, env="direct", expect="deconv2d_direct"),  # the switch keeps the older kernel, inside the same budget
       case((1, 5, 7, 16, 4), 4, 2, expect="deconv2d_direct")]                              # thin OC is not a shape of the new kernel
)


@functools.lru_cache(maxsize=None)
def _refs(layer):
    (n, h, w, ic, oc), k, s, same, act, bn, f16 = layer
    q = (lambda a: a.astype(np.float16).astype(np.float32)) if f16 else (lambda a: a)
    x, wt, b = q(_rand((n, h, w, ic), 41)), q(_rand((oc, ic, k, k), 42, 1.0 / np.sqrt(k * k * ic / (s * s)))), _rand((oc,), 43, 0.1)
    bnp = _bn(oc, 44) if bn else None
    y64, y32 = deconv_ref.deconv_layer(x, wt, b, s, same, bnp, act, LEAKY)
    for a in (x, wt, b, y64, y32):
        a.setflags(write=False)
    return x, wt, b, bnp, y64, y32


@pytest.mark.parametrize("layer,env,expect", CASES)
def test_deconv_within_the_float64_budget(ctx, monkeypatch, request, layer, env, expect):
    import shadernn_amd as snn

    (n, h, w, ic, oc), k, s, same, act, bn, f16 = layer
    x, wt, b, bnp, y64, y32 = _refs(layer)
    dt = snn.F16 if f16 else snn.F32
    with monkeypatch.context() as m:
        m.setenv("SNNHIP_DECONV", env)
        plan = snn.deconv2d_plan(ctx, n, h, w, wt, b, stride=s, same=same, act=act, leaky=LEAKY, bn=bnp)
    xt = snn.Tensor.from_numpy(ctx, x, dtype=dt)
    yt = snn.Tensor.from_numpy(ctx, np.full(y64.shape, np.nan, np.float32), dtype=dt)
    try:
        assert plan.out_shape() == y64.shape, (plan.out_shape(), plan.describe())
        plan.run(xt, yt)
        got, desc = yt.numpy(), plan.describe()
    finally:
        for t in (xt, yt):
            t.free()
        plan.destroy()
    assert desc.startswith(expect + (("f16_" if f16 else "f32_") if expect.endswith("mfma_") else "")), desc
    if expect.endswith("mfma_"):
        assert "k=%d s=%d " % (k, s) in desc and "ic=%d oc=%d tile=%dx%d phases=%d " % (ic, oc, TH[s], TW, s * s) in desc and " lds=" in desc, desc
    tile = (s * TH[s], s * TW)
    if f16:
        ratios = ref64.budget_half(got, y64, y32, ref64.M_F16, what=desc, tile=tile)
    else:
        ratios = ref64.budget_pairwise(got, y64, y32, ref64.M_CONV, what=desc, tile=tile)
    print("BUDGET deconv | %s | %s | %.2f %.2f %.2f" % ((request.node.callspec.id, desc) + tuple(ratios)))
