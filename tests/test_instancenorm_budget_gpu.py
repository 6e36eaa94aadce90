"""InstanceNorm in its four forms -- the stand-alone plan (statistics sweep, fold, normalise sweep), graph rule H (norm + Add), chain rule F (the fp16
convolution's tile records, folded in the kernel or by the two fold launches) and, in tests/test_eltwise_gpu.py, graph rule I -- held to the float64
reference of tests/ref64.py on planes that are adverse to an fp32 evaluation of a plane's statistics (tests/norm_cases.py): per (image, channel) plane
the error stays within ref64.M_NORM times the error of a straightforward two-pass fp32 evaluation (ref64.instancenorm32), floored at the rounding of
the shift that the one-FMA form y = x * mul + shift cannot avoid; half tensors within that of the correctly rounded half of the exact result.
Output tensors start as NaN.  Every test prints one line "NORMBUDGET form | case | description | ratio"."""
import functools
import re

import numpy as np
import pytest

import norm_cases
import oracle_lib as O
import ref64
from test_conv_budget_gpu import _free
from test_conv_f16_budget_gpu import WIDE, _figures_then_assert
from test_ops_gpu import _rand

pytestmark = pytest.mark.gpu

LEAKY = 0.1
ACTS = ["", "relu", "leakyRelu"]  # the normalise sweep's three instances: FAST = 2 (none), FAST = 1 (ReLU) and the generic one

# (N, H, W, C) -> the slabs the plan must report (256 CUs: S = ceil(HW / max(256, roundup64(ceil(HW / ceil(2048 / N)))))): the smallest shapes that reach
SHAPES = [((1, 1, 1, 4), 1),         # H*W = 1: variance 0, the output is beta
          ((2, 3, 5, 3), 1),         # one slab, fewer pixels than pixel lanes, CV = 1
          ((1, 1, 257, 4), 2),       # two slabs, the second with one pixel
          ((3, 17, 23, 5), 2),       # CV = 1, 8 channel lanes, ragged everything, N = 3
          ((1, 16, 20, 65), 2),      # CV = 1, 64 channel lanes, a second channel pass with one live lane
          ((2, 16, 20, 128), 2),     # CV = 4 at the 128-channel limit
          ((1, 16, 20, 132), 2),     # ... and a second channel pass with one live lane of four
          ((1, 264, 256, 4), 264),   # the fold's threads 0..7 take a second slab
          ((1, 1030, 256, 1), 1030)]  # S > 1024: several rounds per thread, C = 1
BIG = (1, 264, 256, 4)
RAGGED = (3, 17, 23, 5)
SLABS = dict(SHAPES)


def _name(shape):
    return "x".join(map(str, shape))


def _sweep_cases():
    out = []
    for si, (shape, _) in enumerate(SHAPES):
        for dtype in ("f32", "f16"):
            for fi, family in enumerate(norm_cases.families(dtype)):
                out.append(pytest.param(shape, dtype, family, ACTS[(si + fi) % 3], 1e-5, id="%s-%s-%s" % (_name(shape), dtype, family)))
    for dtype in ("f32", "f16"):  # a second eps on one shape
        for family, act in (("benign", "relu"), ("pivot10", ""), ("tiny", "leakyRelu")):
            out.append(pytest.param(RAGGED, dtype, family, act, 1e-3, id="%s-%s-%s-eps1e-3" % (_name(RAGGED), dtype, family)))
    return out


@functools.lru_cache(maxsize=16)
def _refs(shape, dtype, family, act, eps):
    """(x, beta, gamma, float64 reference, fp32 model, floor) of one case, computed once and read-only; x is rounded to half first where the tensor is half."""
    x = norm_cases.plane(family, shape, dtype, seed=len(family) + shape[1])
    beta, gamma = norm_cases.params(shape[3], seed=shape[2])
    want64 = ref64.instancenorm(x, beta, gamma, eps, act, LEAKY)
    model32 = ref64.instancenorm32(x, beta, gamma, eps, act, LEAKY)
    floor = ref64.norm_floor(x, beta, gamma, eps)
    for a in (want64, model32, floor):
        a.setflags(write=False)
    return x, beta, gamma, want64, model32, floor


def _dt(dtype):
    import shadernn_amd as snn

    return snn.F16 if dtype == "f16" else snn.F32


def _nan_tensor(ctx, shape, dt):
    import shadernn_amd as snn

    t = snn.Tensor.from_numpy(ctx, np.full(shape, np.nan, np.float32), dtype=dt)
    return t


def _run_into_nan(ctx, plan, ins, shape, dt):
    yt = _nan_tensor(ctx, shape, dt)
    plan.run(ins, yt)
    y = yt.numpy()
    yt.free()
    return y


def _norm_plan(ctx, shape, beta, gamma, act, eps):
    import shadernn_amd as snn

    plan = snn.instancenorm_plan(ctx, *shape, beta, gamma, act=act, leaky=LEAKY, eps=eps)
    desc = plan.describe()
    m = re.search(r"slabs=(\d+)", desc)
    assert m and int(m.group(1)) == SLABS[shape], "the slab rule changed: %s, expected slabs=%d" % (desc, SLABS[shape])
    return plan, desc


def _held(form, case, desc, got, refs, dtype):
    x, beta, gamma, want64, model32, floor = refs
    try:
        ratio = ref64.budget_norm(got, want64, model32, ref64.M_NORM, floor, what=desc, x=x, half_out=dtype == "f16")
    except AssertionError as e:
        print("NORMBUDGET-FAIL %s | %s | %s" % (form, case, e))
        raise
    print("NORMBUDGET %s | %s | %s | %.2f" % (form, case, desc, ratio))
    return ratio


@pytest.mark.parametrize("shape,dtype,family,act,eps", _sweep_cases())
def test_instancenorm_within_the_float64_budget(ctx, request, shape, dtype, family, act, eps):
    """The stand-alone plan on every family, shape and tensor type.

    Measured on an MI355X (largest ratio to E over the shapes): fp32 benign 2.25, mean30 0.63, mean1000 0.50, pivot10 5.65, pivot100 3.08, sparse 5.68,
    constant 0.50, tiny 0.89, mixed 2.04; fp16 at most 0.93 (pivot10) on all eight families.  The fp32 figures of the pivot and sparse planes are those of a
    float64 evaluation of the statistics with multiplier and shift rounded once each: on such a plane E is the model's error at the one outlying output, often
    a twentieth of an ulp, and statistics kept in fp32 (1 to 2 ulps off there) stood at 39 to 160 E.  With the single-sample pivot this sweep replaced, these
    families stood at 7 000 to 160 000 E, in fp32 and fp16, and benign / mixed fp32 planes at 12 to 14 E (DESIGN.md section 3 has the table)."""
    import shadernn_amd as snn

    refs = _refs(shape, dtype, family, act, eps)
    x, beta, gamma = refs[:3]
    plan, desc = _norm_plan(ctx, shape, beta, gamma, act, eps)
    xt = snn.Tensor.from_numpy(ctx, x, dtype=_dt(dtype))
    try:
        got = _run_into_nan(ctx, plan, xt, shape, _dt(dtype))
    finally:
        xt.free()
        plan.destroy()
    _held("standalone-" + dtype, request.node.callspec.id, desc, got, refs, dtype)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("family", ["benign", "pivot100"])
def test_the_fold_is_repeatable(ctx, request, family, dtype):
    """S = 264: some fold threads merge two slab records.  A second run through the same plan is bit-identical (a fixed merge order, nothing left over)."""
    import shadernn_amd as snn

    refs = _refs(BIG, dtype, family, "", 1e-5)
    x, beta, gamma = refs[:3]
    plan, desc = _norm_plan(ctx, BIG, beta, gamma, "", 1e-5)
    xt = snn.Tensor.from_numpy(ctx, x, dtype=_dt(dtype))
    try:
        got, again = (_run_into_nan(ctx, plan, xt, BIG, _dt(dtype)) for _ in range(2))
    finally:
        xt.free()
        plan.destroy()
    _held("standalone-" + dtype, request.node.callspec.id, desc, got, refs, dtype)
    np.testing.assert_array_equal(got, again, err_msg="second run differs: " + desc)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("family", ["mean30", "pivot10"])
@pytest.mark.parametrize("shape", [BIG, RAGGED], ids=_name)
def test_rule_h_is_the_pair_and_the_pair_is_within_the_budget(ctx, request, shape, family, dtype):
    """Graph rule H: the fused norm + Add is bit-identical to the two launches, with a full-size skip and with a ragged one (either summand), and the
    pair's norm -- whose statistics the fused plan shares -- is within the budget, here also where the fold merges more than 256 slab records."""
    import shadernn_amd as snn

    n, h, w, c = shape
    dt = _dt(dtype)
    act = "relu" if family == "pivot10" else ""
    refs = _refs(shape, dtype, family, act, 1e-5)
    x, beta, gamma = refs[:3]
    skip = _rand(shape, 21)
    pre = snn.activation_plan(ctx, n, h, w, c, "tanh")  # a producer in front, so that the norm's input is a graph tensor (never run)
    norm, desc = _norm_plan(ctx, shape, beta, gamma, act, 1e-5)
    add = snn.add_plan(ctx, n, h, w, c, act="")
    xt = snn.Tensor.from_numpy(ctx, x, dtype=dt)
    made = [xt]
    try:
        normed = norm(xt)
        made.append(normed)
        _held("ruleH-pair-" + dtype, request.node.callspec.id, desc, normed.numpy(), refs, dtype)
        for small, order in ((False, [1, -2]), (True, [1, -2]), (True, [-2, 1])):
            s = np.ascontiguousarray(skip[:, : h - 4, : w - 4, :]) if small else skip
            st = snn.Tensor.from_numpy(ctx, s, dtype=dt)
            made.append(st)
            fused = snn.graph_fuse(ctx, [(pre, [-1], False), (norm, [0], False), (add, order, True)])
            fdesc = fused[2][0].describe()
            assert fused[1][0] is None and "+add" in fdesc and ("residual first" in fdesc) == (order[0] == -2), fdesc
            y = _run_into_nan(ctx, fused[2][0], [xt, st], shape, dt)
            assert np.isfinite(y).all(), fdesc
            two = add([normed, st] if order[0] == 1 else [st, normed])
            made.append(two)
            np.testing.assert_array_equal(y, two.numpy(), err_msg=fdesc)
            fused[2][0].destroy()
    finally:
        for t in made:
            t.free()
        for p in (pre, norm, add):
            p.destroy()


# ---------------------------------------------------------------------------------------------------------------- chain rule F
# (N, H, W, IC, OC): 3x3 stride-1 "same" layers of conv2d_wide_f16, whose blocks leave (mean, M2) records of their 8 x 32 / 16 x 32 pixel tiles
F_ONE, F_RAGGED, F_TWO, F_MANY = (1, 8, 32, 16, 128), (1, 33, 70, 16, 128), (2, 37, 45, 64, 32), (1, 100, 130, 16, 128)
F_KINDS = ["bias30", "nearconst", "corner"]


@functools.lru_cache(maxsize=None)
def _conv_refs(shape, kind):
    """A convolution whose output is adverse by construction (operands rounded to half, bias fp32), its float64 result and the pairwise fp32 evaluation:
    bias30 -- a bias of +-30 per channel on an output of unit deviation; nearconst -- weights scaled down by 1e-3 around a bias of 0.5, a few half
    values per plane; corner -- a quiet input with one bright pixel in the corner, which the first thread of the first tile reads first."""
    n, h, w, ic, oc = shape
    x, wt, b = _rand((n, h, w, ic), 41), _rand((oc, ic, 3, 3), 42, 1.0 / np.sqrt(9 * ic)), _rand((oc,), 43, 0.1)
    if kind == "bias30":
        b = (30.0 * np.where(np.arange(oc) % 2 == 0, 1.0, -1.0) + b).astype(np.float32)
    elif kind == "nearconst":
        wt, b = 1e-3 * wt, (0.5 + b).astype(np.float32)
    elif kind == "corner":
        x = 0.05 * x
        x[:, 0, 0, :] = 30.0
    else:
        raise ValueError(kind)
    x, wt = norm_cases._h(x), norm_cases._h(wt)
    pads = O.padding_offsets("same", 3)
    c64 = ref64.conv_layer_general(x, wt, b, 1, pads, "constant", (h, w))
    c32 = ref64.conv_layer_pairwise32(x, wt, b, 1, pads, "constant", (h, w))
    for a in (x, wt, b, c64, c32):
        a.setflags(write=False)
    return x, wt, b, pads, c64, c32


def _tiles(desc, h, w):
    """(tiles per image, PARTS of tile_stats_fold) from the convolution's description "tile=THx32px x BNoc"."""
    m = re.search(r"tile=(\d+)x32px x (\d+)oc", desc)
    assert m, desc
    th, bn = int(m.group(1)), int(m.group(2))
    return -(-h // th) * -(-w // 32), 256 // (bn // 2)


def _rule_f(ctx, monkeypatch, request, shape, kind, route, act, second_input=None):
    """Conv -> InstanceNorm as one chain step on the tile records.  The convolution alone (the same kernel without the statistics epilogue) is held to
    its own budget exactly as tests/test_conv_f16_budget_gpu.py holds it; the norm is then held to the float64 norm of that half tensor, i.e. of the
    float64 convolution rounded to half except where the kernel's fp32 sum, within its allowance of a rounding tie, stored the other neighbour."""
    import shadernn_amd as snn

    n, h, w, ic, oc = shape
    x, wt, b, pads, c64, c32 = _conv_refs(shape, kind)
    beta, gamma = norm_cases.params(oc, seed=7)
    monkeypatch.setenv("SNNHIP_NORM_FUSION", "1")
    monkeypatch.setenv("SNNHIP_CONV", "wide")
    if route == "launches":
        monkeypatch.setenv("SNNHIP_NO_KERNEL_FOLD", "1")
    else:
        monkeypatch.delenv("SNNHIP_NO_KERNEL_FOLD", raising=False)
    conv = snn.conv2d_plan(ctx, n, h, w, wt, b, stride=1, pads=pads, act="", dtype=snn.F16)
    norm = snn.instancenorm_plan(ctx, n, h, w, oc, beta, gamma, act=act, leaky=LEAKY)
    fused = snn.chain_plan(ctx, [conv, norm])
    desc, cdesc = fused.describe(), conv.describe()
    made = []
    try:
        assert WIDE in cdesc and "persistent" not in cdesc, cdesc
        assert fused.num_steps() == 1 and "+tile-stats" in desc, desc
        if route == "kernel":
            assert "+fold" in desc and "instancenorm(1 sweep)" in desc, desc
        else:
            assert "+fold" not in desc and "fold of tile stats + 1 sweep" in desc, desc
        tiles, parts = _tiles(cdesc, h, w)
        if shape == F_ONE:
            assert tiles == 1, cdesc
        if shape == F_MANY:  # tile_stats_fold: thread (channel pair, part) takes B = 16 records per round, PARTS = 256 / (BN / 2) parts
            assert tiles > 16 * parts, "the fold's outer loop no longer runs twice: %d tiles, 16 x %d per round (%s)" % (tiles, parts, cdesc)
        xt = snn.Tensor.from_numpy(ctx, x, dtype=snn.F16)
        made.append(xt)
        c_got = _run_into_nan(ctx, conv, xt, (n, h, w, oc), snn.F16)
        _figures_then_assert(c_got, c64, c32, cdesc)
        want64 = ref64.instancenorm(c_got, beta, gamma, 1e-5, act, LEAKY)
        model32 = ref64.instancenorm32(c_got, beta, gamma, 1e-5, act, LEAKY)
        refs = (c_got, beta, gamma, want64, model32, ref64.norm_floor(c_got, beta, gamma, 1e-5))
        got = _run_into_nan(ctx, fused, xt, (n, h, w, oc), snn.F16)
        case = request.node.callspec.id
        _held("ruleF-" + route, case, desc, got, refs, "f16")
        if second_input is not None:  # other statistics through the same plan, then the first input again: every launch folds its own records
            x2 = _conv_refs(shape, second_input)[0]
            x2t = snn.Tensor.from_numpy(ctx, x2, dtype=snn.F16)
            made.append(x2t)
            c2 = _run_into_nan(ctx, conv, x2t, (n, h, w, oc), snn.F16)
            refs2 = (c2, beta, gamma, ref64.instancenorm(c2, beta, gamma, 1e-5, act, LEAKY), ref64.instancenorm32(c2, beta, gamma, 1e-5, act, LEAKY),
                     ref64.norm_floor(c2, beta, gamma, 1e-5))
            _held("ruleF-" + route, case + "-second-input", desc, _run_into_nan(ctx, fused, x2t, (n, h, w, oc), snn.F16), refs2, "f16")
        again = _run_into_nan(ctx, fused, xt, (n, h, w, oc), snn.F16)
        np.testing.assert_array_equal(got, again, err_msg="a replayed run differs (the block counter of the in-kernel fold?): " + desc)
    finally:
        for t in made:
            t.free()
        _free(fused)


@pytest.mark.parametrize("route", ["kernel", "launches"])
@pytest.mark.parametrize("kind", F_KINDS)
@pytest.mark.parametrize("shape", [F_ONE, F_RAGGED, F_TWO], ids=_name)
def test_rule_f_within_the_budget(ctx, monkeypatch, request, shape, kind, route):
    _rule_f(ctx, monkeypatch, request, shape, kind, route, ACTS[(F_KINDS.index(kind) + (route == "kernel")) % 3])


@pytest.mark.parametrize("route", ["kernel", "launches"])
def test_rule_f_where_the_fold_loops_twice(ctx, monkeypatch, request, route):
    """More tiles than 16 x PARTS: tile_stats_fold's outer loop runs a second time (65 tiles of 8 x 32 pixels at 128 output channels, 64 per round)."""
    _rule_f(ctx, monkeypatch, request, F_MANY, "bias30", route, "")


@pytest.mark.parametrize("route", ["kernel", "launches"])
def test_rule_f_statistics_follow_the_input(ctx, monkeypatch, request, route):
    """The same plan on a second input with other statistics (a counter that is not reset would leave the first run's multiplier and shift in place),
    then the first input again, bit-identical to its first run."""
    _rule_f(ctx, monkeypatch, request, F_RAGGED, "bias30", route, "relu", second_input="corner")
