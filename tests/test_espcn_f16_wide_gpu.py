"""The fused fp16 ESPCN chain at the published widths 1 -> 64 -> 32 -> r*r (espcn_f16_wide.hip, SNNHIP_ESPCN_F16=1) through the C-ABI: two launches on
the f16 matrix cores for upscale 2, 3 and 4, the 8- and 16-bit frame ends folded in, against the oracle with the same quantisation points, the
per-layer fp16 plans of the same build and the fp32 oracle; every other width pair, the option unset and fp32 stay per layer; the 16-channel net keeps
its own kernels; everything once more between red zones (SNNHIP_GUARD=1)."""
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
WIDE = (64, 32)


def _tiles():
    txt = open(os.path.join(ROOT, "shadernn_amd", "csrc", "espcn_f16_wide.h")).read()
    return {k: int(re.search(r"\b%s = (\d+)" % k, txt).group(1)) for k in ("kEspcnF16WideTW_A", "kEspcnF16WideTH_A", "kEspcnF16WideTW_B", "kEspcnF16WideTH_B")}


T = _tiles()
# smaller than any tile with an odd width; batch, ragged in both axes, odd width (the x3 store alignment); whole tiles and a ragged last tile row; one
# row and one column past a tile edge of each kernel (the two coincide while the kernels share a tile size)
SHAPES = list(dict.fromkeys([(1, 5, 7), (2, 19, 33), (1, 40, 48), (1, T["kEspcnF16WideTH_A"] + 1, T["kEspcnF16WideTW_A"] + 1),
                             (1, T["kEspcnF16WideTH_B"] + 1, T["kEspcnF16WideTW_B"] + 1)]))
DEMO = ((127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1), (127.5, 0, 0, 0), (127.5, 0, 0, 0))  # means, norms, scale, offset (tests/test_frame_u8_gpu.py)
# (means, norms, scale, offset, maxval, shift): 10 bits in the high bits of the container (P010), and all 16 bits (tests/test_frame_u16_gpu.py)
P010 = ((511.5, 0, 0, 0), (1 / 511.5, 1, 1, 1), (511.5, 0, 0, 0), (511.5, 0, 0, 0), 1023, 6)
FULL16 = ((32767.5, 0, 0, 0), (1 / 32767.5, 1, 1, 1), (32767.5, 0, 0, 0), (32767.5, 0, 0, 0), 65535, 0)


@pytest.fixture
def f16_rules():
    from shadernn_amd import capi

    capi.set_option("SNNHIP_ESPCN_F16", "1")
    yield
    capi.set_option("SNNHIP_ESPCN_F16", None)


@functools.lru_cache(maxsize=None)
def _net(r, variant="plain", widths=WIDE):
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r, widths=widths)
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
    if variant == "k3":  # a 3x3 first convolution: the centre of the 5x5 one
        l0 = net["layers"][0]
        l0["w"] = np.ascontiguousarray(l0["w"][:, :, 1:4, 1:4])
        l0["kernel"] = 3
    return net


@functools.lru_cache(maxsize=None)
def _case(r, n, h, w, variant="plain", widths=WIDE):
    """(input, quantised oracle, fp32 oracle) of one case, computed once and shared (read-only)."""
    net = _net(r, variant, widths)
    x = np.random.default_rng(8).random((n, h, w, 1), dtype=np.float32)
    head = dict(net, layers=net["layers"][:-1])
    want16 = O._h(O.subpixel(O.forward(head, x, fp16=True), r, 0))
    want32 = O.subpixel(O.forward(head, x), r, 0)
    for a in (x, want16, want32):
        a.setflags(write=False)
    return x, want16, want32


def _layer_plans(ctx, net, n, h, w, dtype=None):
    from shadernn_amd import capi
    from shadernn_amd.runner import _layer_plan

    plans, shape = [], (n, h, w, 1)
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape, capi.F16 if dtype is None else dtype)
        plans.append(p)
        shape = p.out_shape()
    return plans


def _one_by_one(ctx, plans, src, raw=None):
    """The plans run one after the other; raw: the dtype of the last plan's output frame (U8 / U16), None = halfs."""
    from shadernn_amd import capi

    for k, p in enumerate(plans):
        last = raw is not None and k == len(plans) - 1
        dst = capi.Tensor(ctx, *p.out_shape(), dtype=raw if last else capi.F16)
        p.run(src, dst)
        src = dst
    return src


def _steps(chain):
    return [chain.step_describe(i) for i in range(chain.num_steps())]


def _nan_filled(ctx, n, h, w):
    from shadernn_amd import capi

    return capi.Tensor.from_numpy(ctx, np.full((n, h, w, 1), np.nan, np.float32), dtype=capi.F16)


def _check_fused(ctx, r, n, h, w, variant="plain"):
    """The assertions every fused case shares; returns (chain, steps)."""
    from shadernn_amd import capi

    net = _net(r, variant)
    x, want16, want32 = _case(r, n, h, w, variant)
    plans = _layer_plans(ctx, net, n, h, w)
    chain = capi.chain_plan(ctx, plans)
    steps = _steps(chain)
    assert len(steps) == 2 and all(s.startswith("fused[") and "mfma_f32_16x16x32_f16" in s for s in steps), steps  # (the parent commit: four steps)
    assert "kernel=espcn_f16_wide_conv_pair_kernel " in steps[0] and "kernel=espcn_f16_wide_d2s_kernel<%d> " % r in steps[1], steps
    assert "tile=%dx%d" % (T["kEspcnF16WideTW_A"], T["kEspcnF16WideTH_A"]) in steps[0] and "tile=%dx%d" % (T["kEspcnF16WideTW_B"], T["kEspcnF16WideTH_B"]) in steps[1]
    xt = capi.Tensor.from_numpy(ctx, x, dtype=capi.F16)
    yt = _nan_filled(ctx, n, r * h, r * w)
    chain.run(xt, yt)
    y = yt.numpy()
    per_layer = _one_by_one(ctx, plans, xt).numpy()
    print("r=%d %dx%dx%d %s: max |fused - quantised oracle| %.3e, |fused - per layer| %.3e, |fused - fp32 oracle| %.3e, |per layer - quantised oracle| %.3e"
          % (r, n, h, w, variant, np.abs(y - want16).max(), np.abs(y - per_layer).max(), np.abs(y - want32).max(), np.abs(per_layer - want16).max()))
    assert np.isfinite(y).all(), "an output pixel was not written"
    np.testing.assert_allclose(per_layer, want16, err_msg="the per-layer fp16 plans against the quantised oracle", **TOLH)
    np.testing.assert_allclose(y, want16, err_msg="; ".join(steps), **TOLH)
    np.testing.assert_allclose(y, per_layer, err_msg="; ".join(steps), **TOLH)
    assert np.abs(y - want32).max() < 0.02, steps
    return chain, steps


@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("r", [2, 3, 4])
def test_fused_wide_chain_is_two_f16_launches_within_the_fp16_bounds(ctx, f16_rules, r, n, h, w):
    _check_fused(ctx, r, n, h, w)


@pytest.mark.parametrize("r", [2, 3])
def test_fused_wide_chain_with_bn_and_other_activations(ctx, f16_rules, r):
    _check_fused(ctx, r, 1, 21, 35, "acts")


def test_a_3x3_first_convolution_takes_the_rule_too(ctx, f16_rules):
    _, steps = _check_fused(ctx, 2, 1, 18, 37, "k3")
    assert "fused[conv3x3(1->64)+conv3x3(64->32)]" in steps[0], steps


@pytest.mark.parametrize("r,k", [(2, 5), (3, 5), (4, 3)])
def test_step_costs_and_issued_mfma_flops(ctx, f16_rules, r, k):
    """The steps are priced on their own bytes (fp16 = 2 B), their flops are the layers' flops, and mfma_flops counts what the kernels issue (16384 per
    16x16x32 MFMA): per tile of kernel A, 4 row blocks for each of the 22 sixteen-pixel groups of the 10 x 34 halo region and 18 K-steps x 2 row
    blocks for each of the 16 groups of the tile; per tile of kernel B, 9 K-steps for each of 16 groups."""
    from shadernn_amd import capi

    n, h, w = 2, 19, 33
    c1, c2 = WIDE
    net = _net(r, "k3" if k == 3 else "plain")
    plans = _layer_plans(ctx, net, n, h, w)
    chain = capi.chain_plan(ctx, plans)
    steps = _steps(chain)
    assert len(steps) == 2, steps
    px = n * h * w
    assert chain.step_cost(0)[1] == pytest.approx(2.0 * (px * (1 + c2) + c1 * k * k + c1 * c2 * 9))
    assert chain.step_cost(1)[1] == pytest.approx(2.0 * (px * (c2 + r * r) + r * r * c2 * 9))
    assert chain.step_cost(0)[0] == pytest.approx(plans[0].cost()[0] + plans[1].cost()[0])
    assert chain.step_cost(1)[0] == pytest.approx(plans[2].cost()[0] + plans[3].cost()[0])
    ta = n * -(-h // T["kEspcnF16WideTH_A"]) * -(-w // T["kEspcnF16WideTW_A"])
    tb = n * -(-h // T["kEspcnF16WideTH_B"]) * -(-w // T["kEspcnF16WideTW_B"])
    groups1 = -(-((T["kEspcnF16WideTH_A"] + 2) * (T["kEspcnF16WideTW_A"] + 2)) // 16)
    groups1 += groups1 % 2  # the waves take two groups a turn
    groups2 = T["kEspcnF16WideTH_A"] * T["kEspcnF16WideTW_A"] // 16
    flops = [float(re.search(r"mfma_flops=(\S+)", s).group(1)) for s in steps]
    assert flops[0] == pytest.approx(ta * 16384.0 * (groups1 * (c1 // 16) + groups2 * (9 * c1 // 32) * (c2 // 16)), rel=1e-5)
    assert flops[1] == pytest.approx(tb * 16384.0 * (T["kEspcnF16WideTH_B"] * T["kEspcnF16WideTW_B"] // 16) * (9 * c2 // 32), rel=1e-5)


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
    c1, c2 = WIDE
    body = _layer_plans(ctx, _net(r), n, h, w)
    head = capi.u8_in_plan(ctx, n, h, w, 1, means, norms, dtype=capi.F16)
    tail = capi.u8_out_plan(ctx, n, r * h, r * w, 1, scale, offset, dtype=capi.F16)
    chain = capi.chain_plan(ctx, [head] + body + [tail])
    steps = _steps(chain)
    assert len(steps) == 2 and all("fused[" in s and "espcn_f16_wide_" in s for s in steps), steps
    assert "u8_in(1ch)" in steps[0] and "u8_out(1ch)" in steps[1], steps
    assert "espcn_f16_wide_conv_pair_kernel<u8>" in steps[0] and "espcn_f16_wide_d2s_kernel<%d,u8>" % r in steps[1], steps
    px = n * h * w
    assert chain.step_cost(0)[1] == pytest.approx(2.0 * (px * (1 + c2) + c1 * 25 + c1 * c2 * 9) - px)
    assert chain.step_cost(1)[1] == pytest.approx(2.0 * (px * (c2 + r * r) + r * r * c2 * 9) - r * r * px)
    xt = capi.Tensor.from_numpy(ctx, _frame(n, h, w, 7), dtype=capi.U8)
    yt = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=capi.U8)
    chain.run(xt, yt)
    # bit-identical to the u8_in plan, the fused fp16 chain and the u8_out plan run one by one
    fused_body = capi.chain_plan(ctx, body)
    assert fused_body.num_steps() == 2
    want = _one_by_one(ctx, [head, fused_body, tail], xt, raw=capi.U8).numpy_u8()
    np.testing.assert_array_equal(yt.numpy_u8(), want, err_msg="; ".join(steps))


def _frame16(n, h, w, seed, maxval, shift):
    u = np.random.default_rng(seed).integers(0, maxval + 1, size=(n, h, w, 1)).astype(np.uint16)
    u.reshape(-1)[:4] = (0, maxval, (maxval + 1) // 2, 1)
    return (u << shift).astype(np.uint16)


@pytest.mark.parametrize("conv", [P010, FULL16], ids=["p010", "full16"])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_16bit_ends_fold_into_the_two_launches(ctx, f16_rules, r, conv):
    from shadernn_amd import capi

    n, h, w = 2, 19, 33
    means, norms, scale, offset, maxval, shift = conv
    body = _layer_plans(ctx, _net(r), n, h, w)
    head = capi.u16_in_plan(ctx, n, h, w, 1, means, norms, shift=shift, dtype=capi.F16)
    tail = capi.u16_out_plan(ctx, n, r * h, r * w, 1, scale, offset, maxval=maxval, shift=shift, dtype=capi.F16)
    chain = capi.chain_plan(ctx, [head] + body + [tail])
    steps = _steps(chain)
    assert len(steps) == 2, steps
    assert "u16_in(1ch)" in steps[0] and "espcn_f16_wide_conv_pair_u16_kernel" in steps[0], steps
    assert "u16_out(1ch)" in steps[1] and "espcn_f16_wide_d2s_u16_kernel<%d>" % r in steps[1], steps
    xt = capi.Tensor.from_numpy(ctx, _frame16(n, h, w, 11, maxval, shift), dtype=capi.U16)
    yt = capi.Tensor.from_numpy(ctx, np.full((n, r * h, r * w, 1), 0xFFFF, np.uint16))  # (0xFFFF has bits the P010 container never carries)
    chain.run(xt, yt)
    got = yt.numpy_u16()
    fused_body = capi.chain_plan(ctx, body)
    assert fused_body.num_steps() == 2
    want = _one_by_one(ctx, [head, fused_body, tail], xt, raw=capi.U16).numpy_u16()
    np.testing.assert_array_equal(got, want, err_msg="; ".join(steps))
    assert int(got.max()) <= (maxval << shift) and not np.any(got & ((1 << shift) - 1)), "bits outside the container's layout"


def _stays_per_layer(ctx, net, case, dtype):
    import shadernn_amd as snn
    from shadernn_amd import capi

    r, n, h, w = 3, 2, 19, 33
    x, want16, _ = case
    plans = _layer_plans(ctx, net, n, h, w, dtype)
    try:
        chain = capi.chain_plan(ctx, plans)
    except capi.SnnHipError as e:
        assert e.code == capi.E_UNSUPPORTED, str(e)
    else:
        assert not any("fused[" in s for s in _steps(chain)), _steps(chain)
    runner = snn.GraphRunner(ctx, net, n, h, w, dtype=snn.F16 if dtype == capi.F16 else snn.F32)
    assert not any("fused[" in d for d in runner.describe()), runner.describe()
    y = runner(x)
    print("max |per layer - quantised oracle| %.3e" % np.abs(y - want16).max())
    np.testing.assert_allclose(y, want16, **TOLH)


@pytest.mark.parametrize("widths", [(32, 32), (64, 16)])
def test_other_width_pairs_stay_per_layer(ctx, f16_rules, widths):
    from shadernn_amd import capi

    _stays_per_layer(ctx, _net(3, "plain", widths), _case(3, 2, 19, 33, "plain", widths), capi.F16)


def test_with_the_option_unset_the_wide_fp16_chain_stays_per_layer(ctx):
    from shadernn_amd import capi

    assert capi.get_option("SNNHIP_ESPCN_F16") is None
    _stays_per_layer(ctx, _net(3), _case(3, 2, 19, 33), capi.F16)


def test_the_wide_net_in_fp32_stays_per_layer(ctx, f16_rules):
    from shadernn_amd import capi

    _stays_per_layer(ctx, _net(3), _case(3, 2, 19, 33), capi.F32)


@pytest.mark.parametrize("r", [2, 3, 4])
def test_the_narrow_net_keeps_its_own_kernels(ctx, f16_rules, r):
    from shadernn_amd import capi

    n, h, w = 1, 9, 33
    plans = _layer_plans(ctx, _net(r, "plain", (16, 16)), n, h, w)
    steps = _steps(capi.chain_plan(ctx, plans))
    assert len(steps) == 2 and "kernel=espcn_f16_conv_pair_kernel " in steps[0] and "kernel=espcn_f16_d2s_kernel<%d> " % r in steps[1], steps


def test_the_shape_sweep_is_clean_under_the_guard(ctx):
    """Every shape, every factor, fp16 and 8-bit ends, with each allocation between red zones: a fresh process (the mode is fixed at the library's
    first allocation), ending in a clean snnhip_guard_check."""
    code = """
        import numpy as np
        import shadernn_amd as snn
        from shadernn_amd import capi
        import test_espcn_f16_wide_gpu as t
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
                assert chain.num_steps() == 2 and "espcn_f16_wide" in chain.describe(), chain.describe()
                xt = capi.Tensor.from_numpy(ctx, x, dtype=capi.F16)
                yt = t._nan_filled(ctx, n, r * h, r * w)
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
                np.testing.assert_array_equal(qt.numpy_u8(), t._one_by_one(ctx, [head, chain, tail], ut, raw=capi.U8).numpy_u8())
                ctx.sync()
        capi.check(capi.lib().snnhip_guard_check(ctx.h))
        print("GUARD-OK")
    """
    env = dict(os.environ, SNNHIP_GUARD="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0 and "GUARD-OK" in p.stdout, p.stdout[-3000:]
