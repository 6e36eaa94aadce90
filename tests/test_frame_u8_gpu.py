"""8-bit frames at both ends of a model: the stand-alone u8_in / u8_out plans against their numpy contract, chain rules A8 / B8 (the conversions
folded into the ESPCN kernels) bit-identical to the same plans run one by one, and the quantised oracle."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


def _q_ref(x, scale, offset):
    """numpy statement of the u8_out contract: clamp(rint(fmaf(x, scale, offset)), 0, 255), NaN -> 0.  The product and sum are formed in float64
    and rounded to float32: a single rounding (= fmaf) only while the float64 sum is exact, which holds for the power-of-two scales and small
    offsets used here; other constants would need math.fma / exact rationals."""
    C = x.shape[-1]
    s = np.asarray(scale[:C], np.float32).astype(np.float64)
    o = np.asarray(offset[:C], np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x.astype(np.float64) * s + o).astype(np.float32)  # the float64 product is exact; the sum is exact for these constants
        y = np.rint(y)
        y = np.where(np.isnan(y), 0.0, np.clip(y, 0.0, 255.0))
    return y.astype(np.uint8)


def _in_ref(u, means, norms, half):
    C = u.shape[-1]
    m = np.asarray(means[:C], np.float32)
    n = np.asarray(norms[:C], np.float32)
    y = (u.astype(np.float32) - m) * n
    return y.astype(np.float16).astype(np.float32) if half else y


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_u8_out_matches_contract_exactly(ctx, half, C):
    from shadernn_amd import capi

    N, H, W = 2, 5, 37  # odd W: 370 pixels, a tail of 2
    rng = np.random.default_rng(C)
    x = (rng.standard_normal((N, H, W, C)) * 200 + 100).astype(np.float32)
    crafted = np.array([0.5, 1.5, 2.5, 254.5, -0.49, 255.5, 1e30, np.inf, -np.inf, np.nan, -1e30, 3.5, 127.5, 0.0, -0.0, 255.0], np.float32)
    flat = x.reshape(-1)
    flat[: crafted.size] = crafted
    flat[-crafted.size:] = crafted[::-1]
    scale, offset = (1.0, 0.5, 2.0, 1.0), (0.0, 0.25, -3.0, 0.0)
    if half:
        flat[np.abs(flat) > 60000] = np.sign(flat[np.abs(flat) > 60000]) * np.inf
        x = x.astype(np.float16).astype(np.float32)
    dt = capi.F16 if half else capi.F32
    plan = capi.u8_out_plan(ctx, N, H, W, C, scale, offset, dtype=dt)
    assert "u8_out_kernel" in plan.describe()
    flops, nbytes = plan.cost()
    assert nbytes == N * H * W * C * (1 + (2 if half else 4))
    t = capi.Tensor.from_numpy(ctx, x, dtype=dt)
    y = capi.Tensor(ctx, N, H, W, C, dtype=capi.U8)
    plan.run(t, y)
    got = y.numpy_u8()
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, _q_ref(x, scale, offset))


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_u8_in_matches_contract_exactly(ctx, half, C):
    from shadernn_amd import capi

    N, H, W = 2, 3, 43
    u = (np.arange(N * H * W * C) % 256).astype(np.uint8).reshape(N, H, W, C)
    np.random.default_rng(5).shuffle(u.reshape(-1))
    means, norms = (127.5, 0.0, 13.25, 255.0), (1 / 127.5, 1 / 255.0, 0.37, -2.0)
    dt = capi.F16 if half else capi.F32
    plan = capi.u8_in_plan(ctx, N, H, W, C, means, norms, dtype=dt)
    assert "u8_in_kernel" in plan.describe()
    x = capi.Tensor.from_numpy(ctx, u, dtype=capi.U8)
    y = capi.Tensor(ctx, N, H, W, C, dtype=dt)
    plan.run(x, y)
    np.testing.assert_array_equal(y.numpy(), _in_ref(u, means, norms, half))


def _espcn_plans(ctx, net, n, h, w, u8in, u8out, means, norms, scale, offset):
    from shadernn_amd import capi
    from shadernn_amd.runner import _layer_plan

    plans, shape = [], (n, h, w, 1)
    if u8in:
        plans.append(capi.u8_in_plan(ctx, n, h, w, 1, means, norms))
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape)
        plans.append(p)
        shape = p.out_shape()
    if u8out:
        plans.append(capi.u8_out_plan(ctx, *shape, scale, offset))
    return plans


def _run_unfused(ctx, plans, x):
    """The same plans one by one: the u8_in launch, the fp32 ESPCN chain (rules A + B, or whatever the switches select), the u8_out launch."""
    from shadernn_amd import capi

    head = plans[0] if "u8_in" in plans[0].describe() else None
    tail = plans[-1] if "u8_out" in plans[-1].describe() else None
    body = capi.chain_plan(ctx, plans[(1 if head else 0):(len(plans) - 1 if tail else len(plans))])
    src = x
    for p, u8 in ((head, False), (body, False), (tail, True)):
        if p is None:
            continue
        dst = capi.Tensor(ctx, *p.out_shape(), dtype=capi.U8 if u8 else capi.F32)
        p.run(src, dst)
        src = dst
    return src.numpy_u8() if src.dtype == capi.U8 else src.numpy()


def _frame(n, h, w, seed):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 256, size=(n, h, w, 1), dtype=np.uint8)
    k = min(4, u.size)
    u.reshape(-1)[:k] = (0, 255, 128, 1)[:k]
    return u


CONVENTIONS = [((127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1), (127.5, 0, 0, 0), (127.5, 0, 0, 0)),  # the ShaderNN demo's normalisation, tanh output back to bytes
               ((0, 0, 0, 0), (1 / 255.0, 1, 1, 1), (255.0, 0, 0, 0), (0, 0, 0, 0))]  # the Keras script's Y plane /255 ... *255


# the 1080p frame with both ends 8-bit; the halves (8-bit in, fp32 out and the reverse) at the smaller sizes
@pytest.mark.parametrize("n,h,w,ends", [(1, 1080, 1920, "both")] + [(n, h, w, e) for (n, h, w) in [(3, 37, 53), (1, 8, 8), (1, 1, 1)] for e in ("both", "in", "out")])
def test_fused_u8_chain_is_bit_identical_to_the_plans_one_by_one(ctx, n, h, w, ends):
    from shadernn_amd import capi, models

    net = models.espcn_weights(seed=3)
    means, norms, scale, offset = CONVENTIONS[0]
    u8in, u8out = ends in ("both", "in"), ends in ("both", "out")
    plans = _espcn_plans(ctx, net, n, h, w, u8in, u8out, means, norms, scale, offset)
    chain = capi.chain_plan(ctx, plans)
    desc = chain.describe()
    assert chain.num_steps() == 2, desc
    steps = [chain.step_describe(i) for i in range(2)]
    assert ("conv_kxk_c1o16_wino3x3_c16o16_u8_kernel" in steps[0]) == u8in, steps
    assert ("conv3x3_c16o4_d2s_tanh_u8_kernel" in steps[1]) == u8out, steps
    u = _frame(n, h, w, n * h + w)
    x_host = u if u8in else _in_ref(u, means, norms, False)
    x = capi.Tensor.from_numpy(ctx, x_host, dtype=capi.U8 if u8in else capi.F32)
    y = capi.Tensor(ctx, n, 2 * h, 2 * w, 1, dtype=capi.U8 if u8out else capi.F32)
    chain.run(x, y)
    got = y.numpy_u8() if u8out else y.numpy()
    want = _run_unfused(ctx, plans, x)
    np.testing.assert_array_equal(got, want, err_msg=desc)
    # the fused plan's own bytes: 1 B per input pixel / output pixel instead of 4
    f0, b0 = chain.step_cost(0)
    f1, b1 = chain.step_cost(1)
    px = n * h * w
    assert b0 == pytest.approx(4.0 * (px * (1 + 16) + 16 * 25 + 16 * 16 * 9) - (3.0 * px if u8in else 0.0))
    assert b1 == pytest.approx(4.0 * (px * (16 + 4) + 4 * 16 * 9) - (12.0 * px if u8out else 0.0))


@pytest.mark.parametrize("switch", [("SNNHIP_ESPCN_A", "direct"), ("SNNHIP_ESPCN_B", "wino"), ("SNNHIP_ESPCN_FUSION", "stream")])
@pytest.mark.parametrize("n,h,w", [(3, 37, 53), (1, 8, 8)])
def test_u8_chain_under_the_other_kernel_forms(ctx, monkeypatch, switch, n, h, w):
    """Where no 8-bit form of a kernel exists the conversion stays a launch of its own; the bytes are still the one-by-one bytes."""
    from shadernn_amd import capi, models

    monkeypatch.setenv(*switch)
    net = models.espcn_weights(seed=4)
    means, norms, scale, offset = CONVENTIONS[1]
    plans = _espcn_plans(ctx, net, n, h, w, True, True, means, norms, scale, offset)
    chain = capi.chain_plan(ctx, plans)
    steps = [chain.step_describe(i) for i in range(chain.num_steps())]
    if switch[0] == "SNNHIP_ESPCN_A":
        assert steps[0].startswith("u8_in") and "conv3x3_c16o4_d2s_tanh_u8_kernel" in steps[-1], steps
    elif switch[0] == "SNNHIP_ESPCN_B":
        assert "conv_kxk_c1o16_wino3x3_c16o16_u8_kernel" in steps[0] and steps[-1].startswith("u8_out"), steps
    else:
        assert steps[0].startswith("u8_in") and steps[-1].startswith("u8_out") and len(steps) == 3, steps
    u = _frame(n, h, w, 11)
    x = capi.Tensor.from_numpy(ctx, u, dtype=capi.U8)
    y = capi.Tensor(ctx, n, 2 * h, 2 * w, 1, dtype=capi.U8)
    chain.run(x, y)
    np.testing.assert_array_equal(y.numpy_u8(), _run_unfused(ctx, plans, x))


@pytest.mark.parametrize("conv", [0, 1])
@pytest.mark.parametrize("n,h,w", [(2, 19, 71), (1, 72, 96)])
def test_fused_u8_chain_against_the_quantised_oracle(ctx, conv, n, h, w):
    from shadernn_amd import capi, models

    net = models.espcn_weights(seed=1)
    means, norms, scale, offset = CONVENTIONS[conv]
    plans = _espcn_plans(ctx, net, n, h, w, True, True, means, norms, scale, offset)
    chain = capi.chain_plan(ctx, plans)
    u = _frame(n, h, w, 7)
    x = capi.Tensor.from_numpy(ctx, u, dtype=capi.U8)
    y = capi.Tensor(ctx, n, 2 * h, 2 * w, 1, dtype=capi.U8)
    chain.run(x, y)
    got = y.numpy_u8().astype(np.int32)
    pre = O.espcn_forward(net, _in_ref(u, means, norms, False)).astype(np.float64) * scale[0] + offset[0]
    want = np.clip(np.rint(pre), 0, 255).astype(np.int32)
    assert np.max(np.abs(got - want)) <= 1
    frac = np.abs(pre - np.floor(pre) - 0.5)
    safe = (frac > 0.02) | (pre < -0.5) | (pre > 255.5)
    np.testing.assert_array_equal(got[safe], want[safe])


def test_graph_fuse_folds_the_conversions_into_two_launches(ctx):
    from shadernn_amd import capi, models

    n, h, w = 1, 24, 40
    net = models.espcn_weights(seed=1)
    means, norms, scale, offset = CONVENTIONS[0]
    plans = _espcn_plans(ctx, net, n, h, w, True, True, means, norms, scale, offset)
    nodes = [(p, [k - 1 if k else -1], k == len(plans) - 1) for k, p in enumerate(plans)]
    fused = capi.graph_fuse(ctx, nodes)
    live = [(p, ins) for p, ins in fused if p is not None]
    assert len(live) == 1
    plan, ins = live[0]
    assert ins == [-1] and plan.num_steps() == 2
    assert "u8_kernel" in plan.step_describe(0) and "u8_kernel" in plan.step_describe(1)
    u = _frame(n, h, w, 2)
    x = capi.Tensor.from_numpy(ctx, u, dtype=capi.U8)
    y = capi.Tensor(ctx, n, 2 * h, 2 * w, 1, dtype=capi.U8)
    plan.run(x, y)
    np.testing.assert_array_equal(y.numpy_u8(), _run_unfused(ctx, plans, x))


def test_captured_graph_replays_fresh_frames(ctx):
    from shadernn_amd import capi, models

    n, h, w = 2, 33, 47
    net = models.espcn_weights(seed=1)
    means, norms, scale, offset = CONVENTIONS[0]
    plans = _espcn_plans(ctx, net, n, h, w, True, True, means, norms, scale, offset)
    chain = capi.chain_plan(ctx, plans)
    x = capi.Tensor(ctx, n, h, w, 1, dtype=capi.U8)
    y = capi.Tensor(ctx, n, 2 * h, 2 * w, 1, dtype=capi.U8)
    x.upload_u8(_frame(n, h, w, 0))
    with capi.Graph.capture(ctx) as g:
        chain.run(x, y)
    for seed in (1, 2, 3):
        u = _frame(n, h, w, seed)
        x.upload_u8(u)
        g.launch()
        got = y.numpy_u8()
        np.testing.assert_array_equal(got, _run_unfused(ctx, plans, x))
    g.destroy()


def test_errors_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    for kw in (dict(N=0, H=4, W=4, Cc=1), dict(N=1, H=4, W=4, Cc=5), dict(N=1, H=4, W=4, Cc=0), dict(N=1, H=4, W=4, Cc=1, dtype=capi.U8)):
        for make in (capi.u8_in_plan, capi.u8_out_plan):
            with pytest.raises(capi.SnnHipError) as e:
                make(ctx, **kw)
            assert e.value.code == -1 and ("desc" in str(e.value))
    t = capi.Tensor(ctx, 1, 3, 5, 1, dtype=capi.U8)
    buf = np.zeros(14, np.uint8)
    rc = capi.lib().snnhip_tensor_download_raw(t.h, buf.ctypes.data_as(capi._P), buf.size)
    assert rc == -1 and b"15" in capi.lib().snnhip_last_error()
    plan = capi.u8_out_plan(ctx, 1, 3, 5, 1)
    with pytest.raises(capi.SnnHipError):  # float output tensor for an 8-bit plan
        plan.run(capi.Tensor(ctx, 1, 3, 5, 1), capi.Tensor(ctx, 1, 3, 5, 1))
