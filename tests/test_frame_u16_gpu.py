"""16-bit frames (10 / 12 / 16-bit video in 2-byte containers) at both ends of a model: the stand-alone u16_in / u16_out plans against a numpy
statement of their contract, exactly; the conversions folded into the fp32 ESPCN kernels bit-identical to the same plans run one by one; the
quantised oracle."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

LAYOUTS = [(1023, 0), (1023, 6), (4095, 0), (65535, 0)]  # low-aligned 10-bit, P010-style high-aligned 10-bit, low-aligned 12-bit, full 16-bit


def _q_ref(x, scale, offset, maxval, shift):
    """numpy statement of the u16_out contract: unsigned(clamp(rint(fmaf(x, scale, offset)), 0, maxval)) << shift, NaN -> 0.  The product and sum are
    formed in float64 and rounded to float32: a single rounding (= fmaf) only while the float64 sum is exact or the addend is below half an ulp of the
    product, which holds for the power-of-two scales and small offsets used here (as in test_frame_u8_gpu._q_ref)."""
    C = x.shape[-1]
    s = np.asarray(scale[:C], np.float32).astype(np.float64)
    o = np.asarray(offset[:C], np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x.astype(np.float64) * s + o).astype(np.float32)
        y = np.rint(y)
        y = np.where(np.isnan(y), 0.0, np.clip(y, 0.0, float(maxval)))
    return (y.astype(np.uint32) << shift).astype(np.uint16)


def _in_ref(u, means, norms, shift, half):
    C = u.shape[-1]
    m = np.asarray(means[:C], np.float32)
    n = np.asarray(norms[:C], np.float32)
    y = ((u >> shift).astype(np.float32) - m) * n  # float32 throughout: a subtract, then a multiply
    return y.astype(np.float16).astype(np.float32) if half else y


@pytest.mark.parametrize("maxval,shift", LAYOUTS)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_u16_out_matches_contract_exactly(ctx, half, C, maxval, shift):
    from shadernn_amd import capi

    N, H, W = 2, 5, 37  # 370 pixels: a tail of 2
    rng = np.random.default_rng(C)
    x = rng.uniform(-0.1 * maxval, 1.1 * maxval, size=(N, H, W, C)).astype(np.float32)
    m = float(maxval)
    crafted = np.array([0.5, 1.5, 2.5, m - 0.5, -0.49, m + 0.5, 1e30, np.inf, -np.inf, np.nan, -1e30, 3.5, m / 2, 0.0, -0.0, m], np.float32)
    flat = x.reshape(-1)
    flat[: crafted.size] = crafted
    flat[-crafted.size:] = crafted[::-1]
    scale, offset = (1.0, 0.5, 2.0, 1.0), (0.0, 0.25, -3.0, 0.0)
    if half:
        big = np.abs(flat) > 60000
        flat[big] = np.sign(flat[big]) * np.inf
        x = x.astype(np.float16).astype(np.float32)
    dt = capi.F16 if half else capi.F32
    plan = capi.u16_out_plan(ctx, N, H, W, C, scale, offset, maxval=maxval, shift=shift, dtype=dt)
    desc = plan.describe()
    assert desc.startswith("u16_out_%s c=%d" % ("f16" if half else "f32", C)) and "kernel=u16_out_kernel" in desc, desc
    flops, nbytes = plan.cost()
    assert nbytes == N * H * W * C * (2 + (2 if half else 4))
    t = capi.Tensor.from_numpy(ctx, x, dtype=dt)
    y = capi.Tensor.from_numpy(ctx, np.full((N, H, W, C), 0xFFFF, np.uint16))
    assert y.dtype == capi.U16
    plan.run(t, y)
    got = y.numpy_u16()
    assert got.dtype == np.uint16
    np.testing.assert_array_equal(got, _q_ref(x, scale, offset, maxval, shift))


@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_u16_in_matches_contract_exactly(ctx, half, C, shift):
    from shadernn_amd import capi

    N, H, W = 2, 3, 43  # 258 pixels: a tail of 2
    u = np.linspace(0, 65535, N * H * W * C).astype(np.uint16)  # a ramp through the whole range, both ends included
    np.random.default_rng(5).shuffle(u)
    u = u.reshape(N, H, W, C)
    means, norms = (511.5, 0.0, 13.25, 1023.0), (1 / 511.5, 1 / 1023.0, 0.37, -0.25)
    dt = capi.F16 if half else capi.F32
    plan = capi.u16_in_plan(ctx, N, H, W, C, means, norms, shift=shift, dtype=dt)
    desc = plan.describe()
    assert desc.startswith("u16_in_%s c=%d" % ("f16" if half else "f32", C)) and "kernel=u16_in_kernel" in desc, desc
    flops, nbytes = plan.cost()
    assert nbytes == N * H * W * C * (2 + (2 if half else 4))
    x = capi.Tensor.from_numpy(ctx, u)
    y = capi.Tensor(ctx, N, H, W, C, dtype=dt)
    plan.run(x, y)
    np.testing.assert_array_equal(y.numpy(), _in_ref(u, means, norms, shift, half))


# (means, norms, scale, offset, maxval, shift)
SYM10 = ((511.5, 0, 0, 0), (1 / 511.5, 1, 1, 1), (511.5, 0, 0, 0), (511.5, 0, 0, 0), 1023, 0)
P010 = ((511.5, 0, 0, 0), (1 / 511.5, 1, 1, 1), (511.5, 0, 0, 0), (511.5, 0, 0, 0), 1023, 6)
KERAS10 = ((0, 0, 0, 0), (1 / 1023.0, 1, 1, 1), (1023.0, 0, 0, 0), (0, 0, 0, 0), 1023, 0)
SYM12 = ((2047.5, 0, 0, 0), (1 / 2047.5, 1, 1, 1), (2047.5, 0, 0, 0), (2047.5, 0, 0, 0), 4095, 0)
FULL16 = ((32767.5, 0, 0, 0), (1 / 32767.5, 1, 1, 1), (32767.5, 0, 0, 0), (32767.5, 0, 0, 0), 65535, 0)


def _espcn_plans(ctx, net, n, h, w, conv, u16in=True, u16out=True, dtype=None):
    from shadernn_amd import capi
    from shadernn_amd.runner import _layer_plan

    dtype = capi.F32 if dtype is None else dtype
    means, norms, scale, offset, maxval, shift = conv
    plans, shape = [], (n, h, w, 1)
    if u16in:
        plans.append(capi.u16_in_plan(ctx, n, h, w, 1, means, norms, shift=shift, dtype=dtype))
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape, dtype)
        plans.append(p)
        shape = p.out_shape()
    if u16out:
        plans.append(capi.u16_out_plan(ctx, *shape, scale, offset, maxval=maxval, shift=shift, dtype=dtype))
    return plans


def _run_one_by_one(ctx, plans, x, dtype=None):
    """The same plans as three separate runs: the u16_in launch, the ESPCN chain on float tensors, the u16_out launch."""
    from shadernn_amd import capi

    dtype = capi.F32 if dtype is None else dtype
    head = plans[0] if plans[0].describe().startswith("u16_in") else None
    tail = plans[-1] if plans[-1].describe().startswith("u16_out") else None
    body = capi.chain_plan(ctx, plans[(1 if head else 0):(len(plans) - 1 if tail else len(plans))])
    src = x
    for p, raw in ((head, False), (body, False), (tail, True)):
        if p is None:
            continue
        dst = capi.Tensor(ctx, *p.out_shape(), dtype=capi.U16 if raw else dtype)
        p.run(src, dst)
        src = dst
    return src.numpy_u16() if src.dtype == capi.U16 else src.numpy()


def _frame(n, h, w, seed, maxval, shift):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, maxval + 1, size=(n, h, w, 1)).astype(np.uint16)
    k = min(4, u.size)
    u.reshape(-1)[:k] = (0, maxval, (maxval + 1) // 2, 1)[:k]
    return (u << shift).astype(np.uint16)


@pytest.mark.parametrize("conv", [SYM10, P010, FULL16], ids=["sym10", "p010", "full16"])
@pytest.mark.parametrize("ends", ["both", "in", "out"])
# (3, 37, 53): ragged in both tile directions, batch > 1; (1, 8, 8), (1, 1, 1): below every tile; (2, 19, 71): W odd, so the 6-byte pixel groups of
# r = 3 start on both 4-byte phases; (1, 9, 12): W % 4 == 0
@pytest.mark.parametrize("n,h,w", [(3, 37, 53), (1, 8, 8), (1, 1, 1), (2, 19, 71), (1, 9, 12)])
@pytest.mark.parametrize("r", [2, 3, 4])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_fused_u16_chain_is_bit_identical_to_the_plans_one_by_one(ctx, monkeypatch, half, r, n, h, w, ends, conv):
    """The conversions fold into the two fused launches -- the fp32 kernels A / B and, under SNNHIP_ESPCN_F16=1, the fp16 kernels A16 / B16 -- and the
    frame is, bit for bit, what the three separate runs give.  The output frame is pre-filled with 0xFFFF so that a pixel the chain does not write
    shows."""
    from shadernn_amd import capi, models

    if half:
        monkeypatch.setenv("SNNHIP_ESPCN_F16", "1")
    dt = capi.F16 if half else capi.F32
    net = models.espcn_weights(seed=3, scale=r)
    u16in, u16out = ends in ("both", "in"), ends in ("both", "out")
    plans = _espcn_plans(ctx, net, n, h, w, conv, u16in, u16out, dtype=dt)
    chain = capi.chain_plan(ctx, plans)
    desc = chain.describe()
    assert chain.num_steps() == 2, desc
    steps = [chain.step_describe(i) for i in range(2)]
    ka = "espcn_f16_conv_pair_u16_kernel" if half else "conv_kxk_c1o16_wino3x3_c16o16_u16_kernel"
    kb = "espcn_f16_d2s_u16_kernel<%d>" % r if half else ("conv3x3_c16o4_d2s_tanh_u16_kernel" if r == 2 else "conv3x3_c16oR_d2s_tanh_u16_kernel")
    assert (ka in steps[0]) == u16in and ("u16_in(1ch)" in steps[0]) == u16in, steps
    assert (kb in steps[1]) == u16out and ("u16_out(1ch)" in steps[1]) == u16out, steps
    assert ("_u16_" in steps[0]) == u16in and ("_u16_" in steps[1]) == u16out, steps
    # the fused steps price their own bytes: a frame pixel is 2 B -- instead of the fp32 tensor's 4; the fp16 kernels move 2 B either way
    body = capi.chain_plan(ctx, plans[(1 if u16in else 0):(len(plans) - 1 if u16out else len(plans))])
    px = n * h * w
    saved = 0.0 if half else 2.0
    assert body.step_cost(0)[1] - chain.step_cost(0)[1] == pytest.approx(saved * px if u16in else 0.0)
    assert body.step_cost(1)[1] - chain.step_cost(1)[1] == pytest.approx(saved * r * r * px if u16out else 0.0)
    maxval, shift = conv[4], conv[5]
    u = _frame(n, h, w, n * h + w, maxval, shift)
    x_host = u if u16in else _in_ref(u, conv[0], conv[1], shift, half)
    x = capi.Tensor.from_numpy(ctx, x_host, dtype=capi.U16 if u16in else dt)
    if u16out:
        y = capi.Tensor.from_numpy(ctx, np.full((n, r * h, r * w, 1), 0xFFFF, np.uint16))
    else:
        y = capi.Tensor(ctx, n, r * h, r * w, 1, dtype=dt)
    chain.run(x, y)
    got = y.numpy_u16() if u16out else y.numpy()
    want = _run_one_by_one(ctx, plans, x, dt)
    np.testing.assert_array_equal(got, want, err_msg=desc)
    if u16out:
        assert int(got.max()) <= (maxval << shift) and not np.any(got & ((1 << shift) - 1)), "bits outside the container's layout"


def test_persistent_loop_of_kernel_a_with_a_16bit_frame(ctx):
    """Kernel A's 16-bit form keeps the NEXT tile's raw values in registers while it computes: the "two" and "boundary" shapes of
    tests/test_espcn_budget_gpu.py (from the CU count; 256 CUs: boundary = (2, 264, 512), 544 tiles over 512 resident blocks, blocks walk from image 0
    into image 1) are the smallest at which that register of a second tile is live.  16-bit in, fp32 out, against u16_in + the fp32 chain."""
    from shadernn_amd import capi, models
    from test_espcn_budget_gpu import _loop_shapes

    S, shapes = _loop_shapes()
    net = models.espcn_weights(seed=1)
    for which in ("two", "boundary"):
        n, h, w = shapes[which]
        plans = _espcn_plans(ctx, net, n, h, w, P010, True, False)
        chain = capi.chain_plan(ctx, plans)
        assert chain.num_steps() == 2 and "conv_kxk_c1o16_wino3x3_c16o16_u16_kernel" in chain.step_describe(0), chain.describe()
        x = capi.Tensor.from_numpy(ctx, _frame(n, h, w, 5, 1023, 6))
        y = capi.Tensor.from_numpy(ctx, np.full((n, 2 * h, 2 * w, 1), np.nan, np.float32))
        chain.run(x, y)
        np.testing.assert_array_equal(y.numpy(), _run_one_by_one(ctx, plans, x), err_msg="%s %dx%dx%d" % (which, n, h, w))


_ORACLE = {}


def _oracle_pre(seed, n, h, w, conv):
    """float64 oracle output in output-code units, computed once per case and shared."""
    from shadernn_amd import models

    key = (seed, n, h, w, conv)
    if key not in _ORACLE:
        net = models.espcn_weights(seed=seed)
        u = _frame(n, h, w, 7, conv[4], conv[5])
        pre = O.espcn_forward(net, _in_ref(u, conv[0], conv[1], conv[5], False)).astype(np.float64) * conv[2][0] + conv[3][0]
        pre.setflags(write=False)
        _ORACLE[key] = (net, u, pre)
    return _ORACLE[key]


@pytest.mark.parametrize("conv", [SYM10, KERAS10, SYM12], ids=["sym10", "keras10", "sym12"])
@pytest.mark.parametrize("n,h,w", [(2, 19, 71), (1, 72, 96), (3, 37, 53)])
@pytest.mark.parametrize("seed", [1, 3])
def test_u16_chain_against_the_quantised_oracle(ctx, seed, n, h, w, conv):
    """10- and 12-bit, fp32, r = 2.  |got - want| <= 1 everywhere, and equality on every pixel whose pre-rounding value is farther than 0.02 from a
    rounding tie (or outside [-0.5, maxval + 0.5]).  The margin is the 8-bit test's: the fused fp32 kernels are held to 8 x the oracle's own float64
    error (tests/ref64.py: <= 8 x 5e-7 in output units), which is <= 0.008 code values at scale 2047.5.  The pixels the margin leaves out must be at
    most 5 % of the frame; that cap is asserted before the comparison."""
    from shadernn_amd import capi

    net, u, pre = _oracle_pre(seed, n, h, w, conv)
    maxval = conv[4]
    frac = np.abs(pre - np.floor(pre) - 0.5)
    safe = (frac > 0.02) | (pre < -0.5) | (pre > maxval + 0.5)
    left_out = 1.0 - float(np.mean(safe))
    print("left out by the tie margin: %.2f %%" % (100 * left_out))
    assert left_out <= 0.05
    plans = _espcn_plans(ctx, net, n, h, w, conv)
    chain = capi.chain_plan(ctx, plans)
    x = capi.Tensor.from_numpy(ctx, u)
    y = capi.Tensor.from_numpy(ctx, np.full((n, 2 * h, 2 * w, 1), 0xFFFF, np.uint16))
    chain.run(x, y)
    got = y.numpy_u16().astype(np.int64)
    want = np.clip(np.rint(pre), 0, maxval).astype(np.int64)
    print("max |got - want| = %d" % int(np.max(np.abs(got - want))))
    assert np.max(np.abs(got - want)) <= 1
    np.testing.assert_array_equal(got[safe], want[safe])


@pytest.mark.parametrize("n,h,w", [(2, 19, 71), (1, 72, 96), (3, 37, 53)])
def test_full_16bit_chain_against_the_quantised_oracle(ctx, n, h, w):
    """Scale 32767.5: the float64 budget (8 x 5e-7 in output units) is 0.13 code values there, so a tie margin would leave out a quarter of the frame;
    the exact check is bit-identity with the one-by-one plans (above), and against the oracle only |got - want| <= 1 holds everywhere."""
    from shadernn_amd import capi

    net, u, pre = _oracle_pre(1, n, h, w, FULL16)
    plans = _espcn_plans(ctx, net, n, h, w, FULL16)
    chain = capi.chain_plan(ctx, plans)
    x = capi.Tensor.from_numpy(ctx, u)
    y = capi.Tensor.from_numpy(ctx, np.full((n, 2 * h, 2 * w, 1), 0xFFFF, np.uint16))
    chain.run(x, y)
    got = y.numpy_u16().astype(np.int64)
    want = np.clip(np.rint(pre), 0, 65535).astype(np.int64)
    print("max |got - want| = %d" % int(np.max(np.abs(got - want))))
    assert np.max(np.abs(got - want)) <= 1


@pytest.mark.parametrize("switch", [("SNNHIP_ESPCN_A", "direct"), ("SNNHIP_ESPCN_B", "wino"), ("SNNHIP_ESPCN_FUSION", "stream")])
@pytest.mark.parametrize("n,h,w", [(3, 37, 53), (1, 8, 8)])
def test_u16_chain_under_the_other_kernel_forms(ctx, monkeypatch, switch, n, h, w):
    """Where no 16-bit form of a kernel exists the conversion stays a step of its own (u16_in... / u16_out...); the frame is still the one-by-one frame."""
    from shadernn_amd import capi, models

    monkeypatch.setenv(*switch)
    net = models.espcn_weights(seed=4)
    plans = _espcn_plans(ctx, net, n, h, w, KERAS10)
    chain = capi.chain_plan(ctx, plans)
    steps = [chain.step_describe(i) for i in range(chain.num_steps())]
    if switch[0] == "SNNHIP_ESPCN_A":
        assert len(steps) == 3 and steps[0].startswith("u16_in") and "conv3x3_c16o4_d2s_tanh_u16_kernel" in steps[-1], steps
    elif switch[0] == "SNNHIP_ESPCN_B":
        assert len(steps) == 3 and "conv_kxk_c1o16_wino3x3_c16o16_u16_kernel" in steps[0] and steps[-1].startswith("u16_out"), steps
    else:
        assert steps[0].startswith("u16_in") and steps[-1].startswith("u16_out") and len(steps) == 3, steps
    x = capi.Tensor.from_numpy(ctx, _frame(n, h, w, 11, 1023, 0))
    y = capi.Tensor.from_numpy(ctx, np.full((n, 2 * h, 2 * w, 1), 0xFFFF, np.uint16))
    chain.run(x, y)
    np.testing.assert_array_equal(y.numpy_u16(), _run_one_by_one(ctx, plans, x))


def test_graph_fuse_folds_the_conversions_into_two_launches(ctx):
    from shadernn_amd import capi, models

    n, h, w = 1, 24, 40
    net = models.espcn_weights(seed=1)
    plans = _espcn_plans(ctx, net, n, h, w, P010)
    nodes = [(p, [k - 1 if k else -1], k == len(plans) - 1) for k, p in enumerate(plans)]
    fused = capi.graph_fuse(ctx, nodes)
    live = [(p, ins) for p, ins in fused if p is not None]
    assert len(live) == 1
    plan, ins = live[0]
    assert ins == [-1] and plan.num_steps() == 2
    assert "_u16_kernel" in plan.step_describe(0) and "_u16_kernel" in plan.step_describe(1)
    x = capi.Tensor.from_numpy(ctx, _frame(n, h, w, 2, 1023, 6))
    y = capi.Tensor.from_numpy(ctx, np.full((n, 2 * h, 2 * w, 1), 0xFFFF, np.uint16))
    plan.run(x, y)
    np.testing.assert_array_equal(y.numpy_u16(), _run_one_by_one(ctx, plans, x))


def test_captured_graph_replays_fresh_frames(ctx):
    from shadernn_amd import capi, models

    n, h, w = 2, 33, 47
    net = models.espcn_weights(seed=1)
    plans = _espcn_plans(ctx, net, n, h, w, SYM10)
    chain = capi.chain_plan(ctx, plans)
    x = capi.Tensor(ctx, n, h, w, 1, dtype=capi.U16)
    y = capi.Tensor(ctx, n, 2 * h, 2 * w, 1, dtype=capi.U16)
    x.upload_u16(_frame(n, h, w, 0, 1023, 0))
    with capi.Graph.capture(ctx) as g:
        chain.run(x, y)
    for seed in (1, 2, 3):
        x.upload_u16(_frame(n, h, w, seed, 1023, 0))
        g.launch()
        np.testing.assert_array_equal(y.numpy_u16(), _run_one_by_one(ctx, plans, x))
    g.destroy()


def test_errors_are_invalid_with_a_message(ctx):
    from shadernn_amd import capi

    for kw in (dict(N=0, H=4, W=4, Cc=1), dict(N=1, H=4, W=4, Cc=5), dict(N=1, H=4, W=4, Cc=0), dict(N=1, H=4, W=4, Cc=1, dtype=capi.U8),
               dict(N=1, H=4, W=4, Cc=1, dtype=capi.U16), dict(N=1, H=4, W=4, Cc=1, shift=16), dict(N=1, H=4, W=4, Cc=1, shift=-1)):
        for make in (capi.u16_in_plan, capi.u16_out_plan):
            with pytest.raises(capi.SnnHipError) as e:
                make(ctx, **kw)
            assert e.value.code == -1 and ("desc" in str(e.value))
    for kw in (dict(maxval=0), dict(maxval=65536), dict(maxval=1024, shift=6), dict(maxval=65535, shift=1)):
        with pytest.raises(capi.SnnHipError) as e:
            capi.u16_out_plan(ctx, 1, 4, 4, 1, **kw)
        assert e.value.code == -1 and "maxval" in str(e.value)
    capi.u16_out_plan(ctx, 1, 4, 4, 1, maxval=1023, shift=6)  # 1023 << 6 = 65472 fits

    t = capi.Tensor(ctx, 1, 3, 5, 1, dtype=capi.U16)
    assert capi.lib().snnhip_tensor_bytes(t.h) == 30
    buf = np.zeros(15, np.uint8)
    rc = capi.lib().snnhip_tensor_download_raw(t.h, buf.ctypes.data_as(capi._P), buf.size)
    assert rc == -1 and b"30" in capi.lib().snnhip_last_error()
    # the float entry points refuse a 16-bit tensor
    f = np.zeros(15, np.float32)
    for call in (lambda: capi.lib().snnhip_tensor_upload(t.h, capi._fptr(f)), lambda: capi.lib().snnhip_tensor_download(t.h, capi._fptr(f)),
                 lambda: capi.lib().snnhip_tensor_fill(t.h, 0.0)):
        assert call() == -1 and b"16-bit" in capi.lib().snnhip_last_error()
    # a 16-bit tensor is accepted exactly where a plan declares one
    out16 = capi.u16_out_plan(ctx, 1, 3, 5, 1)
    in16 = capi.u16_in_plan(ctx, 1, 3, 5, 1)
    out8 = capi.u8_out_plan(ctx, 1, 3, 5, 1)
    in8 = capi.u8_in_plan(ctx, 1, 3, 5, 1)
    f32 = capi.Tensor(ctx, 1, 3, 5, 1)
    t8 = capi.Tensor(ctx, 1, 3, 5, 1, dtype=capi.U8)
    for plan, src, dst in ((out16, f32, f32), (out16, f32, t8), (out16, t, t), (in16, f32, f32), (in16, t8, f32), (in16, t, t), (out8, f32, t), (in8, t, f32),
                           (out8, t, t8)):
        with pytest.raises(capi.SnnHipError) as e:
            plan.run(src, dst)
        assert e.value.code == -1
    act = capi.activation_plan(ctx, 1, 3, 5, 1, "relu")  # adapts to any float dtype, not to frames
    with pytest.raises(capi.SnnHipError) as e:
        act.run(t, f32)
    assert "16-bit" in str(e.value)
    with pytest.raises(capi.SnnHipError) as e:
        act.run(f32, t)
    assert "16-bit" in str(e.value)
