"""The fused fp32 ESPCN chain (rules A / B / C, the 8-bit ends A8 / B8) held to fp32 accuracy: every selectable kernel at the edges of its own tile,
the persistent tile loop of the default kernel A with blocks that take a second and a third tile and walk across a batch boundary, and the 8-bit
output byte for byte -- all against the float64 reference of tests/ref64.py, within ref64.M times the fp32 oracle's own error on the same input
(ref64.budget), into output tensors that start as NaN."""
import functools

import numpy as np
import pytest

import ref64
from test_ref64 import kernel_tiles, net_of, oracle32

pytestmark = pytest.mark.gpu

T = kernel_tiles()
DEMO = ((127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1), (127.5, 0, 0, 0), (127.5, 0, 0, 0))  # means, norms, scale, offset (tests/test_frame_u8_gpu.py)

# name: (upscale, switches, net variant, kernels of the two launches)
VARIANTS = {
    "default": (2, {}, "plain", ("A wino", "B direct")),
    "a_direct": (2, {"SNNHIP_ESPCN_A": "direct"}, "plain", ("A direct", "B direct")),
    "b_wino": (2, {"SNNHIP_ESPCN_B": "wino"}, "plain", ("A wino", "B wino")),
    "stream": (2, {"SNNHIP_ESPCN_FUSION": "stream"}, "plain", ("stream",)),
    "r3": (3, {}, "plain", ("A wino", "B mfma")),
    "r3_a_direct": (3, {"SNNHIP_ESPCN_A": "direct"}, "plain", ("A direct", "B mfma")),
    "r4": (4, {}, "plain", ("A wino", "B mfma")),
    "r4_a_direct": (4, {"SNNHIP_ESPCN_A": "direct"}, "plain", ("A direct", "B mfma")),
    "k3": (2, {}, "k3", ("A wino", "B direct")),
    "acts": (2, {}, "acts", ("A wino", "B direct")),
}


def _edge_shapes(kernels):
    """(n, h, w) for a variant: per kernel tile (TW, TH) the widths TW-1, TW, TW+1, 2TW+1 and the heights TH-1, TH, TH+1 (paired, not crossed; the
    ragged ones in batches of 2 and 3), a 3x3-tile shape, which has an interior tile, and its two neighbours at which the last tile stops being
    interior or the last column of tiles loses a pixel; then the shapes smaller than any tile."""
    shapes = []
    for k in kernels:
        tw, th = T[k]
        shapes += [(1, th - 1, tw - 1), (1, th, tw), (2, th + 1, tw + 1), (3, th - 1, 2 * tw + 1),
                   (1, 3 * th, 3 * tw), (2, 3 * th + 1, 3 * tw + 1), (1, 3 * th, 3 * tw - 1)]
    shapes += [(1, 1, 1), (2, 1, 37), (1, 37, 1)]
    return list(dict.fromkeys(shapes))


# (kernel B of r = 3, 4 has all its edges in "r3" / "r4": the direct kernel A in front of it runs at the edges of its own tile only)
SWEEP = [(v, s) for v, spec in VARIANTS.items() for s in _edge_shapes(spec[3][:1] if v in ("r3_a_direct", "r4_a_direct") else spec[3])]


def _x(n, h, w):
    return np.random.default_rng(1000 * h + w).random((n, h, w, 1), dtype=np.float32)


def _frame(n, h, w):
    u = np.random.default_rng(1000 * h + w).integers(0, 256, size=(n, h, w, 1), dtype=np.uint8)
    k = min(4, u.size)
    u.reshape(-1)[:k] = (0, 255, 128, 1)[:k]
    return u


@functools.lru_cache(maxsize=None)
def _case(r, variant, n, h, w, u8in=False):
    """(net, input, float64 reference, fp32 oracle) of one case: computed once, shared by the tests that need it, read-only."""
    net = net_of(r, variant=variant)
    if u8in:
        x = _frame(n, h, w)
        x64 = ref64.u8_in(x, DEMO[0][0], DEMO[1][0])
        x32 = (x.astype(np.float32) - np.float32(DEMO[0][0])) * np.float32(DEMO[1][0])
    else:
        x = x64 = x32 = _x(n, h, w)
    want64 = ref64.espcn(net, x64, r)
    want32 = oracle32(net, x32, r, threads=8 if n * h * w > 65536 else 1)
    for a in (x, want64, want32):
        a.setflags(write=False)
    return net, x, want64, want32


def _chain(ctx, net, n, h, w, u8in=False, u8out=False):
    from shadernn_amd import capi
    from shadernn_amd.runner import _layer_plan

    means, norms, scale, offset = DEMO
    plans, shape = [], (n, h, w, 1)
    if u8in:
        plans.append(capi.u8_in_plan(ctx, n, h, w, 1, means, norms))
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape)
        plans.append(p)
        shape = p.out_shape()
    if u8out:
        plans.append(capi.u8_out_plan(ctx, *shape, scale, offset))
    chain = capi.chain_plan(ctx, plans)  # (it keeps the layer plans it borrows alive)
    return chain, [chain.step_describe(i) for i in range(chain.num_steps())], shape


def _run(ctx, chain, x, out_shape, u8in=False, u8out=False):
    """One run into an output tensor that starts as NaN (8-bit: as 0xA5), so that a pixel no block writes cannot pass on stale data."""
    from shadernn_amd import capi

    xt = capi.Tensor.from_numpy(ctx, x, dtype=capi.U8 if u8in else capi.F32)
    if u8out:
        yt = capi.Tensor.from_numpy(ctx, np.full(out_shape, 0xA5, np.uint8), dtype=capi.U8)
    else:
        yt = capi.Tensor.from_numpy(ctx, np.full(out_shape, np.nan, np.float32))
    chain.run(xt, yt)
    y = yt.numpy_u8() if u8out else yt.numpy()
    xt.free()
    yt.free()
    return y


def _free(chain):
    chain.destroy()
    for p in chain._keep:
        p.destroy()


def _check_steps(steps, kernels, r, k1):
    """The launches are the kernels the variant names, with the tiles read from the sources."""
    tile = lambda k: "tile=%dx%d" % T[k]
    if kernels == ("stream",):
        assert len(steps) == 1 and " stream " in steps[0] and "strip=%d" % T["stream"][0] in steps[0], steps
        return
    assert len(steps) == 2 and "fused[conv%dx%d(1->16)+conv3x3(16->16)" % (k1, k1) in steps[0] and "depth_to_space(%d)" % r in steps[1], steps
    a, b = kernels
    assert ("winograd" in steps[0]) == (a == "A wino") and tile(a) in steps[0], steps
    assert ("conv_kxk_c1o16_wino3x3_c16o16" if a == "A wino" else "kernel=conv_kxk_c1o16_conv3x3_c16o16_kernel") in steps[0], steps
    want = {"B direct": "valu_f32", "B wino": "mfma_f32_4x4x1", "B mfma": "conv3x3_c16oR_d2s_tanh"}[b]
    assert want in steps[1] and tile(b) in steps[1] and ("mfma_f32_4x4x1" in steps[1]) == (b == "B wino"), steps


@pytest.mark.parametrize("variant,shape", SWEEP, ids=["%s-%dx%dx%d" % ((v,) + s) for v, s in SWEEP])
def test_every_kernel_at_the_edges_of_its_tile(ctx, monkeypatch, variant, shape):
    r, switches, netv, kernels = VARIANTS[variant]
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    n, h, w = shape
    net, x, want64, want32 = _case(r, netv, n, h, w)
    chain, steps, out_shape = _chain(ctx, net, n, h, w)
    _check_steps(steps, kernels, r, net["layers"][0]["kernel"])
    assert out_shape == (n, r * h, r * w, 1)
    y = _run(ctx, chain, x, out_shape)
    tiles = {k: T[k] for k in kernels}
    rmax, rmean = ref64.budget(y, want64, want32, ref64.M, r=r, tiles=tiles, what="; ".join(steps))
    print("BUDGET sweep %s %dx%dx%d max %.3f mean %.3f" % (variant, n, h, w, rmax, rmean))
    _free(chain)


def _loop_shapes():
    """The three shapes of the persistent-loop tests, from the CU count: W = 16 tiles of kernel A; S = W_WPS x CUs resident blocks."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tw, th = T["A wino"]
    S = T["W_WPS"] * cus
    tx = 16
    up = lambda a, b: -(-a // b)
    return S, {"two": (1, up(S + 1, tx) * th - 5, tx * tw),              # one or a few blocks take a second tile; ragged bottom row of tiles
               "boundary": (2, up(S + 1, 2 * tx) * th - th // 2, tx * tw),  # blocks walk from image 0 into image 1; 256 CUs: (2, 264, 512), 544 tiles
               "three": (3, up(2 * S + 1, 3 * tx) * th - th // 2, tx * tw)}  # every block takes a second tile, some a third, across two boundaries


@pytest.mark.parametrize("u8in", [False, True], ids=["f32", "u8in"])
@pytest.mark.parametrize("which", ["two", "boundary", "three"])
def test_persistent_loop_of_kernel_a(ctx, which, u8in):
    S, shapes = _loop_shapes()
    n, h, w = shapes[which]
    tw, th = T["A wino"]
    ntiles = n * -(-h // th) * -(-w // tw)
    print("LOOP %s: %dx%dx%d, %d tiles over %d resident blocks" % (which, n, h, w, ntiles, S))
    assert ntiles > S, "no block takes a second tile: %d tiles, %d blocks" % (ntiles, S)
    if which == "boundary":
        assert h % th and S < ntiles <= 1.25 * S, (h, ntiles, S)
    if which == "three":
        assert ntiles > 2 * S, (ntiles, S)
    r = 2
    net, x, want64, want32 = _case(r, "plain", n, h, w, u8in)
    chain, steps, out_shape = _chain(ctx, net, n, h, w, u8in=u8in)
    _check_steps(steps, ("A wino", "B direct"), r, 5)
    assert ("conv_kxk_c1o16_wino3x3_c16o16_u8_kernel" in steps[0]) == u8in, steps
    y = _run(ctx, chain, x, out_shape, u8in=u8in)
    rmax, rmean = ref64.budget(y, want64, want32, ref64.M, r=r, tiles={"A wino": T["A wino"], "B direct": T["B direct"]}, what="; ".join(steps))
    print("BUDGET loop %s %s %dx%dx%d max %.3f mean %.3f" % (which, "u8in" if u8in else "f32", n, h, w, rmax, rmean))
    np.testing.assert_array_equal(_run(ctx, chain, x, out_shape, u8in=u8in), y, err_msg="a second run differs")
    # the arithmetic of a tile does not depend on the block that runs it, nor on what that block ran before
    one, _, one_shape = _chain(ctx, net, 1, h, w, u8in=u8in)
    for i in range(n):
        y1 = _run(ctx, one, x[i:i + 1], one_shape, u8in=u8in)
        diff = np.argwhere(y1[0] != y[i])
        assert diff.size == 0, "image %d of the batch differs from the same frame run alone at %d pixels, first (y, x) = (%d, %d): input pixel (%d, %d), tile (ty, tx) = (%d, %d)" % (
            i, len(diff), diff[0][0], diff[0][1], diff[0][0] // r, diff[0][1] // r, diff[0][0] // r // th, diff[0][1] // r // tw)
    _free(one)
    _free(chain)


@pytest.mark.parametrize("which", ["ragged", "boundary"])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_8bit_ends_byte_for_byte(ctx, r, which):
    """Rules A8 + B8.  The bytes equal the float64 reference's wherever its value before rounding is further than delta = M E32max |scale| from a
    rounding boundary -- at most 0.5 % of the frame is closer -- and are within one level everywhere."""
    n, h, w = (2, 19, 71) if which == "ragged" else _loop_shapes()[1]["boundary"]
    scale, offset = DEMO[2][0], DEMO[3][0]
    net, u, want64, want32 = _case(r, "plain", n, h, w, True)
    chain, steps, out_shape = _chain(ctx, net, n, h, w, u8in=True, u8out=True)
    assert len(steps) == 2 and "conv_kxk_c1o16_wino3x3_c16o16_u8_kernel" in steps[0] and "_d2s_tanh_u8_kernel" in steps[1], steps
    got = _run(ctx, chain, u, out_shape, u8in=True, u8out=True).astype(np.int32)
    pre = ref64.u8_out_pre(want64, scale, offset)
    want = ref64.u8_out(want64, scale, offset).astype(np.int32)
    delta = ref64.M * float(np.abs(want32.astype(np.float64) - want64).max()) * abs(scale)
    safe = np.abs(pre - np.floor(pre) - 0.5) > delta
    excluded = 1.0 - safe.mean()
    print("BYTES r=%d %dx%dx%d: delta %.2e, %.3f %% of the pixels excluded, %d bytes differ, %d of them away from a boundary"
          % (r, n, h, w, delta, 100 * excluded, int((got != want).sum()), int((got != want)[safe].sum())))
    assert excluded <= 0.005
    assert np.abs(got - want).max() <= 1
    np.testing.assert_array_equal(got[safe], want[safe], err_msg="; ".join(steps))
    _free(chain)

