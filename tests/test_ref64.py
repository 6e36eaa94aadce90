"""tests/ref64.py on the CPU: the float64 reference against torch's float64 convolution, the fp32 C oracle inside its own budget, and the comparator
against mutants of the oracle that rtol = atol = 1e-4 lets through (they must be rejected at the margin M the GPU tests use) and one it must accept;
the half budget of the fp16 kernels (ulp16, budget_half) against honest fp32 evaluations rounded to half and against the wrong kernels that
rtol = atol = 4e-3 lets through."""
import copy
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def kernel_tiles():
    """The tile constants of the fused ESPCN kernels, read from the sources: {name: (TW, TH)} in input-resolution pixels, and W_WPS."""
    def src(name):
        return open(os.path.join(ROOT, "shadernn_amd", "csrc", name)).read()

    def find(txt, pat, flags=0):
        m = re.search(pat, txt, flags)
        assert m, "kernel_tiles: the sources no longer match %r (a tile constant was renamed or moved)" % pat
        return m

    def num(txt, pat):
        return int(find(txt, pat).group(1))

    fused, mfma, stream = src("espcn_fused.hip"), src("espcn_d2s_mfma.h"), src("espcn_stream.hip")
    c = {k: num(fused, r"\b%s = (\d+)" % k) for k in ("A_TW", "A_TH", "W_TH", "W_WPS", "B_TW", "B_TH")}
    wino_tw = num(fused, r"struct WinoTile \{\s*static constexpr int TW = (\d+);")
    find(fused, r"BR_TW = kD2sMfmaTW, BR_TH = kD2sMfmaTH")
    br = (num(mfma, r"\bkD2sMfmaTW = (\d+)"), num(mfma, r"\bkD2sMfmaTH = (\d+)"))
    # the Winograd kernel B's tile is local to the kernel
    wb = find(fused, r"conv3x3_c16o4_wino_d2s_tanh_kernel\(.*?constexpr int TW = (\d+), TH = (\d+)", re.S)
    # rule C: a wave owns a strip of STRIP columns and a segment of at least `rows` rows
    st = (num(stream, r"\bconstexpr int STRIP = (\d+)"), num(stream, r"if \(rows < (\d+)\)"))
    return {"A wino": (wino_tw, c["W_TH"]), "A direct": (c["A_TW"], c["A_TH"]), "B direct": (c["B_TW"], c["B_TH"]),
            "B wino": (int(wb.group(1)), int(wb.group(2))), "B mfma": br, "stream": st, "W_WPS": c["W_WPS"]}


def net_of(r, seed=1, variant="plain"):
    """models.espcn_weights, or one of its variants: "k3" = a 3x3 first convolution, "acts" = BN + leakyRelu / sigmoid / tanh on the three convolutions
    (the net of test_espcn_fused_with_bn_and_other_activations), "acts6" = BN + relu6 / tanh / relu6 (the remaining activation)."""
    from shadernn_amd import models

    net = models.espcn_weights(seed=seed, scale=r)
    if variant == "k3":
        l0 = net["layers"][0]
        l0["w"] = np.ascontiguousarray(l0["w"][:, :, 1:4, 1:4])
        l0["kernel"] = 3
    elif variant in ("acts", "acts6"):
        rng = np.random.default_rng(5)
        for i, act in enumerate(["leakyRelu", "sigmoid", "tanh"] if variant == "acts" else ["relu6", "tanh", "relu6"]):
            l = net["layers"][i]
            l["activation"] = act
            l["alpha"] = 0.2
            c = l["oc"]
            l["bn"] = {"beta": rng.uniform(-0.1, 0.1, c).astype(np.float32), "gamma": rng.uniform(0.5, 1.5, c).astype(np.float32),
                       "mean": rng.uniform(-0.1, 0.1, c).astype(np.float32), "var": rng.uniform(0.5, 1.5, c).astype(np.float32)}
    else:
        assert variant == "plain", variant
    return net


def oracle32(net, x, r, threads=1):
    """The fp32 C oracle on an ESPCN-shaped net of any upscale factor (oracle_lib.forward knows factor 2 only)."""
    return O.subpixel(O.forward(dict(net, layers=net["layers"][:-1]), x, threads=threads), r, 0)


def _torch64(net, x, r):
    import torch
    import torch.nn.functional as F

    v = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    for l in net["layers"][:-1]:
        v = F.conv2d(v, torch.from_numpy(l["w"].astype(np.float64)), torch.from_numpy(l["b"].astype(np.float64)), padding=l["kernel"] // 2)
        if l["bn"] is not None:
            bn = {k: torch.from_numpy(a.astype(np.float64)).view(1, -1, 1, 1) for k, a in l["bn"].items()}
            s = torch.clamp(torch.sqrt(bn["var"] + float(np.float32(0.001))), min=float(np.float32(0.0001)))
            v = (bn["gamma"] / s) * (v - bn["mean"]) + bn["beta"]
        a = l["activation"]
        v = {"relu": F.relu, "relu6": F.relu6, "sigmoid": torch.sigmoid, "tanh": torch.tanh, "linear": lambda t: t,
             "leakyRelu": lambda t: torch.maximum(t, t * float(np.float32(l.get("alpha", 0.0))))}[a](v)
    return torch.tanh(F.pixel_shuffle(v, r)).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("variant", ["plain", "k3", "acts", "acts6"])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_ref64_agrees_with_torch_float64(r, variant):
    net = net_of(r, seed=3, variant=variant)
    x = np.random.default_rng(r).random((2, 13, 21, 1), dtype=np.float32)
    got = ref64.espcn(net, x, r)
    assert got.dtype == np.float64 and got.shape == (2, 13 * r, 21 * r, 1)
    np.testing.assert_allclose(got, _torch64(net, x, r), rtol=0, atol=1e-12)


def test_ref64_8bit_maps():
    u = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    x = ref64.u8_in(u, 127.5, 1 / 127.5)
    assert x.dtype == np.float64 and x[0, 0, 0, 0] == -127.5 * float(np.float32(1 / 127.5))
    pre = np.array([-3.0, -0.5, 0.49, 0.5, 1.5, 2.5, 254.5, 255.49, 300.0])
    np.testing.assert_array_equal(ref64.u8_out(pre, 1.0, 0.0), [0, 0, 0, 0, 2, 2, 254, 255, 255])  # rint: ties to even
    np.testing.assert_array_equal(ref64.u8_out(x, 127.5, 127.5), u)


N, H, W = 2, 40, 100


@functools.lru_cache(maxsize=None)
def _case(r):
    net = net_of(r)
    x = np.random.default_rng(7).random((N, H, W, 1), dtype=np.float32)
    want64, want32 = ref64.espcn(net, x, r), oracle32(net, x, r)
    for a in (x, want64, want32):
        a.setflags(write=False)
    return net, x, want64, want32


@pytest.mark.parametrize("shape", [(N, H, W), (2, 264, 512)])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_oracle_passes_its_own_budget_and_stays_fp32(r, shape):
    if shape == (N, H, W):
        net, x, want64, want32 = _case(r)
    else:  # the batch-boundary shape of the persistent-loop tests on 256 CUs
        net = net_of(r)
        x = np.random.default_rng(7).random(shape + (1,), dtype=np.float32)
        want64, want32 = ref64.espcn(net, x, r), oracle32(net, x, r)
    assert ref64.budget(want32, want64, want32, 1) == (1.0, 1.0)
    e = np.abs(want32.astype(np.float64) - want64)
    print("r=%d %s: E32max %.3e E32mean %.3e" % (r, shape, e.max(), e.mean()))
    # a broken reference (or oracle) would loosen every bound silently: measured 2.1e-7 to 4.6e-7 max, 2.9e-8 to 3.3e-8 mean
    assert e.max() < 1e-6 and e.mean() < 1e-7


def _truncated(w, bits):
    """fp32 values with the mantissa cut to `bits` explicit bits (toward zero)."""
    u = np.ascontiguousarray(w, np.float32).view(np.uint32) & np.uint32((0xFFFFFFFF << (23 - bits)) & 0xFFFFFFFF)
    return u.view(np.float32)


def _mutant(r, kind):
    net, x, want64, want32 = _case(r)
    m = copy.deepcopy(net)
    tw = kernel_tiles()["B direct"][0]
    if kind in ("w16", "w21"):
        m["layers"][1]["w"] = _truncated(m["layers"][1]["w"], 16 if kind == "w16" else 21)
        return oracle32(m, x, r)
    if kind == "bias":
        m["layers"][1]["b"][3] += np.float32(2e-6)
        return oracle32(m, x, r)
    if kind == "seam":  # the last output column of kernel B's first tile, as if the halo column to its right had read zeros
        m["layers"][2]["w"][:, :, :, 2] = 0.0
        y = want32.copy()
        col = r * tw - 1
        y[:, :, col, :] = oracle32(m, x, r)[:, :, col, :]
        return y
    if kind == "row":
        y = want32.copy()
        y[:, -1, :, :] = np.nan
        return y
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["w16", "bias", "seam", "row"])
@pytest.mark.parametrize("r", [2, 3])
def test_budget_rejects_the_mutants(r, kind):
    net, x, want64, want32 = _case(r)
    y = _mutant(r, kind)
    if kind in ("w16", "bias"):  # both are inside the suite's older bound
        np.testing.assert_allclose(y, want32, rtol=1e-4, atol=1e-4)
    t = kernel_tiles()
    with pytest.raises(AssertionError) as e:
        ref64.budget(y, want64, want32, ref64.M, r=r, tiles={"A": t["A wino"], "B": t["B direct"]})
    print(e.value)
    if kind == "seam":
        assert re.search(r"worst pixel .*; B tile %dx%d: tile \(ty, tx\) = \(\d+, 0\), at \(\d+, %d\) inside it, on the [a-z/]*right" % (t["B direct"] + (t["B direct"][0] - 1,)), str(e.value))
    if kind == "row":
        assert "not finite" in str(e.value) and "(n, y, x) = (0, %d, 0)" % (r * H - 1) in str(e.value)


@pytest.mark.parametrize("r", [2, 3])
def test_budget_accepts_21_mantissa_bits(r):
    """conv2's weights cut to 21 mantissa bits stay within about 1.1 x E32: a bound that rejected this would be a bound on the summation order."""
    net, x, want64, want32 = _case(r)
    rmax, rmean = ref64.budget(_mutant(r, "w21"), want64, want32, ref64.M)
    print("r=%d: 21-bit mutant at %.2f x E32max, %.2f x E32mean" % (r, rmax, rmean))
    assert rmax < 2 and rmean < 2


def test_the_margin_is_a_power_of_two_of_at_most_eight():
    assert ref64.M <= 8 and ref64.M & (ref64.M - 1) == 0
    assert ref64.M_CONV <= 32 and ref64.M_CONV & (ref64.M_CONV - 1) == 0
    assert ref64.M_CONV <= ref64.M_CONV_UNSPLIT <= 32 and ref64.M_CONV_UNSPLIT & (ref64.M_CONV_UNSPLIT - 1) == 0


# ---- the general convolution reference, the pairwise fp32 unit and budget_pairwise (the fp32 convolution kernels: tests/test_conv_budget_gpu.py) ----

def _rand(shape, seed, scale=1.0):  # (tests/test_ops_gpu.py: the inputs of the GPU tests)
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def _geometry(h, w, k, stride, padding):
    """(pads, (OH, OW)) by the reference's rules, which stay with the oracle: "same" offsets (asymmetric for even k, Q1) and its output extent (Q2; "valid"
    keeps the unshrunk extent, Q20)."""
    pads = O.padding_offsets(padding, k)
    return pads, (O.out_dim(h, k, stride, pads[0], pads[1]), O.out_dim(w, k, stride, pads[0], pads[1]))


# even kernels come with "same" only: the reference's size rule wraps around for an even kernel without padding (Q2) and the library refuses such a layer
GRID = [(k, s, mode, padding) for k in (1, 2, 3, 4, 5, 7) for s in (1, 2) for mode in ("constant", "replicate", "reflect")
        for padding in (("same", "valid") if k % 2 else ("same",))]
SHAPES = [(2, 11, 14, 5, 7), (1, 9, 8, 3, 4)]


def _grid_case(shape, k, s):
    n, h, w, ic, oc = shape
    return _rand((n, h, w, ic), 11 * k + s), _rand((oc, ic, k, k), 12 * k + s, 1.0 / np.sqrt(ic * k * k)), _rand((oc,), 13, 0.1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("k,s,mode,padding", GRID, ids=lambda v: str(v))
def test_conv2d_general_agrees_with_torch_float64(shape, k, s, mode, padding):
    """torch's side: F.pad with the matching mode (the near pads as given, the far pads as large as the extent needs) + F.conv2d with the stride, cropped
    to the extent."""
    import torch
    import torch.nn.functional as F

    n, h, w, ic, oc = shape
    x, wt, b = _grid_case(shape, k, s)
    pads, (oh, ow) = _geometry(h, w, k, s, padding)
    got = ref64.conv2d_general(x, wt, b, s, pads, mode, (oh, ow))
    assert got.dtype == np.float64 and got.shape == (n, oh, ow, oc)
    top, left = (0, 0) if k == 1 else (pads[2], pads[0])
    bottom, right = max(0, (oh - 1) * s + k - h - top), max(0, (ow - 1) * s + k - w - left)
    v = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    v = F.pad(v, (left, right, top, bottom), mode=mode)
    want = F.conv2d(v, torch.from_numpy(wt.astype(np.float64)), torch.from_numpy(b.astype(np.float64)), stride=s)[:, :, :oh, :ow].permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("k,s,mode,padding", GRID, ids=lambda v: str(v))
def test_conv2d_general_agrees_with_the_c_oracle(shape, k, s, mode, padding):
    """Independent of the oracle's code, not of its conventions: the Q1 offsets, the Q20 extent, what a read beyond the data returns in each pad mode."""
    n, h, w, ic, oc = shape
    x, wt, b = _grid_case(shape, k, s)
    pads, out_hw = _geometry(h, w, k, s, padding)
    want = O.conv2d(x, wt, b, s, pads, mode)
    assert want.shape == (n,) + out_hw + (oc,)
    np.testing.assert_allclose(ref64.conv2d_general(x, wt, b, s, pads, mode, out_hw), want, rtol=1e-4, atol=1e-4)
    pair = ref64.conv2d_pairwise32(x, wt, b, s, pads, mode, out_hw)
    assert pair.dtype == np.float32
    np.testing.assert_allclose(pair, want, rtol=1e-4, atol=1e-4)


def test_epilogues_and_maxpool_agree_with_the_c_oracle():
    x, wt, b = _rand((2, 13, 10, 6), 1), _rand((9, 6, 3, 3), 2, 0.15), _rand((9,), 3, 0.1)
    r = np.random.default_rng(4)
    bn = {"beta": r.uniform(-0.1, 0.1, 9).astype(np.float32), "gamma": r.uniform(0.5, 1.5, 9).astype(np.float32),
          "mean": r.uniform(-0.1, 0.1, 9).astype(np.float32), "var": r.uniform(0.5, 1.5, 9).astype(np.float32)}
    for act in ("", "relu", "relu6", "tanh", "sigmoid", "leakyRelu", "SiLU"):
        want = O.conv2d(x, wt, b, 1, (1, 1, 1, 1), "constant", act, 0.1, bn)
        y64 = ref64.conv_layer_general(x, wt, b, 1, (1, 1, 1, 1), "constant", (13, 10), bn, act, 0.1)
        y32 = ref64.conv_layer_pairwise32(x, wt, b, 1, (1, 1, 1, 1), "constant", (13, 10), bn, act, 0.1)
        np.testing.assert_allclose(y64, want, rtol=1e-5, atol=1e-5, err_msg=act)
        np.testing.assert_allclose(y32, y64, rtol=0, atol=2e-6, err_msg=act)
    out_hw = (O.pool_out_dim(13, 3, 2, True), O.pool_out_dim(10, 3, 2, True))
    np.testing.assert_array_equal(ref64.maxpool(want, 3, 2, out_hw), O.pool2d(want, 3, 2, kind="max", same=True))
    assert ref64.maxpool(y64, 3, 2, out_hw).dtype == np.float64


# N, H, W, IC, OC, k: K = 360, 288, 2304, 4608
UNIT_SHAPES = [(1, 9, 9, 40, 16, 3), (2, 17, 23, 32, 48, 3), (1, 14, 14, 256, 128, 3), (1, 7, 7, 512, 128, 3)]
SHALLOW, DEEP = UNIT_SHAPES[0], UNIT_SHAPES[3]
SEAM_TILE = (4, 4)  # (TH, TW) of the tile-seam mutant: both shapes have more than one such tile


@functools.lru_cache(maxsize=None)
def _conv_case(shape):
    """(x, w, bias, float64 reference, pairwise fp32, fp32 C oracle) of a 3x3 "same" layer with the inputs of tests/test_conv_wino_gpu.py: read-only."""
    n, h, w, ic, oc, k = shape
    x, wt, b = _rand((n, h, w, ic), 31), _rand((oc, ic, k, k), 32, 1.0 / np.sqrt(k * k * ic)), _rand((oc,), 33, 0.1)
    pads, out_hw = _geometry(h, w, k, 1, "same")
    out = (x, wt, b, ref64.conv2d_general(x, wt, b, 1, pads, "constant", out_hw), ref64.conv2d_pairwise32(x, wt, b, 1, pads, "constant", out_hw),
           O.conv2d(x, wt, b, 1, pads, "constant", threads=8))
    for a in out:
        a.setflags(write=False)
    return out


def _blocked32(x, wt, b, skip=None):
    """An honest fp32 kernel on the CPU: per tap and 16-channel chunk an fp32 product block, the blocks added up in fp32 in (dy, dx, chunk) order -- the
    summation order of the implicit-GEMM kernels.  skip = (dy, dx, chunk, column): that block is left out on that output column."""
    n, h, w, ic = x.shape
    oc, _, k, _ = wt.shape
    p = k // 2
    xp = np.zeros((n, h + 2 * p, w + 2 * p, ic), np.float32)
    xp[:, p:p + h, p:p + w] = x
    y = np.zeros((n, h, w, oc), np.float32)
    for dy in range(k):
        for dx in range(k):
            for c in range(0, ic, 16):
                part = xp[:, dy:dy + h, dx:dx + w, c:c + 16] @ np.ascontiguousarray(wt[:, c:c + 16, dy, dx].T)
                if skip is not None and skip[:3] == (dy, dx, c // 16):
                    part[:, :, skip[3]] = 0.0
                y += part
    y += np.asarray(b, np.float32)
    assert y.dtype == np.float32
    return y


def _conv_mutant(shape, kind):
    x, wt, b, want64, pair32, want32 = _conv_case(shape)
    if kind == "blocked":
        return _blocked32(x, wt, b)
    if kind in ("w16", "w21"):
        return _blocked32(x, _truncated(wt, 16 if kind == "w16" else 21), b)
    if kind == "bias":
        b2 = b.copy()
        b2[3] += np.float32(2e-6)
        return _blocked32(x, wt, b2)
    if kind == "seam":  # the last 16-channel chunk of the centre-right tap, on the last column of the first tile
        return _blocked32(x, wt, b, skip=(1, 2, (x.shape[3] - 1) // 16, SEAM_TILE[1] - 1))
    if kind == "row":
        y = _blocked32(x, wt, b)
        y[:, -1] = np.nan
        return y
    raise ValueError(kind)


@pytest.mark.parametrize("shape", UNIT_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_the_pairwise_unit_is_fp32_sized(shape):
    x, wt, b, want64, pair32, want32 = _conv_case(shape)
    rmax, rmean, rchan = ref64.budget_pairwise(pair32, want64, pair32, 1)
    assert (rmax, rmean) == (1.0, 1.0) and rchan <= 1.0
    e = np.abs(pair32.astype(np.float64) - want64)
    print("%s K=%d: E32p max %.3e mean %.3e" % (shape, shape[3] * shape[5] ** 2, e.max(), e.mean()))
    # a broken unit would loosen every bound silently: measured 3.7e-7 to 5.8e-7 max, 6.5e-8 to 7.4e-8 mean
    assert e.max() < 1e-6 and e.mean() < 1.5e-7


@pytest.mark.parametrize("kind", ["w16", "bias", "seam", "row"])
@pytest.mark.parametrize("shape", [SHALLOW, DEEP], ids=["K360", "K4608"])
def test_budget_pairwise_rejects_the_mutants(shape, kind):
    """Each mutant of a blocked fp32 evaluation is rejected at M_CONV.  The two that are wrong by a little (16-bit weights, the bias) first pass the
    suite's older bound against the oracle; a missing block and an unwritten row would not pass any bound, they check the message."""
    x, wt, b, want64, pair32, want32 = _conv_case(shape)
    y = _conv_mutant(shape, kind)
    if kind in ("w16", "bias"):
        np.testing.assert_allclose(y, want32, rtol=1e-4, atol=1e-4)
    with pytest.raises(AssertionError) as e:
        ref64.budget_pairwise(y, want64, pair32, ref64.M_CONV, what=kind, tile=SEAM_TILE)
    msg = str(e.value)
    print(msg)
    if kind == "bias":  # max and mean alone would let it through: only the mean signed error of its channel stands out
        assert re.search(r"out of the float64 budget \([a-z, ]*per-channel mean\)", msg) and "(channel 3)" in msg, msg
    if kind == "seam":
        assert re.search(r"worst \(n, y, x, channel\) = \(0, \d+, %d, \d+\); tile 4x4 \(TH x TW\): tile \(ty, tx\) = \(\d+, 0\), at \(\d+, 3\) inside it, on the [a-z/]*right"
                         % (SEAM_TILE[1] - 1), msg), msg
    if kind == "row":
        assert "not finite" in msg and "(n, y, x, channel) = (0, %d, 0, 0)" % (shape[1] - 1) in msg, msg


def test_what_the_unsplit_margin_still_rejects():
    """M_CONV_UNSPLIT (one chain of 4608 terms, conv2d_mfma with its split pinned off) at the depth it is used at: the 16-bit weights, the missing block and the
    unwritten row are rejected; the 2e-6 bias (28 x per channel) is the one mutant it lets through -- which is why no other case is held to it."""
    x, wt, b, want64, pair32, want32 = _conv_case(DEEP)
    for kind in ("w16", "seam", "row"):
        with pytest.raises(AssertionError):
            ref64.budget_pairwise(_conv_mutant(DEEP, kind), want64, pair32, ref64.M_CONV_UNSPLIT, what=kind)
    rmax, rmean, rchan = ref64.budget_pairwise(_conv_mutant(DEEP, "bias"), want64, pair32, ref64.M_CONV_UNSPLIT, what="bias")
    print("bias mutant at K = 4608: %.1f x max, %.1f x mean, %.1f x per channel" % (rmax, rmean, rchan))
    assert rchan > ref64.M_CONV


@pytest.mark.parametrize("kind", ["blocked", "w21"])
@pytest.mark.parametrize("shape", [SHALLOW, DEEP], ids=["K360", "K4608"])
def test_budget_pairwise_accepts_honest_fp32(shape, kind):
    """The blocked evaluation itself, and with weights cut to 21 mantissa bits: a bound that rejected these would be a bound on the summation order."""
    x, wt, b, want64, pair32, want32 = _conv_case(shape)
    r = ref64.budget_pairwise(_conv_mutant(shape, kind), want64, pair32, ref64.M_CONV, what=kind)
    print("%s %s: %.2f x E32p max, %.2f x E32p mean, %.2f x per channel" % ((shape, kind) + r))


@pytest.mark.parametrize("shape", UNIT_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_the_oracle_does_not_scale_in_the_pairwise_unit(shape):
    """Why the unit of ref64.budget was not enough here: the oracle adds its K terms one after the other, and its distance from float64 in units of a
    pairwise sum's grows with K.  (Not asserted to pass: it is the reference of the 1e-4 tests, not a kernel.)"""
    x, wt, b, want64, pair32, want32 = _conv_case(shape)
    d = want32.astype(np.float64) - want64
    e = np.abs(pair32.astype(np.float64) - want64)
    rmax, rmean, rchan = np.abs(d).max() / e.max(), np.abs(d).mean() / e.mean(), np.abs(d.mean(axis=(0, 1, 2))).max() / e.mean()
    print("%s K=%d: the fp32 C oracle at %.1f x E32p max, %.1f x E32p mean, %.1f x per channel" % (shape, shape[3] * shape[5] ** 2, rmax, rmean, rchan))
    if shape == DEEP:
        assert rmax > 4


# ---- the half budget (the fp16 convolution kernels: tests/test_conv_f16_budget_gpu.py) ----

TOLH = dict(rtol=4e-3, atol=4e-3)  # the bound of every older test of the f16 kernels, against the quantised oracle


def _h32(a):
    """Round to half (nearest even) and back to float32: what a half tensor stores."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def test_ulp16_is_the_spacing_of_binary16():
    r = np.random.default_rng(16)
    v = np.concatenate([
        r.standard_normal(60000) * np.exp2(r.integers(-12, 14, 60000)),          # the normal range, both signs
        r.uniform(-2.0 ** -14, 2.0 ** -14, 20000),                               # subnormals
        np.exp2(r.integers(-16, 15, 20000)) * (1.0 + r.uniform(-2e-4, 2e-4, 20000)) * r.choice([-1.0, 1.0], 20000),  # either side of powers of two
        np.exp2(np.arange(-26, 16.0)), -np.exp2(np.arange(-26, 16.0)), np.nextafter(np.exp2(np.arange(-26, 16.0)), 0), [0.0, 65504.0, -65504.0]])
    assert v.dtype == np.float64 and v.size >= 100000
    u = ref64.ulp16(v)
    assert (np.abs(ref64.half(v) - v) <= 0.5 * u).all()
    assert u[np.abs(v) < 2.0 ** -14].tolist() == [2.0 ** -24] * int((np.abs(v) < 2.0 ** -14).sum())
    assert ref64.ulp16(1.0) == 2.0 ** -10 and ref64.ulp16(np.nextafter(1.0, 0)) == 2.0 ** -11 and ref64.ulp16(-0.75) == 2.0 ** -11
    h = np.arange(0, 0x7BFF, dtype=np.uint16).view(np.float16)  # every non-negative half below the largest (whose np.spacing overflows)
    np.testing.assert_array_equal(ref64.ulp16(h.astype(np.float64)), np.spacing(h).astype(np.float64))
    np.testing.assert_array_equal(ref64.ulp16(-h.astype(np.float64)), np.spacing(h).astype(np.float64))  # (np.spacing of a negative power of two steps toward zero)
    assert ref64.ulp16(65504.0) == 32.0


# N, H, W, IC, OC, k, activation: two images of more than one 8 x 32 tile, ragged against it.  K = 576, 1152, 2304, 243
HALF_LAYERS = [(2, 9, 33, 64, 64, 3, ""), (2, 9, 33, 128, 128, 3, "relu"), (2, 9, 33, 256, 64, 3, "tanh"), (2, 9, 33, 3, 32, 9, "")]
HALF_IDS = ["64-64", "128-128_relu", "256-64_tanh", "3-32_9x9"]
HALF_TILE = (8, 32)


@functools.lru_cache(maxsize=None)
def _half_case(layer):
    """(x, w) rounded to half, the fp32 bias, the float64 reference, the pairwise fp32 evaluation and the quantised C oracle of one layer: read-only."""
    n, h, w, ic, oc, k, act = layer
    x, wt, b = _h32(_rand((n, h, w, ic), 31)), _h32(_rand((oc, ic, k, k), 32, 1.0 / np.sqrt(k * k * ic))), _rand((oc,), 33, 0.1)
    pads, out_hw = _geometry(h, w, k, 1, "same")
    out = (x, wt, b, ref64.conv_layer_general(x, wt, b, 1, pads, "constant", out_hw, None, act), ref64.conv_layer_pairwise32(x, wt, b, 1, pads, "constant", out_hw, None, act),
           O.conv2d(x, wt, b, 1, pads, "constant", act, threads=8))
    for a in out:
        a.setflags(write=False)
    return out


def _truncated_half(y):
    """fp32 -> half toward zero: the store of a kernel that cuts the mantissa instead of rounding it."""
    y = np.asarray(y, np.float32)
    h = y.astype(np.float16)
    away = np.abs(h.astype(np.float32)) > np.abs(y)
    return np.where(away, np.nextafter(h, np.float16(0)), h).astype(np.float32)


def _tap_parts(x, wt):
    """The k*k tap contributions of a "same" stride-1 layer, each an fp32 matmul over the input channels: [k*k][N,H,W,OC]."""
    n, h, w, ic = x.shape
    oc, _, k, _ = wt.shape
    p = k // 2
    xp = np.zeros((n, h + 2 * p, w + 2 * p, ic), np.float32)
    xp[:, p:p + h, p:p + w] = x
    return [xp[:, dy:dy + h, dx:dx + w] @ np.ascontiguousarray(wt[:, :, dy, dx].T) for dy in range(k) for dx in range(k)]


HALF_MUTANTS = ["trunc", "splitk16", "acc16", "bias16", "preact16", "hole", "swap"]


def _half_mutant(layer, kind):
    """What a wrong f16 kernel would store, as float32 holding halves; None where the mutant does not apply to the layer."""
    n, h, w, ic, oc, k, act = layer
    x, wt, b, want64, pair32, oracle = _half_case(layer)
    pads, out_hw = _geometry(h, w, k, 1, "same")
    if kind == "trunc":
        return _truncated_half(pair32)
    if kind == "splitk16":  # K in two halves (kernel rows 0 .. k/2 and the rest), each partial sum rounded to half before they are added
        parts = _tap_parts(x, wt)
        cut = (k // 2 + 1) * k
        v = _h32(np.sum(parts[:cut], axis=0, dtype=np.float32)) + _h32(np.sum(parts[cut:], axis=0, dtype=np.float32)) + b
        return _h32(ref64.activation32(act, v))
    if kind == "acc16":  # the accumulator kept in half from tap to tap
        acc = np.zeros((n,) + out_hw + (oc,), np.float32)
        for part in _tap_parts(x, wt):
            acc = _h32(acc + part)
        return _h32(ref64.activation32(act, acc + b))
    if kind == "bias16":
        return _h32(ref64.conv_layer_pairwise32(x, wt, _h32(b), 1, pads, "constant", out_hw, None, act))
    if kind == "preact16":  # the pre-activation rounded to half before a transcendental activation
        if act not in ("tanh", "sigmoid"):
            return None
        return _h32(ref64.activation32(act, _h32(ref64.conv2d_pairwise32(x, wt, b, 1, pads, "constant", out_hw))))
    y = _h32(pair32)
    if kind == "hole":  # one tile never written
        y[1, :HALF_TILE[0], :HALF_TILE[1]] = np.nan
        return y
    if kind == "swap":  # one tile taken from the neighbouring image
        y[1, :HALF_TILE[0], :HALF_TILE[1]] = y[0, :HALF_TILE[0], :HALF_TILE[1]]
        return y
    raise ValueError(kind)


def _torch32(layer):
    import torch
    import torch.nn.functional as F

    n, h, w, ic, oc, k, act = layer
    x, wt, b, want64, pair32, oracle = _half_case(layer)
    v = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt), torch.from_numpy(b), padding=k // 2).permute(0, 2, 3, 1).numpy()
    return ref64.activation32(act, np.ascontiguousarray(v))


@pytest.mark.parametrize("how", ["pairwise", "oracle", "torch"])
@pytest.mark.parametrize("layer", HALF_LAYERS, ids=HALF_IDS)
def test_budget_half_accepts_honest_evaluations(layer, how):
    """Three fp32 evaluations of different summation order, each rounded to half once: all inside M_F16, the pairwise one below 1 by construction."""
    x, wt, b, want64, pair32, oracle = _half_case(layer)
    y32 = {"pairwise": lambda: pair32, "oracle": lambda: oracle, "torch": lambda: _torch32(layer)}[how]()
    assert y32.dtype == np.float32
    ratio, mismatch, chan = ref64.budget_half(_h32(y32), want64, pair32, ref64.M_F16, what=how, tile=HALF_TILE)
    print("HALF honest %s %s: %.2f x E32p max, %.3f %% mismatch, %.4f ulp per channel" % (how, layer, ratio, 100 * mismatch, chan))
    if how == "pairwise":
        assert ratio <= 1.0


@pytest.mark.parametrize("kind", HALF_MUTANTS)
@pytest.mark.parametrize("layer", HALF_LAYERS, ids=HALF_IDS)
def test_budget_half_rejects_the_mutants(layer, kind):
    x, wt, b, want64, pair32, oracle = _half_case(layer)
    y = _half_mutant(layer, kind)
    if y is None:
        assert kind == "preact16" and layer[6] not in ("tanh", "sigmoid")
        return
    with pytest.raises(AssertionError) as e:
        ref64.budget_half(y, want64, pair32, ref64.M_F16, what=kind, tile=HALF_TILE)
    msg = str(e.value)
    print("HALF mutant %s %s: %s" % (kind, layer, msg[:330]))
    if kind == "hole":
        assert "%d of %d values are not finite" % (8 * 32 * layer[4], y.size) in msg and "(n, y, x, channel) = (1, 0, 0, 0)" in msg, msg
    else:
        assert "out of the half budget" in msg, msg
    if kind == "swap":
        assert re.search(r"worst \(n, y, x, channel\) = \(1, [0-7], ([0-9]|[12][0-9]|3[01]), \d+\); tile 8x32 \(TH x TW\): tile \(ty, tx\) = \(0, 0\)", msg), msg


# Whether the mutant passes allclose(..., rtol 4e-3, atol 4e-3) against the quantised oracle, per layer in the order of HALF_LAYERS: measured, and asserted
# so that a change is noticed.  Every arithmetic mutant passes on every layer it applies to: the truncating store, the half split-K partials, the half
# accumulator, the half bias and the half pre-activation.
PASSES_TOLH = {"trunc": (True, True, True, True), "splitk16": (True, True, True, True), "acc16": (True, True, True, True),
               "bias16": (True, True, True, True), "preact16": (None, None, True, None), "hole": (False,) * 4, "swap": (False,) * 4}


def test_what_the_older_bound_lets_through():
    """The gap this budget closes: TOLH against the quantised oracle accepts a store that truncates, split-K partials kept in half, an accumulator kept in
    half from tap to tap, a half bias and a half pre-activation on every layer they apply to, while budget_half rejects each of them (116 x E32p max at the
    least, the half bias; 800 x and more for the others).  Only a missing or misplaced tile fails both."""
    for kind in HALF_MUTANTS:
        for layer, expected in zip(HALF_LAYERS, PASSES_TOLH[kind]):
            y = _half_mutant(layer, kind)
            if y is None:
                assert expected is None
                continue
            x, wt, b, want64, pair32, oracle = _half_case(layer)
            want = _h32(oracle)
            passes = bool(np.isfinite(y).all() and np.allclose(y, want, **TOLH))
            over = np.maximum(np.abs(np.nan_to_num(y).astype(np.float64) - want64) - 0.5 * ref64.ulp16(want64), 0).max() / np.abs(pair32.astype(np.float64) - want64).max()
            print("HALF gap %-9s %-13s passes TOLH: %-5s  budget_half statistic %.0f" % (kind, "x".join(map(str, layer[3:6])), passes, over))
            assert passes == expected, (kind, layer)
            with pytest.raises(AssertionError):
                ref64.budget_half(y, want64, pair32, ref64.M_F16, what=kind)


def test_the_half_margin_is_a_power_of_two_below_every_mutant():
    """The cap of M_F16: the largest power of two at which every mutant above is still rejected (the half bias, 116 x at its smallest: 64)."""
    assert ref64.M_F16 & (ref64.M_F16 - 1) == 0 and ref64.M_F16 <= 64
    for layer in HALF_LAYERS:
        x, wt, b, want64, pair32, oracle = _half_case(layer)
        for kind in HALF_MUTANTS:
            y = _half_mutant(layer, kind)
            if y is not None:
                with pytest.raises(AssertionError):
                    ref64.budget_half(y, want64, pair32, 64, what=kind)


# ---------------------------------------------------------------------------------------------------------------- instance norm
import norm_cases  # noqa: E402

NORM_SHAPES = [(1, 40, 60, 4), (3, 17, 23, 5)]
NORM_CASES = [(s, d, f) for s in NORM_SHAPES for d in ("f32", "f16") for f in norm_cases.families(d)]
NORM_IDS = ["%s-%s-%s" % ("x".join(map(str, s)), d, f) for s, d, f in NORM_CASES]


@functools.lru_cache(maxsize=None)
def _norm_case(shape, dtype, family, act="leakyRelu"):
    x = norm_cases.plane(family, shape, dtype, seed=3)
    beta, gamma = norm_cases.params(shape[3], seed=3)
    want64 = ref64.instancenorm(x, beta, gamma, 1e-5, act, 0.1)
    model32 = ref64.instancenorm32(x, beta, gamma, 1e-5, act, 0.1)
    floor = ref64.norm_floor(x, beta, gamma, 1e-5)
    for a in (want64, model32, floor):
        a.setflags(write=False)
    return x, beta, gamma, want64, model32, floor


def _norm_got(model32, dtype):
    """What a tensor of that type hands back of an fp32 evaluation."""
    return ref64.half(model32) if dtype == "f16" else model32


def test_instancenorm_agrees_with_the_c_oracle():
    """ref64.instancenorm against the fp32 C oracle (two passes over the plane, one term after the other) on a benign plane, to the oracle's precision:
    its outputs are of magnitude 4 and its sums of 2400 terms lose a few ulps, 1e-5 leaves a factor of ten."""
    shape = (2, 40, 60, 5)
    x = norm_cases.plane("benign", shape)
    beta, gamma = norm_cases.params(shape[3])
    for act in ("", "relu", "leakyRelu"):
        want = ref64.instancenorm(x, beta, gamma, 1e-5, act, 0.1)
        assert want.dtype == np.float64
        np.testing.assert_allclose(O.instancenorm(x, beta, gamma, act, 0.1), want, rtol=0, atol=1e-5)
    np.testing.assert_allclose(O.instancenorm(x, beta, gamma, "", 0.0, eps=1e-3), ref64.instancenorm(x, beta, gamma, 1e-3), rtol=0, atol=1e-5)


@pytest.mark.parametrize("shape,dtype,family", NORM_CASES, ids=NORM_IDS)
def test_the_norm_stick_is_sound_on_every_family(shape, dtype, family):
    """instancenorm32 on the adverse planes.  It is inside budget_norm at M = 1 by construction (it is the unit), rounded to half where the tensor is half.
    That the unit itself is fp32-sized is the second assertion: per plane, E stays below half of M_NORM fp32 ulps of the largest output plus the shift
    term |mean * mul| + |beta| -- an fp32 evaluation rounds the mean, the multiplier, the shift and the result once each, and a pairwise sum adds little
    to that -- so M_NORM x E never grows into a tolerance that a lost digit passes."""
    x, beta, gamma, want64, model32, floor = _norm_case(shape, dtype, family)
    assert model32.dtype == np.float32 and want64.dtype == np.float64
    ratio = ref64.budget_norm(_norm_got(model32, dtype), want64, model32, 1, floor, what=family, x=x, half_out=dtype == "f16")
    assert ratio <= 1.0
    e = np.abs(model32.astype(np.float64) - want64).max(axis=(1, 2))
    unit = np.spacing(np.abs(want64).max(axis=(1, 2)).astype(np.float32)).astype(np.float64) + floor
    worst = float((e / unit).max())
    print("NORMSTICK %s %s %s: E = %.2f fp32 ulps of (largest output, shift term)" % ("x".join(map(str, shape)), dtype, family, worst))
    assert worst <= ref64.M_NORM / 2, worst


NORM_MUTANTS = {"variance": dict(var_scale=1.0 + 1e-3), "mean": dict(mean_shift=1e-3)}


@pytest.mark.parametrize("kind", sorted(NORM_MUTANTS))
@pytest.mark.parametrize("shape,dtype,family", NORM_CASES, ids=NORM_IDS)
def test_budget_norm_rejects_the_mutants(shape, dtype, family, kind):
    """The budget can fail: statistics off by 1e-3 -- var + eps scaled by 1 + 1e-3, or the mean moved by 1e-3 sqrt(var + eps) -- are rejected on every
    family at M_NORM.  (Relative to var + eps, not to var: on a constant plane, and where the variance is far below eps, the result does not depend on
    the variance at all and a mutant of it alone is no mutant.)  The variance mutant scales (x - mean) mul by 5e-4: on a constant plane that product
    is zero and the exact result is unchanged, which is the one combination that must pass instead."""
    x, beta, gamma, want64, model32, floor = _norm_case(shape, dtype, family)
    y = ref64.instancenorm(x, beta, gamma, 1e-5, "leakyRelu", 0.1, **NORM_MUTANTS[kind])
    y = ref64.half(y) if dtype == "f16" else y.astype(np.float32)
    check = lambda: ref64.budget_norm(y, want64, model32, ref64.M_NORM, floor, what=kind, x=x, half_out=dtype == "f16")
    if kind == "variance" and family == "constant":
        check()
        return
    with pytest.raises(AssertionError) as info:
        check()
    assert "plane (n, c) = (" in str(info.value) and "std from the mean" in str(info.value), str(info.value)
