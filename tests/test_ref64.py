"""tests/ref64.py on the CPU: the float64 reference against torch's float64 convolution, the fp32 C oracle inside its own budget, and the comparator
against mutants of the oracle that rtol = atol = 1e-4 lets through (they must be rejected at the margin M the GPU tests use) and one it must accept."""
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
