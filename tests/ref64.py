"""A plain float64 restatement of the ESPCN-shaped nets, NumPy only and independent of oracle/snn_oracle.c, and the error budget that holds the
fused kernels to fp32 accuracy.

The fp32 C oracle is itself 2e-7 to 5e-7 (max) and about 3e-8 (mean) away from the exact result: those two numbers, measured on the very input of a
test (E32max, E32mean), are the unit in which a kernel's own distance from the exact result is expressed.  A kernel that computes in fp32 lands within
a small multiple M of them; one that lost mantissa bits somewhere (a TF32 or split-f16 product, a truncated weight, a bias off by 2e-6) does not,
although all of these pass rtol = atol = 1e-4 against the oracle.

The general fp32 convolution kernels (deep reductions: K = IC k^2 up to 4608, split-K, Winograd) get a reference of any kernel size, stride, pad mode and
output extent (conv2d_general) and a sharper unit: the oracle sums its K terms one after the other, so its own error grows with K (21 x a pairwise sum's at
K = 4608) and a budget in units of it lets 16-bit weights through.  conv2d_pairwise32 forms every product in fp32 and reduces K by a tree of fp32 additions;
its distance from float64 (E32p) is what an fp32 kernel with a blocked or tree-shaped reduction can reach, and budget_pairwise holds a kernel to M_CONV times it,
with a third bound on the mean signed error per output channel (a bias off by 2e-6 hides in max and mean at these depths).

The fp16 convolution kernels (half storage, products of half operands accumulated in fp32, an fp32 epilogue, one round-to-nearest-even store) are held to
the correctly rounded half of the exact result: budget_half allows M_F16 times E32p max beyond half a binary16 ulp (ulp16), where a tolerance of a few
half ulps lets a truncating store or partial sums kept in half through.

InstanceNorm (the stand-alone plan, the convolution's tile statistics, the norm + Add pair) is held plane by plane: instancenorm is the float64 reference,
instancenorm32 a straightforward two-pass fp32 model of the contract whose distance from it is the unit, floored at the rounding of the shift of the one-FMA form
(norm_floor); budget_norm holds a result to M_NORM times that, half tensors through budget_half."""
import numpy as np

# The margin of every budget test: twice the largest ratio any fp32 kernel family showed against float64 on an MI355X (2.02, DESIGN.md section 3
# has the table), rounded up to a power of two.  It is also the largest at which the 2e-6 bias mutant of tests/test_ref64.py (9.7 x E32mean) is rejected.
M = 8

# The margin of the convolution budget tests (budget_pairwise), one value for all fp32 convolution families.  Measured on an MI355X in units of E32p
# (DESIGN.md section 3 has the table): up to 8.4 where no accumulator adds more than 1152 terms one after the other, 12.1 to 13.2 in the three cases with a
# chain of 2304 (conv2d_generic at K = 2304, conv2d_mfma split two ways and conv2d_ksplit over two waves at K = 4608).  The rule of M (twice the largest,
# rounded up to a power of two) gives 32, but from 27 on the 2e-6 bias mutant of tests/test_ref64.py is no longer rejected: the constant is the largest power
# of two at which all four mutants are, and the chain-2304 cases keep a factor of 1.2 instead of two (the kernels are deterministic: the ratios reproduce).
M_CONV = 16
# conv2d_mfma with the split over K pinned off at K = 4608 (SNNHIP_CONV_SPLITK=1: one chain of 4608 terms per output, which the planner never chooses):
# 24.5 x max, the fp32 C oracle's own ratio on that layer (18.8 x: it adds one term after the other too).  Summation order, not lost bits; held to the cap
# of 32, at which the 16-bit-weight mutant (52 x max, 64 x mean at its smallest), the missing block and the unwritten row are rejected and the bias mutant
# (27 x to 31 x per channel) is not.
M_CONV_UNSPLIT = 32

# The margin of the fp16 convolution budget tests (budget_half), one value for all f16 convolution families: how far beyond half a binary16 ulp of the exact
# value a result may lie, in units of E32p max.  Measured on an MI355X (DESIGN.md section 3 has the table): at most 1.56 (conv2d_widep_f16, a row of ten
# tiles), 1.22 on conv2d_wide_f16, 1.11 on conv2d_mfma with one chain of K = 4608, below 1 elsewhere.  The rule of M (twice the largest, rounded up to a power
# of two) gives 4.  An fp32 sum taken one term after the other is just as honest as the kernels' blocked sums, though, and tests/test_ref64.py holds the budget
# to accepting it: the C oracle and torch's fp32 convolution, rounded to half, reach 5.8 at K = 2304.  The constant is the smallest power of two that accepts
# every honest evaluation; the smallest mutant of tests/test_ref64.py (a bias rounded to half) stands at 116, so every power of two up to 64 rejects them all.
M_F16 = 8

_BN_EPS = float(np.float32(0.001))    # oracle/snn_oracle.c:bn_apply: sqrtf(var + 0.001f) ...
_BN_FLOOR = float(np.float32(0.0001))  # ... floored at 0.0001f


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def conv2d(x, w_oihw, bias=None):
    """k x k convolution, stride 1, "same" zero padding (k odd): k*k shifted matmuls.  x [N,H,W,IC], w [OC,IC,k,k] -> [N,H,W,OC]."""
    x, w = _f64(x), _f64(w_oihw)
    n, h, wd, ic = x.shape
    oc, ic2, k, k2 = w.shape
    assert ic == ic2 and k == k2 and k % 2 == 1, (x.shape, w.shape)
    p = k // 2
    xp = np.zeros((n, h + 2 * p, wd + 2 * p, ic), np.float64)
    xp[:, p:p + h, p:p + wd, :] = x
    y = np.zeros((n, h, wd, oc), np.float64)
    for dy in range(k):
        for dx in range(k):
            y += xp[:, dy:dy + h, dx:dx + wd, :] @ w[:, :, dy, dx].T
    if bias is not None:
        y += _f64(bias)
    return y


def batchnorm(v, bn):
    s = np.maximum(np.sqrt(_f64(bn["var"]) + _BN_EPS), _BN_FLOOR)
    return (_f64(bn["gamma"]) / s) * (_f64(v) - _f64(bn["mean"])) + _f64(bn["beta"])


def activation(name, v, alpha=0.0):
    v = _f64(v)
    if name in ("", "linear", "none", None):
        return v
    if name == "relu":
        return np.maximum(v, 0.0)
    if name == "relu6":
        return np.clip(v, 0.0, 6.0)
    if name == "leakyRelu":
        return np.maximum(v, v * float(np.float32(alpha)))
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if name == "tanh":
        return np.tanh(v)
    if name == "SiLU":
        return v / (1.0 + np.exp(-v))
    raise ValueError("ref64: unknown activation %r" % (name,))


def _resolve(lo, count, size, pad_mode):
    """The source coordinates lo .. lo + count - 1 under a pad mode; -1 = the read returns zero.  Reflect mirrors once about the first / last sample
    (no repeated edge) and reads zero where that still falls outside, replicate clamps, constant (and "none") reads zero outside."""
    s = np.arange(lo, lo + count)
    if pad_mode == "replicate":
        return np.clip(s, 0, size - 1)
    if pad_mode == "reflect":
        s = np.abs(s)
        s = np.where(s >= size, 2 * size - 2 - s, s)
    elif pad_mode not in ("constant", "none"):
        raise ValueError("ref64: unknown pad mode %r" % (pad_mode,))
    return np.where((s >= 0) & (s < size), s, -1)


def _padded(x, k, stride, pads, pad_mode, out_hw):
    """x [N,H,W,C] as the explicitly padded array an output of out_hw reads: rows -padL .. (OH - 1) stride + k - 1 - padL, columns likewise from -padT
    (pads = (T, B, L, R); the reference hands T to the column offset and L to the row offset, its quirk Q3 -- every "same" / "valid" layer has T = L).
    The far pads are not used: the extent comes from the caller, and what lies beyond the data reads padding.  A 1 x 1 kernel has no padding at all."""
    n, h, w, c = x.shape
    oh, ow = out_hw
    padx, pady = (0, 0) if k == 1 else (pads[0], pads[2])
    rows = _resolve(-pady, (oh - 1) * stride + k, h, "constant" if k == 1 else pad_mode)
    cols = _resolve(-padx, (ow - 1) * stride + k, w, "constant" if k == 1 else pad_mode)
    xp = x[:, np.maximum(rows, 0)][:, :, np.maximum(cols, 0)]
    xp[:, rows < 0] = 0
    xp[:, :, cols < 0] = 0
    return xp


def conv2d_general(x, w_oihw, bias=None, stride=1, pads=(0, 0, 0, 0), pad_mode="constant", out_hw=None):
    """k x k convolution in float64: any k (even k with the asymmetric "same" offsets of quirk Q1 in pads), stride 1 or 2, constant / replicate / reflect
    padding, the output extent out_hw = (OH, OW) from the caller (the reference's size rules Q2 / Q20 stay with oracle_lib.out_dim).  k*k shifted matmuls
    over the padded array.  x [N,H,W,IC], w [OC,IC,k,k] -> [N,OH,OW,OC]."""
    x, w = _f64(x), _f64(w_oihw)
    oc, ic, k, k2 = w.shape
    assert x.ndim == 4 and x.shape[3] == ic and k == k2 and stride in (1, 2), (x.shape, w.shape, stride)
    oh, ow = out_hw
    xp = _padded(x, k, stride, pads, pad_mode, out_hw)
    y = np.zeros((x.shape[0], oh, ow, oc), np.float64)
    for dy in range(k):
        for dx in range(k):
            y += xp[:, dy:dy + (oh - 1) * stride + 1:stride, dx:dx + (ow - 1) * stride + 1:stride, :] @ w[:, :, dy, dx].T
    if bias is not None:
        y += _f64(bias)
    return y


def maxpool(x, k=3, stride=2, out_hw=None):
    """Max-pooling with the window clipped to the image (no padding), in the dtype of x; the extent from the caller (oracle_lib.pool_out_dim)."""
    x = np.asarray(x)
    n, h, w, c = x.shape
    oh, ow = out_hw
    assert (oh - 1) * stride < h and (ow - 1) * stride < w, (x.shape, out_hw)
    y = np.full((n, oh, ow, c), -np.inf, x.dtype)
    for fy in range(k):
        for fx in range(k):
            v = x[:, fy::stride, fx::stride][:, :oh, :ow]
            y[:, :v.shape[1], :v.shape[2]] = np.maximum(y[:, :v.shape[1], :v.shape[2]], v)
    return y


_PAIRWISE_BYTES = 1 << 27  # the product array of one output-channel chunk


def conv2d_pairwise32(x, w_oihw, bias=None, stride=1, pads=(0, 0, 0, 0), pad_mode="constant", out_hw=None):
    """The same convolution in fp32 with a pairwise reduction: every product x * w formed in np.float32, the K = k*k*IC products of an output ordered
    (dy, dx, ic) and summed by a tree of fp32 additions (neighbours added level by level; an odd level is padded with one zero), then the bias added in
    fp32.  No matmul, no einsum: deterministic on every machine.  Its distance from conv2d_general is the unit E32p of budget_pairwise."""
    x, w = np.asarray(x, np.float32), np.asarray(w_oihw, np.float32)
    oc, ic, k, k2 = w.shape
    assert x.ndim == 4 and x.shape[3] == ic and k == k2 and stride in (1, 2), (x.shape, w.shape, stride)
    oh, ow = out_hw
    xp = _padded(x, k, stride, pads, pad_mode, out_hw)
    pix, kk = x.shape[0] * oh * ow, k * k * ic
    xs = np.empty((kk, pix), np.float32)
    for dy in range(k):
        for dx in range(k):
            xs[(dy * k + dx) * ic:(dy * k + dx + 1) * ic] = xp[:, dy:dy + (oh - 1) * stride + 1:stride, dx:dx + (ow - 1) * stride + 1:stride, :].reshape(pix, ic).T
    ws = np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(kk, oc))
    y = np.empty((pix, oc), np.float32)
    step = max(1, _PAIRWISE_BYTES // (4 * kk * pix))
    for o in range(0, oc, step):
        p = xs[:, :, None] * ws[:, None, o:o + step]
        assert p.dtype == np.float32
        while p.shape[0] > 1:
            q = p[0:p.shape[0] - 1:2] + p[1::2]
            p = np.concatenate([q, p[-1:]]) if p.shape[0] & 1 else q  # (the odd one out + 0.0f)
        y[:, o:o + step] = p[0]
    if bias is not None:
        y += np.asarray(bias, np.float32)
    return y.reshape(x.shape[0], oh, ow, oc)


def batchnorm32(v, bn):
    """batchnorm in fp32 NumPy, in the oracle's order of operations."""
    f = lambda a: np.asarray(a, np.float32)
    s = np.maximum(np.sqrt(f(bn["var"]) + np.float32(0.001)), np.float32(0.0001))
    y = (f(bn["gamma"]) / s) * (f(v) - f(bn["mean"])) + f(bn["beta"])
    assert y.dtype == np.float32
    return y


def activation32(name, v, alpha=0.0):
    """activation in fp32 NumPy."""
    v = np.asarray(v, np.float32)
    one = np.float32(1.0)
    if name in ("", "linear", "none", None):
        return v
    if name == "relu":
        return np.maximum(v, np.float32(0.0))
    if name == "relu6":
        return np.clip(v, np.float32(0.0), np.float32(6.0))
    if name == "leakyRelu":
        return np.maximum(v, v * np.float32(alpha))
    if name == "sigmoid":
        return one / (one + np.exp(-v))
    if name == "tanh":
        return np.tanh(v)
    if name == "SiLU":
        return v / (one + np.exp(-v))
    raise ValueError("ref64: unknown activation %r" % (name,))


def conv_layer_general(x, w_oihw, bias, stride, pads, pad_mode, out_hw, bn=None, act="", alpha=0.0):
    """convolution -> batchnorm -> activation in float64."""
    v = conv2d_general(x, w_oihw, bias, stride, pads, pad_mode, out_hw)
    if bn is not None:
        v = batchnorm(v, bn)
    return activation(act, v, alpha)


def conv_layer_pairwise32(x, w_oihw, bias, stride, pads, pad_mode, out_hw, bn=None, act="", alpha=0.0):
    """The same layer with conv2d_pairwise32 and the fp32 epilogue."""
    v = conv2d_pairwise32(x, w_oihw, bias, stride, pads, pad_mode, out_hw)
    if bn is not None:
        v = batchnorm32(v, bn)
    y = activation32(act, v, alpha)
    assert y.dtype == np.float32
    return y


def depth_to_space_tanh(x, r):
    """[N,H,W,r*r] -> [N,rH,rW,1]: output pixel (r*y + dy, r*x + dx) takes channel r*dy + dx, then tanh."""
    x = _f64(x)
    n, h, w, c = x.shape
    assert c == r * r, (x.shape, r)
    y = x.reshape(n, h, w, r, r).transpose(0, 1, 3, 2, 4).reshape(n, h * r, w * r, 1)
    return np.tanh(y)


def u8_in(u, mean, norm):
    """The 8-bit input map: (u - mean) * norm, with the plan's fp32 constants."""
    return (np.asarray(u).astype(np.float64) - float(np.float32(mean))) * float(np.float32(norm))


def u8_out_pre(x, scale, offset):
    """The value the 8-bit output map rounds: x * scale + offset."""
    return _f64(x) * float(np.float32(scale)) + float(np.float32(offset))


def u8_out(x, scale, offset):
    """The 8-bit output map: clamp(rint(x * scale + offset), 0, 255)."""
    return np.clip(np.rint(u8_out_pre(x, scale, offset)), 0.0, 255.0).astype(np.uint8)


def conv_layer(layer, x):
    assert layer["type"] == "Conv2D" and layer["stride"] == 1 and layer["padding"] == "same" and layer.get("pad_mode", "constant") == "constant", layer["name"]
    v = conv2d(x, layer["w"], layer["b"])
    if layer["bn"] is not None:
        v = batchnorm(v, layer["bn"])
    return activation(layer["activation"], v, layer.get("alpha", 0.0))


def espcn(net, x, r):
    """The dict models.espcn_weights returns (its fp32 weights cast to float64, nothing rounded in between) on x [N,H,W,1]."""
    v = _f64(x)
    for layer in net["layers"]:
        if layer["type"] == "Subpixel":
            assert int(layer.get("upscale", 2)) == r and layer.get("mode", 0) == 0, layer
            v = depth_to_space_tanh(v, r)
        else:
            v = conv_layer(layer, v)
    return v


def _where(idx, shape, r, tiles):
    """The worst pixel in words: (n, y, x) of the output, its input-resolution pixel, and per kernel tile the tile and the place inside it."""
    n, y, x = (int(v) for v in np.unravel_index(idx, shape)[:3])
    ly, lx = y // r, x // r
    txt = "worst pixel (n, y, x) = (%d, %d, %d)" % (n, y, x)
    if r != 1:
        txt += ", input pixel (%d, %d)" % (ly, lx)
    for name, (tw, th) in (tiles or {}).items():
        iy, ix = ly % th, lx % tw
        seam = [s for s, hit in (("left", ix == 0), ("right", ix == tw - 1), ("top", iy == 0), ("bottom", iy == th - 1)) if hit]
        txt += "; %s tile %dx%d: tile (ty, tx) = (%d, %d), at (%d, %d) inside it, %s" % (
            name, tw, th, ly // th, lx // tw, iy, ix, ("on the " + "/".join(seam) + " seam") if seam else "not on a seam")
    return txt


def budget(got, ref64, oracle32, M, r=1, tiles=None, what=""):
    """Holds `got` to M times the fp32 oracle's own distance from the float64 reference, measured on this very input:
        max |got - ref64| <= M * E32max     and     mean |got - ref64| <= M * E32mean,     E32 = |oracle32 - ref64|.
    Returns (max ratio, mean ratio).  r and tiles ({name: (TW, TH)} in input-resolution pixels) only serve the failure message."""
    ref64 = _f64(ref64)
    got = np.asarray(got)
    assert got.shape == ref64.shape == np.asarray(oracle32).shape, (got.shape, ref64.shape, np.asarray(oracle32).shape)
    e32 = np.abs(_f64(oracle32) - ref64)
    e32max, e32mean = float(e32.max()), float(e32.mean())
    bad = ~np.isfinite(got)
    if bad.any():
        raise AssertionError("%s%d of %d values are not finite (never written, or NaN / Inf computed): first at %s"
                             % (what and what + ": ", int(bad.sum()), bad.size, _where(int(np.argmax(bad)), got.shape, r, tiles)))
    err = np.abs(_f64(got) - ref64)
    emax, emean = float(err.max()), float(err.mean())
    rmax = emax / e32max if e32max > 0 else (0.0 if emax == 0 else np.inf)
    rmean = emean / e32mean if e32mean > 0 else (0.0 if emean == 0 else np.inf)
    if not (emax <= M * e32max and emean <= M * e32mean):
        raise AssertionError("%sout of the float64 budget: max error %.3e = %.2f x E32max (%.3e), mean error %.3e = %.2f x E32mean (%.3e), allowed %g x; %s"
                             % (what and what + ": ", emax, rmax, e32max, emean, rmean, e32mean, M, _where(int(np.argmax(err)), got.shape, r, tiles)))
    return rmax, rmean


def _where_conv(idx, shape, tile):
    """The worst output element in words: (n, y, x, channel) and, given the kernel's pixel tile (TH, TW), the tile and the place inside it."""
    n, y, x, c = (int(v) for v in np.unravel_index(idx, shape))
    txt = "worst (n, y, x, channel) = (%d, %d, %d, %d)" % (n, y, x, c)
    if tile:
        th, tw = tile
        iy, ix = y % th, x % tw
        seam = [s for s, hit in (("left", ix == 0), ("right", ix == tw - 1), ("top", iy == 0), ("bottom", iy == th - 1)) if hit]
        txt += "; tile %dx%d (TH x TW): tile (ty, tx) = (%d, %d), at (%d, %d) inside it, %s" % (
            th, tw, y // th, x // tw, iy, ix, ("on the " + "/".join(seam) + " seam") if seam else "not on a seam")
    return txt


def budget_pairwise(got, ref64, pair32, M, what="", tile=None):
    """Holds `got` [N,H,W,C] to M times the distance of the pairwise fp32 evaluation from the float64 reference on this very input, E32p = |pair32 - ref64|:
        max |got - ref64| <= M * E32p_max,     mean |got - ref64| <= M * E32p_mean     and
        max over channels |mean over (n, y, x) of (got - ref64)| <= M * E32p_mean       (a systematic offset of one channel: a bias, a folded BN shift).
    Returns (max ratio, mean ratio, per-channel ratio).  tile = (TH, TW) in output pixels only serves the failure message."""
    ref64 = _f64(ref64)
    got = np.asarray(got)
    assert got.ndim == 4 and got.shape == ref64.shape == np.asarray(pair32).shape, (got.shape, ref64.shape, np.asarray(pair32).shape)
    e32 = np.abs(_f64(pair32) - ref64)
    e32max, e32mean = float(e32.max()), float(e32.mean())
    bad = ~np.isfinite(got)
    if bad.any():
        raise AssertionError("%s%d of %d values are not finite (never written, or NaN / Inf computed): first at %s"
                             % (what and what + ": ", int(bad.sum()), bad.size, _where_conv(int(np.argmax(bad)), got.shape, tile)))
    diff = _f64(got) - ref64
    err = np.abs(diff)
    chan = np.abs(diff.mean(axis=(0, 1, 2)))
    emax, emean, echan = float(err.max()), float(err.mean()), float(chan.max())
    ratio = lambda e, unit: e / unit if unit > 0 else (0.0 if e == 0 else np.inf)
    rmax, rmean, rchan = ratio(emax, e32max), ratio(emean, e32mean), ratio(echan, e32mean)
    failed = [name for name, ok in (("max", emax <= M * e32max), ("mean", emean <= M * e32mean), ("per-channel mean", echan <= M * e32mean)) if not ok]
    if failed:
        raise AssertionError("%sout of the float64 budget (%s): max error %.3e = %.2f x E32p max (%.3e), mean error %.3e = %.2f x E32p mean (%.3e), "
                             "per-channel mean signed error %.3e = %.2f x E32p mean (channel %d), allowed %g x; %s"
                             % (what and what + ": ", ", ".join(failed), emax, rmax, e32max, emean, rmean, e32mean, echan, rchan, int(np.argmax(chan)), M,
                                _where_conv(int(np.argmax(err)), got.shape, tile)))
    return rmax, rmean, rchan


def half(v):
    """v rounded to binary16 (nearest, ties to even) and back, as float64."""
    with np.errstate(over="ignore"):
        return _f64(v).astype(np.float16).astype(np.float64)


def ulp16(v):
    """The spacing of binary16 at a float64 value: 2^(floor(log2 |v|) - 10) for |v| >= 2^-14, 2^-24 below (the subnormals and zero)."""
    a = np.abs(_f64(v))
    e = np.where(a > 0, np.frexp(a)[1] - 1, -14)  # |v| = m 2^(e + 1), m in [0.5, 1): e = floor(log2 |v|), exactly (frexp(0) = (0, 0))
    return np.ldexp(1.0, np.maximum(e, -14) - 10)


def budget_half(got, ref64, pair32, M, what="", tile=None, floor=0.0):
    """Holds `got` [N,H,W,C], read back from a half tensor, to the correctly rounded half of the exact result.  ref64 is the float64 layer on the
    half-rounded inputs and weights (bias and BN parameters fp32), pair32 the pairwise fp32 evaluation of the same values, not rounded to half.
        max over elements of max(|got - ref64| - 0.5 ulp16(ref64), 0) <= M * E32p_max,     E32p_max = max |pair32 - ref64|.
    Two half operands multiply exactly in fp32, so a kernel that accumulates in fp32, runs its epilogue in fp32 and rounds once on store is within half
    an ulp of the exact value everywhere, except where its fp32 error carried the value across a rounding tie: the right side is that error (about 1 % of
    an ulp at unit scale).  Returns (the ratio of the left side to E32p_max, the share of elements that differ from ref64 rounded to half, the largest
    per-channel mean signed error in ulps) for printing.  tile = (TH, TW) in output pixels only serves the failure message."""
    ref64 = _f64(ref64)
    got = np.asarray(got)
    assert got.ndim == 4 and got.shape == ref64.shape == np.asarray(pair32).shape, (got.shape, ref64.shape, np.asarray(pair32).shape)
    e32max = max(float(np.abs(_f64(pair32) - ref64).max()), float(floor))  # (floor: a unit the caller derives where pair32 can be exact, budget_norm)
    bad = ~np.isfinite(got)
    if bad.any():
        raise AssertionError("%s%d of %d values are not finite (never written, or NaN / Inf computed): first at %s"
                             % (what and what + ": ", int(bad.sum()), bad.size, _where_conv(int(np.argmax(bad)), got.shape, tile)))
    ulp = ulp16(ref64)
    diff = _f64(got) - ref64
    over = np.maximum(np.abs(diff) - 0.5 * ulp, 0.0)
    omax = float(over.max())
    ratio = omax / e32max if e32max > 0 else (0.0 if omax == 0 else np.inf)
    mismatch = float(np.mean(_f64(got) != half(ref64)))
    chan = diff / ulp
    chan = np.abs(chan.mean(axis=(0, 1, 2)))
    if not omax <= M * e32max:
        i = int(np.argmax(over))
        raise AssertionError("%sout of the half budget: %.3e beyond half an ulp of the exact value = %.2f x E32p max (%.3e), allowed %g x; got %.9g, exact %.9g "
                             "(ulp %.3e, off by %.3f ulp), %.2f %% of the elements differ from the rounded exact value, per-channel mean signed error %.4f ulp "
                             "(channel %d); %s"
                             % (what and what + ": ", omax, ratio, e32max, M, got.flat[i], ref64.flat[i], ulp.flat[i], diff.flat[i] / ulp.flat[i], 100 * mismatch,
                                float(chan.max()), int(np.argmax(chan)), _where_conv(i, got.shape, tile)))
    return ratio, mismatch, float(chan.max())


# ---------------------------------------------------------------------------------------------------------------- instance norm
# The margin of the InstanceNorm budget tests (budget_norm): the project's own margin for the ESPCN kernels (M) and the fp16 convolutions (M_F16).
M_NORM = 8


def _plane_stats64(x):
    """(mean, population variance) per (image, channel) of x [N,H,W,C] in float64, each [N,1,1,C]."""
    x = _f64(x)
    mean = x.mean(axis=(1, 2), keepdims=True)
    return mean, ((x - mean) ** 2).mean(axis=(1, 2), keepdims=True)


def instancenorm(x, beta, gamma, eps=1e-5, act="", alpha=0.0, mean_shift=0.0, var_scale=1.0):
    """InstanceNorm in float64: per (n, c) the mean and the population variance over H*W, y = act((x - mean) gamma / sqrt(var + eps) + beta); eps and
    alpha are the plan's fp32 constants.  mean_shift (in units of sqrt(var + eps)) and var_scale (on var + eps) build the mutants of tests/test_ref64.py."""
    x = _f64(x)
    mean, var = _plane_stats64(x)
    ve = (var + float(np.float32(eps))) * var_scale
    y = (x - (mean + mean_shift * np.sqrt(ve))) * (_f64(gamma) / np.sqrt(ve)) + _f64(beta)
    return activation(act, y, alpha)


def _pairwise_sum32(a):
    """fp32 sum over axis 0 by a tree of fp32 additions (neighbours added level by level, an odd one out carried up unchanged)."""
    p = np.asarray(a, np.float32)
    while p.shape[0] > 1:
        q = p[0:p.shape[0] - 1:2] + p[1::2]
        p = np.concatenate([q, p[-1:]]) if p.shape[0] & 1 else q
    assert p.dtype == np.float32
    return p[0]


def instancenorm32(x, beta, gamma, eps=1e-5, act="", alpha=0.0):
    """A float32 NumPy model of the contract, evaluated the straightforward way (no pivot, two passes): the mean a pairwise fp32 sum, the variance a
    pairwise fp32 sum of (x - mean)^2, mul = gamma / sqrtf(var + eps), shift = beta - mean * mul, y = fma(x, mul, shift) (formed in float64 and
    rounded once).  A model of a correct fp32 implementation, not of the kernel: its distance from instancenorm() is the unit E of budget_norm."""
    f = np.float32
    x = np.asarray(x, f)
    n, h, w, c = x.shape
    xs = np.ascontiguousarray(x.reshape(n, h * w, c).transpose(1, 0, 2))  # [HW, N, C]
    hw = f(h * w)
    mean = _pairwise_sum32(xs) / hw
    dv = xs - mean
    var = _pairwise_sum32(dv * dv) / hw
    mul = np.asarray(gamma, f) / np.sqrt(var + f(eps))
    shift = np.asarray(beta, f) - mean * mul
    assert mean.dtype == var.dtype == mul.dtype == shift.dtype == f
    y = (xs.astype(np.float64) * mul.astype(np.float64) + shift.astype(np.float64)).astype(f)
    y = activation32(act, y, alpha)
    assert y.dtype == f
    return np.ascontiguousarray(y.transpose(1, 0, 2)).reshape(n, h, w, c)


def norm_floor(x, beta, gamma, eps=1e-5):
    """[N, C]: one fp32 ulp of |mean * mul| + |beta|, the rounding of shift = beta - mean * mul that the one-FMA form cannot avoid (and what keeps a
    constant plane, on which the model's own error is 0, from a budget of zero)."""
    mean, var = _plane_stats64(x)
    mul = _f64(gamma) / np.sqrt(var + float(np.float32(eps)))
    return np.spacing((np.abs(mean * mul) + np.abs(_f64(beta))).astype(np.float32)).astype(np.float64)[:, 0, 0, :]


def _plane_words(x, n, c, idx, w):
    """What a failure says of the plane: where the worst pixel is, |mean| / std, and how far x[n, 0, 0, c] is from the mean in standard deviations."""
    txt = "plane (n, c) = (%d, %d), worst pixel (y, x) = (%d, %d)" % (n, c, idx // w, idx % w)
    if x is not None:
        p = _f64(x)[n, :, :, c]
        m, s = float(p.mean()), float(p.std())
        txt += ", |mean|/std = %s, x[n,0,0,c] is %s std from the mean" % (("%.3g" % (abs(m) / s)) if s > 0 else "inf (std = 0)",
                                                                       ("%.3g" % (abs(p[0, 0] - m) / s)) if s > 0 else "0 (std = 0)")
    return txt


def budget_norm(got, ref64, model32, M, floor, what="", x=None, half_out=False):
    """Holds an InstanceNorm result `got` [N,H,W,C] to the float64 reference plane by plane.  Per (image, channel) plane
        E = max(max over the plane |model32 - ref64|, floor[n, c]),     floor = norm_floor(...),
    and both the max and the mean of |got - ref64| over the plane must be <= M * E.  half_out: `got` was read back from a half tensor and ref64 is the
    float64 result on the half-rounded input; the allowance is half a binary16 ulp of the exact value plus M * E (budget_half, per plane).
    x (the norm's input) only serves the failure message.  Returns the largest ratio reached over the planes (error, or in half the excess over half
    an ulp, in units of E)."""
    ref64 = _f64(ref64)
    got = np.asarray(got)
    model32 = np.asarray(model32)
    assert got.ndim == 4 and got.shape == ref64.shape == model32.shape, (got.shape, ref64.shape, model32.shape)
    n_, h, w, c_ = got.shape
    floor = _f64(floor)
    assert floor.shape == (n_, c_), (floor.shape, got.shape)
    pre = what and what + ": "
    bad = ~np.isfinite(got)
    if bad.any():
        n, y, xx, c = (int(v) for v in np.unravel_index(int(np.argmax(bad)), got.shape))
        raise AssertionError("%s%d of %d values are not finite (never written, or NaN / Inf computed): first at (n, y, x, c) = (%d, %d, %d, %d)"
                             % (pre, int(bad.sum()), bad.size, n, y, xx, c))
    err = np.abs(_f64(got) - ref64)
    e = np.maximum(np.abs(_f64(model32) - ref64).max(axis=(1, 2)), floor)  # [N, C]
    worst, failed = 0.0, []  # every plane is measured; a failure reports the plane with the largest ratio and how many planes are out
    for n in range(n_):
        for c in range(c_):
            pe = err[n, :, :, c]
            if half_out:
                sl = (slice(n, n + 1), slice(None), slice(None), slice(c, c + 1))
                try:
                    ratio = budget_half(got[sl], ref64[sl], model32[sl], M, floor=float(floor[n, c]))[0]
                except AssertionError as exc:
                    over = np.maximum(pe - 0.5 * ulp16(ref64[n, :, :, c]), 0.0)
                    ratio = float(over.max()) / e[n, c]
                    failed.append((ratio, "%s; %s" % (exc, _plane_words(x, n, c, int(np.argmax(over)), w))))
            else:
                emax, emean = float(pe.max()), float(pe.mean())
                ratio = emax / e[n, c]
                if not (emax <= M * e[n, c] and emean <= M * e[n, c]):
                    failed.append((ratio, "out of the float64 budget: max error %.3e = %.2f x E (%.3e), mean error %.3e = %.2f x E, allowed %g x; %s"
                                   % (emax, ratio, e[n, c], emean, emean / e[n, c], M, _plane_words(x, n, c, int(np.argmax(pe)), w))))
            worst = max(worst, ratio)
    if failed:
        raise AssertionError("%s%d of %d planes out of the budget, the worst: %s" % (pre, len(failed), n_ * c_, max(failed, key=lambda t: t[0])[1]))
    return worst
