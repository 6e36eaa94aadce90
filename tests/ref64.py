"""A plain float64 restatement of the ESPCN-shaped nets, NumPy only and independent of oracle/snn_oracle.c, and the error budget that holds the
fused kernels to fp32 accuracy.

The fp32 C oracle is itself 2e-7 to 5e-7 (max) and about 3e-8 (mean) away from the exact result: those two numbers, measured on the very input of a
test (E32max, E32mean), are the unit in which a kernel's own distance from the exact result is expressed.  A kernel that computes in fp32 lands within
a small multiple M of them; one that lost mantissa bits somewhere (a TF32 or split-f16 product, a truncated weight, a bias off by 2e-6) does not,
although all of these pass rtol = atol = 1e-4 against the oracle."""
import numpy as np

# The margin of every budget test: twice the largest ratio any fp32 kernel family showed against float64 on an MI355X (2.02, DESIGN.md section 3
# has the table), rounded up to a power of two.  It is also the largest at which the 2e-6 bias mutant of tests/test_ref64.py (9.7 x E32mean) is rejected.
M = 8

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
    raise ValueError("ref64: unknown activation %r" % (name,))


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
