"""Float64 NumPy restatement of the colour-frame contract of include/snnhip.h (snnhip_rgb_luma_plan_create / snnhip_ycc_merge_plan_create): the luma
split in front of a luma-only model and the bicubic chroma merge behind it.  The coefficients are the fp32 values the device sees (kr, kb rounded to
float32, kg = 1 - kr - kb formed in double and rounded to float32); everything else is float64."""
import numpy as np

BT601 = (0.299, 0.114)
BT709 = (0.2126, 0.0722)


def coefficients(kr, kb):
    kr32, kb32 = np.float32(kr), np.float32(kb)
    kg32 = np.float32(1.0 - float(kr32) - float(kb32))
    return float(kr32), float(kg32), float(kb32)


def luma_values(rgb, kr=BT601[0], kb=BT601[1]):
    """ylo = kr*R + kg*G + kb*B in float64, unquantised; rgb is uint8 [..., C] with C = 3 or 4; the result keeps a last axis of 1."""
    k = coefficients(kr, kb)
    x = np.asarray(rgb)[..., :3].astype(np.float64)
    return (k[0] * x[..., 0] + k[1] * x[..., 1] + k[2] * x[..., 2])[..., None]


def quantise(v):
    return np.clip(np.rint(v), 0.0, 255.0).astype(np.uint8)  # np.rint: ties to even


def luma(rgb, kr=BT601[0], kb=BT601[1]):
    return quantise(luma_values(rgb, kr, kb))


def keys(d):
    """Keys cubic, a = -0.5 (Catmull-Rom), at distance d >= 0; the products are written out so that any IEEE double arithmetic gives the same bits."""
    d = np.asarray(d, np.float64)
    a = -0.5
    near = (a + 2.0) * (d * d * d) - (a + 3.0) * (d * d) + 1.0
    far = a * (d * d * d) - 5.0 * a * (d * d) + 8.0 * a * d - 4.0 * a
    return np.where(d <= 1.0, near, np.where(d < 2.0, far, 0.0))


def taps(r):
    """The [r][4] float64 weight table of an r-fold upscale: row p = the phase of output sample X = r*x + p."""
    rows = []
    for p in range(r):
        sx = (p + 0.5) / r - 0.5
        t = sx - np.floor(sx)
        rows.append(keys(np.array([1.0 + t, t, 1.0 - t, 2.0 - t])))
    return np.stack(rows)


def _resample(a, r, axis):
    """`a` resampled r-fold along `axis`: aligned pixel centres, taps i0 - 1 .. i0 + 2 with replicate edge, Keys weights."""
    size = a.shape[axis]
    X = np.arange(r * size, dtype=np.float64)
    sx = (X + 0.5) / r - 0.5
    i0 = np.floor(sx)
    t = sx - i0
    w = np.stack([keys(1.0 + t), keys(t), keys(1.0 - t), keys(2.0 - t)])  # [4][r*size]
    out = 0.0
    shape = [1] * a.ndim
    shape[axis] = r * size
    for k in range(4):
        idx = np.clip(i0.astype(np.int64) - 1 + k, 0, size - 1)
        out = out + np.take(a, idx, axis=axis) * w[k].reshape(shape)
    return out


def merge_values(yhi, rgb, r, kr=BT601[0], kb=BT601[1]):
    """The values in front of the rounding, float64 [N][r*H][r*W][3] (R', G', B'); yhi uint8 [N][r*H][r*W][1], rgb uint8 [N][H][W][C]."""
    k = coefficients(kr, kb)
    rgb = np.asarray(rgb)
    ylo = luma_values(rgb, kr, kb)[..., 0]
    d_r = rgb[..., 0].astype(np.float64) - ylo
    d_b = rgb[..., 2].astype(np.float64) - ylo
    d_r = _resample(_resample(d_r, r, 2), r, 1)  # horizontal, then vertical
    d_b = _resample(_resample(d_b, r, 2), r, 1)
    y = np.asarray(yhi)[..., 0].astype(np.float64)
    assert y.shape == d_r.shape, (y.shape, d_r.shape)
    return np.stack([y + d_r, y - (k[0] * d_r + k[2] * d_b) / k[1], y + d_b], axis=-1)


def merge(yhi, rgb, r, kr=BT601[0], kb=BT601[1]):
    """The output frame, uint8 [N][r*H][r*W][C]; for C = 4 the alpha of low-resolution pixel (Y // r, X // r)."""
    rgb = np.asarray(rgb)
    out = quantise(merge_values(yhi, rgb, r, kr, kb))
    if rgb.shape[-1] == 4:
        alpha = np.repeat(np.repeat(rgb[..., 3:4], r, axis=1), r, axis=2)
        out = np.concatenate([out, alpha], axis=-1)
    return out


def near_tie(v, eps=1e-3):
    v = np.asarray(v, np.float64)
    return np.abs(v - np.floor(v) - 0.5) < eps


def compare(got, want_values, max_tie_fraction=0.01, eps=1e-3):
    """The comparison rule: bytes equal the reference's wherever its pre-rounding value is no near tie, and differ by at most 1 on near ties; near ties
    are at most `max_tie_fraction` of the compared values (asserted on the reference alone; None: the caller pools several inputs and asserts it
    itself, see compare_all).  Returns (near ties, values compared, bytes that differ)."""
    want = quantise(want_values)
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    tie = near_tie(want_values, eps)
    if max_tie_fraction is not None:
        assert tie.mean() <= max_tie_fraction, "near ties are %.3f %% of the reference values" % (100 * tie.mean())
    diff = got.astype(np.int32) - want.astype(np.int32)
    bad = (diff != 0) & ~tie
    assert not bad.any(), "%d bytes differ off the near ties, first at %s: got %s, reference value %s" % (
        int(bad.sum()), tuple(np.argwhere(bad)[0]), got[bad][0], want_values[bad][0])
    assert np.abs(diff).max(initial=0) <= 1, "a near-tie byte differs by %d" % int(np.abs(diff).max())
    return int(tie.sum()), int(tie.size), int((diff != 0).sum())


def compare_all(pairs, max_tie_fraction=0.01):
    """compare() over the (got, want_values) pairs of one sweep; the near-tie bound holds for the sweep's inputs taken together (its smallest frames
    have three values each).  Returns (near-tie fraction, bytes that differ)."""
    ties = total = ndiff = 0
    for got, want_values in pairs:
        t, n, d = compare(got, want_values, None)
        ties, total, ndiff = ties + t, total + n, ndiff + d
    assert ties <= max_tie_fraction * total, "near ties are %d of %d reference values" % (ties, total)
    return ties / max(total, 1), ndiff
