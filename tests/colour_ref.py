"""Float64 NumPy restatement of the colour-frame contract of include/snnhip.h (snnhip_rgb_luma_plan_create / snnhip_ycc_merge_plan_create): the luma
split in front of a luma-only model and the bicubic chroma merge behind it.  The coefficients are the fp32 values the device sees (kr, kb rounded to
float32, kg = 1 - kr - kb formed in double and rounded to float32); everything else is float64."""
import numpy as np

import resample_ref
from resample_ref import keys, near_tie  # noqa: F401  (re-exported for the tests)
from resample_ref import quantise as _quantise

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
    return _quantise(v, 255, 0, np.uint8)


def luma(rgb, kr=BT601[0], kb=BT601[1]):
    return quantise(luma_values(rgb, kr, kb))


def taps(r):
    """The [r][4] float64 weight table of an r-fold upscale with aligned pixel centres: row p = the phase of output sample X = r*x + p."""
    return resample_ref.taps(r, 0.5, 0.5)[0]


def _resample(a, r, axis):
    """`a` resampled r-fold along `axis`: aligned pixel centres, taps i0 - 1 .. i0 + 2 with replicate edge, Keys weights."""
    return resample_ref._resample(a, r, axis, 0.5, 0.5)


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


def compare(got, want_values, max_tie_fraction=0.01, eps=1e-3):
    """The comparison rule (resample_ref.compare on bytes): bytes equal the reference's wherever its pre-rounding value is no near tie, and differ by
    at most 1 on near ties; near ties are at most `max_tie_fraction` of the compared values (asserted on the reference alone; None: the caller pools
    several inputs and asserts it itself, see compare_all).  Returns (near ties, values compared, bytes that differ)."""
    ties, total, ndiff = resample_ref.compare(got, want_values, 255, 0, eps)
    if max_tie_fraction is not None:
        assert ties / total <= max_tie_fraction, "near ties are %.3f %% of the reference values" % (100 * ties / total)
    return ties, total, ndiff


def compare_all(pairs, max_tie_fraction=0.01):
    """compare() over the (got, want_values) pairs of one sweep; the near-tie bound holds for the sweep's inputs taken together.  Returns (near-tie
    fraction, bytes that differ)."""
    return resample_ref.compare_all(pairs, lambda got, want_values: compare(got, want_values, None), max_tie_fraction)
