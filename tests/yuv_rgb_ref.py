"""Float64 NumPy restatement of the NV12 / P010 -> RGB contract of include/snnhip.h (snnhip_yuv_rgb_plan_create / snnhip_bicubic_taps_420 /
snnhip_yuv_rgb_coefficients): the model's upscaled luma frame and the original half-resolution CbCr plane in, full-range RGB at the output
resolution out.  The five matrix coefficients are the fp32 values the device sees (computed in double from the float32 kr, kb, rounded to float32);
everything else is float64.  The filter, the quantiser and the comparison rule are tests/resample_ref.py's.  values32() evaluates the same
expression in float32 and sets the comparison rule's eps (measured_distance)."""
import numpy as np

import resample_ref
from colour_ref import BT601, BT709  # noqa: F401  (re-exported for the tests)
from resample_ref import CENTRE, LEFT, SITING_OFFSET, keys, near_tie, quantise  # noqa: F401  (re-exported for the tests)

LIMITED, FULL = 0, 1
RANGES = {LIMITED: LIMITED, FULL: FULL, "limited": LIMITED, "full": FULL}
# near-tie half-width by bit depth.  Measured with this file's own float32 path (measured_distance: r = 1..4, both ranges, both sitings, the input
# recipe below, 12 x 16 chroma planes): the largest fp32-to-float64 distance of the value in front of the rounding is
#     2.5e-5 at 8 bits, 1.0e-4 at 10 bits, 3.6e-4 at 12 bits   (30 x 40 planes: 2.9e-5 / 1.1e-4 / 5.2e-4)
# -- smaller than an evaluation that filters the samples themselves (9.6e-5 / 4.0e-4 / 1.7e-3), because what is filtered is sample - Coff.  eps stays
# at the values chosen against the larger figures: 34, 26 and 15 times the distance (tests/test_frame_yuv_rgb.py re-measures and holds eps to at least
# 4 times it).  At eps = 8e-3 the 12-bit near-tie share of the recipe is 1.4 - 1.8 %, under the 3 % cap.
MEASURED_DISTANCE = {255: 2.9e-5, 1023: 1.1e-4, 4095: 5.2e-4}
EPS = {255: 1e-3, 1023: 3e-3, 4095: 8e-3}
MAX_TIE_FRACTION = 0.03
MAX_CLAMP_FRACTION = 0.02


def taps(r, siting):
    """(weights float64 [2r][4], base int [2r]) of a chroma plane resampled 2r-fold straight to the output luma grid: lead = 0.5, off by siting."""
    return resample_ref.taps(2 * r, 0.5, SITING_OFFSET[siting])


def coefficients(maxval=255, rng=LIMITED, kr=BT601[0], kb=BT601[1]):
    """(Yoff, Coff, cy, crv, cbu, cgv, cgu) as the device sees them: float32 values, returned as a float32 array."""
    k = (maxval + 1) / 256.0
    m = float(maxval)
    limited = RANGES[rng] == LIMITED
    yoff, yrange, crange = (16.0 * k, 219.0 * k, 224.0 * k) if limited else (0.0, m, m)
    kr, kb = float(np.float32(kr)), float(np.float32(kb))
    kg = 1.0 - kr - kb
    crv = 2.0 * (1.0 - kr) * m / crange
    cbu = 2.0 * (1.0 - kb) * m / crange
    return np.array([yoff, 128.0 * k, m / yrange, crv, cbu, kr * crv / kg, kb * cbu / kg], np.float64).astype(np.float32)


def _resample(a, r, axis, siting, dtype=np.float64):
    """`a` resampled 2r-fold along `axis` to the output luma grid; with dtype float32 the weights are rounded and the sum runs in float32."""
    return resample_ref._resample(a, 2 * r, axis, 0.5, SITING_OFFSET[siting], dtype)


def _values(yhi, cbcr, r, siting, rng, maxval, shift, kr, kb, dtype):
    c = coefficients(maxval, rng, kr, kb).astype(dtype)
    yoff, coff, cy, crv, cbu, cgv, cgu = c
    y = (np.asarray(yhi).astype(np.int64) >> shift).astype(dtype)[..., 0]
    ch = (np.asarray(cbcr).astype(np.int64) >> shift).astype(dtype) - coff  # exact: integers minus a multiple of (maxval + 1) / 256
    ch = _resample(_resample(ch, r, 2, siting, dtype), r, 1, CENTRE, dtype)  # horizontal (sited), then vertical (centred)
    assert ch.shape[:3] == y.shape, (ch.shape, y.shape)
    cb, cr = ch[..., 0], ch[..., 1]
    yl = cy * (y - yoff)
    out = np.stack([yl + crv * cr, yl - (cgv * cr + cgu * cb), yl + cbu * cb], axis=-1)
    assert out.dtype == dtype
    return out


def values(yhi, cbcr, r, siting=LEFT, rng=LIMITED, maxval=255, shift=0, kr=BT601[0], kb=BT601[1]):
    """The values in front of the rounding, float64 [N][2rH][2rW][3] (R, G, B); yhi [N][2rH][2rW][1], cbcr [N][H][W][2], uint8 / uint16."""
    return _values(yhi, cbcr, r, siting, rng, maxval, shift, kr, kb, np.float64)


def values32(yhi, cbcr, r, siting=LEFT, rng=LIMITED, maxval=255, shift=0, kr=BT601[0], kb=BT601[1]):
    """The same expression with float32 weights, coefficients and arithmetic (no fused multiply-add): what sets eps."""
    return _values(yhi, cbcr, r, siting, rng, maxval, shift, kr, kb, np.float32)


def rgb(yhi, cbcr, r, C=3, siting=LEFT, rng=LIMITED, maxval=255, shift=0, kr=BT601[0], kb=BT601[1]):
    """The output frame [N][2rH][2rW][C]; C = 4 adds A = maxval << shift."""
    yhi = np.asarray(yhi)
    out = quantise(values(yhi, cbcr, r, siting, rng, maxval, shift, kr, kb), maxval, shift, yhi.dtype)
    if C == 4:
        out = np.concatenate([out, np.full(out.shape[:3] + (1,), maxval << shift, yhi.dtype)], axis=-1)
    return out


def frame(n, h, w, r, maxval, shift, dtype, seed, whole_range=False):
    """(yhi [n][2rh][2rw][1], cbcr [n][h][w][2]) of the input recipe: Y uniform in [40k, 200k), chroma uniform in [96k, 160k), k = (maxval + 1) / 256,
    so that the rounding is exercised and not the clamp; whole_range draws both over 0 .. maxval (the clamp sweep).  h, w: the CHROMA plane."""
    k = (maxval + 1) // 256
    g = np.random.default_rng(seed)
    ylo, yhi_, clo, chi = (0, maxval + 1, 0, maxval + 1) if whole_range else (40 * k, 200 * k, 96 * k, 160 * k)
    y = g.integers(ylo, yhi_, size=(n, 2 * r * h, 2 * r * w, 1))
    c = g.integers(clo, chi, size=(n, h, w, 2))
    return (y << shift).astype(dtype), (c << shift).astype(dtype)


def clamp_fraction(v, maxval):
    v = np.asarray(v)
    return float(((v < -0.5) | (v > maxval + 0.5)).mean())


def measured_distance(maxval, shift=0, dtype=None, shape=(12, 16)):
    """The largest |float32 - float64| of the value in front of the rounding over r = 1..4, both ranges and both sitings, on the input recipe."""
    dtype = dtype or (np.uint8 if maxval == 255 else np.uint16)
    worst = 0.0
    for r in (1, 2, 3, 4):
        yhi, cbcr = frame(1, shape[0], shape[1], r, maxval, shift, dtype, seed=900 + r)
        for rng in (LIMITED, FULL):
            for siting in (CENTRE, LEFT):
                d = np.abs(values32(yhi, cbcr, r, siting, rng, maxval, shift).astype(np.float64) - values(yhi, cbcr, r, siting, rng, maxval, shift))
                worst = max(worst, float(d.max()))
    return worst


def compare(got, want_values, maxval, shift):
    """resample_ref.compare on the R, G, B channels with this contract's near-tie half-width EPS[maxval]; alpha, if any, must be maxval << shift."""
    got = np.asarray(got)
    if got.shape[-1] == 4:
        assert (got[..., 3] == (maxval << shift)).all(), "alpha is not maxval << shift everywhere"
        got = got[..., :3]
    return resample_ref.compare(got, want_values, maxval, shift, EPS[maxval])


def compare_all(items):
    """compare() over the (got, want_values, maxval, shift) items of one sweep, near ties at most MAX_TIE_FRACTION of the sweep's values."""
    return resample_ref.compare_all(items, compare, MAX_TIE_FRACTION)
