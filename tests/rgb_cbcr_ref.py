"""Float64 NumPy restatement of the RGB -> 4:2:0 CbCr contract of include/snnhip.h (snnhip_rgb_cbcr_plan_create / snnhip_bicubic_taps_rgb420 /
snnhip_rgb_cbcr_coefficients): the original low-resolution RGB frame in, the chroma plane of the r-fold upscaled NV12 frame out.  The matrix
coefficients are the fp32 values the device sees (kr, kb rounded to float32, kg and the two scales formed in double and rounded to float32);
everything else is float64.  The Keys cubic, the quantiser and the comparison rule are tests/resample_ref.py's; the near-tie half-width and cap are
the 8-bit ones of tests/yuv_rgb_ref.py.  values32() evaluates the same expression in float32 (measured_distance)."""
import numpy as np

import colour_ref
import resample_ref
from colour_ref import BT601, BT709  # noqa: F401  (re-exported for the tests)
from resample_ref import CENTRE, LEFT, keys, near_tie, quantise  # noqa: F401  (re-exported for the tests)
from yuv_rgb_ref import EPS as _EPS
from yuv_rgb_ref import FULL, LIMITED, MAX_TIE_FRACTION, RANGES  # noqa: F401

EPS = _EPS[255]  # 1e-3
# the expression's worst case: sixteen fp32 roundings (the luma's three products and two sums, the difference, four products and three sums per
# filter pass ... of values below 256) at half an ulp of 256, 2^-16 = 1.5e-5 each
DISTANCE_BOUND = 2.4e-4
# measured with this file's own float32 path (measured_distance: r = 2, 3, 4, both ranges, both sitings, 12 x 16 and 30 x 40 frames of the recipe): 2.53e-5
MEASURED_DISTANCE = 2.6e-5
LEAD = {CENTRE: 1.0, LEFT: 0.5, "centre": 1.0, "left": 0.5}


def pattern(r):
    """(P, S): the output chroma grid has r / 2 samples per input pixel; the pattern repeats every P outputs over S inputs"""
    g = 2 if r % 2 == 0 else 1
    return r // g, 2 // g


def taps(r, siting):
    """(weights float64 [P][4], base int [P]): output P x' + p reads S x' + s_p, s_p = (2p + lead) / r - 0.5, taps S x' + base[p] - 1 .. + 2."""
    P, _ = pattern(r)
    rows, bases = [], []
    for p in range(P):
        s = (2 * p + LEAD[siting]) / r - 0.5
        b = np.floor(s)
        t = s - b
        rows.append(keys(np.array([1.0 + t, t, 1.0 - t, 2.0 - t])))
        bases.append(int(b))
    return np.stack(rows), np.array(bases, np.int64)


def coefficients(rng=LIMITED, kr=BT601[0], kb=BT601[1]):
    """(Coff, cbs, crs) as the device sees them: float32 values, returned as a float32 array."""
    crange = 224.0 if RANGES[rng] == LIMITED else 255.0
    kr, kb = float(np.float32(kr)), float(np.float32(kb))
    return np.array([128.0, crange / (2.0 * (1.0 - kb) * 255.0), crange / (2.0 * (1.0 - kr) * 255.0)], np.float64).astype(np.float32)


def _resample(a, r, axis, siting, dtype=np.float64):
    """`a` resampled along `axis` from `size` low-resolution samples to r * size / 2 chroma samples, replicate edge; with dtype float32 the weights
    are rounded and the sum runs in float32."""
    size = a.shape[axis]
    assert (r * size) % 2 == 0, (r, size)
    P, S = pattern(r)
    w, base = taps(r, siting)
    w = w.astype(dtype)
    out_n = r * size // 2
    idx_i = np.arange(out_n)
    x, p = idx_i // P, idx_i % P
    shape = [1] * a.ndim
    shape[axis] = out_n
    out = None
    for k in range(4):
        idx = np.clip(S * x + base[p] - 1 + k, 0, size - 1)
        term = np.take(a, idx, axis=axis) * w[p, k].reshape(shape)
        out = term if out is None else out + term
    return out


def _values(rgb, r, siting, rng, kr, kb, dtype):
    kr_, kg_, kb_ = (dtype(v) for v in colour_ref.coefficients(kr, kb))
    coff, cbs, crs = coefficients(rng, kr, kb).astype(dtype)
    x = np.asarray(rgb)[..., :3].astype(dtype)
    ylo = kr_ * x[..., 0] + kg_ * x[..., 1] + kb_ * x[..., 2]
    d = np.stack([x[..., 2] - ylo, x[..., 0] - ylo], axis=-1)  # (dB, dR)
    d = _resample(_resample(d, r, 2, siting, dtype), r, 1, CENTRE, dtype)  # horizontal (sited), then vertical (centred)
    out = coff + np.array([cbs, crs], dtype) * d
    assert out.dtype == dtype
    return out


def values(rgb, r, siting=LEFT, rng=LIMITED, kr=BT601[0], kb=BT601[1]):
    """The values in front of the rounding, float64 [N][rH/2][rW/2][2] (Cb, Cr); rgb uint8 [N][H][W][C], C = 3 or 4 (alpha ignored)."""
    return _values(rgb, r, siting, rng, kr, kb, np.float64)


def values32(rgb, r, siting=LEFT, rng=LIMITED, kr=BT601[0], kb=BT601[1]):
    """The same expression with float32 weights, coefficients and arithmetic (no fused multiply-add)."""
    return _values(rgb, r, siting, rng, kr, kb, np.float32)


def cbcr(rgb, r, siting=LEFT, rng=LIMITED, kr=BT601[0], kb=BT601[1]):
    return quantise(values(rgb, r, siting, rng, kr, kb), 255, 0, np.uint8)


def per_pixel(rgb, rng=LIMITED, kr=BT601[0], kb=BT601[1]):
    """The unfiltered conversion of every pixel, float64 [N][H][W][2]: what r = 2 with centre siting must give."""
    kr_, kg_, kb_ = colour_ref.coefficients(kr, kb)
    coff, cbs, crs = coefficients(rng, kr, kb).astype(np.float64)
    x = np.asarray(rgb)[..., :3].astype(np.float64)
    ylo = kr_ * x[..., 0] + kg_ * x[..., 1] + kb_ * x[..., 2]
    return np.stack([coff + cbs * (x[..., 2] - ylo), coff + crs * (x[..., 0] - ylo)], axis=-1)


def frame(seed, n=1, h=4, w=4, c=3, primaries=False):
    """uint8 [n][h][w][c]: R, G, B uniform in [24, 232) so that the rounding is exercised and not the clamp.  primaries: the whole code range -- half
    the pixels uniform over 0 .. 255, half saturated primaries, every channel within 3 codes of 0 or of 255 (the overshoot of the cubic between them
    leaves [0, 255] in full range; exact primaries would crowd the near-tie cap instead: pure blue is Cb = 255.5 in full range, yellow 0.5).
    Alpha, if any, is uniform over 0 .. 255."""
    g = np.random.default_rng(seed)
    if primaries:
        x = g.integers(0, 256, size=(n, h, w, c))
        sat = g.integers(0, 2, size=(n, h, w, c)) * 252 + g.integers(0, 4, size=(n, h, w, c))
        x = np.where(g.integers(0, 2, size=(n, h, w, 1)) == 1, sat, x)
    else:
        x = g.integers(24, 232, size=(n, h, w, c))
    if c == 4:
        x[..., 3] = g.integers(0, 256, size=(n, h, w))
    return x.astype(np.uint8)


# the kernel's tile in INPUT pixels by r (the plan's describe reports it in output chroma pixels, r / 2 times these: tests/test_frame_rgb_cbcr_gpu.py
# checks that they agree), so that the CPU suite can bound the near ties of exactly the frames the GPU sweep compares
TILE_IN = {2: (8, 256), 3: (8, 256), 4: (4, 256)}
SITINGS = ["centre", "left"]
RANGE_NAMES = ["limited", "full"]


def shapes_for(r, tile_in=None):
    """(N, H, W) of the input frame, the smallest where the kernel can go wrong, from its tile (TH, TW) in input pixels: one pixel; an odd width whose
    RGB8 rows do not start on a dword; one short of a tile, a tile, one past it in both directions (a second block either way); N = 2 on the tile
    seam for the batch stride; three rows of two tiles and a few pixels.  Every extent is even for r = 3 (rH and rW must be)."""
    th, tw = tile_in or TILE_IN[r]
    if r == 3:
        return [(1, 2, 2), (1, 2, 6), (1, th - 2, tw - 2), (1, th, tw), (1, th + 2, tw + 2), (2, th, tw + 2), (1, 4, 2 * tw + 6)]
    return [(1, 1, 1), (1, 2, 3), (1, 5, 7), (1, th - 1, tw - 1), (1, th, tw), (1, th + 1, tw + 1), (2, th, tw + 1), (1, 3, 2 * tw + 5)]


def sweep_cases(r, C, shapes=None, sitings=SITINGS, ranges=RANGE_NAMES):
    """(siting, range, (n, h, w), seed) of one (r, C) sweep: every shape at both sitings and both ranges, each on a frame of its own"""
    for si, siting in enumerate(sitings):
        for ri, rng in enumerate(ranges):
            for k, shape in enumerate(shapes or shapes_for(r)):
                yield siting, rng, shape, 1000 * r + 100 * C + 10 * k + 2 * si + ri


def clamp_fraction(v):
    v = np.asarray(v)
    return float(((v < -0.5) | (v > 255.5)).mean())


def measured_distance(shape=(12, 16)):
    """The largest |float32 - float64| of the value in front of the rounding over r = 2, 3, 4, both ranges and both sitings, on the input recipe."""
    worst = 0.0
    for r in (2, 3, 4):
        x = frame(900 + r, 1, shape[0], shape[1], 3)
        for rng in (LIMITED, FULL):
            for siting in (CENTRE, LEFT):
                d = np.abs(values32(x, r, siting, rng).astype(np.float64) - values(x, r, siting, rng))
                worst = max(worst, float(d.max()))
    return worst


def compare(got, want_values):
    """resample_ref.compare on bytes with the 8-bit near-tie half-width EPS"""
    return resample_ref.compare(got, want_values, 255, 0, EPS)


def compare_all(items):
    """compare() over the (got, want_values) items of one sweep, near ties at most MAX_TIE_FRACTION of the sweep's values taken together."""
    return resample_ref.compare_all(items, compare, MAX_TIE_FRACTION)
