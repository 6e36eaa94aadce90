"""Float64 NumPy restatement of the video-frame -> input-tensor contract of include/snnhip.h (snnhip_yuv_tensor_plan_create /
snnhip_yuv_tensor_planar_plan_create / snnhip_yuv_tensor_taps): the source pixel is yuv_rgb_ref's value at r = 1 in front of
its rounding, clamped to [0, maxval]; the sampling table is the rule in exact rational arithmetic with the weight rounded to float32, as the plan's
own table holds it; the blend and the normalisation are float64.  tensor32() evaluates the same expression in float32 (no fused multiply-add):
measured_distance() over the sweeps' own frames sets the tolerance E = 4 x that distance (the factor covers FMA contraction and a summation order
other than NumPy's).  Planar input goes through planar_ref's (de)interleave.  The sweeps of tests/test_frame_yuv_tensor_gpu.py are defined here, so
that the CPU suite measures exactly the frames the GPU suite compares."""
from fractions import Fraction

import numpy as np

import planar_ref
import yuv_rgb_ref
from yuv_rgb_ref import BT601, BT709, CENTRE, LEFT, LIMITED, FULL  # noqa: F401  (re-exported for the tests)

NEAREST, LINEAR = 0, 1
FILTERS = {NEAREST: NEAREST, LINEAR: LINEAR, "nearest": NEAREST, "linear": LINEAR}
DEPTHS = planar_ref.DEPTHS
DEPTH_IDS = planar_ref.DEPTH_IDS
SITINGS = planar_ref.SITINGS
RANGES = planar_ref.RANGES
EPS = yuv_rgb_ref.EPS  # the family's near-tie half-widths, for the ratio-1 comparison with yuv_rgb's bytes
MAX_TIE_FRACTION = 0.01  # ... of which at most 1 % of a sweep's values may be excluded
# The tolerance per unit of |norm|, by maxval: 4 x the largest fp32-to-float64 distance over the GPU sweeps' frames, measured by
# tests/test_frame_yuv_tensor.py (which prints the distances and holds these figures to them)
MEASURED_DISTANCE = {255: 3.9e-5, 1023: 1.8e-4, 4095: 5.9e-4}
E = {m: 4.0 * d for m, d in MEASURED_DISTANCE.items()}
# flat output pixels per block, by (C, fp16 output): the tile the plan's describe reports (the GPU suite checks that they agree)
TILE = {(3, False): 256, (4, False): 256, (3, True): 512, (4, True): 256}


def taps(n_in, n_out, flt=LINEAR):
    """(a float32 [n_out], index int64 [n_out][2]): u = ((2o + 1) in - out) / (2 out) exactly; linear: i0 = floor(u), a = float32(float64(u - i0)),
    indices i0, i0 + 1 clamped; nearest: floor(((2o + 1) in) / (2 out)) twice, a = 0."""
    a = np.zeros(n_out, np.float32)
    idx = np.zeros((n_out, 2), np.int64)
    for o in range(n_out):
        if FILTERS[flt] == NEAREST:
            idx[o] = ((2 * o + 1) * n_in) // (2 * n_out)
        else:
            u = Fraction((2 * o + 1) * n_in - n_out, 2 * n_out)
            i0 = u.numerator // u.denominator
            a[o] = np.float32(float(u - i0))  # float(Fraction) rounds correctly to double
            idx[o] = min(max(i0, 0), n_in - 1), min(max(i0 + 1, 0), n_in - 1)
    return a, idx


def source(y, cbcr, siting=LEFT, rng=LIMITED, maxval=255, shift=0, kr=BT601[0], kb=BT601[1], dtype=np.float64):
    """[N][H][W][3]: yuv_rgb's value at r = 1 in front of the rounding, clamped to [0, maxval]; y [N][H][W][1], cbcr [N][H/2][W/2][2]."""
    v = yuv_rgb_ref._values(y, cbcr, 1, siting, rng, maxval, shift, kr, kb, dtype)
    out = np.clip(v, dtype(0), dtype(maxval))
    assert out.dtype == dtype
    return out


def _tensor(y, cbcr, OH, OW, C, flt, siting, rng, maxval, shift, kr, kb, means, norms, alpha, dtype):
    v = source(y, cbcr, siting, rng, maxval, shift, kr, kb, dtype)
    n, H, W, _ = v.shape
    ay, iy = taps(H, OH, flt)
    ax, ix = taps(W, OW, flt)
    if FILTERS[flt] == NEAREST:
        s = v[:, iy[:, 0]][:, :, ix[:, 0]]
    else:
        ax_, ay_ = ax.astype(dtype).reshape(1, 1, OW, 1), ay.astype(dtype).reshape(1, OH, 1, 1)
        one = dtype(1)
        rows0, rows1 = v[:, iy[:, 0]], v[:, iy[:, 1]]
        top = rows0[:, :, ix[:, 0]] * (one - ax_) + rows0[:, :, ix[:, 1]] * ax_
        bot = rows1[:, :, ix[:, 0]] * (one - ax_) + rows1[:, :, ix[:, 1]] * ax_
        s = top * (one - ay_) + bot * ay_
    m = np.asarray(means, np.float32)[:3].astype(dtype)
    k = np.asarray(norms, np.float32)[:3].astype(dtype)
    t = (s - m) * k
    assert t.dtype == dtype
    if C == 4:
        t = np.concatenate([t, np.full(t.shape[:3] + (1,), np.float32(alpha), dtype)], axis=-1)
    return t


def tensor(y, cbcr, OH, OW, C=3, flt=LINEAR, siting=LEFT, rng=LIMITED, maxval=255, shift=0, kr=BT601[0], kb=BT601[1], means=(0, 0, 0), norms=(1, 1, 1), alpha=1.0):
    """The output tensor [N][OH][OW][C] in float64 (means, norms, alpha and the table's weights at their float32 values)."""
    return _tensor(y, cbcr, OH, OW, C, flt, siting, rng, maxval, shift, kr, kb, means, norms, alpha, np.float64)


def tensor32(y, cbcr, OH, OW, C=3, flt=LINEAR, siting=LEFT, rng=LIMITED, maxval=255, shift=0, kr=BT601[0], kb=BT601[1], means=(0, 0, 0), norms=(1, 1, 1), alpha=1.0):
    """The same expression in float32 throughout: what sets E."""
    return _tensor(y, cbcr, OH, OW, C, flt, siting, rng, maxval, shift, kr, kb, means, norms, alpha, np.float32)


def brute(y, cbcr, OH, OW, flt, siting, rng, maxval, shift, kr, kb, means, norms):
    """The contract pixel by pixel in Python floats (float64), from the tap table of the 4:2:0 filter and the matrix: for small frames only."""
    y, cbcr = np.asarray(y), np.asarray(cbcr)
    n, H, W, _ = y.shape
    ch, cw = H // 2, W // 2
    yoff, coff, cy, crv, cbu, cgv, cgu = (float(c) for c in yuv_rgb_ref.coefficients(maxval, rng, kr, kb))
    wh, bh = yuv_rgb_ref.taps(1, siting)
    wv, bv = yuv_rgb_ref.taps(1, CENTRE)

    def px(i, Y, X):
        c = [0.0, 0.0]
        for comp in range(2):
            acc = 0.0
            for kv in range(4):
                row = min(max(Y // 2 + int(bv[Y % 2]) - 1 + kv, 0), ch - 1)
                h = 0.0
                for kh in range(4):
                    col = min(max(X // 2 + int(bh[X % 2]) - 1 + kh, 0), cw - 1)
                    h += float(wh[X % 2][kh]) * ((int(cbcr[i, row, col, comp]) >> shift) - coff)
                acc += float(wv[Y % 2][kv]) * h
            c[comp] = acc
        yl = cy * ((int(y[i, Y, X, 0]) >> shift) - yoff)
        return [min(max(e, 0.0), float(maxval)) for e in (yl + crv * c[1], yl - (cgv * c[1] + cgu * c[0]), yl + cbu * c[0])]

    ay, iy = taps(H, OH, flt)
    ax, ix = taps(W, OW, flt)
    out = np.zeros((n, OH, OW, 3))
    for i in range(n):
        for oy in range(OH):
            for ox in range(OW):
                p = [[px(i, int(iy[oy][a]), int(ix[ox][b])) for b in range(2)] for a in range(2)]
                fx, fy = float(ax[ox]), float(ay[oy])
                for c in range(3):
                    top = p[0][0][c] * (1.0 - fx) + p[0][1][c] * fx
                    bot = p[1][0][c] * (1.0 - fx) + p[1][1][c] * fx
                    out[i, oy, ox, c] = (top * (1.0 - fy) + bot * fy - float(np.float32(means[c]))) * float(np.float32(norms[c]))
    return out


def frame(n, h, w, maxval, shift, dtype, seed, whole_range=False):
    """(y [n][h][w][1], cbcr [n][h/2][w/2][2]) of yuv_rgb_ref's input recipe; h, w: the LUMA plane (even)."""
    assert h % 2 == 0 and w % 2 == 0
    return yuv_rgb_ref.frame(n, h // 2, w // 2, 1, maxval, shift, dtype, seed, whole_range=whole_range)


def half_ulp16(v):
    """half an fp16 ulp at magnitude |v| (subnormals: 2^-25)"""
    v = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    return 0.5 * 2.0 ** (np.floor(np.log2(v)) - 10)


def tolerance(want, norms, maxval, half):
    """|norms[c]| E(bits), plus half an fp16 ulp (at the far end of the fp32 allowance) for fp16 output; the alpha channel is exact up to its fp16
    rounding."""
    want = np.asarray(want, np.float64)
    k = np.abs(np.asarray(norms, np.float32)[:3].astype(np.float64))
    tol = np.zeros(want.shape)
    tol[..., :3] = k * E[maxval]
    if half:
        tol = tol + half_ulp16(np.abs(want) + tol)
    return tol


def compare(got, want, norms, maxval, half):
    """Every output element within the tolerance, nothing left out.  Returns the largest |got - want| / tolerance of the colour channels."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), "%d output values were not written (or are not finite)" % int((~np.isfinite(got)).sum())
    tol = tolerance(want, norms, maxval, half)
    err = np.abs(got - want)
    bad = err > tol
    assert not bad.any(), "%d values are outside the tolerance, first at %s: got %r, reference %r, allowed %g" % (
        int(bad.sum()), tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0], tol[bad][0])
    return float((err[..., :3] / tol[..., :3]).max()) if err.size else 0.0


# ---- the sweeps of tests/test_frame_yuv_tensor_gpu.py

def shapes(C, half):
    """(n, h, w, oh, ow), luma extents: one chroma sample to 1 x 1, 2 x 2 and (enlarging) 5 rows x 3 columns; 64 x 48 to 7 x 5 (a ratio above 8); ratio 1
    at 6 x 8; from the tile T (flat output pixels of a block): exactly one tile, one pixel more (a second block of one pixel; for fp16 RGB a lone
    6-byte tail), and N = 2 of 9 rows of T / 8 + 1 columns: an odd width and an odd pixel count per image, a block seam inside a row, and for fp16
    RGB rows and the second image starting 2 bytes off a dword."""
    T = TILE[(C, half)]
    return [(1, 2, 2, 1, 1), (1, 2, 2, 2, 2), (1, 2, 2, 5, 3), (1, 48, 64, 5, 7), (1, 6, 8, 6, 8), (1, 8, 8, 16, T // 16), (1, 4, 6, 1, T + 1), (2, 10, 12, 9, T // 8 + 1)]


def normalisation(k, maxval):
    """(means, norms) of case k: the identity, an ImageNet-like one scaled to the depth, one with a negative and a large factor"""
    s = (maxval + 1) / 256.0
    return [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((123.675 * s, 116.28 * s, 103.53 * s), (1 / (58.395 * s), 1 / (57.12 * s), 1 / (57.375 * s))),
            ((127.5 * s, 0.0, 64.0 * s), (-1 / (127.5 * s), 2.0, 1 / (255.0 * s)))][k % 3]


def sweep_cases(C, half, container, maxval, shift):
    """(shape, filter, siting, range, (kr, kb), whole_range, means, norms, seed) of one sweep: both filters, sitings and ranges on every shape, the
    matrix, the input recipe (whole-range frames exercise the clamp) and the normalisation alternating."""
    for fi, flt in enumerate(("linear", "nearest")):
        for si, siting in enumerate(SITINGS):
            for ri, rng in enumerate(RANGES):
                for k, shape in enumerate(shapes(C, half)):
                    means, norms = normalisation(k + si + ri, maxval)
                    yield shape, flt, siting, rng, (BT709 if (k + si) % 2 else BT601), (k + ri + fi) % 2 == 1, means, norms, 100 * k + 10 * si + 2 * ri + fi + maxval + shift


ALPHA = 0.75


def case_frames(case, container, maxval, shift):
    (n, h, w, oh, ow), flt, siting, rng, matrix, whole, means, norms, seed = case
    return frame(n, h, w, maxval, shift, planar_ref.np_dtype(container), seed, whole_range=whole)


def case_tensor(case, y, cbcr, C, maxval, shift, fn=tensor):
    (n, h, w, oh, ow), flt, siting, rng, (kr, kb), whole, means, norms, seed = case
    return fn(y, cbcr, oh, ow, C, flt, siting, rng, maxval, shift, kr, kb, means, norms, ALPHA)


def measured_distance(container, maxval, shift):
    """The largest |float32 - float64| / |norm| of a colour value over the GPU sweeps' frames of one depth (C = 3 and 4 and both output types share
    the colour values; their shapes differ by the tile)."""
    worst = 0.0
    for C, half in ((3, False), (3, True)):
        for case in sweep_cases(C, half, container, maxval, shift):
            y, cbcr = case_frames(case, container, maxval, shift)
            k = np.abs(np.asarray(case[7], np.float32).astype(np.float64))
            d = np.abs(case_tensor(case, y, cbcr, 3, maxval, shift, tensor32).astype(np.float64) - case_tensor(case, y, cbcr, 3, maxval, shift)) / k
            worst = max(worst, float(d.max()))
    return worst


# ---- ratio 1 against yuv_rgb's own bytes (tests/test_frame_yuv_tensor.py bounds the near ties of exactly these frames)

RATIO1_SHAPES = [(1, 6, 8), (2, 10, 12), (1, 34, 66)]  # (n, h, w), luma


def ratio1_frame(n, h, w, maxval, shift, dtype, seed):
    """yuv_rgb_ref's recipe where its near ties fit under MAX_TIE_FRACTION (8 and 10 bits: 2 eps is 0.2 % and 0.6 % of uniformly spread fractions).
    At 12 bits 2 eps is 1.6 %: there luma is drawn over the whole range and chroma from the outer quarters of its range, which puts about 40 % of the
    values on the clamp (never a tie) and leaves the other 60 % to be compared."""
    if 2 * EPS[maxval] <= MAX_TIE_FRACTION:
        return frame(n, h, w, maxval, shift, dtype, seed)
    k = (maxval + 1) // 256
    g = np.random.default_rng(seed)
    y = g.integers(0, maxval + 1, size=(n, h, w, 1))
    c = g.integers(0, 64 * k, size=(n, h // 2, w // 2, 2))
    c = np.where(g.integers(0, 2, size=c.shape).astype(bool), maxval - c, c)
    return (y << shift).astype(dtype), (c << shift).astype(dtype)


def ratio1_cases(container, maxval, shift):
    """(y, cbcr, siting, range) of the ratio-1 comparison: every shape, siting and range"""
    for k, (n, h, w) in enumerate(RATIO1_SHAPES):
        for si, siting in enumerate(SITINGS):
            for ri, rng in enumerate(RANGES):
                y, cbcr = ratio1_frame(n, h, w, maxval, shift, planar_ref.np_dtype(container), seed=500 + 10 * k + 2 * si + ri + maxval)
                yield y, cbcr, siting, rng


def compare_ratio1(items, maxval):
    """items: (rint of the tensor at ratio 1 with means 0 and norms 1, yuv_rgb's values >> shift, the float64 source values).  Equal wherever the
    source value is farther than EPS[maxval] from a rounding tie, at most 1 apart on the near ties, which are at most MAX_TIE_FRACTION of all values.
    Returns (near-tie fraction, values that differ)."""
    ties = total = ndiff = 0
    for got, fixed, values in items:
        tie = yuv_rgb_ref.near_tie(values, EPS[maxval])
        diff = np.asarray(got, np.int64) - np.asarray(fixed, np.int64)
        assert not ((diff != 0) & ~tie).any(), "%d values differ off the near ties" % int(((diff != 0) & ~tie).sum())
        assert np.abs(diff).max(initial=0) <= 1
        ties, total, ndiff = ties + int(tie.sum()), total + tie.size, ndiff + int((diff != 0).sum())
    assert ties <= MAX_TIE_FRACTION * total, "near ties are %d of %d values" % (ties, total)
    return ties / max(total, 1), ndiff
