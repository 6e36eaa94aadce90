"""Float64 NumPy restatement of the fitted-RGB contract of include/snnhip.h (snnhip_rgb_fit_plan_create / snnhip_rgb_fit_taps): the luma frame
already at the output size and the original low-resolution chroma source in, packed RGB / RGBA at the output size out.  The source -- a CbCr
plane, two planes, or a colour frame -- is enlarged 1- to 8-fold, each axis with its own ratio, four normalised Keys weights per output
coordinate, the phase in integers, vertical then horizontal.  The cubic, the quantiser and the comparison rule are tests/resample_ref.py's, the
video matrix tests/yuv_rgb_ref.py's (coefficients), the colour matrix tests/colour_ref.py's (coefficients).  dtype=np.float32 evaluates the same
expressions with rounded weights and float32 sums (no fused multiply-add): what sets eps (measured_distance)."""
import numpy as np

import colour_ref
import resample_ref
import yuv_rgb_ref
from colour_ref import BT601, BT709  # noqa: F401  (re-exported for the tests)
from resample_ref import CENTRE, LEFT, keys, near_tie, quantise  # noqa: F401  (re-exported for the tests)
from yuv_rgb_ref import FULL, LIMITED, clamp_fraction  # noqa: F401

# near-tie half-width by bit depth: the family's values (tests/yuv_rgb_ref.py, tests/fit_ref.py), not new numbers.  Measured with this file's own
# float32 path over SHAPES, both ranges and both sitings (measured_distance), the largest fp32-to-float64 distance in front of the rounding is
#     video: 2.7e-5 at 8 bits, 1.2e-4 at 10 bits, 4.6e-4 at 12 bits;   RGB source (whole-range random bytes): 6.3e-5
# (with other seeds of the same recipe: 2.4e-5 / 1.1e-4 / 4.1e-4 and 4.5e-5), so eps is 37 / 25 / 17 and 16 times the distance;
# tests/test_frame_rgb_fit.py re-measures and holds eps to at least 4 times it.  Near ties at that eps: 0.20 / 0.59 / 1.62 % and 0.19 %.
EPS = {255: 1e-3, 1023: 3e-3, 4095: 8e-3}
MAX_TIE_FRACTION = {"video": 0.03, "rgb": 0.01}
MAX_CLAMP_FRACTION = 0.02
TAPS = 4
# (N, H, W, OH, OW), H x W the chroma source: ratio 1, ratio 8, odd sizes, rows that are not dword-aligned, two ratios in one plan, N = 2
SHAPES = [(1, 1, 1, 1, 1), (1, 1, 1, 8, 8), (1, 2, 3, 4, 5), (1, 5, 7, 5, 7), (1, 5, 7, 40, 56), (1, 5, 7, 13, 19), (1, 19, 35, 27, 100), (1, 12, 16, 36, 48),
          (2, 9, 11, 23, 30), (1, 30, 40, 90, 150), (1, 24, 70, 48, 141)]
OFF4 = {CENTRE: 2, LEFT: 1, "centre": 2, "left": 1}  # a = 4 * off


def table(I, O, siting):
    """(weights float64 [O][4], base int64 [O]) of one axis: output X reads in[clip(base[X] - 1 + k)] with weights[X][k]."""
    assert I >= 1 and I <= O <= 8 * I, (I, O)
    a = OFF4[siting]
    D = 4 * O
    w = np.zeros((O, TAPS), np.float64)
    base = np.zeros(O, np.int64)
    for X in range(O):
        Nn = (4 * X + 2) * I - a * O
        b = Nn // D  # floor
        t = (Nn - b * D) / D
        row = [float(keys(abs(float(k - 3) - t))) for k in range(8)]
        total = 0.0
        for v in row:  # ascending tap order
            total += v
        assert row[0] == row[1] == row[6] == row[7] == 0.0, (I, O, X, row)  # enlarging: the outer four are exactly 0
        base[X] = b
        w[X] = [v / total for v in row[2:6]]
    return w, base


def _resample(a, O, axis, siting, dtype=np.float64):
    """`a` enlarged to O samples along `axis`, replicate edge; with dtype float32 the weights are rounded and the sum runs in float32."""
    size = a.shape[axis]
    w, base = table(size, O, siting)
    w = w.astype(np.float32).astype(dtype) if dtype == np.float32 else w
    shape = [1] * a.ndim
    shape[axis] = O
    out = None
    for k in range(TAPS):
        idx = np.clip(base - 1 + k, 0, size - 1)
        term = np.take(a, idx, axis=axis) * w[:, k].reshape(shape)
        out = term if out is None else out + term
    assert out.dtype == dtype
    return out


def _enlarge(a, OH, OW, siting, dtype):
    """[N][H][W][2] -> [N][OH][OW][2]: vertical (aligned centres), then horizontal (sited)."""
    return _resample(_resample(a, OH, 1, CENTRE, dtype), OW, 2, siting, dtype)


def video_values(yfit, cbcr, siting=LEFT, rng=LIMITED, maxval=255, shift=0, kr=BT601[0], kb=BT601[1], dtype=np.float64):
    """The values in front of the rounding, [N][OH][OW][3] (R, G, B); yfit [N][OH][OW][1], cbcr [N][H][W][2], uint8 / uint16."""
    yoff, coff, cy, crv, cbu, cgv, cgu = yuv_rgb_ref.coefficients(maxval, rng, kr, kb).astype(dtype)
    yfit = np.asarray(yfit)
    y = (yfit.astype(np.int64) >> shift).astype(dtype)[..., 0]
    ch = (np.asarray(cbcr).astype(np.int64) >> shift).astype(dtype) - coff  # exact: integers minus a multiple of (maxval + 1) / 256
    ch = _enlarge(ch, yfit.shape[1], yfit.shape[2], siting, dtype)
    cb, cr = ch[..., 0], ch[..., 1]
    yl = cy * (y - yoff)
    out = np.stack([yl + crv * cr, yl - (cgv * cr + cgu * cb), yl + cbu * cb], axis=-1)
    assert out.dtype == dtype
    return out


def rgb_values(yfit, frame, kr=BT601[0], kb=BT601[1], dtype=np.float64):
    """The values in front of the rounding, [N][OH][OW][3] (R', G', B'); yfit uint8 [N][OH][OW][1], frame uint8 [N][H][W][C], C = 3 | 4."""
    k = [dtype(v) for v in colour_ref.coefficients(kr, kb)]  # (kr, kg, kb) as the device sees them
    yfit = np.asarray(yfit)
    x = np.asarray(frame)[..., :3].astype(dtype)
    ylo = k[0] * x[..., 0] + k[1] * x[..., 1] + k[2] * x[..., 2]
    d = np.stack([x[..., 2] - ylo, x[..., 0] - ylo], axis=-1)  # (dB, dR)
    d = _enlarge(d, yfit.shape[1], yfit.shape[2], CENTRE, dtype)
    d_b, d_r = d[..., 0], d[..., 1]
    y = yfit[..., 0].astype(dtype)
    out = np.stack([y + d_r, y - (k[0] * d_r + k[2] * d_b) / k[1], y + d_b], axis=-1)
    assert out.dtype == dtype
    return out


def alpha_of(frame, OH, OW):
    """The alpha plane of the output, [N][OH][OW][1]: source pixel ((2Y + 1) H // (2 OH), (2X + 1) W // (2 OW))."""
    frame = np.asarray(frame)
    _, H, W, _ = frame.shape
    sy = (2 * np.arange(OH) + 1) * H // (2 * OH)
    sx = (2 * np.arange(OW) + 1) * W // (2 * OW)
    return frame[:, sy][:, :, sx][..., 3:4]


def video_rgb(yfit, cbcr, C=3, siting=LEFT, rng=LIMITED, maxval=255, shift=0, kr=BT601[0], kb=BT601[1]):
    """The output frame [N][OH][OW][C]; C = 4 adds A = maxval << shift."""
    yfit = np.asarray(yfit)
    out = quantise(video_values(yfit, cbcr, siting, rng, maxval, shift, kr, kb), maxval, shift, yfit.dtype)
    if C == 4:
        out = np.concatenate([out, np.full(out.shape[:3] + (1,), maxval << shift, yfit.dtype)], axis=-1)
    return out


def rgb_rgb(yfit, frame, kr=BT601[0], kb=BT601[1]):
    """The output frame uint8 [N][OH][OW][C] of the RGB source, C that of `frame`."""
    yfit, frame = np.asarray(yfit), np.asarray(frame)
    out = quantise(rgb_values(yfit, frame, kr, kb), 255, 0, np.uint8)
    if frame.shape[-1] == 4:
        out = np.concatenate([out, alpha_of(frame, yfit.shape[1], yfit.shape[2])], axis=-1)
    return out


def to_planar(cbcr):
    """[N][H][W][2] -> [2N][H][W][1]: plane 2n = Cb, 2n + 1 = Cr of image n."""
    cbcr = np.asarray(cbcr)
    n, h, w, _ = cbcr.shape
    return np.ascontiguousarray(cbcr.transpose(0, 3, 1, 2).reshape(2 * n, h, w, 1))


def video_frame(n, h, w, oh, ow, maxval, shift, dtype, seed, whole_range=False):
    """(yfit [n][oh][ow][1], cbcr [n][h][w][2]) of tests/yuv_rgb_ref.py's input recipe: Y uniform in [40k, 200k), chroma uniform in [96k, 160k),
    k = (maxval + 1) / 256, so that the rounding is exercised and not the clamp; whole_range draws both over 0 .. maxval."""
    k = (maxval + 1) // 256
    g = np.random.default_rng(seed)
    ylo, yhi, clo, chi = (0, maxval + 1, 0, maxval + 1) if whole_range else (40 * k, 200 * k, 96 * k, 160 * k)
    y = g.integers(ylo, yhi, size=(n, oh, ow, 1))
    c = g.integers(clo, chi, size=(n, h, w, 2))
    return (y << shift).astype(dtype), (c << shift).astype(dtype)


def rgb_frame(n, h, w, oh, ow, C, seed):
    """(yfit uint8 [n][oh][ow][1], frame uint8 [n][h][w][C]): whole-range random bytes."""
    g = np.random.default_rng(seed)
    return g.integers(0, 256, size=(n, oh, ow, 1)).astype(np.uint8), g.integers(0, 256, size=(n, h, w, C)).astype(np.uint8)


def measured(kind, maxval=255, shapes=None):
    """Over `shapes` (SHAPES), both ranges and both sitings (video) on the input recipe: (the largest |float32 - float64| of the value in front of the
    rounding, the near-tie share at EPS[maxval], the share of values outside [-0.5, maxval + 0.5])."""
    worst, ties, clamps, total = 0.0, 0, 0, 0
    dtype = np.uint8 if maxval == 255 else np.uint16
    for i, (n, h, w, oh, ow) in enumerate(shapes or SHAPES):
        if kind == "video":
            yfit, cbcr = video_frame(n, h, w, oh, ow, maxval, 0, dtype, seed=700 + i)
            runs = [(video_values(yfit, cbcr, s, r, maxval, 0), video_values(yfit, cbcr, s, r, maxval, 0, dtype=np.float32)) for r in (LIMITED, FULL) for s in (CENTRE, LEFT)]
        else:
            yfit, frame = rgb_frame(n, h, w, oh, ow, 3, seed=800 + i)
            runs = [(rgb_values(yfit, frame), rgb_values(yfit, frame, dtype=np.float32))]
        for v64, v32 in runs:
            worst = max(worst, float(np.abs(v32.astype(np.float64) - v64).max()))
            ties += int(near_tie(v64, EPS[maxval]).sum())
            clamps += int(((v64 < -0.5) | (v64 > maxval + 0.5)).sum())
            total += v64.size
    return worst, ties / total, clamps / total


def compare(got, want_values, maxval, shift, alpha=None):
    """resample_ref.compare on the R, G, B channels with the near-tie half-width EPS[maxval]; the alpha channel, if any, must equal `alpha` (an array
    [N][OH][OW][1]; None: maxval << shift everywhere)."""
    got = np.asarray(got)
    if got.shape[-1] == 4:
        if alpha is None:
            assert (got[..., 3] == (maxval << shift)).all(), "alpha is not maxval << shift everywhere"
        else:
            np.testing.assert_array_equal(got[..., 3:4], alpha)
        got = got[..., :3]
    return resample_ref.compare(got, want_values, maxval, shift, EPS[maxval])


def compare_all(items, kind="video"):
    """compare() over the (got, want_values, maxval, shift[, alpha]) items of one sweep, near ties at most MAX_TIE_FRACTION[kind] of its values."""
    return resample_ref.compare_all(items, compare, MAX_TIE_FRACTION[kind])
