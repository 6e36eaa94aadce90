"""Float64 NumPy restatement of the plane-fit contract of include/snnhip.h (snnhip_plane_fit_plan_create / snnhip_fit_taps): a plane [N][H][W][C]
resampled to [N][OH][OW][C], each axis with its own ratio in [1/2, 4], eight normalised weights of the stretched Keys cubic per output coordinate,
the phase in integers.  The cubic, the quantiser and the comparison rule are tests/resample_ref.py's."""
import numpy as np

import resample_ref
from resample_ref import CENTRE, LEFT, keys, near_tie, quantise  # noqa: F401  (re-exported for the tests)

# near-tie half-width by bit depth, the values of tests/yuv_rgb_ref.py: 22 / 14 / 11 times the fp32-to-float64 distance of this expression
# (4.6e-5 / 2.1e-4 / 7.3e-4)
EPS = {255: 1e-3, 1023: 3e-3, 4095: 8e-3}
MAX_TIE_FRACTION = 0.025
TAPS = 8
# (N, H, W, OH, OW) of the GPU sweep: ratios 1, 1/2, 3/4, 4, odd sizes, rows that are not dword-aligned, one axis copying, two ratios in one plan
SHAPES = [(1, 1, 1, 1, 1), (1, 2, 3, 1, 2), (1, 5, 7, 3, 4), (1, 5, 7, 5, 7), (1, 5, 7, 20, 28), (1, 37, 29, 19, 15), (1, 19, 67, 27, 100), (1, 31, 33, 31, 20),
          (1, 20, 20, 45, 80), (2, 13, 21, 7, 11)]
DEPTHS = [("u8", 255, 0), ("u16", 1023, 0), ("u16", 1023, 6), ("u16", 4095, 0)]  # (container, maxval, shift): tests/test_frame_chroma_gpu.py's
LEAD4 = {CENTRE: 2, LEFT: 1, "centre": 2, "left": 1}  # a = 4 * lead


def table(I, O, siting):
    """(weights float64 [O][8], base int64 [O]) of one axis: output X reads in[clip(base[X] - 3 + k)] with weights[X][k]."""
    assert I >= 1 and O >= 1 and 2 * O >= I and O <= 4 * I, (I, O)
    a = LEAD4[siting]
    D = 4 * O
    f = min(O / I, 1.0)
    w = np.zeros((O, TAPS), np.float64)
    base = np.zeros(O, np.int64)
    for X in range(O):
        Nn = (4 * X + a) * I - a * O
        b = Nn // D  # floor
        t = (Nn - b * D) / D
        row = [float(keys(abs(float(k - 3) - t) * f)) for k in range(TAPS)]
        total = 0.0
        for v in row:  # ascending tap order
            total += v
        base[X] = b
        w[X] = [v / total for v in row]
    return w, base


def _resample(a, O, axis, siting, dtype=np.float64):
    """`a` resampled to O samples along `axis`, replicate edge; with dtype float32 the weights are rounded and the sum runs in float32."""
    size = a.shape[axis]
    w, base = table(size, O, siting)
    w = w.astype(np.float32).astype(dtype) if dtype == np.float32 else w
    shape = [1] * a.ndim
    shape[axis] = O
    out = None
    for k in range(TAPS):
        idx = np.clip(base - 3 + k, 0, size - 1)
        term = np.take(a, idx, axis=axis) * w[:, k].reshape(shape)
        out = term if out is None else out + term
    return out


def fit_values(u, OH, OW, siting, shift=0, dtype=np.float64):
    """The values in front of the rounding, [N][OH][OW][C]; u is uint8 / uint16 [N][H][W][C].  Vertical (aligned centres), then horizontal (sited)."""
    v = (np.asarray(u).astype(np.int64) >> shift).astype(dtype)
    return _resample(_resample(v, OH, 1, CENTRE, dtype), OW, 2, siting, dtype)


def fit(u, OH, OW, siting, maxval, shift=0):
    u = np.asarray(u)
    return quantise(fit_values(u, OH, OW, siting, shift), maxval, shift, u.dtype)


def compare(got, want_values, maxval, shift):
    """resample_ref.compare with this contract's near-tie half-width EPS[maxval]."""
    return resample_ref.compare(got, want_values, maxval, shift, EPS[maxval])


def compare_all(items):
    """compare() over the (got, want_values, maxval, shift) items of one sweep, near ties at most MAX_TIE_FRACTION of the sweep's values."""
    return resample_ref.compare_all(items, compare, MAX_TIE_FRACTION)
