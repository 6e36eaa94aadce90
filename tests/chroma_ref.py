"""Float64 NumPy restatement of the chroma-plane contract of include/snnhip.h (snnhip_chroma_up_plan_create / snnhip_bicubic_taps_sited): a 4:2:0
chroma plane [N][H][W][C] upsampled r-fold with the separable Keys cubic, the horizontal axis sited, the vertical axis on aligned centres.  The
filter, the quantiser and the comparison rule are tests/resample_ref.py's."""
import numpy as np

import resample_ref
from resample_ref import CENTRE, LEFT, SITING_OFFSET, keys, near_tie, quantise  # noqa: F401  (re-exported for the tests)

# near-tie half-width by bit depth: six to seventeen times the fp32-to-float64 distance of the expression (6e-5 / 2e-4 / 1e-3)
EPS = {255: 1e-3, 1023: 2e-3, 4095: 6e-3}
MAX_TIE_FRACTION = 0.025


def taps(r, siting):
    """(weights float64 [r][4], base int [r]) of an r-fold upscale whose output is a chroma grid of the same siting: lead = off."""
    return resample_ref.taps(r, SITING_OFFSET[siting], SITING_OFFSET[siting])


def _resample(a, r, axis, siting):
    return resample_ref._resample(a, r, axis, SITING_OFFSET[siting], SITING_OFFSET[siting])


def up_values(u, r, siting, shift=0):
    """The values in front of the rounding, float64 [N][r*H][r*W][C]; u is uint8 / uint16 [N][H][W][C]."""
    v = (np.asarray(u).astype(np.int64) >> shift).astype(np.float64)
    return _resample(_resample(v, r, 2, siting), r, 1, CENTRE)  # horizontal (sited), then vertical (aligned centres)


def up(u, r, siting, maxval, shift=0):
    u = np.asarray(u)
    return quantise(up_values(u, r, siting, shift), maxval, shift, u.dtype)


def compare(got, want_values, maxval, shift):
    """resample_ref.compare with this contract's near-tie half-width EPS[maxval]."""
    return resample_ref.compare(got, want_values, maxval, shift, EPS[maxval])


def compare_all(items):
    """compare() over the (got, want_values, maxval, shift) items of one sweep, near ties at most MAX_TIE_FRACTION of the sweep's values."""
    return resample_ref.compare_all(items, compare, MAX_TIE_FRACTION)
