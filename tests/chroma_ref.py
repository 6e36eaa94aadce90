"""Float64 NumPy restatement of the chroma-plane contract of include/snnhip.h (snnhip_chroma_up_plan_create / snnhip_bicubic_taps_sited): a 4:2:0
chroma plane [N][H][W][C] upsampled r-fold with the separable Keys cubic, the horizontal axis sited, the vertical axis on aligned centres.  The
Keys kernel and the near-tie helper are tests/colour_ref.py's."""
import numpy as np

from colour_ref import keys, near_tie

CENTRE, LEFT = 0, 1
SITING_OFFSET = {CENTRE: 0.5, LEFT: 0.25, "centre": 0.5, "left": 0.25}
# near-tie half-width by bit depth: six to seventeen times the fp32-to-float64 distance of the expression (6e-5 / 2e-4 / 1e-3)
EPS = {255: 1e-3, 1023: 2e-3, 4095: 6e-3}
MAX_TIE_FRACTION = 0.025


def phase(r, p, siting):
    """(base, t) of output sample r*x + p: it reads source position x + s, s = (p + off) / r - off, base = floor(s), t = s - base."""
    off = SITING_OFFSET[siting]
    s = (p + off) / r - off
    base = np.floor(s)
    return int(base), s - base


def taps(r, siting):
    """(weights float64 [r][4], base int [r]): phase p reads x + base[p] - 1 .. x + base[p] + 2."""
    rows, bases = [], []
    for p in range(r):
        b, t = phase(r, p, siting)
        rows.append(keys(np.array([1.0 + t, t, 1.0 - t, 2.0 - t])))
        bases.append(b)
    return np.stack(rows), np.array(bases, np.int64)


def _resample(a, r, axis, siting):
    size = a.shape[axis]
    w, base = taps(r, siting)
    X = np.arange(r * size)
    x, p = X // r, X % r
    out = 0.0
    shape = [1] * a.ndim
    shape[axis] = r * size
    for k in range(4):
        idx = np.clip(x + base[p] - 1 + k, 0, size - 1)
        out = out + np.take(a, idx, axis=axis) * w[p, k].reshape(shape)
    return out


def up_values(u, r, siting, shift=0):
    """The values in front of the rounding, float64 [N][r*H][r*W][C]; u is uint8 / uint16 [N][H][W][C]."""
    v = (np.asarray(u).astype(np.int64) >> shift).astype(np.float64)
    return _resample(_resample(v, r, 2, siting), r, 1, CENTRE)  # horizontal (sited), then vertical (aligned centres)


def quantise(values, maxval, shift, dtype):
    return (np.clip(np.rint(values), 0.0, float(maxval)).astype(np.int64) << shift).astype(dtype)  # np.rint: ties to even


def up(u, r, siting, maxval, shift=0):
    u = np.asarray(u)
    return quantise(up_values(u, r, siting, shift), maxval, shift, u.dtype)


def compare(got, want_values, maxval, shift):
    """The comparison rule for one output: equal to the reference wherever its pre-rounding value is farther than EPS[maxval] from a tie, at most
    1 << shift off on near ties.  Returns (near ties, values compared, values that differ); the caller bounds the near ties of its sweep."""
    got = np.asarray(got)
    want = quantise(want_values, maxval, shift, got.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    tie = near_tie(want_values, EPS[maxval])
    assert not (got.astype(np.int64) & ((1 << shift) - 1)).any(), "bits below the shift are set"
    diff = (got.astype(np.int64) >> shift) - (want.astype(np.int64) >> shift)
    bad = (diff != 0) & ~tie
    assert not bad.any(), "%d values differ off the near ties, first at %s: got %s, reference value %s" % (
        int(bad.sum()), tuple(np.argwhere(bad)[0]), got[bad][0], want_values[bad][0])
    assert np.abs(diff).max(initial=0) <= 1, "a near-tie value differs by %d" % int(np.abs(diff).max())
    return int(tie.sum()), int(tie.size), int((diff != 0).sum())


def compare_all(items):
    """compare() over the (got, want_values, maxval, shift) items of one sweep; near ties are at most MAX_TIE_FRACTION of the sweep's values taken
    together (asserted on the reference alone).  Returns (near-tie fraction, values that differ)."""
    ties = total = ndiff = 0
    for got, want_values, maxval, shift in items:
        t, n, d = compare(got, want_values, maxval, shift)
        ties, total, ndiff = ties + t, total + n, ndiff + d
    assert ties <= MAX_TIE_FRACTION * total, "near ties are %d of %d reference values: change the seed" % (ties, total)
    return ties / max(total, 1), ndiff
