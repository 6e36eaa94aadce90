"""What the float64 references of the three frame paths share (tests/colour_ref.py, tests/chroma_ref.py, tests/yuv_rgb_ref.py): the Keys cubic, the
general phase and its tap table, the separable resampling, the quantiser and the comparison rule.  The counterpart of shadernn_amd/csrc/frame_resample.h;
each reference module keeps its own matrices, input recipes and bounds and passes the bounds in."""
import numpy as np

CENTRE, LEFT = 0, 1
SITING_OFFSET = {CENTRE: 0.5, LEFT: 0.25, "centre": 0.5, "left": 0.25}


def keys(d):
    """Keys cubic, a = -0.5 (Catmull-Rom), at distance d >= 0; the products are written out so that any IEEE double arithmetic gives the same bits."""
    d = np.asarray(d, np.float64)
    a = -0.5
    near = (a + 2.0) * (d * d * d) - (a + 3.0) * (d * d) + 1.0
    far = a * (d * d * d) - 5.0 * a * (d * d) + 8.0 * a * d - 4.0 * a
    return np.where(d <= 1.0, near, np.where(d < 2.0, far, 0.0))


def near_tie(v, eps=1e-3):
    v = np.asarray(v, np.float64)
    return np.abs(v - np.floor(v) - 0.5) < eps


def phase(R, p, lead, off):
    """(base, t) of output sample R*x + p of an R-fold resampling: it reads source position x + s, s = (p + lead) / R - off, base = floor(s),
    t = s - base.  Aligned centres: lead = off = 0.5; a sited chroma grid to one of its own siting: lead = off; to the luma grid: lead = 0.5."""
    s = (p + lead) / R - off
    base = np.floor(s)
    return int(base), s - base


def taps(R, lead, off):
    """(weights float64 [R][4], base int [R]): phase p reads x + base[p] - 1 .. x + base[p] + 2."""
    rows, bases = [], []
    for p in range(R):
        b, t = phase(R, p, lead, off)
        rows.append(keys(np.array([1.0 + t, t, 1.0 - t, 2.0 - t])))
        bases.append(b)
    return np.stack(rows), np.array(bases, np.int64)


def _resample(a, R, axis, lead, off, dtype=np.float64):
    """`a` resampled R-fold along `axis`, replicate edge; with dtype float32 the weights are rounded and the sum runs in float32."""
    size = a.shape[axis]
    w, base = taps(R, lead, off)
    w = w.astype(dtype)
    X = np.arange(R * size)
    x, p = X // R, X % R
    out = None
    shape = [1] * a.ndim
    shape[axis] = R * size
    for k in range(4):
        idx = np.clip(x + base[p] - 1 + k, 0, size - 1)
        term = np.take(a, idx, axis=axis) * w[p, k].reshape(shape)
        out = term if out is None else out + term
    return out


def quantise(v, maxval, shift, dtype):
    return (np.clip(np.rint(v), 0.0, float(maxval)).astype(np.int64) << shift).astype(dtype)  # np.rint: ties to even


def compare(got, want_values, maxval, shift, eps):
    """The comparison rule for one output: equal to the reference wherever its pre-rounding value is farther than `eps` from a tie, at most
    1 << shift off on near ties.  Returns (near ties, values compared, values that differ); the caller bounds the near ties."""
    got = np.asarray(got)
    want = quantise(want_values, maxval, shift, got.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    tie = near_tie(want_values, eps)
    assert not (got.astype(np.int64) & ((1 << shift) - 1)).any(), "bits below the shift are set"
    diff = (got.astype(np.int64) >> shift) - (want.astype(np.int64) >> shift)
    bad = (diff != 0) & ~tie
    assert not bad.any(), "%d values differ off the near ties, first at %s: got %s, reference value %s" % (
        int(bad.sum()), tuple(np.argwhere(bad)[0]), got[bad][0], want_values[bad][0])
    assert np.abs(diff).max(initial=0) <= 1, "a near-tie value differs by %d" % int(np.abs(diff).max())
    return int(tie.sum()), int(tie.size), int((diff != 0).sum())


def compare_all(items, compare_one, max_tie_fraction):
    """compare_one(*item) over the items of one sweep; near ties are at most `max_tie_fraction` of the sweep's values taken together (asserted on the
    reference alone: its smallest frames have three values each).  Returns (near-tie fraction, values that differ)."""
    ties = total = ndiff = 0
    for item in items:
        t, n, d = compare_one(*item)
        ties, total, ndiff = ties + t, total + n, ndiff + d
    assert ties <= max_tie_fraction * total, "near ties are %d of %d reference values: change the seed" % (ties, total)
    return ties / max(total, 1), ndiff
