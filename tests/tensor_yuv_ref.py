"""Float64 NumPy restatement of the output-tensor -> video-frame contract of include/snnhip.h (snnhip_tensor_yuv_plan_create /
snnhip_tensor_yuv_planar_plan_create / snnhip_tensor_yuv_coefficients): the model's output tensor in, the luma plane and the
4:2:0 chroma of a frame of the same extent out.  The tensor's values are taken exactly as the kernel reads them (an fp16 tensor is passed as float16
and widened); kr, kg, kb, the map and the five coefficients are the fp32 values the device sees; everything else is float64.  values32() evaluates
the same expression in float32 (no fused multiply-add): measured_distance() over the GPU sweeps' own frames decides the near-tie half-width.  The
quantiser and the comparison rule are tests/resample_ref.py's, the ranges tests/yuv_rgb_ref.py's, the luma coefficients tests/colour_ref.py's and the
chroma scales at 8 bits tests/rgb_cbcr_ref.py's.  The sweeps of tests/test_frame_tensor_yuv_gpu.py are defined here, so that the CPU suite measures
exactly the frames the GPU suite compares."""
import numpy as np

import colour_ref
import planar_ref
import resample_ref
import rgb_cbcr_ref
import yuv_rgb_ref
from resample_ref import near_tie, quantise  # noqa: F401  (re-exported for the tests)
from yuv_rgb_ref import BT601, BT709, CENTRE, LEFT, LIMITED, FULL, RANGES  # noqa: F401

DEPTHS = planar_ref.DEPTHS
DEPTH_IDS = planar_ref.DEPTH_IDS
SITINGS = planar_ref.SITINGS
RANGE_NAMES = planar_ref.RANGES
_SITING = {CENTRE: CENTRE, LEFT: LEFT, "centre": CENTRE, "left": LEFT}
# The largest fp32-to-float64 distance of a value in front of the rounding over the GPU sweeps' frames, by maxval (measured_distance below;
# tests/test_frame_tensor_yuv.py prints the distances and holds these figures to them): 8 / 10 / 12 bits.  Each is under a quarter of the family's
# near-tie half-width yuv_rgb_ref.EPS (1e-3 / 3e-3 / 8e-3) -- the 4x margin that covers FMA contraction and a summation order other than NumPy's --
# so the family's EPS is used as it is.
MEASURED_DISTANCE = {255: 3.1e-5, 1023: 1.25e-4, 4095: 4.8e-4}
EPS = yuv_rgb_ref.EPS
assert all(4.0 * MEASURED_DISTANCE[m] <= EPS[m] for m in EPS)
MAX_TIE_FRACTION = 0.025  # per sweep, asserted on the reference alone
# luma pixels of one block by (container, planar): 256 lanes x 2 rows x the strip (8 / 4 columns of planar u8 / u16, 4 / 2 of interleaved); the
# plan's describe reports it and the GPU suite checks that they agree
TILE = {("u8", False): 2048, ("u8", True): 4096, ("u16", False): 1024, ("u16", True): 2048}


def coefficients(maxval=255, rng=LIMITED, kr=BT601[0], kb=BT601[1]):
    """(Yoff, ys, Coff, cbs, crs) as the device sees them: float32 values, returned as a float32 array."""
    k = (maxval + 1) / 256.0
    m = float(maxval)
    limited = RANGES[rng] == LIMITED
    yoff, yrange, crange = (16.0 * k, 219.0 * k, 224.0 * k) if limited else (0.0, m, m)
    kr, kb = float(np.float32(kr)), float(np.float32(kb))
    return np.array([yoff, yrange / m, 128.0 * k, crange / (2.0 * (1.0 - kb) * m), crange / (2.0 * (1.0 - kr) * m)], np.float64).astype(np.float32)


for _rng in (LIMITED, FULL):  # at 8 bits Coff and the two chroma scales are rgb_cbcr's own, bit for bit
    assert coefficients(255, _rng)[2:].tobytes() == rgb_cbcr_ref.coefficients(_rng).tobytes()


def _values(x, scale, offset, siting, rng, maxval, kr, kb, dtype):
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float16) and x.ndim == 4 and x.shape[3] in (3, 4) and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0, (x.dtype, x.shape)
    kr_, kg_, kb_ = (dtype(v) for v in colour_ref.coefficients(kr, kb))
    yoff, ys, coff, cbs, crs = coefficients(maxval, rng, kr, kb).astype(dtype)
    sc = np.asarray(scale, np.float32)[:3].astype(dtype)
    of = np.asarray(offset, np.float32)[:3].astype(dtype)
    p = np.clip(x[..., :3].astype(dtype) * sc + of, dtype(0), dtype(maxval))  # channel 3 is never read
    ylo = kr_ * p[..., 0] + kg_ * p[..., 1] + kb_ * p[..., 2]
    yv = (yoff + ys * ylo)[..., None]
    d = np.stack([p[..., 2] - ylo, p[..., 0] - ylo], axis=-1)  # (dB, dR)
    half, quarter = dtype(0.5), dtype(0.25)
    if _SITING[siting] == LEFT:
        before = d[:, :, np.clip(np.arange(0, d.shape[2], 2) - 1, 0, None)]  # column 2I - 1, clamped: only I = 0
        h = (quarter * before + half * d[:, :, 0::2]) + quarter * d[:, :, 1::2]
    else:
        h = half * d[:, :, 0::2] + half * d[:, :, 1::2]
    v = half * h[:, 0::2] + half * h[:, 1::2]
    cv = coff + np.array([cbs, crs], dtype) * v
    assert yv.dtype == dtype and cv.dtype == dtype
    return yv, cv


def values(x, scale=(1, 1, 1), offset=(0, 0, 0), siting=LEFT, rng=LIMITED, maxval=255, kr=BT601[0], kb=BT601[1]):
    """The values in front of the rounding, float64: (Y [N][H][W][1], CbCr [N][H/2][W/2][2]); x float32 or float16 [N][H][W][C], C = 3 or 4."""
    return _values(x, scale, offset, siting, rng, maxval, kr, kb, np.float64)


def values32(x, scale=(1, 1, 1), offset=(0, 0, 0), siting=LEFT, rng=LIMITED, maxval=255, kr=BT601[0], kb=BT601[1]):
    """The same expression with float32 coefficients and arithmetic (no fused multiply-add)."""
    return _values(x, scale, offset, siting, rng, maxval, kr, kb, np.float32)


def planes(x, scale=(1, 1, 1), offset=(0, 0, 0), siting=LEFT, rng=LIMITED, maxval=255, shift=0, kr=BT601[0], kb=BT601[1]):
    """The frame: (luma [N][H][W][1], cbcr [N][H/2][W/2][2]), uint8 for maxval 255 and uint16 above."""
    dt = np.uint8 if maxval == 255 else np.uint16
    yv, cv = values(x, scale, offset, siting, rng, maxval, kr, kb)
    return quantise(yv, maxval, shift, dt), quantise(cv, maxval, shift, dt)


def brute(x, scale, offset, siting, rng, maxval, kr, kb):
    """The contract sample by sample in Python floats (float64), with explicit loops: for small frames only."""
    x = np.asarray(x)
    n, H, W, _ = x.shape
    kr_, kg_, kb_ = colour_ref.coefficients(kr, kb)
    yoff, ys, coff, cbs, crs = (float(c) for c in coefficients(maxval, rng, kr, kb))
    sc = [float(np.float32(s)) for s in scale]
    of = [float(np.float32(o)) for o in offset]

    def pixel(i, y, xx):
        p = [min(max(float(x[i, y, xx, c]) * sc[c] + of[c], 0.0), float(maxval)) for c in range(3)]
        ylo = kr_ * p[0] + kg_ * p[1] + kb_ * p[2]
        return ylo, p[2] - ylo, p[0] - ylo

    yv = np.zeros((n, H, W, 1))
    cv = np.zeros((n, H // 2, W // 2, 2))
    for i in range(n):
        for y in range(H):
            for xx in range(W):
                yv[i, y, xx, 0] = yoff + ys * pixel(i, y, xx)[0]
        for J in range(H // 2):
            for I in range(W // 2):
                if _SITING[siting] == LEFT:
                    cols = [(min(max(2 * I - 1, 0), W - 1), 0.25), (2 * I, 0.5), (2 * I + 1, 0.25)]
                else:
                    cols = [(2 * I, 0.5), (2 * I + 1, 0.5)]
                for comp, s in ((0, cbs), (1, crs)):
                    acc = 0.0
                    for row in (2 * J, 2 * J + 1):
                        acc += 0.5 * sum(w * pixel(i, row, col)[1 + comp] for col, w in cols)
                    cv[i, J, I, comp] = coff + s * acc
    return yv, cv


# ---- the sweeps of tests/test_frame_tensor_yuv_gpu.py

def shapes(container, planar):
    """(n, h, w), the smallest where the kernel can go wrong, from the tile T (luma pixels of a block, two rows deep): one chroma sample; two in a row
    and in a column; W = 6, 10 and 18, the strip tails at W = 2, 4, 6 mod 8; one block exactly, one strip tail less and more; two blocks and a tail;
    N = 2 of two row pairs of T / 4 + 6 columns: the second image starts inside a block and, for 8-bit planes, every other row 2 bytes off a dword."""
    T = TILE[(container, planar)]
    return [(1, 2, 2), (1, 2, 4), (1, 4, 2), (1, 2, 6), (1, 2, 10), (1, 6, 18), (1, 2, T // 2 - 2), (1, 2, T // 2), (1, 2, T // 2 + 2), (1, 2, T + 2), (2, 4, T // 4 + 6)]


def output_map(k, maxval):
    """(scale, offset) of case k: a model that emits the output depth's own units, a tanh model, and one map per channel (0 .. 255, tanh, unit)"""
    m = float(maxval)
    return [((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ((m / 2, m / 2, m / 2), (m / 2, m / 2, m / 2)), ((m / 255.0, m / 2, 1.0), (0.0, m / 2, 0.0))][k % 3]


def tensor(n, h, w, C, half, maxval, scale, offset, seed):
    """[n][h][w][C] float32, or float16 for half: p = x * scale + offset uniform over [-0.1, 1.1] maxval, so that both clamps are hit and the rounding is
    exercised everywhere between them; channel 3, if any, is NaN (it must never be read)."""
    g = np.random.default_rng(seed)
    p = g.uniform(-0.1 * maxval, 1.1 * maxval, size=(n, h, w, 3))
    x = ((p - np.asarray(offset, np.float64)) / np.asarray(scale, np.float64)).astype(np.float32)
    if C == 4:
        x = np.concatenate([x, np.full((n, h, w, 1), np.nan, np.float32)], axis=-1)
    return x.astype(np.float16) if half else x


def sweep_cases(C, half, container, maxval, shift, planar):
    """(shape, siting, range, (kr, kb), scale, offset, seed) of one sweep: both sitings and ranges on every shape, the matrix and the map alternating"""
    for si, siting in enumerate(SITINGS):
        for ri, rng in enumerate(RANGE_NAMES):
            for k, shape in enumerate(shapes(container, planar)):
                scale, offset = output_map(k + si + ri, maxval)
                yield shape, siting, rng, (BT709 if (k + si) % 2 else BT601), scale, offset, 3000 + 100 * k + 10 * si + 2 * ri + maxval + shift + int(planar)


def case_tensor(case, C, half, maxval):
    (n, h, w), siting, rng, matrix, scale, offset, seed = case
    return tensor(n, h, w, C, half, maxval, scale, offset, seed)


def case_values(case, x, maxval, fn=values):
    (n, h, w), siting, rng, (kr, kb), scale, offset, seed = case
    return fn(x, scale, offset, siting, rng, maxval, kr, kb)


def measured_distance(container, maxval, shift):
    """The largest |float32 - float64| of a value in front of the rounding over the GPU sweeps' frames of one depth (C = 3 and 4 share the values)."""
    worst = 0.0
    for planar in (False, True):
        for half in (False, True):
            for case in sweep_cases(3, half, container, maxval, shift, planar):
                x = case_tensor(case, 3, half, maxval)
                for a, b in zip(case_values(case, x, maxval, values32), case_values(case, x, maxval)):
                    worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()))
    return worst


def compare(got, want_values, maxval, shift):
    """resample_ref.compare with this contract's near-tie half-width"""
    return resample_ref.compare(got, want_values, maxval, shift, EPS[maxval])


def compare_all(items):
    """compare() over the (got, want_values, maxval, shift) items of one sweep -- the luma plane and the chroma of every case -- near ties at most
    MAX_TIE_FRACTION of the sweep's values taken together.  Returns (near-tie fraction, values that differ)."""
    return resample_ref.compare_all(items, compare, MAX_TIE_FRACTION)


def saturated(n, h, w, C, maxval, seed):
    """a tensor of saturated primaries in 2 x 2 blocks (so that the decimation keeps them saturated), at scale 1, offset 0: every channel 0 or maxval"""
    g = np.random.default_rng(seed)
    x = np.repeat(np.repeat(g.integers(0, 2, size=(n, h // 2, w // 2, C)) * maxval, 2, axis=1), 2, axis=2).astype(np.float32)
    return x

