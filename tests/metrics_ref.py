"""The frame-quality definition of include/snnhip.h (snnhip_frame_metrics_plan_create) restated in NumPy: the reference the frame-metrics tests compare
the device against.  Integer moments are exact (int64 holds every one of them up to 16-bit samples: a window's 64 * ss stays below 2^46), t is
evaluated in float64 with the operations in the order the header writes them, and the windows are added with math.fsum.

    sse     = sum (a - b)^2 over all H * W pixels                            (exact)
    psnr_db = 10 log10(maxval^2 pixels / sse), +inf for sse == 0
    SSIM:   bh = H >> 2, bw = W >> 2; per 4x4 block s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b; a window is a 2x2 group of blocks;
            c1 = 0.01^2 maxval^2 64, c2 = 0.03^2 maxval^2 64 63, vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2,
            t = (2 s1 s2 + c1)(2 covar + c2) / ((s1^2 + s2^2 + c1)(vars + c2)), ssim = sum t / windows
"""
import math

import numpy as np


def constants(maxval):
    """(c1, c2), evaluated left to right in double: the library evaluates the same expressions"""
    m = float(maxval)
    return 0.01 * 0.01 * m * m * 64.0, 0.03 * 0.03 * m * m * 64.0 * 63.0


def psnr_db(sse, pixels, maxval):
    if sse == 0:
        return math.inf
    m = float(maxval)
    return 10.0 * math.log10(m * m * float(pixels) / float(sse))


def window_moments(a, b):
    """a, b: [H][W] integer planes of sample VALUES.  Returns int64 arrays [bh - 1][bw - 1]: s1, s2, ss, s12 of every 8x8 window, from 4x4 blocks."""
    a = np.asarray(a).astype(np.int64)
    b = np.asarray(b).astype(np.int64)
    H, W = a.shape
    bh, bw = H >> 2, W >> 2

    def blocks(v):
        return v[: 4 * bh, : 4 * bw].reshape(bh, 4, bw, 4).sum(axis=(1, 3))

    def windows(v):
        return v[:-1, :-1] + v[:-1, 1:] + v[1:, :-1] + v[1:, 1:]

    return windows(blocks(a)), windows(blocks(b)), windows(blocks(a * a + b * b)), windows(blocks(a * b))


def window_terms(s1, s2, ss, s12, maxval):
    """t of every window in float64 from the exact integer moments (each below 2^53, so every product and difference here is exact)"""
    c1, c2 = constants(maxval)
    s1 = np.asarray(s1).astype(np.float64)
    s2 = np.asarray(s2).astype(np.float64)
    ss = np.asarray(ss).astype(np.float64)
    s12 = np.asarray(s12).astype(np.float64)
    vars_ = 64.0 * ss - s1 * s1 - s2 * s2
    covar = 64.0 * s12 - s1 * s2
    return ((2.0 * s1 * s2 + c1) * (2.0 * covar + c2)) / ((s1 * s1 + s2 * s2 + c1) * (vars_ + c2))


def plane_metrics(a, b, maxval):
    """one image, one channel of sample values: dict(sse, pixels, windows, ssim_sum, ssim, psnr_db)"""
    a = np.asarray(a).astype(np.int64)
    b = np.asarray(b).astype(np.int64)
    H, W = a.shape
    d = a - b
    sse = int((d * d).sum(dtype=np.int64))
    t = window_terms(*window_moments(a, b), maxval)
    ssim_sum = math.fsum(t.ravel().tolist())
    windows = int(t.size)
    return {"sse": sse, "pixels": H * W, "windows": windows, "ssim_sum": ssim_sum, "ssim": ssim_sum / windows, "psnr_db": psnr_db(sse, H * W, maxval)}


def frame_metrics(a, b, maxval, shift=0):
    """a (test), b (reference): [N][H][W][C] uint8 / uint16 containers.  One dict per (image, channel), image-major, as snnhip_frame_metrics_read orders
    its rows; the sample value is u >> shift."""
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape and a.ndim == 4 and a.dtype == b.dtype, (a.shape, b.shape)
    va = a.astype(np.int64) >> shift
    vb = b.astype(np.int64) >> shift
    N, _, _, C = a.shape
    return [plane_metrics(va[n, :, :, c], vb[n, :, :, c], maxval) for n in range(N) for c in range(C)]
