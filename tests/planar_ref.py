"""Reference for the planar 4:2:0 units (include/snnhip.h, snnhip_yuv_rgb_planar_plan_create / snnhip_rgb_cbcr_planar_plan_create; DESIGN.md section
4.19).  No arithmetic of its own: the planar chroma tensor [2N][H][W][1] (plane 2n = Cb, 2n + 1 = Cr of image n) is (de)interleaved in NumPy and handed
to the float64 references of the interleaved units -- yuv_rgb_ref, rgb_cbcr_ref, chroma_ref, fit_ref -- whose comparison rule, EPS and
MAX_TIE_FRACTION apply unchanged: the fp32 expression of the planar kernels is the one those were measured for."""
import numpy as np

import chroma_ref
import fit_ref
import rgb_cbcr_ref
import yuv_rgb_ref

DEPTHS = [("u8", 255, 0), ("u16", 1023, 6), ("u16", 1023, 0), ("u16", 4095, 0)]  # tests/test_frame_chroma_gpu.py's (container, maxval, shift)
DEPTH_IDS = ["u8", "p010", "u10", "u12"]
SITINGS = ["centre", "left"]
RANGES = ["limited", "full"]
# the tile of the yuv_rgb plans in chroma pixels by container (the plan's describe reports it; tests/test_frame_planar_gpu.py checks that they agree),
# so that the CPU suite bounds the near ties of exactly the frames the GPU sweep compares
YUV_TILE = {"u8": (4, 128), "u16": (4, 64)}


def interleave(planes):
    """[2N][H][W][1] -> [N][H][W][2]"""
    p = np.asarray(planes)
    assert p.ndim == 4 and p.shape[0] % 2 == 0 and p.shape[3] == 1, p.shape
    return np.ascontiguousarray(np.stack([p[0::2, :, :, 0], p[1::2, :, :, 0]], axis=-1))


def deinterleave(cbcr):
    """[N][H][W][2] -> [2N][H][W][1]"""
    c = np.asarray(cbcr)
    assert c.ndim == 4 and c.shape[3] == 2, c.shape
    n, h, w, _ = c.shape
    return np.ascontiguousarray(np.moveaxis(c, 3, 1).reshape(2 * n, h, w, 1))


def np_dtype(container):
    return np.uint8 if container == "u8" else np.uint16


# ---- yuv_rgb_planar

def yuv_shapes(r, container, tile=None):
    """(N, H, W) of a chroma plane, the smallest where the kernel can go wrong, from the tile (TH, TW): one pixel; 2 x 3 (an odd width: the last lane
    owns a partial piece and rows lose their 2- and 4-byte alignment); one short of a tile, a tile, one past it with N = 2 (odd H * W: the Cr plane
    and the second image start off a dword); a wide three-row plane; for odd r an odd width once more."""
    th, tw = tile or YUV_TILE[container]
    shapes = [(1, 1, 1), (1, 2, 3), (1, th - 1, tw - 1), (1, th, tw), (2, th + 1, tw + 1), (1, 3, 2 * tw + 5)]
    if r % 2:
        shapes.append((1, 5, 7))
    return shapes


def yuv_cases(r, container, maxval, shapes=None, sitings=SITINGS, ranges=RANGES):
    """(siting, range, (n, h, w), seed) of one sweep"""
    for si, siting in enumerate(sitings):
        for ri, rng in enumerate(ranges):
            for k, shape in enumerate(shapes or yuv_shapes(r, container)):
                yield siting, rng, shape, 7000 + 1000 * r + 10 * k + 2 * si + ri + maxval


def yuv_frame(n, h, w, r, maxval, shift, dtype, seed, whole_range=False, disjoint=False):
    """(yhi, planes [2n][h][w][1]) of yuv_rgb_ref's input recipe; disjoint: Cb below and Cr above the neutral code, so that swapped planes show"""
    yhi, cbcr = yuv_rgb_ref.frame(n, h, w, r, maxval, shift, dtype, seed, whole_range=whole_range)
    if disjoint:
        k = (maxval + 1) // 256
        g = np.random.default_rng(seed + 1)
        cbcr[..., 0] = (g.integers(96 * k, 120 * k, size=cbcr.shape[:3]) << shift).astype(dtype)
        cbcr[..., 1] = (g.integers(136 * k, 160 * k, size=cbcr.shape[:3]) << shift).astype(dtype)
    return yhi, deinterleave(cbcr)


def yuv_values(yhi, planes, r, siting, rng, maxval, shift, *matrix):
    return yuv_rgb_ref.values(yhi, interleave(planes), r, siting, rng, maxval, shift, *matrix)


# ---- rgb_cbcr_planar

def cbcr_cases(r, C, shapes=None, sitings=SITINGS, ranges=RANGES):
    """rgb_cbcr_ref's sweep (its shapes, which already hold N = 2 on a tile seam and odd widths) on frames of this module's own"""
    for siting, rng, shape, seed in rgb_cbcr_ref.sweep_cases(r, C, shapes, sitings, ranges):
        yield siting, rng, shape, 7000 + seed


def cbcr_values(rgb, r, siting, rng, *matrix):
    """float64 values in front of the rounding, as the planar tensor [2N][rH/2][rW/2][1]"""
    return deinterleave(rgb_cbcr_ref.values(rgb, r, siting, rng, *matrix))


# ---- planar in, planar out: chroma_up / plane_fit with C = 1 over the 2N planes (channels never mix, so the planes go to the references as they are)

def up_values(planes, r, siting, shift=0):
    return deinterleave(chroma_ref.up_values(interleave(planes), r, siting, shift))


def fit_values(planes, OH, OW, siting, shift=0):
    return deinterleave(fit_ref.fit_values(interleave(planes), OH, OW, siting, shift))
