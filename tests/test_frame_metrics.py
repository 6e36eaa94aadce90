"""Frame metrics without a device: the new symbols are declared, exported and bound; the structs have the documented layout; the host-side dB
formula; tests/metrics_ref.py against an independent brute-force statement of the definition; the refusals that need no GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_c_abi_symbols_are_declared_exported_and_bound(built):
    from shadernn_amd import capi

    txt = _header("snnhip.h")
    lib = capi.lib()
    for name in ("snnhip_frame_metrics_plan_create", "snnhip_frame_metrics_read", "snnhip_frame_metrics_psnr"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct { int N, H, W, C; int dtype; int maxval, shift; } snnhip_frame_metrics_desc;" in txt
    assert "typedef struct { unsigned long long sse, pixels, windows; double ssim_sum; } snnhip_frame_metrics_row;" in txt
    assert capi.SIGNATURES["snnhip_frame_metrics_psnr"][0] is C.c_double
    assert callable(capi.frame_metrics_plan) and callable(capi.frame_metrics_read)
    th, tw = capi.FRAME_METRICS_TILE
    src = open(os.path.join(ROOT, "shadernn_amd", "csrc", "frame_metrics.h")).read()
    assert "kMetricsTileH = %d;" % th in src and "kMetricsTileW = %d;" % tw in src  # the constant the GPU tests build their shapes from


def test_host_mirror_symbols_are_declared_exported_and_bound(built):
    from shadernn_amd import host

    txt = _header("snn_c.h")
    lib = host.lib()
    for name in ("snn_model_reference_frame", "snn_model_reference_frame_planes", "snn_model_frame_metrics"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in host.SIGNATURES and hasattr(lib, name), name
    assert callable(host.Model.set_reference) and callable(host.Model.metrics)


def test_struct_sizes(built):
    from shadernn_amd import capi, host

    assert C.sizeof(capi.FrameMetricsDesc) == 7 * 4
    assert C.sizeof(capi.FrameMetricsRow) == 3 * 8 + 8
    assert [f for f, _ in capi.FrameMetricsRow._fields_] == ["sse", "pixels", "windows", "ssim_sum"]
    assert C.sizeof(host.FrameMetrics) == 3 * 4 + 4 + 2 * 8 + 2 * 8  # three ints, padding to 8, two 64-bit counts, two doubles
    assert host.FrameMetrics.sse.offset == 16 and host.FrameMetrics.psnr_db.offset == 32


def test_psnr_against_the_formula(built):
    from shadernn_amd import capi

    assert capi.frame_metrics_psnr(0, 1920 * 1080, 255) == math.inf
    assert capi.frame_metrics_psnr(0, 0, 255) == math.inf
    for sse, pixels, maxval in ((1, 1, 255), (99, 99, 255), (12345, 3840 * 2160, 255), (7, 64, 1023), (2 ** 40, 3840 * 2160, 65535), (2 ** 64 - 1, 1, 1),
                                (2 ** 64 - 1, 2 ** 40, 65535)):
        want = 10.0 * math.log10(float(maxval) * float(maxval) * float(pixels) / float(sse))
        got = capi.frame_metrics_psnr(sse, pixels, maxval)
        assert got == want or abs(got - want) <= 1e-12 * abs(want), (sse, pixels, maxval, got, want)
        assert got == R.psnr_db(sse, pixels, maxval) or abs(got - R.psnr_db(sse, pixels, maxval)) <= 1e-12 * abs(want)
    assert abs(capi.frame_metrics_psnr(100, 100, 255) - 20 * math.log10(255)) < 1e-12  # one grey level off everywhere: 48.13 dB


def brute_force(a, b, maxval):
    """The definition once more with no 4x4 blocks anywhere: every 8x8 window's sums straight from its 64 pixels, in Python integers"""
    H, W = a.shape
    bh, bw = H >> 2, W >> 2
    a = [[int(v) for v in row] for row in a]
    b = [[int(v) for v in row] for row in b]
    c1 = 0.01 * 0.01 * float(maxval) * float(maxval) * 64.0
    c2 = 0.03 * 0.03 * float(maxval) * float(maxval) * 64.0 * 63.0
    moments, terms = [], []
    for wy in range(bh - 1):
        for wx in range(bw - 1):
            s1 = s2 = ss = s12 = 0
            for y in range(4 * wy, 4 * wy + 8):
                for x in range(4 * wx, 4 * wx + 8):
                    p, q = a[y][x], b[y][x]
                    s1 += p
                    s2 += q
                    ss += p * p + q * q
                    s12 += p * q
            moments.append((s1, s2, ss, s12))
            vars_ = 64 * ss - s1 * s1 - s2 * s2  # exact integers, then one conversion: the reference converts first; both are exact below 2^53
            covar = 64 * s12 - s1 * s2
            terms.append((2.0 * float(s1 * s2) + c1) * (2.0 * float(covar) + c2) / ((float(s1 * s1 + s2 * s2) + c1) * (float(vars_) + c2)))
    sse = sum((p - q) ** 2 for ra, rb in zip(a, b) for p, q in zip(ra, rb))
    return moments, terms, sse


@pytest.mark.parametrize("h,w,maxval", [(8, 8, 255), (9, 11, 255), (21, 30, 255), (16, 19, 1023), (13, 24, 65535)])
def test_reference_agrees_with_a_brute_force_statement(h, w, maxval):
    rng = np.random.default_rng(h * w + maxval)
    b = rng.integers(0, maxval + 1, (h, w))
    a = np.clip(b + rng.integers(-maxval // 8, maxval // 8 + 1, (h, w)), 0, maxval)
    if maxval == 65535:
        a[:8, :8], b[:8, :8] = 0, 65535  # a window with every moment at its largest
    moments, terms, sse = brute_force(a, b, maxval)
    s1, s2, ss, s12 = R.window_moments(a, b)
    assert [tuple(int(v) for v in m) for m in zip(s1.ravel(), s2.ravel(), ss.ravel(), s12.ravel())] == moments  # exactly
    t = R.window_terms(s1, s2, ss, s12, maxval).ravel()
    assert len(t) == len(terms) == ((h >> 2) - 1) * ((w >> 2) - 1)
    assert max(abs(x - y) for x, y in zip(t, terms)) <= 1e-15
    m = R.plane_metrics(a, b, maxval)
    assert m["sse"] == sse and m["pixels"] == h * w and m["windows"] == len(terms)
    assert abs(m["ssim"] - math.fsum(terms) / len(terms)) <= 1e-15
    assert m["psnr_db"] == R.psnr_db(sse, h * w, maxval)


@pytest.mark.parametrize("maxval,shift,dtype", [(255, 0, np.uint8), (1023, 0, np.uint16), (1023, 6, np.uint16), (4095, 4, np.uint16), (65535, 0, np.uint16)])
def test_identical_frames_give_exactly_one(maxval, shift, dtype):
    rng = np.random.default_rng(maxval + shift)
    b = (rng.integers(0, maxval + 1, (2, 37, 53, 3)) << shift).astype(dtype)
    a = b.copy()
    if shift:
        a |= rng.integers(0, 1 << shift, a.shape).astype(dtype)  # bits below the shift take no part
    for r in R.frame_metrics(a, b, maxval, shift):
        assert r["sse"] == 0 and r["psnr_db"] == math.inf
        assert r["ssim"] == 1.0 and r["ssim_sum"] == float(r["windows"])  # exactly
    flat = np.full((1, 16, 16, 1), maxval << shift, dtype)
    assert R.frame_metrics(flat, flat, maxval, shift)[0]["ssim"] == 1.0
    zero = np.zeros_like(flat)
    assert R.frame_metrics(zero, zero, maxval, shift)[0]["ssim"] == 1.0


def test_ragged_edges_count_in_sse_only():
    rng = np.random.default_rng(3)
    b = rng.integers(0, 256, (1, 9, 11, 1)).astype(np.uint8)
    a = b.copy()
    a[0, 8, :, 0] ^= 1   # the ninth row and the last three columns lie past 4 * bh, 4 * bw
    a[0, :8, 8:, 0] ^= 1
    r = R.frame_metrics(a, b, 255)[0]
    assert r["sse"] == 11 + 8 * 3 and r["ssim"] == 1.0 and r["windows"] == 1 and r["pixels"] == 99


def test_device_free_refusals_of_the_host_mirror(built):
    """a null model, a null frame, null planes: -1 each, before anything is touched"""
    from shadernn_amd import host

    lib = host.lib()
    buf = np.zeros(64, np.uint8)
    rows = (host.FrameMetrics * 4)()
    assert lib.snn_model_reference_frame(None, buf.ctypes.data_as(C.c_void_p)) == -1
    assert lib.snn_model_reference_frame_planes(None, None, None, 3) == -1
    assert lib.snn_model_frame_metrics(None, rows, 4) == -1
    m = host.Model.__new__(host.Model)  # no device: only what metrics() reads before the library refuses
    m.h, m.batch = None, 1
    with pytest.raises(AssertionError, match="snn_model_frame_metrics refused"):
        m.metrics()
