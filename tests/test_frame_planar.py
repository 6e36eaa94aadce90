"""Planar 4:2:0 frames (I420 / I010) around the luma model, the CPU side: the two C-ABI plans and the host mirror's entry points are declared,
exported and bound; the structs keep their sizes; every refusal of snn_model_create12 and of the plane functions that needs no device; the argument
checks of host.Model; the build list and the documents name the unit; and the near-tie share of the reference (tests/planar_ref.py, which only
(de)interleaves and calls the references of the interleaved units) over exactly the shapes and seeds of the GPU sweeps stays under those modules' caps."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import planar_ref as P
import resample_ref
import rgb_cbcr_ref as RC
import yuv_rgb_ref as RY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I420, I010, NV12, P010 = 0x401, 0x501, 0x201, 0x301
RGB8, RGBA8, RGB16, RGBA16 = 3, 4, 0x103, 0x104


def _read(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return f.read()


def test_the_plans_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi

    header = re.sub(r"/\*.*?\*/", "", _read("include/snnhip.h"), flags=re.S)
    lib = C.CDLL(snn.load_library())
    for name in ("snnhip_yuv_rgb_planar_plan_create", "snnhip_rgb_cbcr_planar_plan_create"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    for f in (snn.yuv_rgb_planar_plan, snn.rgb_cbcr_planar_plan, capi.yuv_rgb_planar_plan, capi.rgb_cbcr_planar_plan):
        assert callable(f)
    assert C.sizeof(capi.YuvRgbDesc) == 12 * 4 and C.sizeof(capi.RgbCbcrDesc) == 9 * 4  # the descs the planar plans take are the earlier ones, untouched
    assert C.sizeof(capi.ChromaUpDesc) == 9 * 4 and C.sizeof(capi.PlaneFitDesc) == 10 * 4


def test_the_host_mirror_declares_and_binds(built):
    from shadernn_amd import host

    mirror = re.sub(r"/\*.*?\*/", "", _read("include/snn_c.h"), flags=re.S)
    for name in ("snn_model_create12", "snn_model_upload_frame_planes", "snn_model_download_frame_planes"):
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert name in host.SIGNATURES and hasattr(host.lib(), name), name
    assert "snn_planar_io" in mirror and re.search(r"SNN_IO_I420\s*=\s*0x401", mirror) and re.search(r"SNN_IO_I420_16\s*=\s*0x501", mirror)
    assert C.sizeof(host.PlanarIO) == 40
    assert [n for n, _ in host.PlanarIO._fields_] == ["in_format", "out_format", "maxval", "shift", "siting", "range", "kr", "kb", "out_w", "out_h"]
    assert C.sizeof(host.VideoIO) == 8 * 4 and C.sizeof(host.FitIO) == 10 * 4 and C.sizeof(host.VideoRgbIO) == 8 * 4 and C.sizeof(host.EncodeIO) == 6 * 4
    assert host.VIDEO_FORMATS["I420"] == (I420, 255, 0) and host.VIDEO_FORMATS["I010"] == (I010, 1023, 0)
    assert host.VIDEO_FORMATS["NV12"] == (NV12, 255, 0) and host.VIDEO_FORMATS["P010"] == (P010, 1023, 6)
    for f in ("upload_planes", "download_planes"):
        assert callable(getattr(host.Model, f))


def _create12(io, w=32, h=24, in_c=1, batch=1):
    from shadernn_amd import host

    handle = C.c_void_p()
    rc = host.lib().snn_model_create12(b"/nonexistent/model.json", 0, w, h, in_c, 0, 1, 0, 0, 0, batch, None if io is None else C.byref(io), C.byref(handle))
    assert not handle.value
    return rc


def _io(in_format=I420, out_format=I420, maxval=255, shift=0, siting=1, rng=0, kr=0.299, kb=0.114, out_w=0, out_h=0):
    from shadernn_amd import host

    return host.PlanarIO(in_format, out_format, maxval, shift, siting, rng, kr, kb, out_w, out_h)


def test_create12_refuses_without_a_device(built):
    """everything that returns before the model file is opened (the file does not exist: a call that got that far would not return -1 but -2 or
    abort); what needs the model's r is tests/test_frame_planar_host_gpu.py's"""
    assert _create12(None) == -1
    good = _io()
    assert _create12(good, w=31) == -1 and _create12(good, h=23) == -1 and _create12(good, w=0) == -1  # odd or empty extents
    assert _create12(good, in_c=3) == -1 and _create12(good, batch=0) == -1 and _create12(good, batch=-1) == -1
    pairs = [(0, I420), (1, I420), (NV12, NV12), (NV12, I420), (I420, NV12), (I420, I010), (I010, I420), (I420, RGB16), (I420, RGBA16), (I010, RGB8), (I010, RGBA8),
             (I420, 1), (I420, 0), (RGB8, NV12), (RGB8, I010), (RGBA8, RGBA8), (RGB16, I010), (RGB16, I420)]
    for a, b in pairs:  # formats that do not pair up
        assert _create12(_io(a, b, 1023 if a in (I010, RGB16) else 255)) == -1, (hex(a), hex(b))
    for fmt, maxval, shift in ((I420, 256, 0), (I420, 0, 0), (I420, 127, 0), (I420, 1023, 0), (I420, 255, 1), (I420, 255, -1), (I010, 65535, 0), (I010, 8191, 0),
                               (I010, 1000, 0), (I010, 254, 0), (I010, 1023, 7), (I010, 1023, 16), (I010, 4095, 5)):  # depth and shift, on the planar and the RGB path
        assert _create12(_io(fmt, fmt, maxval, shift)) == -1, (hex(fmt), maxval, shift)
        assert _create12(_io(fmt, RGB8 if fmt == I420 else RGB16, maxval, shift)) == -1, (hex(fmt), maxval, shift)
    for a, b in ((I420, I420), (I420, RGB8), (I010, RGBA16), (RGB8, I420), (RGBA8, I420)):  # siting and range on every path
        mv = 1023 if a == I010 else 255
        assert _create12(_io(a, b, mv, siting=2)) == -1 and _create12(_io(a, b, mv, siting=-1)) == -1, (hex(a), hex(b))
        assert _create12(_io(a, b, mv, rng=2)) == -1 and _create12(_io(a, b, mv, rng=-1)) == -1, (hex(a), hex(b))
    for a, b in ((I420, RGB8), (I420, RGBA8), (RGB8, I420), (RGBA8, I420)):  # the matrix of an RGB end
        assert _create12(_io(a, b, kr=0.0)) == -1 and _create12(_io(a, b, kb=-0.1)) == -1 and _create12(_io(a, b, kr=0.7, kb=0.3)) == -1, (hex(a), hex(b))
    for a, b, mv in ((I420, RGB8, 255), (I420, RGBA8, 255), (I010, RGB16, 1023), (RGB8, I420, 255)):  # a fitted size together with an RGB end
        assert _create12(_io(a, b, mv, out_w=48, out_h=36)) == -1 and _create12(_io(a, b, mv, out_w=48)) == -1 and _create12(_io(a, b, mv, out_h=36)) == -1, (hex(a), hex(b))
    for ow, oh in ((47, 36), (48, 35), (0, 36), (48, 0), (1, 1), (-2, 36), (14, 36), (130, 36), (48, 10), (48, 98)):  # the fitted size's own rules (snn_model_create11's)
        assert _create12(_io(out_w=ow, out_h=oh)) == -1, (ow, oh)
        assert _create12(_io(I010, I010, 1023, out_w=ow, out_h=oh)) == -1, (ow, oh)


def test_the_plane_functions_refuse_null_arguments(built):
    from shadernn_amd import host

    y, c = np.zeros((4, 4), np.uint8), np.zeros((2, 2), np.uint8)
    planes = (C.c_void_p * 3)(y.ctypes.data, c.ctypes.data, c.ctypes.data)
    pitch = (C.c_int * 3)(4, 2, 2)
    for fn in (host.lib().snn_model_upload_frame_planes, host.lib().snn_model_download_frame_planes):
        assert fn(None, planes, pitch, 3) == -1
        assert fn(None, None, pitch, 3) == -1
        assert fn(None, planes, None, 3) == -1


def test_host_model_argument_checks(built):
    from shadernn_amd import host

    path = "/nonexistent/model.json"
    for video in ("I420", "I010", "NV12"):  # out_size goes with video= alone, for the planar formats as for NV12
        with pytest.raises(AssertionError, match="out_size"):
            host.Model(path, 32, 24, 1, video=video, video_out="RGB8" if video != "I010" else "RGB16", out_size=(48, 36))
    for video_out in ("I420", "NV12"):
        with pytest.raises(AssertionError, match="out_size"):
            host.Model(path, 32, 24, 1, colour="RGB8", video_out=video_out, out_size=(48, 36))
    with pytest.raises(AssertionError, match="RGB16 / RGBA16"):
        host.Model(path, 32, 24, 1, video="I010", video_out="RGB8")
    with pytest.raises(AssertionError, match="RGB8 / RGBA8"):
        host.Model(path, 32, 24, 1, video="I420", video_out="RGBA16")
    with pytest.raises(AssertionError, match="RGB8 / RGBA8"):
        host.Model(path, 32, 24, 1, video="NV12", video_out="RGB16")  # the existing spelling keeps its message
    with pytest.raises(AssertionError, match="video_out"):
        host.Model(path, 32, 24, 1, colour="RGB8", video_out="I010")  # no 16-bit RGB -> I010
    with pytest.raises(AssertionError, match="colour"):
        host.Model(path, 32, 24, 1, video="I420", colour="RGB8")
    with pytest.raises(AssertionError, match="video_range"):
        host.Model(path, 32, 24, 1, video="I420", video_range="studio")
    with pytest.raises(AssertionError, match="siting"):
        host.Model(path, 32, 24, 1, video="I420", siting="top")
    with pytest.raises(AssertionError, match="kr"):
        host.Model(path, 32, 24, 1, video="I420", video_out="RGB8", kr=0.0)
    with pytest.raises(AssertionError):
        host.Model(path, 31, 24, 1, video="I420")  # snn_model_create12 returns -1: an odd extent
    with pytest.raises(KeyError):
        host.Model(path, 32, 24, 1, video="YV12")  # the caller swaps the planes instead


def test_the_build_list_and_the_documents_name_the_unit():
    build = _read("__graft_entry__.py")
    assert '"frame_yuv_rgb.hip"' in build and '"frame_rgb_cbcr.hip"' in build  # the planar kernels live beside their interleaved siblings
    assert "yuv_rgb_planar_kernel" in _read("shadernn_amd/csrc/frame_yuv_rgb.hip") and "rgb_cbcr_planar_kernel" in _read("shadernn_amd/csrc/frame_rgb_cbcr.hip")
    readme, design, integration = _read("README.md"), _read("DESIGN.md"), _read("INTEGRATION.md")
    assert "4.19" in design and "yuv_rgb_planar_kernel" in design and "rgb_cbcr_planar_kernel" in design and "snn_model_create12" in design
    assert "tools/planar_host_check.cpp" in readme and "tests/planar_ref.py" in readme and "I420" in readme
    assert "snn_model_create12" in integration and "snn_model_upload_frame_planes" in integration


def test_planar_ref_only_reorders_samples():
    rng = np.random.default_rng(3)
    for dt in (np.uint8, np.uint16):
        c = rng.integers(0, 256, size=(3, 5, 7, 2)).astype(dt)
        p = P.deinterleave(c)
        assert p.shape == (6, 5, 7, 1) and p.dtype == dt
        np.testing.assert_array_equal(p[0, :, :, 0], c[0, :, :, 0])  # plane 2n is Cb of image n
        np.testing.assert_array_equal(p[1, :, :, 0], c[0, :, :, 1])  # plane 2n + 1 its Cr
        np.testing.assert_array_equal(p[4, :, :, 0], c[2, :, :, 0])
        np.testing.assert_array_equal(P.interleave(p), c)
    yhi, planes = P.yuv_frame(2, 5, 7, 2, 255, 0, np.uint8, seed=9, disjoint=True)
    assert yhi.shape == (2, 20, 28, 1) and planes.shape == (4, 5, 7, 1)
    assert (planes[0::2] < 128).all() and (planes[1::2] > 128).all()
    u = rng.integers(0, 256, size=(4, 5, 7, 1)).astype(np.uint8)  # channels never mix: the planes go through the C = 2 references as they would alone
    np.testing.assert_array_equal(P.up_values(u, 2, "left"), __import__("chroma_ref").up_values(u, 2, "left"))
    np.testing.assert_array_equal(P.fit_values(u, 7, 9, "left"), __import__("fit_ref").fit_values(u, 7, 9, "left"))


def _tie_fraction(values, eps):
    ties = sum(int(resample_ref.near_tie(v, eps).sum()) for v in values)
    return ties / max(sum(v.size for v in values), 1)


@pytest.mark.parametrize("depth", P.DEPTHS, ids=P.DEPTH_IDS)
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_near_ties_of_the_yuv_rgb_planar_sweeps_stay_under_the_cap(r, depth):
    """the frames of tests/test_frame_planar_gpu.py::test_yuv_rgb_planar_matches_the_reference (both C share them), on the reference alone"""
    container, maxval, shift = depth
    values = []
    for siting, rng, (n, h, w), seed in P.yuv_cases(r, container, maxval):
        yhi, planes = P.yuv_frame(n, h, w, r, maxval, shift, P.np_dtype(container), seed)
        values.append(P.yuv_values(yhi, planes, r, siting, rng, maxval, shift))
    frac = _tie_fraction(values, RY.EPS[maxval])
    print("yuv_rgb_planar %s maxval=%d r=%d: near ties %.3f %% of %d values" % (container, maxval, r, 100 * frac, sum(v.size for v in values)))
    assert frac <= RY.MAX_TIE_FRACTION


@pytest.mark.parametrize("depth", P.DEPTHS, ids=P.DEPTH_IDS)
def test_near_ties_of_the_other_yuv_rgb_planar_sweeps_stay_under_the_cap(depth):
    """the clamp sweep and the disjoint-range sweep of the GPU file"""
    container, maxval, shift = depth
    for r, shapes, kw, ranges in [(r, [(1, 5, 7), (2, 9, 41)], dict(whole_range=True), P.RANGES) for r in (1, 2, 3)] + \
                                 [(r, [(2, 5, 7), (2, 3, 131)], dict(disjoint=True), ["full"]) for r in (1, 2)]:
        values = []
        for siting, rng, (n, h, w), seed in P.yuv_cases(r, container, maxval, shapes, ranges=ranges):
            yhi, planes = P.yuv_frame(n, h, w, r, maxval, shift, P.np_dtype(container), seed, **kw)
            values.append(P.yuv_values(yhi, planes, r, siting, rng, maxval, shift))
        assert _tie_fraction(values, RY.EPS[maxval]) <= RY.MAX_TIE_FRACTION, (r, kw)


@pytest.mark.parametrize("C_", [3, 4])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_near_ties_of_the_rgb_cbcr_planar_sweeps_stay_under_the_cap(r, C_):
    values = [RC.values(RC.frame(seed, n, h, w, C_), r, siting, rng) for siting, rng, (n, h, w), seed in P.cbcr_cases(r, C_)]
    frac = _tie_fraction(values, RC.EPS)
    print("rgb_cbcr_planar r=%d c=%d: near ties %.3f %% of %d values" % (r, C_, 100 * frac, sum(v.size for v in values)))
    assert frac <= RC.MAX_TIE_FRACTION
    if C_ == 3:
        prim = [RC.values(RC.frame(seed, n, h, w, 3, primaries=True), r, siting, rng) for siting, rng, (n, h, w), seed in P.cbcr_cases(r, 3, [(1, 6, 8), (2, 10, 42)])]
        assert _tie_fraction(prim, RC.EPS) <= RC.MAX_TIE_FRACTION


def test_eps_leaves_four_times_the_measured_fp32_distance():
    """the planar kernels evaluate the interleaved kernels' fp32 expression: their references' measured distance, re-measured here"""
    for maxval, shift in ((255, 0), (1023, 0), (4095, 0)):
        d = RY.measured_distance(maxval, shift)
        print("yuv_rgb maxval %d: fp32 to float64 distance %.2e, eps %.0e" % (maxval, d, RY.EPS[maxval]))
        assert RY.EPS[maxval] >= 4 * d
    d = RC.measured_distance()
    print("rgb_cbcr: fp32 to float64 distance %.2e, eps %.0e" % (d, RC.EPS))
    assert RC.EPS >= 4 * d
