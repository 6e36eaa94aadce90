"""NV12 / P010 frames to RGB behind a luma-only model, the CPU side: the entry points are declared, exported and bound; the 4:2:0 tap table and the
matrix coefficients against the float64 formulas; properties of the float64 reference itself (tests/yuv_rgb_ref.py) and the measured fp32 distance
that sets its eps; the refusals of the host mirror and of host.Model that need no device; the build list and the documents name the new unit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yuv_rgb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = [(255, 0, np.uint8), (1023, 6, np.uint16), (1023, 0, np.uint16), (4095, 0, np.uint16)]  # (maxval, shift, container)


def _read(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi, host

    header = re.sub(r"/\*.*?\*/", "", _read("include/snnhip.h"), flags=re.S)
    lib = C.CDLL(snn.load_library())
    for name in ("snnhip_yuv_rgb_plan_create", "snnhip_bicubic_taps_420", "snnhip_yuv_rgb_coefficients"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    assert "snnhip_yuv_rgb_desc" in header and "SNNHIP_RANGE_LIMITED 0" in header and "SNNHIP_RANGE_FULL 1" in header
    mirror = re.sub(r"/\*.*?\*/", "", _read("include/snn_c.h"), flags=re.S)
    assert re.search(r"\bsnn_model_create9\s*\(", mirror) and "snn_video_rgb_io" in mirror
    assert "snn_model_create9" in host.SIGNATURES and hasattr(host.lib(), "snn_model_create9")
    for f in (snn.yuv_rgb_plan, snn.bicubic_taps_420, snn.yuv_rgb_coefficients):
        assert callable(f)


def test_struct_layouts():
    from shadernn_amd import capi, host

    assert [n for n, _ in capi.YuvRgbDesc._fields_] == ["N", "H", "W", "C", "r", "dtype", "maxval", "shift", "siting", "range", "kr", "kb"]
    assert C.sizeof(capi.YuvRgbDesc) == 12 * 4
    assert [n for n, _ in host.VideoRgbIO._fields_] == ["in_format", "out_format", "maxval", "shift", "siting", "range", "kr", "kb"]
    assert C.sizeof(host.VideoRgbIO) == 8 * 4
    # the earlier structs keep their layout
    assert C.sizeof(capi.ChromaUpDesc) == 9 * 4 and C.sizeof(host.VideoIO) == 8 * 4 and C.sizeof(host.ColourIO) == 7 * 4
    assert C.sizeof(host.FrameIO) == 18 * 4 and C.sizeof(host.FrameIO2) == 21 * 4


# ---- the reference's own properties ----

def test_reference_neutral_chroma_gives_grey():
    for maxval, shift, dt in DEPTHS:
        k = (maxval + 1) // 256
        for rng in (R.LIMITED, R.FULL):
            for r in (1, 2, 3):
                yhi, cbcr = R.frame(2, 3, 5, r, maxval, shift, dt, seed=r, whole_range=True)
                cbcr[...] = (128 * k) << shift
                v = R.values(yhi, cbcr, r, R.LEFT, rng, maxval, shift)
                assert (v[..., 0] == v[..., 1]).all() and (v[..., 1] == v[..., 2]).all()  # the chroma terms are exactly 0
                out = R.rgb(yhi, cbcr, r, 4, R.LEFT, rng, maxval, shift)
                assert (out[..., 0] == out[..., 1]).all() and (out[..., 1] == out[..., 2]).all() and (out[..., 3] == maxval << shift).all()
                c = R.coefficients(maxval, rng).astype(np.float64)
                yl = c[2] * ((yhi.astype(np.int64) >> shift)[..., 0] - c[0])
                np.testing.assert_array_equal(out[..., 0], R.quantise(yl, maxval, shift, dt))


def test_reference_constant_planes_stay_constant():
    for maxval, shift, dt in DEPTHS:
        k = (maxval + 1) // 256
        for siting in (R.CENTRE, R.LEFT):
            for r in (1, 2, 3, 4):
                yhi = np.full((1, 2 * r * 3, 2 * r * 4, 1), (100 * k) << shift, dt)
                cbcr = np.empty((1, 3, 4, 2), dt)
                cbcr[..., 0], cbcr[..., 1] = (100 * k) << shift, (150 * k) << shift
                v = R.values(yhi, cbcr, r, siting, R.LIMITED, maxval, shift)
                assert np.ptp(v.reshape(-1, 3), axis=0).max() < 1e-9 * maxval  # constant chroma planes give constant chroma terms
                out = R.rgb(yhi, cbcr, r, 3, siting, R.LIMITED, maxval, shift)
                assert (out == out[0, 0, 0]).all()


def test_reference_a_chroma_ramp_stays_on_its_line_over_output_luma_position():
    """A ramp Cb = a*i + b over chroma index i is a line over low-resolution luma position L: left-sited sample i sits at L = 2i, a centred one at
    L = 2i + 0.5.  Output luma column X sits at L = (X + 0.5) / r - 0.5, and a cubic reproduces a line, so away from the edges B - yl is exactly
    cbu * (line(L) - Coff).  This pins the sign and the size of the siting offset (0.25 against 0.5 of a chroma sample)."""
    w, a, b = 24, 4.0, 60.0
    ramp = (a * np.arange(w) + b).astype(np.uint8)
    cbcr = np.empty((1, 4, w, 2), np.uint8)
    cbcr[..., 0] = ramp[None, None, :]
    cbcr[..., 1] = 128
    c = R.coefficients(255, R.FULL).astype(np.float64)
    for r in (1, 2, 3, 4):
        yhi = np.full((1, 2 * r * 4, 2 * r * w, 1), 90, np.uint8)
        X = np.arange(2 * r * w, dtype=np.float64)
        L = (X + 0.5) / r - 0.5
        yl = c[2] * (90.0 - c[0])
        edge = 2 * 2 * r
        for siting, index in ((R.LEFT, L / 2.0), (R.CENTRE, (L - 0.5) / 2.0)):
            v = R.values(yhi, cbcr, r, siting, R.FULL)
            want = yl + c[4] * (a * index + b - c[1])
            for row in (0, 2 * r * 4 - 1):
                np.testing.assert_allclose(v[0, row, edge:-edge, 2], want[edge:-edge], atol=1e-9)
                np.testing.assert_allclose(v[0, row, edge:-edge, 0], yl, atol=1e-12)  # Cr is neutral: R = yl
        diff = R.values(yhi, cbcr, r, R.LEFT, R.FULL)[0, 0, edge:-edge, 2] - R.values(yhi, cbcr, r, R.CENTRE, R.FULL)[0, 0, edge:-edge, 2]
        np.testing.assert_allclose(diff, c[4] * a * 0.25, atol=1e-9)  # the two sitings are a quarter of a chroma sample apart


def _ycbcr_of(rgb, kr, kb, rng, maxval):
    """Analogue R'G'B' in [0, 1] -> (Y, Cb, Cr) codes, unrounded"""
    k = (maxval + 1) / 256.0
    r, g, b = rgb
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    pb, pr = 0.5 * (b - y) / (1.0 - kb), 0.5 * (r - y) / (1.0 - kr)
    if rng == R.LIMITED:
        return 16 * k + 219 * k * y, 128 * k + 224 * k * pb, 128 * k + 224 * k * pr
    return maxval * y, 128 * k + maxval * pb, 128 * k + maxval * pr


@pytest.mark.parametrize("matrix", [R.BT601, R.BT709], ids=["bt601", "bt709"])
def test_reference_primaries_map_where_they_should(matrix):
    kr, kb = matrix
    for rng in (R.LIMITED, R.FULL):
        for rgb in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 0, 0), (1, 1, 0), (0.25, 0.5, 0.75)):
            y, cb, cr = _ycbcr_of(rgb, kr, kb, rng, 255)
            c = R.coefficients(255, rng, kr, kb).astype(np.float64)
            yl = c[2] * (y - c[0])
            got = np.array([yl + c[3] * (cr - c[1]), yl - (c[5] * (cr - c[1]) + c[6] * (cb - c[1])), yl + c[4] * (cb - c[1])])
            np.testing.assert_allclose(got, 255.0 * np.array(rgb), atol=2e-4)  # (the coefficients are float32 values)
    # through the whole reference: the limited-range BT.601 codes of pure red, as constant planes (the familiar 81 / 90 / 240 after rounding)
    y, cb, cr = (int(round(v)) for v in _ycbcr_of((1, 0, 0), *R.BT601, R.LIMITED, 255))
    assert (y, cb, cr) == (81, 90, 240)
    yhi = np.full((1, 8, 8, 1), y, np.uint8)
    cbcr = np.empty((1, 2, 2, 2), np.uint8)
    cbcr[..., 0], cbcr[..., 1] = cb, cr
    out = R.rgb(yhi, cbcr, 2, 3, R.LEFT, R.LIMITED)
    assert (np.abs(out.astype(int) - np.array([255, 0, 0])) <= 1).all(), out[0, 0, 0]


def test_reference_eps_is_at_least_four_times_the_measured_fp32_distance_and_the_recipe_holds():
    for maxval, shift, dt in ((255, 0, np.uint8), (1023, 6, np.uint16), (4095, 0, np.uint16)):
        d = R.measured_distance(maxval, shift, dt)
        print("maxval %d: fp32-to-float64 distance %.3g, eps %.3g" % (maxval, d, R.EPS[maxval]))
        assert 0.0 < d <= R.MEASURED_DISTANCE[maxval] and R.EPS[maxval] >= 4.0 * R.MEASURED_DISTANCE[maxval]
        for r in (1, 2, 3, 4):
            yhi, cbcr = R.frame(1, 12, 16, r, maxval, shift, dt, seed=40 + r)
            for rng in (R.LIMITED, R.FULL):
                for siting in (R.CENTRE, R.LEFT):
                    v = R.values(yhi, cbcr, r, siting, rng, maxval, shift)
                    assert R.near_tie(v, R.EPS[maxval]).mean() <= R.MAX_TIE_FRACTION
                    assert R.clamp_fraction(v, maxval) < R.MAX_CLAMP_FRACTION
        yhi, cbcr = R.frame(1, 12, 16, 2, maxval, shift, dt, seed=3, whole_range=True)  # the clamp sweep does clamp
        assert R.clamp_fraction(R.values(yhi, cbcr, 2, R.LEFT, R.LIMITED, maxval, shift), maxval) > 0.1


# ---- the host-side tables ----

def test_taps_420_are_the_float64_formula_rounded_to_fp32(built):
    from shadernn_amd import capi

    for siting in ("centre", "left"):
        for r in (1, 2, 3, 4):
            got, base = capi.bicubic_taps_420(r, siting)
            want, want_base = R.taps(r, siting)
            assert got.shape == (2 * r, 4) and got.dtype == np.float32
            assert got.tobytes() == want.astype(np.float32).tobytes(), (siting, r, got, want)  # bit for bit
            np.testing.assert_array_equal(base, want_base)
            np.testing.assert_array_equal(base, [int(np.floor((p + 0.5) / (2 * r) - R.SITING_OFFSET[siting])) for p in range(2 * r)])
            assert set(base.tolist()) <= {-1, 0}
            for row in got:  # the fp32 weights of a phase sum to 1 within one ulp of 1
                s = float(np.sum(row.astype(np.float64)))
                assert abs(s - 1.0) <= float(np.spacing(np.float32(1.0))), (siting, r, row, s)
    # centred chroma resampled 2r-fold is the merge kernel's table at 2r (r = 1, 2); left-sited differs from chroma_up's left phase
    for r in (1, 2):
        assert capi.bicubic_taps_420(r, "centre")[0].tobytes() == capi.bicubic_taps(2 * r).tobytes()
    assert capi.bicubic_taps_420(1, "left")[0].tobytes() != capi.bicubic_taps_sited(2, "left")[0].tobytes()


def test_taps_420_refuses_bad_arguments(built):
    from shadernn_amd import capi

    w = np.zeros(32, np.float32)
    base = (C.c_int * 8)()
    fn = capi.lib().snnhip_bicubic_taps_420
    for r, siting, cap in ((0, 1, 32), (5, 1, 32), (3, 1, 23), (4, 0, 31), (2, 2, 32), (2, -1, 32)):
        assert fn(r, siting, capi._fptr(w), base, cap) == capi.E_INVALID
        assert b"bicubic_taps_420" in capi.lib().snnhip_last_error()
    assert fn(4, 0, capi._fptr(w), base, 31) == capi.E_INVALID and b"room for 31 floats, 32 needed" in capi.lib().snnhip_last_error()  # the capacity refusal
    assert fn(2, 1, None, base, 32) == capi.E_INVALID
    assert fn(2, 1, capi._fptr(w), None, 32) == capi.E_INVALID
    assert fn(4, 1, capi._fptr(w), base, 32) == capi.OK and fn(3, 1, capi._fptr(w), base, 24) == capi.OK


def test_coefficients_are_the_float64_formula_rounded_to_fp32(built):
    from shadernn_amd import capi

    for maxval in (255, 1023, 4095):
        for rng in ("limited", "full"):
            for kr, kb in (R.BT601, R.BT709, (0.2627, 0.0593)):
                got = capi.yuv_rgb_coefficients(maxval, rng, kr, kb)
                assert got.tobytes() == R.coefficients(maxval, rng, kr, kb).tobytes(), (maxval, rng, kr, kb, got)
    k = capi.yuv_rgb_coefficients(255, "limited")
    np.testing.assert_allclose(k, [16, 128, 1.164384, 1.596027, 2.017232, 0.812968, 0.391762], rtol=1e-6)  # the familiar BT.601 numbers
    out = np.zeros(7, np.float32)
    fn = capi.lib().snnhip_yuv_rgb_coefficients
    for args in ((256, 0, 0.299, 0.114, 7), (255, 2, 0.299, 0.114, 7), (255, 0, 0.0, 0.114, 7), (255, 0, 0.6, 0.4, 7), (255, 0, 0.299, 0.114, 6)):
        assert fn(*args[:4], capi._fptr(out), args[4]) == capi.E_INVALID
        assert b"yuv_rgb_coefficients" in capi.lib().snnhip_last_error()


# ---- refusals that need no device ----

def test_host_mirror_refusals_that_need_no_device(built):
    """Each of these returns -1 before the model file is opened or a device context is made: the path does not exist."""
    from shadernn_amd import host

    h = C.c_void_p()
    path = os.path.join(ROOT, "no", "such", "model.json").encode()

    def create9(io, w=32, hh=24, in_c=1, batch=1):
        return host.lib().snn_model_create9(path, 0, w, hh, in_c, 0, 1, 0, 0, 0, batch, C.byref(io) if io is not None else None, C.byref(h))

    def io(fmt=0x201, out=3, maxval=255, shift=0, siting=1, rng=0, kr=0.299, kb=0.114):
        return host.VideoRgbIO(fmt, out, maxval, shift, siting, rng, kr, kb)

    assert create9(None) == -1                                          # a null struct
    for fmt in (0, 1, 3, 0x101, 0x202):                                 # float, R8, RGB8, R16, an unknown value as the input format
        assert create9(io(fmt=fmt)) == -1
    for out in (0, 1, 0x103, 0x104, 0x201):                             # an 8-bit input pairs with RGB8 / RGBA8 only
        assert create9(io(out=out)) == -1
    for out in (3, 4, 0x101, 0x301):                                    # ... a 16-bit one with RGB16 / RGBA16 only
        assert create9(io(fmt=0x301, out=out, maxval=1023, shift=6)) == -1
    assert create9(io(), in_c=3) == -1                                  # not a one-channel model
    assert create9(io(), w=31) == -1 and create9(io(), hh=23) == -1     # odd extents: no 4:2:0 plane
    assert create9(io(fmt=0x301, out=0x103, maxval=65535)) == -1        # above 12 bits
    assert create9(io(fmt=0x301, out=0x103, maxval=1023, shift=7)) == -1  # does not fit the container
    assert create9(io(maxval=1023)) == -1                               # ... nor ten bits a byte
    assert create9(io(maxval=127)) == -1 and create9(io(fmt=0x301, out=0x103, maxval=1000)) == -1  # maxval + 1 is no multiple of 256
    assert create9(io(shift=1)) == -1
    assert create9(io(siting=2)) == -1
    assert create9(io(rng=2)) == -1 and create9(io(rng=-1)) == -1
    assert create9(io(kr=0.0)) == -1 and create9(io(kb=0.0)) == -1 and create9(io(kr=0.7, kb=0.3)) == -1
    assert create9(io(), batch=0) == -1
    assert h.value is None


def test_host_model_argument_checks(built):
    from shadernn_amd import host

    path = os.path.join(ROOT, "no", "such", "model.json")
    for kw in (dict(video_out="RGB8"),                                   # no video=
               dict(video="NV12", video_out="RGB16"), dict(video="P010", video_out="RGBA8"),  # the formats do not pair up
               dict(video="NV12", video_out="BGR8"),
               dict(video="NV12", video_out="RGB8", video_range="studio"),
               dict(video="NV12", video_out="RGB8", siting="right"),
               dict(video="NV12", video_out="RGB8", kr=0.0),
               dict(video="NV12", video_out="RGB8", kr=0.8, kb=0.3),
               dict(video="NV12", video_out="RGB8", output_format="R8")):
        with pytest.raises(AssertionError):
            host.Model(path, 32, 24, 1, **kw)


def test_the_unit_is_built_and_documented():
    import sys

    sys.path.insert(0, ROOT)
    import __graft_entry__ as g

    assert "frame_yuv_rgb.hip" in g.HIP_SOURCES
    assert os.path.exists(os.path.join(g.CSRC, "frame_yuv_rgb.hip")) and os.path.exists(os.path.join(g.CSRC, "frame_yuv_rgb.h"))
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "frame_yuv_rgb" in _read(doc) or "yuv_rgb" in _read(doc), doc
    assert "4.15" in _read("DESIGN.md")
    assert "Limited range is not offered." not in _read("include/snnhip.h")  # the colour contract now points at the video plan
