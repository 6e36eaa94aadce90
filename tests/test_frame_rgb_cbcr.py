"""RGB frames in, NV12 out around a luma-only model, the CPU side: the entry points are declared, exported and bound; the tap table of the upscaled
frame's chroma grid and the two chroma scales against the float64 formulas; every refusal of the two host-only functions; properties of the float64
reference itself (tests/rgb_cbcr_ref.py), its near-tie share over the frames of the GPU sweep and its measured fp32 distance; the refusals of the host
mirror and of host.Model that need no device; the build list and the documents name the new unit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rgb_cbcr_ref as R
import yuv_rgb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi, host

    header = re.sub(r"/\*.*?\*/", "", _read("include/snnhip.h"), flags=re.S)
    lib = C.CDLL(snn.load_library())
    for name in ("snnhip_rgb_cbcr_plan_create", "snnhip_bicubic_taps_rgb420", "snnhip_rgb_cbcr_coefficients"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    assert "snnhip_rgb_cbcr_desc" in header
    mirror = re.sub(r"/\*.*?\*/", "", _read("include/snn_c.h"), flags=re.S)
    assert re.search(r"\bsnn_model_create10\s*\(", mirror) and "snn_encode_io" in mirror
    assert "snn_model_create10" in host.SIGNATURES and hasattr(host.lib(), "snn_model_create10")
    for f in (snn.rgb_cbcr_plan, snn.bicubic_taps_rgb420, snn.rgb_cbcr_coefficients):
        assert callable(f)


def test_struct_layouts():
    from shadernn_amd import capi, host

    assert [n for n, _ in capi.RgbCbcrDesc._fields_] == ["N", "H", "W", "C", "r", "siting", "range", "kr", "kb"]
    assert C.sizeof(capi.RgbCbcrDesc) == 9 * 4
    assert [n for n, _ in host.EncodeIO._fields_] == ["in_format", "out_format", "siting", "range", "kr", "kb"]
    assert C.sizeof(host.EncodeIO) == 6 * 4
    # the earlier structs keep their layout
    assert C.sizeof(capi.YuvRgbDesc) == 12 * 4 and C.sizeof(capi.ChromaUpDesc) == 9 * 4
    assert C.sizeof(host.VideoRgbIO) == 8 * 4 and C.sizeof(host.VideoIO) == 8 * 4 and C.sizeof(host.ColourIO) == 7 * 4


# ---- the host-side tables ----

def test_taps_rgb420_are_the_float64_formula_rounded_to_fp32(built):
    from shadernn_amd import capi

    for siting in ("centre", "left"):
        for r in (2, 3, 4):
            P, S = R.pattern(r)
            got, base = capi.bicubic_taps_rgb420(r, siting)
            want, want_base = R.taps(r, siting)
            assert (P, S) == {2: (1, 1), 3: (3, 2), 4: (2, 1)}[r]
            assert got.shape == (P, 4) and got.dtype == np.float32
            assert got.tobytes() == want.astype(np.float32).tobytes(), (siting, r, got, want)  # bit for bit
            np.testing.assert_array_equal(base, want_base)
            np.testing.assert_array_equal(base, [int(np.floor((2 * p + R.LEAD[siting]) / r - 0.5)) for p in range(P)])
            assert set(base.tolist()) <= {-1, 0, 1}
            for row in got:  # the fp32 weights of a phase sum to 1 within one ulp of 1
                assert abs(float(np.sum(row.astype(np.float64))) - 1.0) <= float(np.spacing(np.float32(1.0))), (siting, r, row)
    # the checkpoints of the contract
    w, b = capi.bicubic_taps_rgb420(2, "centre")  # the identity: s = 0
    assert b.tolist() == [0] and w.tolist() == [[0.0, 1.0, 0.0, 0.0]]
    w, b = capi.bicubic_taps_rgb420(2, "left")    # a quarter-pixel shift: s = -0.25, base -1, t = 0.75
    assert b.tolist() == [-1]
    np.testing.assert_array_equal(w[0], R.keys(np.array([1.75, 0.75, 0.25, 1.25])).astype(np.float32))
    w, b = capi.bicubic_taps_rgb420(3, "left")    # phase 2 is the identity on input 2x' + 1
    assert b.tolist() == [-1, 0, 1] and w[2].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert capi.bicubic_taps_rgb420(4, "centre")[0].tobytes() == capi.bicubic_taps(2).tobytes()  # two outputs per pixel, centred: the x2 merge table


def test_the_three_earlier_tap_tables_are_what_they_were(built):
    """The filler behind all four tables was generalised (a step per output, base 1): the earlier three still are the float64 formula, bit for bit."""
    from shadernn_amd import capi
    import chroma_ref
    import colour_ref

    for r in (1, 2, 3, 4):
        assert capi.bicubic_taps(r).tobytes() == colour_ref.taps(r).astype(np.float32).tobytes()
        for siting in ("centre", "left"):
            w, b = capi.bicubic_taps_sited(r, siting)
            want, want_b = chroma_ref.taps(r, siting)
            assert w.tobytes() == want.astype(np.float32).tobytes() and b.tolist() == want_b.tolist()
            w, b = capi.bicubic_taps_420(r, siting)
            want, want_b = yuv_rgb_ref.taps(r, siting)
            assert w.tobytes() == want.astype(np.float32).tobytes() and b.tolist() == want_b.tolist()


def test_taps_rgb420_refuses_bad_arguments(built):
    from shadernn_amd import capi

    w = np.zeros(12, np.float32)
    base = (C.c_int * 3)()
    fn = capi.lib().snnhip_bicubic_taps_rgb420
    for r, siting, cap in ((0, 1, 12), (1, 1, 12), (5, 1, 12), (-2, 0, 12), (3, 1, 11), (4, 0, 7), (2, 1, 3), (2, 2, 12), (2, -1, 12)):
        assert fn(r, siting, capi._fptr(w), base, cap) == capi.E_INVALID, (r, siting, cap)
        assert b"bicubic_taps_rgb420" in capi.lib().snnhip_last_error()
    assert fn(1, 1, capi._fptr(w), base, 12) == capi.E_INVALID and b"decimation" in capi.lib().snnhip_last_error()  # r = 1 says why
    assert fn(3, 0, capi._fptr(w), base, 11) == capi.E_INVALID and b"room for 11 floats, 12 needed" in capi.lib().snnhip_last_error()
    assert fn(2, 1, None, base, 12) == capi.E_INVALID
    assert fn(2, 1, capi._fptr(w), None, 12) == capi.E_INVALID
    assert fn(3, 1, capi._fptr(w), base, 12) == capi.OK and fn(4, 1, capi._fptr(w), base, 8) == capi.OK and fn(2, 0, capi._fptr(w), base, 4) == capi.OK
    with pytest.raises(capi.SnnHipError):
        capi.bicubic_taps_rgb420(1)


def test_coefficients_are_the_float64_formula_rounded_to_fp32_and_invert_yuv_rgb(built):
    from shadernn_amd import capi

    for rng in ("limited", "full"):
        for kr, kb in (R.BT601, R.BT709, (0.2627, 0.0593)):
            got = capi.rgb_cbcr_coefficients(rng, kr, kb)
            assert got.dtype == np.float32 and got.tobytes() == R.coefficients(rng, kr, kb).tobytes(), (rng, kr, kb, got)
            assert got[0] == 128.0
            back = capi.yuv_rgb_coefficients(255, rng, kr, kb)  # (Yoff, Coff, cy, crv, cbu, cgv, cgu)
            ulp = float(np.spacing(np.float32(1.0)))
            assert abs(float(got[1]) * float(back[4]) - 1.0) <= 2 * ulp and abs(float(got[2]) * float(back[3]) - 1.0) <= 2 * ulp  # cbs cbu = crs crv = 1
    np.testing.assert_allclose(capi.rgb_cbcr_coefficients("limited"), [128, 224 / 255 / 1.772, 224 / 255 / 1.402], rtol=1e-6)  # the familiar BT.601 numbers
    np.testing.assert_allclose(capi.rgb_cbcr_coefficients("full"), [128, 1 / 1.772, 1 / 1.402], rtol=1e-6)
    out = np.zeros(3, np.float32)
    fn = capi.lib().snnhip_rgb_cbcr_coefficients
    for args in ((2, 0.299, 0.114, 3), (-1, 0.299, 0.114, 3), (0, 0.0, 0.114, 3), (0, 0.299, 0.0, 3), (0, 0.6, 0.4, 3), (0, 0.299, 0.114, 2)):
        assert fn(*args[:3], capi._fptr(out), args[3]) == capi.E_INVALID, args
        assert b"rgb_cbcr_coefficients" in capi.lib().snnhip_last_error()
    assert fn(0, 0.299, 0.114, None, 3) == capi.E_INVALID
    assert fn(1, 0.299, 0.114, capi._fptr(out), 3) == capi.OK


# ---- the reference's own properties ----

def test_reference_grey_gives_128_and_a_constant_frame_a_constant_plane():
    for r in (2, 3, 4):
        for siting in (R.CENTRE, R.LEFT):
            for rng in (R.LIMITED, R.FULL):
                grey = np.repeat(R.frame(r, 2, 4, 6, 1), 3, axis=-1)
                v = R.values(grey, r, siting, rng)
                assert np.abs(v - 128.0).max() < 1e-4  # (kr + kg + kb is 1 to fp32 rounding: 255 * 6e-8 * the scale)
                assert (R.cbcr(grey, r, siting, rng) == 128).all()
                const = np.empty((1, 4, 6, 3), np.uint8)
                const[...] = (200, 30, 90)
                v = R.values(const, r, siting, rng)
                assert np.ptp(v.reshape(-1, 2), axis=0).max() < 1e-9 and (R.cbcr(const, r, siting, rng) == R.cbcr(const, r, siting, rng)[0, 0, 0]).all()


def test_reference_r2_centre_is_the_per_pixel_conversion_and_primaries_land_on_their_codes():
    x = R.frame(3, 2, 5, 7, 4)
    for rng in (R.LIMITED, R.FULL):
        np.testing.assert_array_equal(R.values(x, 2, R.CENTRE, rng), R.per_pixel(x, rng))
    prim = np.array([[[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]]], np.uint8)
    got = np.rint(R.per_pixel(prim, R.LIMITED))[0, 0]
    np.testing.assert_array_equal(got, [[90, 240], [54, 34], [240, 110], [128, 128], [128, 128]])  # the familiar BT.601 limited-range codes
    full = R.per_pixel(prim, R.FULL)[0, 0]
    np.testing.assert_allclose(full[2, 0], 255.5, atol=1e-4)  # pure blue: Cb = 128 + 127.5, clamped to 255 by the quantiser
    np.testing.assert_allclose(full[0, 1], 255.5, atol=1e-4)


def test_reference_a_ramp_stays_on_its_line_over_output_luma_position():
    """dB is linear in B at fixed R, G: a ramp over input column x is a line over low-resolution position, and a cubic reproduces a line, so away from
    the edges Cb of output chroma column I is the per-pixel value at position (2I + lead) / r - 0.5.  This pins the sign and size of the siting."""
    w = 24
    x = np.zeros((1, 4, w, 3), np.uint8)
    x[..., 2] = (8 * np.arange(w) + 20).astype(np.uint8)[None, None, :]
    x[..., 0] = 60
    x[..., 1] = 60
    pp = R.per_pixel(x, R.FULL)[0, 0, :, 0]
    slope = pp[1] - pp[0]
    for r in (2, 3, 4):
        n = r * w // 2
        edge = 2 * r
        for siting in (R.LEFT, R.CENTRE):
            pos = (2 * np.arange(n) + R.LEAD[siting]) / r - 0.5
            v = R.values(x, r, siting, R.FULL)[0, 0, :, 0]
            np.testing.assert_allclose(v[edge:-edge], pp[0] + slope * pos[edge:-edge], atol=1e-9)
        diff = R.values(x, r, R.CENTRE, R.FULL)[0, 0, edge:-edge, 0] - R.values(x, r, R.LEFT, R.FULL)[0, 0, edge:-edge, 0]
        np.testing.assert_allclose(diff, slope * 0.5 / r, atol=1e-9)  # half an output luma column apart


def test_reference_near_ties_over_the_frames_of_the_gpu_sweep_stay_under_the_cap():
    """The GPU sweep (tests/test_frame_rgb_cbcr_gpu.py) allows a byte to differ where the reference's value is within EPS of a tie and caps the share of
    such values: here the share itself, on the reference alone, over exactly its seeds and shapes.  Spread fractional parts give 2 EPS = 0.2 %."""
    for r in (2, 3, 4):
        for C_ in (3, 4):
            ties = total = 0
            for siting, rng, (n, h, w), seed in R.sweep_cases(r, C_):
                v = R.values(R.frame(seed, n, h, w, C_), r, siting, rng)
                assert v.shape == (n, r * h // 2, r * w // 2, 2)
                ties += int(R.near_tie(v, R.EPS).sum())
                total += v.size
                assert R.clamp_fraction(v) < 0.02
            print("r=%d c=%d: near ties %.3f %% of %d values" % (r, C_, 100.0 * ties / total, total))
            assert ties <= R.MAX_TIE_FRACTION * total and ties <= 0.005 * total
    for r in (2, 3, 4):  # the clamp sweep does clamp: more than one value in two hundred rounds to a code outside 0 .. 255
        assert R.clamp_fraction(R.values(R.frame(3, 1, 10, 40, 3, primaries=True), r, R.LEFT, R.FULL)) > 0.005


def test_reference_fp32_distance_stays_below_the_bound_of_the_expression():
    d = max(R.measured_distance(), R.measured_distance((30, 40)))
    print("rgb_cbcr: fp32-to-float64 distance %.3g (bound %.3g, eps %.3g)" % (d, R.DISTANCE_BOUND, R.EPS))
    assert 0.0 < d < R.DISTANCE_BOUND and R.EPS >= 4.0 * R.DISTANCE_BOUND
    assert d <= R.MEASURED_DISTANCE  # what include/snnhip.h and DESIGN.md section 4.17 state


# ---- refusals that need no device ----

def test_host_mirror_refusals_that_need_no_device(built):
    """Each of these returns -1 before the model file is opened or a device context is made: the path does not exist."""
    from shadernn_amd import host

    h = C.c_void_p()
    path = os.path.join(ROOT, "no", "such", "model.json").encode()

    def create10(io, w=32, hh=24, in_c=1, batch=1):
        return host.lib().snn_model_create10(path, 0, w, hh, in_c, 0, 1, 0, 0, 0, batch, C.byref(io) if io is not None else None, C.byref(h))

    def io(fmt=3, out=0x201, siting=1, rng=0, kr=0.299, kb=0.114):
        return host.EncodeIO(fmt, out, siting, rng, kr, kb)

    assert create10(None) == -1                                          # a null struct
    for fmt in (0, 1, 0x103, 0x104, 0x201, 0x301, 5):                    # float, R8, the 16-bit formats, NV12, P010, an unknown value at the input
        assert create10(io(fmt=fmt)) == -1
    for out in (0, 1, 3, 4, 0x301, 0x103):                               # NV12 only at the output (P010 needs a 16-bit luma split)
        assert create10(io(out=out)) == -1
    assert create10(io(), in_c=3) == -1 and create10(io(fmt=4), in_c=4) == -1  # not a one-channel model
    assert create10(io(siting=2)) == -1 and create10(io(siting=-1)) == -1
    assert create10(io(rng=2)) == -1 and create10(io(rng=-1)) == -1
    assert create10(io(kr=0.0)) == -1 and create10(io(kb=0.0)) == -1 and create10(io(kr=0.7, kb=0.3)) == -1
    assert create10(io(), batch=0) == -1
    assert h.value is None


def test_host_model_argument_checks(built):
    from shadernn_amd import host

    path = os.path.join(ROOT, "no", "such", "model.json")
    for kw in (dict(colour="RGB8", video_out="RGB8"),                     # a colour frame leaves as NV12
               dict(colour="RGB8", video_out="P010"),
               dict(colour="BGR8", video_out="NV12"),
               dict(colour="RGB8", video_out="NV12", video="NV12"),
               dict(colour="RGB8", video_out="NV12", video_range="studio"),
               dict(colour="RGBA8", video_out="NV12", siting="right"),
               dict(colour="RGB8", video_out="NV12", kr=0.0),
               dict(colour="RGB8", video_out="NV12", kr=0.8, kb=0.3),
               dict(colour="RGB8", video_out="NV12", input_format="R8"),
               dict(video_out="NV12")):                                   # no colour=
        with pytest.raises(AssertionError):
            host.Model(path, 32, 24, 1, **kw)


def test_the_unit_is_built_and_documented():
    import sys

    sys.path.insert(0, ROOT)
    import __graft_entry__ as g

    assert "frame_rgb_cbcr.hip" in g.HIP_SOURCES
    assert os.path.exists(os.path.join(g.CSRC, "frame_rgb_cbcr.hip")) and os.path.exists(os.path.join(g.CSRC, "frame_rgb_cbcr.h"))
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "rgb_cbcr" in _read(doc), doc
    assert "4.17" in _read("DESIGN.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "rgb_nv12_host_check.cpp"))
