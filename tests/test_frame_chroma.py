"""NV12 / P010 chroma planes beside a luma-only model, the CPU side: the two C-ABI entry points, snn_model_create8 and the two frame calls are
declared, exported and bound; the sited tap table against the float64 formula; properties of the float64 reference itself (tests/chroma_ref.py);
the refusals of the host mirror that need no device; the build list and the documents name the new unit.

One statement of the issue is not asserted as written: "centre siting reproduces snnhip_bicubic_taps, with bases all 0".  The contract defines a
phase's base as floor(s), and with aligned centres s = (p + 0.5) / r - 0.5 is negative for the phases 2p + 1 < r (r = 2: phase 0 reads x - 2 .. x + 1,
as the merge kernel's phase_first says).  The test asserts the weights of snnhip_bicubic_taps and bases equal to floor(s); they are all 0 only at r = 1."""
import ctypes as C
import os
import re

import numpy as np

import chroma_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi, host

    header = re.sub(r"/\*.*?\*/", "", _read("include/snnhip.h"), flags=re.S)
    lib = C.CDLL(snn.load_library())
    for name in ("snnhip_chroma_up_plan_create", "snnhip_bicubic_taps_sited"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    assert "snnhip_chroma_up_desc" in header and "SNNHIP_SITING_LEFT" in header and "SNNHIP_SITING_CENTRE" in header
    mirror = re.sub(r"/\*.*?\*/", "", _read("include/snn_c.h"), flags=re.S)
    for name in ("snn_model_create8", "snn_model_upload_frame_nv12", "snn_model_download_frame_nv12"):
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert name in host.SIGNATURES and hasattr(host.lib(), name), name
    assert "snn_video_io" in mirror and "SNN_IO_NV12_16" in mirror
    for f in (snn.chroma_up_plan, snn.bicubic_taps_sited):
        assert callable(f)


def test_struct_sizes():
    from shadernn_amd import capi, host

    assert C.sizeof(capi.ChromaUpDesc) == 9 * 4  # int N, H, W, C, r, dtype, maxval, shift, siting
    assert [n for n, _ in capi.ChromaUpDesc._fields_] == ["N", "H", "W", "C", "r", "dtype", "maxval", "shift", "siting"]
    assert C.sizeof(host.VideoIO) == 8 * 4       # int format, maxval, shift, siting; float in_mean, in_norm, out_scale, out_offset
    assert [n for n, _ in host.VideoIO._fields_] == ["format", "maxval", "shift", "siting", "in_mean", "in_norm", "out_scale", "out_offset"]
    assert C.sizeof(host.ColourIO) == 7 * 4 and C.sizeof(host.FrameIO) == 18 * 4 and C.sizeof(host.FrameIO2) == 21 * 4  # the earlier structs keep their layout


def test_sited_taps_are_the_float64_formula_rounded_to_fp32(built):
    from shadernn_amd import capi

    for siting in ("centre", "left"):
        for r in (1, 2, 3, 4):
            got, base = capi.bicubic_taps_sited(r, siting)
            want, want_base = R.taps(r, siting)
            assert got.shape == (r, 4) and got.dtype == np.float32
            assert got.tobytes() == want.astype(np.float32).tobytes(), (siting, r, got, want)  # bit for bit
            np.testing.assert_array_equal(base, want_base)
            assert set(base.tolist()) <= {-1, 0}
            for row in got:  # the fp32 weights of a phase sum to 1 within one ulp of 1
                s = float(np.sum(row.astype(np.float64)))
                assert abs(s - 1.0) <= float(np.spacing(np.float32(1.0))), (siting, r, row, s)


def test_centre_siting_is_the_existing_table_and_r1_is_the_identity(built):
    from shadernn_amd import capi

    for r in (1, 2, 3, 4):
        got, base = capi.bicubic_taps_sited(r, "centre")
        assert got.tobytes() == capi.bicubic_taps(r).tobytes()
        np.testing.assert_array_equal(base, [int(np.floor((p + 0.5) / r - 0.5)) for p in range(r)])  # (see the module's docstring)
    for siting in ("centre", "left"):
        got, base = capi.bicubic_taps_sited(1, siting)
        np.testing.assert_array_equal(got, [[0.0, 1.0, 0.0, 0.0]])
        np.testing.assert_array_equal(base, [0])
    # the issue's worked example: left siting, phase 0 of r = 2 reads x - 2 .. x + 1 with these weights
    got, base = capi.bicubic_taps_sited(2, "left")
    assert base[0] == -1
    np.testing.assert_allclose(got[0], [-0.0068, 0.0908, 0.9639, -0.0479], atol=5e-5)
    for r in (2, 3, 4):  # with left siting phase 0 alone starts one sample early
        np.testing.assert_array_equal(capi.bicubic_taps_sited(r, "left")[1], [-1] + [0] * (r - 1))


def test_sited_taps_refuses_bad_arguments(built):
    from shadernn_amd import capi

    w = np.zeros(16, np.float32)
    base = (C.c_int * 4)()
    fn = capi.lib().snnhip_bicubic_taps_sited
    for r, siting, cap in ((0, 1, 16), (5, 1, 16), (3, 1, 11), (2, 2, 16), (2, -1, 16)):
        assert fn(r, siting, capi._fptr(w), base, cap) == capi.E_INVALID
        assert b"bicubic_taps_sited" in capi.lib().snnhip_last_error()
    assert fn(2, 1, None, base, 16) == capi.E_INVALID
    assert fn(2, 1, capi._fptr(w), None, 16) == capi.E_INVALID
    assert fn(4, 1, capi._fptr(w), base, 16) == capi.OK


def test_reference_constant_plane_comes_back_constant():
    for r in (1, 2, 3, 4):
        for siting in (R.CENTRE, R.LEFT):
            for value, maxval, shift, dt in ((0, 255, 0, np.uint8), (255, 255, 0, np.uint8), (77, 255, 0, np.uint8), (1023, 1023, 6, np.uint16), (513, 1023, 0, np.uint16),
                                             (4095, 4095, 0, np.uint16)):
                u = np.full((2, 5, 7, 2), value << shift, dt)
                out = R.up(u, r, siting, maxval, shift)
                assert out.shape == (2, 5 * r, 7 * r, 2) and out.dtype == dt
                np.testing.assert_array_equal(out, np.full_like(out, value << shift))


def test_reference_r1_is_the_input_with_the_low_bits_cleared():
    rng = np.random.default_rng(4)
    u = rng.integers(0, 1024, size=(1, 6, 9, 2)).astype(np.uint16) << 6
    dirty = u | rng.integers(0, 64, size=u.shape).astype(np.uint16)
    for siting in (R.CENTRE, R.LEFT):
        np.testing.assert_array_equal(R.up(dirty, 1, siting, 1023, 6), u)


def test_reference_left_siting_keeps_a_ramp_on_its_line_over_the_luma_grid_and_centre_does_not():
    """The check that pins the sign of the quarter-sample shift.  The issue words it as "a horizontal ramp upsampled with left siting, sampled back at
    j = r*i, returns the input"; by the issue's own derivation output sample j = r*i reads chroma index i + 0.25 / r - 0.25, not i (the luma grid is
    scaled about aligned centres, so even output luma columns do not sit on even input luma columns), and no output sample sits on an input sample for
    r = 2..4.  What does hold, and is asserted for every output sample away from the edges: a ramp c = a*i + b over chroma index i is, with left
    siting, the line a*L/2 + b over low-resolution luma position L (sample i sits at L = 2i); output sample j sits at output luma column 2j, which is
    L = (2j + 0.5) / r - 0.5, and a cubic reproduces a line, so the value there is exactly on that line.  With centre siting the same output sample is
    0.25 - 0.25 / r of an input sample off the line, towards smaller values for a rising ramp; with slope 8 the rounded bytes differ."""
    w, a, b = 24, 8.0, 20.0
    ramp = (a * np.arange(w) + b).astype(np.uint8)  # 20 .. 204
    u = np.broadcast_to(ramp[None, None, :, None], (1, 4, w, 2)).copy()
    for r in (2, 3, 4):
        j = np.arange(r * w, dtype=np.float64)
        luma = (2.0 * j + 0.5) / r - 0.5          # low-resolution luma position of output chroma sample j
        line = (a * luma / 2.0 + b)[2 * r:-2 * r]
        left = R.up_values(u, r, R.LEFT)
        centre = R.up_values(u, r, R.CENTRE)
        for row in (0, r * 4 - 1):
            for c in (0, 1):
                np.testing.assert_allclose(left[0, row, 2 * r:-2 * r, c], line, atol=1e-9)
                np.testing.assert_allclose(centre[0, row, 2 * r:-2 * r, c] - line, -a * (0.25 - 0.25 / r), atol=1e-9)
        got_left, got_centre = R.up(u, r, R.LEFT, 255), R.up(u, r, R.CENTRE, 255)
        np.testing.assert_array_equal(got_left[0, 0, 2 * r:-2 * r, 0], np.rint(line).astype(np.uint8))
        assert (got_left[0, 0, 2 * r:-2 * r, 0].astype(int) - got_centre[0, 0, 2 * r:-2 * r, 0].astype(int) >= 1).all()
        # the samples j = r*i: left siting returns the input moved by a * (0.25 / r - 0.25), within rounding only for a gentle ramp
        np.testing.assert_allclose(left[0, 0, ::r, 0][2:-2], ramp[2:-2] + a * (0.25 / r - 0.25), atol=1e-9)


def test_reference_near_ties_stay_under_the_cap_on_random_planes():
    rng = np.random.default_rng(5)
    for maxval, shift, dt in ((255, 0, np.uint8), (1023, 6, np.uint16), (4095, 0, np.uint16)):
        u = (rng.integers(0, maxval + 1, size=(1, 37, 29, 2)) << shift).astype(dt)
        for r in (2, 3, 4):
            for siting in (R.CENTRE, R.LEFT):
                assert R.near_tie(R.up_values(u, r, siting, shift), R.EPS[maxval]).mean() < R.MAX_TIE_FRACTION


def test_host_mirror_refusals_that_need_no_device(built):
    """Each of these returns -1 before the model file is opened or a device context is made: the path does not exist."""
    from shadernn_amd import host

    h = C.c_void_p()
    path = os.path.join(ROOT, "no", "such", "model.json").encode()

    def create8(io, w=32, hh=24, in_c=1, batch=1):
        return host.lib().snn_model_create8(path, 0, w, hh, in_c, 0, 1, 0, 0, 0, batch, C.byref(io) if io is not None else None, C.byref(h))

    def io(fmt=0x201, maxval=255, shift=0, siting=1):
        return host.VideoIO(fmt, maxval, shift, siting, 0.0, 1.0 / maxval, float(maxval), 0.0)

    assert create8(None) == -1                                   # a null struct
    for fmt in (0, 1, 3, 0x101, 0x202):                          # float, R8, RGB8, R16, an unknown value
        assert create8(io(fmt=fmt)) == -1
    assert create8(io(), in_c=3) == -1                           # not a one-channel model
    assert create8(io(), w=31) == -1 and create8(io(), hh=23) == -1  # odd extents: no 4:2:0 plane
    assert create8(io(fmt=0x301, maxval=65535)) == -1            # P016 chroma is not built
    assert create8(io(fmt=0x301, maxval=4096)) == -1
    assert create8(io(fmt=0x301, maxval=1023, shift=7)) == -1    # does not fit the container
    assert create8(io(maxval=1023)) == -1                        # ... nor ten bits a byte
    assert create8(io(shift=1)) == -1
    assert create8(io(siting=2)) == -1
    assert create8(io(), batch=0) == -1
    assert h.value is None
    assert host.lib().snn_model_upload_frame_nv12(None, None) == -1 and host.lib().snn_model_download_frame_nv12(None, None) == -1


def test_the_unit_is_built_and_documented():
    import sys

    sys.path.insert(0, ROOT)
    import __graft_entry__ as g

    assert "frame_chroma.hip" in g.HIP_SOURCES
    assert os.path.exists(os.path.join(g.CSRC, "frame_chroma.hip")) and os.path.exists(os.path.join(g.CSRC, "frame_chroma.h"))
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "frame_chroma" in _read(doc), doc
    assert "4.14" in _read("DESIGN.md")
