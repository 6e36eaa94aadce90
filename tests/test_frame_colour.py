"""Colour frames around a luma-only model, the CPU side: the three C-ABI entry points and snn_model_create7 are declared, exported and bound; the
host-side bicubic tap table against the float64 Keys formula; properties of the float64 reference itself (tests/colour_ref.py); the build list and
the documents name the new unit."""
import ctypes as C
import os
import re

import numpy as np

import colour_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("snnhip_rgb_luma_plan_create", "snnhip_ycc_merge_plan_create", "snnhip_bicubic_taps")


def _read(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi, host

    header = re.sub(r"/\*.*?\*/", "", _read("include/snnhip.h"), flags=re.S)
    lib = C.CDLL(snn.load_library())
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    for typ in ("snnhip_rgb_luma_desc", "snnhip_ycc_merge_desc"):
        assert typ in header
    mirror = re.sub(r"/\*.*?\*/", "", _read("include/snn_c.h"), flags=re.S)
    assert re.search(r"\bsnn_model_create7\s*\(", mirror) and "snn_colour_io" in mirror
    assert "snn_model_create7" in host.SIGNATURES and hasattr(host.lib(), "snn_model_create7")
    for f in (snn.rgb_luma_plan, snn.ycc_merge_plan, snn.bicubic_taps):
        assert callable(f)


def test_struct_sizes():
    from shadernn_amd import capi, host

    assert C.sizeof(capi.RgbLumaDesc) == 6 * 4   # int N, H, W, C; float kr, kb
    assert C.sizeof(capi.YccMergeDesc) == 7 * 4  # int N, H, W, C, r; float kr, kb
    assert C.sizeof(host.ColourIO) == 7 * 4      # int format; float kr, kb, in_mean, in_norm, out_scale, out_offset
    assert C.sizeof(host.FrameIO) == 18 * 4      # snn_frame_io keeps its layout
    assert C.sizeof(host.FrameIO2) == 21 * 4     # ... and so does snn_frame_io2
    assert [n for n, _ in host.ColourIO._fields_] == ["format", "kr", "kb", "in_mean", "in_norm", "out_scale", "out_offset"]


def test_bicubic_taps_are_the_float64_keys_formula_rounded_to_fp32(built):
    from shadernn_amd import capi

    for r in (1, 2, 3, 4):
        got = capi.bicubic_taps(r)
        want = R.taps(r).astype(np.float32)
        assert got.shape == (r, 4) and got.dtype == np.float32
        assert got.tobytes() == want.tobytes(), (r, got, want)  # bit for bit
        for row in got:  # the fp32 weights of a phase sum to 1 within one ulp of 1
            s = float(np.sum(row.astype(np.float64)))
            assert abs(s - 1.0) <= float(np.spacing(np.float32(1.0))), (r, row, s)
    np.testing.assert_array_equal(capi.bicubic_taps(1), [[0.0, 1.0, 0.0, 0.0]])
    half = np.array([-0.0703125, 0.8671875, 0.2265625, -0.0234375], np.float32)
    t2 = capi.bicubic_taps(2)
    np.testing.assert_array_equal(t2[1], half)        # phase 1: t = 0.25
    np.testing.assert_array_equal(t2[0], half[::-1])  # phase 0: t = 0.75, the mirror


def test_bicubic_taps_refuses_bad_arguments(built):
    from shadernn_amd import capi

    buf = np.zeros(16, np.float32)
    for r, cap in ((0, 16), (5, 16), (3, 11)):
        assert capi.lib().snnhip_bicubic_taps(r, capi._fptr(buf), cap) == capi.E_INVALID
        assert b"bicubic_taps" in capi.lib().snnhip_last_error()


def test_reference_grey_frame_returns_yhi_in_every_channel():
    rng = np.random.default_rng(1)
    for r in (1, 2, 3, 4):
        for coeff in (R.BT601, R.BT709):
            g = rng.integers(0, 256, size=(2, 5, 7, 1), dtype=np.uint8)
            yhi = rng.integers(0, 256, size=(2, 5 * r, 7 * r, 1), dtype=np.uint8)
            out = R.merge(yhi, np.repeat(g, 3, axis=-1), r, *coeff)
            np.testing.assert_array_equal(out, np.repeat(yhi, 3, axis=-1))
            rgba = np.concatenate([np.repeat(g, 3, axis=-1), 255 - g], axis=-1)
            out = R.merge(yhi, rgba, r, *coeff)
            np.testing.assert_array_equal(out[..., :3], np.repeat(yhi, 3, axis=-1))
            np.testing.assert_array_equal(out[..., 3:], np.repeat(np.repeat(255 - g, r, axis=1), r, axis=2))


def test_reference_constant_colour_comes_back_within_one():
    rng = np.random.default_rng(2)
    for r in (1, 2, 3, 4):
        for _ in range(8):
            colour = rng.integers(0, 256, size=3, dtype=np.uint8)
            rgb = np.broadcast_to(colour, (1, 4, 6, 3)).copy()
            yhi = np.repeat(np.repeat(R.luma(rgb), r, axis=1), r, axis=2)
            out = R.merge(yhi, rgb, r).astype(np.int32)
            assert np.abs(out - colour.astype(np.int32)).max() <= 1, (r, colour, out[0, 0, 0])


def test_reference_luma_and_near_tie():
    rgb = np.array([[[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]]]], np.uint8)
    np.testing.assert_array_equal(R.luma(rgb).reshape(-1), [255, 0, 76, 150, 29])  # BT.601: 76.245, 149.685, 29.07
    np.testing.assert_array_equal(R.luma(rgb, *R.BT709).reshape(-1), [255, 0, 54, 182, 18])
    np.testing.assert_array_equal(R.near_tie(np.array([0.5, 1.4995, 1.4985, 2.0, -0.5004, 7.5009])), [True, True, False, False, True, True])
    # uniform random bytes: near ties are well under the 1 % the comparison rule allows
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, size=(1, 37, 29, 3), dtype=np.uint8)
    assert R.near_tie(R.luma_values(x)).mean() < 0.01
    for r in (2, 3, 4):
        yhi = rng.integers(0, 256, size=(1, 37 * r, 29 * r, 1), dtype=np.uint8)
        assert R.near_tie(R.merge_values(yhi, x, r)).mean() < 0.01


def test_the_unit_is_built_and_documented():
    import sys

    sys.path.insert(0, ROOT)
    import __graft_entry__ as g

    assert "frame_colour.hip" in g.HIP_SOURCES
    assert os.path.exists(os.path.join(g.CSRC, "frame_colour.hip")) and os.path.exists(os.path.join(g.CSRC, "frame_colour.h"))
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "frame_colour" in _read(doc), doc
    assert "4.13" in _read("DESIGN.md")
