"""Planes fitted to any size between half and four times their own, the CPU side: the two C-ABI entry points are declared, exported and bound;
snnhip_fit_taps against the float64 table of tests/fit_ref.py, bit for bit, and against the fixed-phase table of the chroma upsampler; its
refusals; properties of the float64 reference itself; the build list and the documents name the new unit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(1, 1), (3, 2), (7, 5), (4, 3), (2562, 1920), (100, 50), (5, 20), (9, 27), (17, 17)]  # (inputs, outputs) of one axis
SITINGS = ["centre", "left"]


def _read(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi

    header = re.sub(r"/\*.*?\*/", "", _read("include/snnhip.h"), flags=re.S)
    lib = C.CDLL(snn.load_library())
    for name in ("snnhip_plane_fit_plan_create", "snnhip_fit_taps"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    assert "snnhip_plane_fit_desc" in header
    for f in (snn.plane_fit_plan, snn.fit_taps):
        assert callable(f)
    assert C.sizeof(capi.PlaneFitDesc) == 10 * 4  # int N, H, W, C, OH, OW, dtype, maxval, shift, siting
    assert [n for n, _ in capi.PlaneFitDesc._fields_] == ["N", "H", "W", "C", "OH", "OW", "dtype", "maxval", "shift", "siting"]
    assert C.sizeof(capi.ChromaUpDesc) == 9 * 4  # the earlier structs keep their layout


def test_the_build_list_and_the_documents_name_the_unit():
    assert '"frame_fit.hip"' in _read("__graft_entry__.py")
    assert "frame_fit.hip" in _read("README.md") and "4.18" in _read("DESIGN.md") and "snnhip_plane_fit_plan_create" in _read("INTEGRATION.md")


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("pair", PAIRS, ids=["%dto%d" % p for p in PAIRS])
def test_fit_taps_are_the_float64_table_rounded_to_fp32(built, pair, siting):
    from shadernn_amd import capi

    I, O = pair
    got, base = capi.fit_taps(I, O, siting)
    want, want_base = R.table(I, O, siting)
    assert got.shape == (O, 8) and got.dtype == np.float32
    np.testing.assert_array_equal(base, want_base)
    assert got.tobytes() == want.astype(np.float32).tobytes()  # bit for bit
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6  # every row sums to 1
    assert (np.diff(base) >= 0).all() and (np.diff(base) <= 2).all()       # what the kernel's window relies on


def test_nonzero_taps_follow_the_ratio(built):
    from shadernn_amd import capi

    for I, O, live in ((4, 3, 6), (100, 50, 8), (2, 1, 8), (5, 20, 4), (7, 7, 1)):
        w, _ = capi.fit_taps(I, O, "centre")
        assert int((w != 0).sum(axis=1).max()) == live, (I, O)
    w, base = capi.fit_taps(100, 50, "centre")  # exactly 1/2: the two middle taps carry the same weight, the outermost are live
    assert (w[:, 0] != 0).all() and (w[:, 7] != 0).all() and np.array_equal(w[:, 3], w[:, 4])
    np.testing.assert_array_equal(base, 2 * np.arange(50))


@pytest.mark.parametrize("siting", SITINGS)
def test_an_integer_factor_is_the_sited_table_of_the_chroma_upsampler(built, siting):
    from shadernn_amd import capi

    for r in (1, 2, 3, 4):
        want, want_base = capi.bicubic_taps_sited(r, siting)
        for I in (1, 5, 9):
            got, base = capi.fit_taps(I, r * I, siting)
            X = np.arange(r * I)
            np.testing.assert_array_equal(base, X // r + want_base[X % r])  # the same bases
            inner, ref = got[:, 2:6], want[X % r]
            assert (np.abs(inner - ref) <= np.spacing(np.maximum(np.abs(inner), np.abs(ref)))).all(), (r, I)  # within one float ulp
            assert not got[:, :2].any() and not got[:, 6:].any()  # the outer four are 0.0


def test_equal_extents_give_the_identity_table(built):
    from shadernn_amd import capi

    for siting in SITINGS:
        for I in (1, 2, 17, 1920):
            w, base = capi.fit_taps(I, I, siting)
            np.testing.assert_array_equal(base, np.arange(I))
            np.testing.assert_array_equal(w, np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 0], np.float32), (I, 1)))


def test_fit_taps_refuses_bad_arguments(built):
    from shadernn_amd import capi

    w = np.zeros(8 * 32, np.float32)
    base = (C.c_int * 32)()
    fn = capi.lib().snnhip_fit_taps
    for I, O, siting, cap in ((5, 2, 0, 256), (2, 9, 0, 256), (0, 1, 0, 256), (4, 0, 0, 256), (-1, -1, 0, 256), (4, 6, 2, 256), (4, 6, -1, 256), (4, 6, 1, 47), (1, 1, 0, 7)):
        assert fn(I, O, siting, capi._fptr(w), base, cap) == capi.E_INVALID, (I, O, siting, cap)
        assert b"fit_taps" in capi.lib().snnhip_last_error()
    assert fn(5, 2, 0, capi._fptr(w), base, 256) == capi.E_INVALID and b"[1/2, 4]" in capi.lib().snnhip_last_error()
    assert fn(4, 6, 1, None, base, 256) == capi.E_INVALID
    assert fn(4, 6, 1, capi._fptr(w), None, 256) == capi.E_INVALID
    assert fn(4, 6, 1, capi._fptr(w), base, 48) == capi.OK
    assert fn(4, 2, 1, capi._fptr(w), base, 16) == capi.OK and fn(4, 16, 0, capi._fptr(w), base, 128) == capi.OK  # the two ends of the range
    with pytest.raises(capi.SnnHipError):
        capi.fit_taps(5, 2)


def test_the_host_mirror_declares_binds_and_refuses_without_a_device(built):
    from shadernn_amd import host

    mirror = re.sub(r"/\*.*?\*/", "", _read("include/snn_c.h"), flags=re.S)
    assert re.search(r"\bsnn_model_create11\s*\(", mirror) and "snn_fit_io" in mirror
    assert "snn_model_create11" in host.SIGNATURES and hasattr(host.lib(), "snn_model_create11")
    assert C.sizeof(host.FitIO) == 10 * 4 and [n for n, _ in host.FitIO._fields_] == ["video", "out_w", "out_h"]
    assert C.sizeof(host.VideoIO) == 8 * 4  # the earlier struct keeps its layout
    h = C.c_void_p()

    def create11(ow, oh, w=32, hh=24, fmt=0x201, maxval=255, shift=0, siting=1, in_c=1, batch=1):
        io = host.FitIO(host.VideoIO(fmt, maxval, shift, siting, 127.5, 1 / 127.5, 127.5, 127.5), ow, oh)
        return host.lib().snn_model_create11(b"/nonexistent/model.json", 0, w, hh, in_c, 0, 1, 0, 0, 0, batch, C.byref(io), C.byref(h))

    assert host.lib().snn_model_create11(b"/nonexistent/model.json", 0, 32, 24, 1, 0, 1, 0, 0, 0, 1, None, C.byref(h)) == -1  # a null struct
    for ow, oh in ((47, 36), (48, 35), (0, 36), (48, 0), (1, 1), (-2, 36)):  # odd or below 2
        assert create11(ow, oh) == -1, (ow, oh)
    for ow, oh in ((14, 36), (130, 36), (48, 10), (48, 98)):  # out / in outside [1/2, 4]
        assert create11(ow, oh) == -1, (ow, oh)
    # what snn_model_create8 refuses: other formats, an odd input extent, an unknown siting, a depth that does not fit, three channels, batch 0
    assert create11(48, 36, fmt=1) == -1 and create11(48, 36, fmt=0x101) == -1
    assert create11(48, 36, w=31) == -1 and create11(48, 36, hh=23) == -1
    assert create11(48, 36, siting=2) == -1 and create11(48, 36, maxval=256) == -1 and create11(48, 36, fmt=0x301, maxval=65535) == -1
    assert create11(48, 36, shift=1) == -1 and create11(48, 36, in_c=3) == -1 and create11(48, 36, batch=0) == -1
    with pytest.raises(AssertionError, match="out_size"):
        host.Model("/nonexistent/model.json", 32, 24, 1, video="NV12", video_out="RGB8", out_size=(48, 36))
    with pytest.raises(AssertionError, match="out_size"):
        host.Model("/nonexistent/model.json", 32, 24, 1, colour="RGB8", out_size=(48, 36))
    with pytest.raises(AssertionError, match="out_size"):
        host.Model("/nonexistent/model.json", 32, 24, 1, out_size=(48, 36))


def test_reference_constant_plane_comes_back_constant():
    for _, h, w, oh, ow in R.SHAPES:
        for siting in SITINGS:
            for container, maxval, shift in R.DEPTHS:
                dt = np.uint8 if container == "u8" else np.uint16
                for value in (0, maxval, maxval // 3):
                    u = np.full((1, h, w, 2), value << shift, dt)
                    out = R.fit(u, oh, ow, siting, maxval, shift)
                    assert out.shape == (1, oh, ow, 2) and out.dtype == dt
                    np.testing.assert_array_equal(out, np.full_like(out, value << shift))


def test_reference_ratio_one_returns_the_input():
    rng = np.random.default_rng(5)
    for container, maxval, shift in R.DEPTHS:
        dt = np.uint8 if container == "u8" else np.uint16
        u = (rng.integers(0, maxval + 1, size=(2, 9, 13, 2)) << shift).astype(dt)
        for siting in SITINGS:
            np.testing.assert_array_equal(R.fit_values(u, 9, 13, siting, shift), u.astype(np.float64) / (1 << shift))  # exact: weights 0 and 1
            np.testing.assert_array_equal(R.fit(u, 9, 13, siting, maxval, shift), u)


@pytest.mark.parametrize("depth", R.DEPTHS, ids=["u8", "u10", "p010", "u12"])
def test_reference_in_float32_stays_within_a_sixth_of_eps(depth):
    """The kernel's arithmetic (weights rounded to float, sums in float32) against the float64 reference on the GPU sweep's shapes and two the size
    of a tile: the near-tie half-width leaves six times this distance."""
    container, maxval, shift = depth
    dt = np.uint8 if container == "u8" else np.uint16
    rng = np.random.default_rng(17 + maxval + shift)
    worst = 0.0
    for n, h, w, oh, ow in R.SHAPES + [(1, 55, 676, 41, 507), (2, 46, 258, 23, 129)]:
        for siting in SITINGS:
            u = (rng.integers(0, maxval + 1, size=(n, h, w, 2)) << shift).astype(dt)
            d = np.abs(R.fit_values(u, oh, ow, siting, shift, np.float32).astype(np.float64) - R.fit_values(u, oh, ow, siting, shift))
            worst = max(worst, float(d.max()))
    print("fit reference, maxval %d: float32 to float64 distance %.2e, eps %.0e" % (maxval, worst, R.EPS[maxval]))
    assert worst <= R.EPS[maxval] / 6


def lane_set_frames(th):
    """The frames of tests/test_frame_fit_gpu.py::test_rows_dealt_to_lane_sets_meet_at_the_chunk_boundaries as (u, OH, OW), for a tile of `th` rows:
    U8, C = 1, 11 rows enlarged to th - 1 and th + 1 (a tile one row short; a full tile and a tile of one row), 20 -> 30 and 200 -> 300 columns.  An
    enlarged tile's column span has fewer than 128 dword strips, so pass 1 deals the tile's rows to two or more lane sets: 30 columns take 7 strips
    and 36 sets, more sets than rows, chunks of one row; the 256 columns of a full tile at 3/2 take 44 strips and 5 sets, the last chunk short."""
    assert 11 <= th - 1 and th + 1 <= 4 * 11, th
    frames = []
    for k, (w, ow) in enumerate([(20, 30), (200, 300)]):
        for j, oh in enumerate((th - 1, th + 1)):
            u = np.random.default_rng(900 + 2 * k + j).integers(0, 256, size=(1, 11, w, 1)).astype(np.uint8)
            frames.append((u, oh, ow))
    return frames


@pytest.mark.parametrize("th", range(12, 33))
def test_near_ties_of_the_lane_set_frames_stay_under_the_cap(th):
    """The GPU test reads the tile height from the plan; the kernel's tiles have at most 32 rows and these frames need at least 12.  On the reference
    alone, for every height the frames can take."""
    values = [R.fit_values(u, oh, ow, "left") for u, oh, ow in lane_set_frames(th)]
    ties = sum(int(R.near_tie(v, R.EPS[255]).sum()) for v in values)
    assert ties <= R.MAX_TIE_FRACTION * sum(v.size for v in values)
