"""RGB frames at any output size behind the luma model, the CPU side: the two C-ABI entry points are declared, exported and bound;
snnhip_rgb_fit_taps against the float64 table of tests/rgb_fit_ref.py, bit for bit, and against the fixed-phase tables of yuv_rgb and ycc_merge;
its refusals; the properties and the measured distances of the float64 reference itself; the build list and the documents name the new unit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rgb_fit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = sorted({(h, oh) for _, h, _, oh, _ in R.SHAPES} | {(w, ow) for _, _, w, _, ow in R.SHAPES})  # (inputs, outputs) of one axis
SITINGS = ["centre", "left"]
DEPTHS = [(255, 0, np.uint8), (1023, 0, np.uint16), (1023, 6, np.uint16), (4095, 0, np.uint16)]


def _read(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi

    header = re.sub(r"/\*.*?\*/", "", _read("include/snnhip.h"), flags=re.S)
    lib = C.CDLL(snn.load_library())
    for name in ("snnhip_rgb_fit_plan_create", "snnhip_rgb_fit_taps"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    assert "snnhip_rgb_fit_desc" in header
    for name, value in (("SNNHIP_RGB_FIT_CBCR", 0), ("SNNHIP_RGB_FIT_PLANAR", 1), ("SNNHIP_RGB_FIT_RGB", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert capi.RGB_FIT_SOURCE == {"cbcr": 0, "planar": 1, "rgb": 2}
    for f in (capi.rgb_fit_plan, capi.rgb_fit_taps):
        assert callable(f)
    assert C.sizeof(capi.RgbFitDesc) == 14 * 4  # int N, H, W, OH, OW, C, source, dtype, maxval, shift, siting, range; float kr, kb
    assert [n for n, _ in capi.RgbFitDesc._fields_] == ["N", "H", "W", "OH", "OW", "C", "source", "dtype", "maxval", "shift", "siting", "range", "kr", "kb"]
    assert C.sizeof(capi.PlaneFitDesc) == 10 * 4 and C.sizeof(capi.YuvRgbDesc) == 12 * 4  # the earlier structs keep their layout


def test_the_build_list_and_the_documents_name_the_unit():
    assert '"frame_rgb_fit.hip"' in _read("__graft_entry__.py")
    assert "frame_rgb_fit.hip" in _read("README.md") and "4.24" in _read("DESIGN.md")


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("pair", PAIRS, ids=["%dto%d" % p for p in PAIRS])
def test_rgb_fit_taps_are_the_float64_table_rounded_to_fp32(built, pair, siting):
    from shadernn_amd import capi

    I, O = pair
    got, base = capi.rgb_fit_taps(I, O, siting)
    want, want_base = R.table(I, O, siting)
    assert got.shape == (O, 4) and got.dtype == np.float32
    np.testing.assert_array_equal(base, want_base)
    assert got.tobytes() == want.astype(np.float32).tobytes()  # bit for bit
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6  # every row sums to 1
    assert (np.diff(base) >= 0).all() and (np.diff(base) <= 1).all()       # what the kernel's window relies on
    assert base[0] >= -1 and base[-1] <= I - 1


def test_fit_taps_still_returns_the_bits_of_its_own_reference(built):
    """snnhip_fit_taps is untouched by its sibling: bit for bit the table of tests/fit_ref.py, as before."""
    import fit_ref
    from shadernn_amd import capi

    for I, O in ((3, 2), (7, 5), (5, 20), (17, 17), (100, 50)):
        for siting in SITINGS:
            got, base = capi.fit_taps(I, O, siting)
            want, want_base = fit_ref.table(I, O, siting)
            np.testing.assert_array_equal(base, want_base)
            assert got.tobytes() == want.astype(np.float32).tobytes()


# the float64 tables against the fixed-phase ones: the division by a sum that is 1 to a few ulps moves a weight by at most five double ulps of 1
# (1.11e-15, the 1.1e-15 of DESIGN.md section 4.24 to two digits); nothing of the code under test enters this figure
FIVE_ULP = 5 * 2.0 ** -52


def _one_ulp(a, b):
    return (np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all()


@pytest.mark.parametrize("siting", SITINGS)
def test_an_integer_factor_of_a_chroma_plane_is_the_table_of_yuv_rgb(built, siting):
    from shadernn_amd import capi

    for r in (1, 2, 3, 4):
        want, want_base = capi.bicubic_taps_420(r, siting)
        for I in (1, 5, 9):
            got, base = capi.rgb_fit_taps(I, 2 * r * I, siting)
            X = np.arange(2 * r * I)
            np.testing.assert_array_equal(base, X // (2 * r) + want_base[X % (2 * r)])  # the same bases
            assert _one_ulp(got, want[X % (2 * r)]), (r, I)                              # within one float ulp
            w64, b64 = R.table(I, 2 * r * I, siting)
            ref64, rb64 = R.yuv_rgb_ref.taps(r, siting)
            np.testing.assert_array_equal(b64, X // (2 * r) + rb64[X % (2 * r)])
            assert np.abs(w64 - ref64[X % (2 * r)]).max() <= FIVE_ULP


def test_an_integer_factor_of_a_colour_frame_is_the_table_of_ycc_merge(built):
    from shadernn_amd import capi

    for r in (1, 2, 3, 4):
        want = capi.bicubic_taps(r)
        want_base = R.resample_ref.taps(r, 0.5, 0.5)[1]
        for I in (1, 5, 9):
            got, base = capi.rgb_fit_taps(I, r * I, "centre")
            X = np.arange(r * I)
            np.testing.assert_array_equal(base, X // r + want_base[X % r])
            assert _one_ulp(got, np.asarray(want).reshape(r, 4)[X % r]), (r, I)
            assert np.abs(R.table(I, r * I, "centre")[0] - R.colour_ref.taps(r)[X % r]).max() <= FIVE_ULP


def test_equal_extents_with_aligned_centres_give_the_identity_table(built):
    from shadernn_amd import capi

    for I in (1, 2, 17, 1920):
        w, base = capi.rgb_fit_taps(I, I, "centre")
        np.testing.assert_array_equal(base, np.arange(I))
        np.testing.assert_array_equal(w, np.tile(np.array([0, 1, 0, 0], np.float32), (I, 1)))
    w, base = capi.rgb_fit_taps(9, 9, "left")  # a left-sited plane of the luma grid's own extent: a quarter-sample shift, not a copy
    np.testing.assert_array_equal(base, np.arange(9))
    assert (w[:, 2] != 0).all()


def test_rgb_fit_taps_refuses_bad_arguments(built):
    from shadernn_amd import capi

    w = np.zeros(4 * 64, np.float32)
    base = (C.c_int * 64)()
    fn = capi.lib().snnhip_rgb_fit_taps
    for I, O, siting, cap in ((5, 4, 0, 256), (2, 17, 0, 256), (0, 1, 0, 256), (4, 0, 0, 256), (-1, -1, 0, 256), (4, 6, 2, 256), (4, 6, -1, 256), (4, 6, 1, 23), (1, 1, 0, 3),
                              (4, 6, 1, -1)):
        assert fn(I, O, siting, capi._fptr(w), base, cap) == capi.E_INVALID, (I, O, siting, cap)
        assert b"rgb_fit_taps" in capi.lib().snnhip_last_error()
    assert fn(5, 4, 0, capi._fptr(w), base, 256) == capi.E_INVALID and b"[1, 8]" in capi.lib().snnhip_last_error()
    assert fn(4, 6, 1, None, base, 256) == capi.E_INVALID
    assert fn(4, 6, 1, capi._fptr(w), None, 256) == capi.E_INVALID
    assert fn(4, 6, 1, capi._fptr(w), base, 24) == capi.OK
    assert fn(4, 4, 1, capi._fptr(w), base, 16) == capi.OK and fn(4, 32, 0, capi._fptr(w), base, 128) == capi.OK  # the two ends of the range
    with pytest.raises(capi.SnnHipError):
        capi.rgb_fit_taps(5, 4)


# ---- the reference's own properties

def test_reference_neutral_chroma_gives_the_quantised_luma_term():
    for maxval, shift, dt in DEPTHS:
        k = (maxval + 1) // 256
        for i, (n, h, w, oh, ow) in enumerate(R.SHAPES[:9]):
            yfit, _ = R.video_frame(n, h, w, oh, ow, maxval, shift, dt, seed=i, whole_range=True)
            cbcr = np.full((n, h, w, 2), (128 * k) << shift, dt)
            for rng in ("limited", "full"):
                c = R.yuv_rgb_ref.coefficients(maxval, rng).astype(np.float64)
                yl = R.quantise(c[2] * ((yfit.astype(np.int64) >> shift).astype(np.float64) - c[0]), maxval, shift, dt)
                out = R.video_rgb(yfit, cbcr, 4, "left", rng, maxval, shift)
                np.testing.assert_array_equal(out[..., :3], np.repeat(yl, 3, axis=-1))
                assert (out[..., 3] == maxval << shift).all()


def test_reference_grey_frame_gives_the_luma_frame():
    for i, (n, h, w, oh, ow) in enumerate(R.SHAPES[:9]):
        yfit, frame = R.rgb_frame(n, h, w, oh, ow, 4, seed=i)
        frame[..., :3] = frame[..., :1]
        out = R.rgb_rgb(yfit, frame)
        np.testing.assert_array_equal(out[..., :3], np.repeat(yfit, 3, axis=-1))
        np.testing.assert_array_equal(out[..., 3:], R.alpha_of(frame, oh, ow))


def test_reference_constant_chroma_planes_give_constant_chroma_terms():
    for n, h, w, oh, ow in R.SHAPES[:9]:
        yfit = np.full((n, oh, ow, 1), 100, np.uint8)
        cbcr = np.zeros((n, h, w, 2), np.uint8)
        cbcr[..., 0], cbcr[..., 1] = 90, 170
        for siting in SITINGS:
            v = R.video_values(yfit, cbcr, siting)
            assert np.abs(v - v[:1, :1, :1]).max() <= 1e-12, (h, w, oh, ow)


def test_reference_alpha_rule_is_the_pixel_underneath():
    frame = np.arange(2 * 3 * 5 * 4, dtype=np.uint8).reshape(2, 3, 5, 4)
    for r in (1, 2, 3, 4):  # at OH = rH: ycc_merge's Y // r
        np.testing.assert_array_equal(R.alpha_of(frame, 3 * r, 5 * r), np.repeat(np.repeat(frame[..., 3:4], r, axis=1), r, axis=2))
    a = R.alpha_of(frame, 4, 7)
    assert a.shape == (2, 4, 7, 1) and a[0, 0, 0, 0] == frame[0, 0, 0, 3] and a[1, 3, 6, 0] == frame[1, 2, 4, 3]


def test_reference_planar_layout_round_trips():
    cbcr = np.arange(2 * 3 * 4 * 2, dtype=np.uint8).reshape(2, 3, 4, 2)
    p = R.to_planar(cbcr)
    assert p.shape == (4, 3, 4, 1)
    np.testing.assert_array_equal(p[2, ..., 0], cbcr[1, ..., 0])
    np.testing.assert_array_equal(p[3, ..., 0], cbcr[1, ..., 1])


@pytest.mark.parametrize("case", [("video", 255, 2.4e-5, 0.03), ("video", 1023, 1.1e-4, 0.03), ("video", 4095, 4.1e-4, 0.03), ("rgb", 255, 4.5e-5, 0.01)],
                         ids=["video8", "video10", "video12", "rgb8"])
def test_reference_in_float32_stays_within_a_quarter_of_eps(case):
    """The kernel's arithmetic (weights rounded to float, sums in float32) against the float64 reference over SHAPES, both ranges and both sitings,
    on the input recipe: eps is at least 4 times the distance, and the recipe's near ties and clamped values stay under their caps -- asserted on
    the reference alone."""
    kind, maxval, stated, tie_cap = case
    worst, ties, clamps = R.measured(kind, maxval)
    print("rgb_fit reference, %s maxval %d: float32 to float64 distance %.2e (stated %.1e), eps %.0e = %.0fx; near ties %.2f %%, outside the range %.2f %%"
          % (kind, maxval, worst, stated, R.EPS[maxval], R.EPS[maxval] / worst, 100 * ties, 100 * clamps))
    assert 4 * worst <= R.EPS[maxval]
    assert ties <= tie_cap == R.MAX_TIE_FRACTION[kind]
    if kind == "video":
        assert clamps <= R.MAX_CLAMP_FRACTION


def lane_set_frames(th):
    """The frames of tests/test_frame_rgb_fit_gpu.py::test_rows_dealt_to_lane_sets_meet_at_the_chunk_boundaries as (yfit, cbcr), for a tile of `th`
    rows: the CbCr source, U8, 11 rows enlarged to th - 1 and th + 1 (a tile one row short; a full tile and a tile of one row), 20 -> 30 and
    200 -> 300 columns.  An enlarged tile's column span has fewer than 128 strips, so pass 1 deals the tile's rows to two or more lane sets: 30
    columns take 12 strips and 21 sets, chunks of one or two rows; the 256 columns of a full tile at 3/2 take 88 strips and 2 sets."""
    assert 11 <= th - 1 and th + 1 <= 8 * 11, th
    return [R.video_frame(1, 11, w, oh, ow, 255, 0, np.uint8, seed=900 + 2 * k + j) for k, (w, ow) in enumerate([(20, 30), (200, 300)])
            for j, oh in enumerate((th - 1, th + 1))]


@pytest.mark.parametrize("th", range(12, 33))
def test_near_ties_of_the_lane_set_frames_stay_under_the_cap(th):
    """The GPU test reads the tile height from the plan; the kernel's tiles have at most 32 rows and these frames need at least 12.  On the reference
    alone, for every height the frames can take."""
    values = [R.video_values(yfit, cbcr) for yfit, cbcr in lane_set_frames(th)]
    ties = sum(int(R.near_tie(v, R.EPS[255]).sum()) for v in values)
    assert ties <= R.MAX_TIE_FRACTION["video"] * sum(v.size for v in values)


# ---- the host mirror: snn_model_create13 and its resolver, device-free

W, H = 32, 24
NV12, P010, I420, I010 = 0x201, 0x301, 0x401, 0x501
R8, RGB8, RGBA8, RGB16, RGBA16 = 1, 3, 4, 0x103, 0x104


def _io(a=NV12, b=RGB8, maxval=255, shift=0, siting=1, rng=0, kr=0.299, kb=0.114, ow=48, oh=36):
    from shadernn_amd import host

    return host.RgbFitIO(a, b, maxval, shift, siting, rng, kr, kb, ow, oh)


def _refusals():
    """(io, w, h, c, batch) of every request snn_model_create13 refuses before it opens the model file."""
    out = [(None, W, H, 1, 1)]

    def add(io, w=W, h=H, c=1, batch=1):
        out.append((io, w, h, c, batch))

    for a, b, mv in ((NV12, RGB16, 255), (NV12, NV12, 255), (NV12, R8, 255), (NV12, 0, 255), (P010, RGB8, 1023), (I420, RGBA16, 255), (I420, I420, 255), (I010, RGBA8, 1023),
                     (RGB8, RGBA8, 255), (RGBA8, RGB8, 255), (RGB8, NV12, 255), (RGB16, RGB16, 1023), (R8, R8, 255), (0, RGB8, 255), (0x601, RGB8, 255)):
        add(_io(a, b, mv))  # formats that do not pair up
    for ow, oh in ((0, 36), (48, 0), (-2, 36), (48, -1)):  # below 1
        add(_io(ow=ow, oh=oh)), add(_io(RGB8, RGB8, ow=ow, oh=oh))
    for ow, oh in ((15, 36), (129, 36), (48, 11), (48, 97)):  # video in: out / in outside [1/2, 4]
        add(_io(ow=ow, oh=oh)), add(_io(I010, RGB16, 1023, ow=ow, oh=oh))
    for ow, oh in ((31, 36), (129, 36), (48, 23), (48, 97), (16, 12)):  # RGB in: outside [1, 4]
        add(_io(RGB8, RGB8, ow=ow, oh=oh)), add(_io(RGBA8, RGBA8, ow=ow, oh=oh))
    # what snn_model_create9 / snn_model_create12 refuse: an odd input extent, an unknown siting or range, a depth that does not fit, a bad matrix
    good = _io()
    add(good, w=31), add(good, h=23), add(good, c=3), add(good, batch=0), add(good, w=0)
    add(_io(siting=2)), add(_io(rng=2)), add(_io(maxval=256)), add(_io(maxval=127)), add(_io(shift=1)), add(_io(P010, RGB16, 65535)), add(_io(P010, RGB16, 1023, 7))
    add(_io(I420, RGB8, siting=-1)), add(_io(I010, RGB16, 1000))
    for a, b in ((NV12, RGB8), (I420, RGBA8), (RGB8, RGB8)):
        add(_io(a, b, kr=0.0)), add(_io(a, b, kb=-0.1)), add(_io(a, b, kr=0.7, kb=0.3))
    add(_io(RGB8, RGB8), c=3), add(_io(RGB8, RGB8), batch=0)  # what snn_model_create7 refuses
    return out


def test_the_host_mirror_declares_binds_and_refuses_without_a_device(built):
    from shadernn_amd import host

    mirror = re.sub(r"/\*.*?\*/", "", _read("include/snn_c.h"), flags=re.S)
    assert re.search(r"\bsnn_model_create13\s*\(", mirror) and "snn_rgb_fit_io" in mirror
    assert "snn_model_create13" in host.SIGNATURES and hasattr(host.lib(), "snn_model_create13")
    assert C.sizeof(host.RgbFitIO) == 10 * 4
    assert [n for n, _ in host.RgbFitIO._fields_] == ["in_format", "out_format", "maxval", "shift", "siting", "range", "kr", "kb", "out_w", "out_h"]
    assert C.sizeof(host.PlanarIO) == 10 * 4 and C.sizeof(host.VideoRgbIO) == 8 * 4 and C.sizeof(host.FitIO) == 10 * 4  # the earlier structs keep their layout
    h = C.c_void_p()
    cases = _refusals()
    assert len(cases) > 60
    for io, w, hh, c, batch in cases:
        key = None if io is None else tuple(getattr(io, n) for n, _ in host.RgbFitIO._fields_)
        rc = host.lib().snn_model_create13(b"/nonexistent/model.json", 0, w, hh, c, 0, 1, 0, 0, 0, batch, None if io is None else C.byref(io), C.byref(h))
        assert rc == -1, (key, w, hh, c, batch)  # (-2 would be the model file: the request got past the resolver)
        assert host.frames_resolve(13, io, w, hh, c, batch) is None, (key, w, hh, c, batch)


def test_the_resolved_model_is_that_of_create9_and_create7(built):
    from shadernn_amd import host

    def model_part(line):
        assert line is not None
        return line.split(" | ")[0]

    for a, b, mv, sh in ((NV12, RGB8, 255, 0), (NV12, RGBA8, 255, 0), (P010, RGB16, 1023, 6), (P010, RGBA16, 1023, 6), (NV12 + 0x100, RGB16, 4095, 0)):
        for rng in (0, 1):
            for ow, oh in ((48, 36), (64, 48), (40, 36), (47, 35), (16, 12), (128, 96)):
                line = host.frames_resolve(13, _io(a, b, mv, sh, 1, rng, ow=ow, oh=oh), W, H, 1)
                want = host.frames_resolve(9, host.VideoRgbIO(a, b, mv, sh, 1, rng, 0.299, 0.114), W, H, 1)
                assert model_part(line) == model_part(want)
                assert "sink=rgb_from_yuv_fitted" in line and "fit=%dx%d planar=0 | entry=snn_model_create13" % (ow, oh) in line
                # ... and the frame ends are create9's but for the sink and the size
                assert line.split(" | ")[1].replace("rgb_from_yuv_fitted", "rgb_from_yuv").replace("fit=%dx%d" % (ow, oh), "fit=0x0") == want.split(" | ")[1]
    for a, b, mv in ((I420, RGB8, 255), (I420, RGBA8, 255), (I010, RGB16, 1023)):
        line = host.frames_resolve(13, _io(a, b, mv, ow=47, oh=35), W, H, 1)
        want = host.frames_resolve(12, host.PlanarIO(a, b, mv, 0, 1, 0, 0.299, 0.114, 0, 0), W, H, 1)
        nv = host.frames_resolve(9, host.VideoRgbIO(a - 0x200, b, mv, 0, 1, 0, 0.299, 0.114), W, H, 1)
        assert model_part(line) == model_part(want) == model_part(nv)
        assert "sink=rgb_from_yuv_fitted" in line and "fit=47x35 planar=1 | entry=snn_model_create13" in line
    for fmt in (RGB8, RGBA8):
        for ow, oh in ((32, 24), (48, 36), (47, 35), (128, 96)):
            line = host.frames_resolve(13, _io(fmt, fmt, ow=ow, oh=oh), W, H, 1)
            want = host.frames_resolve(7, host.ColourIO(fmt, 0.299, 0.114, 0.0, 1.0 / 255.0, 255.0, 0.0), W, H, 1)
            assert model_part(line) == model_part(want)
            assert "source=rgb sink=rgb_merged_fitted channels=%d" % fmt in line and "fit=%dx%d planar=0 | entry=snn_model_create13" % (ow, oh) in line
    # the earlier entry points resolve as before: create12 still refuses a fitted size together with an RGB end
    assert host.frames_resolve(12, host.PlanarIO(I420, RGB8, 255, 0, 1, 0, 0.299, 0.114, 48, 36), W, H, 1) is None
    assert "sink=fitted" in host.frames_resolve(11, host.FitIO(host.VideoIO(NV12, 255, 0, 1, 16.0, 1 / 219.0, 219.0, 16.0), 48, 36), W, H, 1)


def test_host_model_argument_checks():
    from shadernn_amd import host

    bad = [dict(rgb_size=(48, 36)), dict(video="NV12", rgb_size=(48, 36)), dict(video="NV12", video_out="RGB8", out_size=(48, 36), rgb_size=(48, 36)),
           dict(colour="RGB8", video_out="NV12", rgb_size=(48, 36)), dict(colour="RGB8", video="NV12", video_out="RGB8", rgb_size=(48, 36)),
           dict(input_format="R8", output_format="R8", rgb_size=(48, 36)), dict(colour="RGB8", output_format="RGB8", rgb_size=(48, 36)),
           dict(video="NV12", video_out="NV12", rgb_size=(48, 36)), dict(video="P010", video_out="RGB8", rgb_size=(48, 36)), dict(colour="R8", rgb_size=(48, 36)),
           dict(video="NV12", out_size=(48, 36), rgb_size=(48, 36))]
    for kw in bad:
        with pytest.raises(AssertionError, match="rgb_size|come back as|out_size"):
            host.Model("/nonexistent/model.json", 32, 24, 1, **kw)
    with pytest.raises(AssertionError, match="out_size"):  # the earlier keyword keeps its rule
        host.Model("/nonexistent/model.json", 32, 24, 1, video="NV12", video_out="RGB8", out_size=(48, 36))
