"""Video frames in front of RGB models, the CPU side: the entry points are declared, exported and bound and the structs have their sizes;
snnhip_yuv_tensor_taps against the sampling rule in exact rational arithmetic, and its refusals; the float64 reference of tests/yuv_tensor_ref.py
against a per-pixel statement of the contract and, at ratio 1, against yuv_rgb's bytes; the fp32-to-float64 distance on exactly the frames of the GPU
sweeps, which sets their tolerance; every device-free snn_model_create14 refusal, the resolved lines of the earlier entry points, host.Model's
argument checks; the build list and the documents name the unit."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import yuv_rgb_ref
import yuv_tensor_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(2, 1), (2, 2), (2, 5), (2, 3), (48, 5), (64, 7), (6, 6), (8, 8), (1080, 224), (1920, 224), (1080, 416), (720, 720), (7, 19), (1, 3), (3, 1), (100, 33)]


def _read(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi

    header = re.sub(r"/\*.*?\*/", "", _read("include/snnhip.h"), flags=re.S)
    lib = C.CDLL(snn.load_library())
    for name in ("snnhip_yuv_tensor_plan_create", "snnhip_yuv_tensor_planar_plan_create", "snnhip_yuv_tensor_taps"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    assert "snnhip_yuv_tensor_desc" in header
    for name, value in (("SNNHIP_YUV_TENSOR_NEAREST", 0), ("SNNHIP_YUV_TENSOR_LINEAR", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert capi.YUV_TENSOR_FILTER == {"nearest": 0, "linear": 1}
    for f in (capi.yuv_tensor_plan, capi.yuv_tensor_taps, snn.yuv_tensor_plan, snn.yuv_tensor_taps):
        assert callable(f)
    assert C.sizeof(capi.YuvTensorDesc) == 22 * 4
    assert [n for n, _ in capi.YuvTensorDesc._fields_] == ["N", "H", "W", "OH", "OW", "C", "src_dtype", "out_dtype", "maxval", "shift", "siting", "range", "kr", "kb", "filter",
                                                            "means", "norms", "alpha"]
    assert C.sizeof(capi.RgbFitDesc) == 14 * 4 and C.sizeof(capi.YuvRgbDesc) == 12 * 4  # the earlier structs keep their layout


def test_the_build_list_and_the_documents_name_the_unit():
    assert '"frame_yuv_tensor.hip"' in _read("__graft_entry__.py")
    assert "frame_yuv_tensor.hip" in _read("README.md") and "4.26" in _read("DESIGN.md") and "snn_model_create14" in _read("INTEGRATION.md")


@pytest.mark.parametrize("pair", PAIRS, ids=["%dto%d" % p for p in PAIRS])
def test_the_tap_table_is_the_rule_in_exact_rational_arithmetic(built, pair):
    from shadernn_amd import capi

    n_in, n_out = pair
    a, idx = capi.yuv_tensor_taps(n_in, n_out, "linear")
    assert a.dtype == np.float32 and a.shape == (n_out,) and idx.shape == (n_out, 2)
    for o in range(n_out):
        u = (Fraction(o) + Fraction(1, 2)) * n_in / n_out - Fraction(1, 2)  # resize's rule
        i0 = u.numerator // u.denominator  # floor
        assert a[o] == np.float32(float(u - i0)), (o, a[o], u)
        assert 0.0 <= a[o] < 1.0
        assert tuple(idx[o]) == (min(max(i0, 0), n_in - 1), min(max(i0 + 1, 0), n_in - 1)), o
        if u.denominator == 1:
            assert a[o] == 0.0  # an integer position: the second pixel has weight 0
    near, nidx = capi.yuv_tensor_taps(n_in, n_out, "nearest")
    assert not near.any()
    for o in range(n_out):
        want = ((2 * o + 1) * n_in) // (2 * n_out)
        assert tuple(nidx[o]) == (want, want) and 0 <= want < n_in
    # ... and the reference's own table is the same one
    ra, ridx = R.taps(n_in, n_out, "linear")
    assert ra.tobytes() == a.tobytes() and (ridx == idx).all()
    assert (R.taps(n_in, n_out, "nearest")[1] == nidx).all()
    if n_in == n_out:
        assert not a.any() and (idx[:, 0] == np.arange(n_out)).all()  # ratio 1: every output pixel is its own source pixel


def test_the_tap_table_refuses_with_a_message(built):
    from shadernn_amd import capi

    lib = capi.lib()
    w = (C.c_float * 16)()
    idx = (C.c_int * 32)()
    wp = C.cast(w, C.POINTER(C.c_float))
    for args, needle in (((0, 4, 1, wp, idx, 16), "0 inputs"), ((4, 0, 1, wp, idx, 16), "0 outputs"), ((-4, 4, 1, wp, idx, 16), "-4 inputs"), ((4, -1, 1, wp, idx, 16), "-1 outputs"),
                         ((4, 4, 2, wp, idx, 16), "filter 2"), ((4, 4, -1, wp, idx, 16), "filter -1"), ((4, 8, 1, wp, idx, 7), "room for 7"), ((4, 8, 0, wp, idx, -1), "room for -1"),
                         ((4, 4, 1, None, idx, 16), "null"), ((4, 4, 1, wp, None, 16), "null"), (((1 << 30) + 1, 4, 1, wp, idx, 16), "2^30")):
        assert lib.snnhip_yuv_tensor_taps(*args) == capi.E_INVALID, args
        assert needle in lib.snnhip_last_error().decode(), (args, lib.snnhip_last_error())
    assert lib.snnhip_yuv_tensor_taps(4, 16, 1, wp, idx, 16) == 0  # exactly enough room


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_the_reference_is_the_contract_pixel_by_pixel(depth):
    """A 6 x 8 frame (six rows of eight luma pixels) to 5 x 7, to 9 x 11 and to itself, both filters: the vectorised reference against the per-pixel
    statement from the 4:2:0 tap table and the matrix.  Both are float64: they differ by the order of a few sums."""
    container, maxval, shift = depth
    means, norms = R.normalisation(1, maxval)
    for k, (oh, ow) in enumerate([(5, 7), (9, 11), (6, 8)]):
        for si, siting in enumerate(R.SITINGS):
            y, cbcr = R.frame(2, 6, 8, maxval, shift, np.uint8 if container == "u8" else np.uint16, seed=10 * k + si, whole_range=bool(k % 2))
            for flt in ("linear", "nearest"):
                for rng, (kr, kb) in (("limited", R.BT601), ("full", R.BT709)):
                    want = R.brute(y, cbcr, oh, ow, flt, siting, rng, maxval, shift, kr, kb, means, norms)
                    got = R.tensor(y, cbcr, oh, ow, 3, flt, siting, rng, maxval, shift, kr, kb, means, norms)
                    assert np.abs(got - want).max() <= 1e-9 * maxval * np.abs(np.asarray(norms)).max()
    y, cbcr = R.frame(1, 6, 8, maxval, shift, np.uint8 if container == "u8" else np.uint16, seed=3)
    t = R.tensor(y, cbcr, 6, 8, 4, maxval=maxval, shift=shift, alpha=0.25)
    assert (t[..., 3] == 0.25).all() and np.array_equal(t[..., :3], R.source(y, cbcr, maxval=maxval, shift=shift))  # ratio 1: the source pixel itself


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_ratio_one_rounds_to_the_bytes_of_yuv_rgb(depth):
    """rint of the reference at OH = H, OW = W, means 0, norms 1 against yuv_rgb_ref.rgb(r = 1) off the near ties; the near ties of exactly the frames
    the GPU test uses are at most 1 % of their values."""
    container, maxval, shift = depth
    items = []
    for y, cbcr, siting, rng in R.ratio1_cases(container, maxval, shift):
        n, h, w, _ = y.shape
        t = R.tensor(y, cbcr, h, w, 3, "linear", siting, rng, maxval, shift)
        assert np.array_equal(t, R.tensor(y, cbcr, h, w, 3, "nearest", siting, rng, maxval, shift))
        fixed = yuv_rgb_ref.rgb(y, cbcr, 1, 3, siting, rng, maxval, shift).astype(np.int64) >> shift
        items.append((np.rint(t), fixed, R.source(y, cbcr, siting, rng, maxval, shift)))
    frac, ndiff = R.compare_ratio1(items, maxval)
    print("ratio 1, %s maxval=%d shift=%d, %d frames: near ties %.3f %% (cap %.0f %%), %d values differ" % (container, maxval, shift, len(items), 100 * frac,
                                                                                                          100 * R.MAX_TIE_FRACTION, ndiff))
    assert ndiff == 0  # the reference against itself: clamping before or behind the rounding is the same


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_the_measured_fp32_distance_sets_the_tolerance(depth):
    """The reference in float32 against itself in float64 on exactly the frames of the GPU sweeps, per unit of |norm|: E is four times this, and
    stays under the family's near-tie eps (above it the expression would have a defect to find)."""
    container, maxval, shift = depth
    d = R.measured_distance(container, maxval, shift)
    print("yuv_tensor reference, %s maxval=%d shift=%d: float32 to float64 distance %.3e (stated %.1e), E = %.2e, the family's eps %.0e" % (container, maxval, shift, d,
                                                                                                                                        R.MEASURED_DISTANCE[maxval], R.E[maxval], R.EPS[maxval]))
    assert np.isfinite(d) and d > 0
    assert 0.75 * R.MEASURED_DISTANCE[maxval] <= max(R.measured_distance(c, m, s) for c, m, s in R.DEPTHS if m == maxval) <= R.MEASURED_DISTANCE[maxval]
    assert R.E[maxval] == 4 * R.MEASURED_DISTANCE[maxval] and R.E[maxval] < R.EPS[maxval]


def test_the_sweeps_hold_the_cases_the_contract_names():
    for (c, half), tile in R.TILE.items():
        shapes = R.shapes(c, half)
        assert {(1, 2, 2, 1, 1), (1, 2, 2, 2, 2), (1, 2, 2, 5, 3), (1, 48, 64, 5, 7), (1, 6, 8, 6, 8)} <= set(shapes)
        flat = [n * oh * ow for n, _, _, oh, ow in shapes]
        assert tile in flat and tile + 1 in flat  # one tile, one tile and a pixel
        n, h, w, oh, ow = shapes[-1]
        assert n == 2 and ow % 2 == 1 and (oh * ow) % 2 == 1 and oh * ow > tile and (tile % ow) != 0  # a seam inside a row, rows and images off a dword for fp16 RGB
        cases = list(R.sweep_cases(c, half, "u8", 255, 0))
        assert {x[1] for x in cases} == {"linear", "nearest"} and {x[2] for x in cases} == set(R.SITINGS) and {x[3] for x in cases} == set(R.RANGES)
        assert {x[4] for x in cases} == {R.BT601, R.BT709} and {x[5] for x in cases} == {False, True}
        assert len({x[6] for x in cases}) == 3


# ---- the host mirror: snn_model_create14 and its resolver, device-free

W, H = 16, 12
NV12, P010, I420, I010 = 0x201, 0x301, 0x401, 0x501
R8, RGB8, RGBA8, RGB16 = 1, 3, 4, 0x103


def _io(a=NV12, b=0, sw=64, sh=48, maxval=255, shift=0, siting=1, rng=0, kr=0.299, kb=0.114, flt=1):
    from shadernn_amd import host

    four = lambda *v: (C.c_float * 4)(*v)  # noqa: E731
    return host.VideoTensorIO(a, b, sw, sh, maxval, shift, siting, rng, kr, kb, flt, four(0, 0, 0, 0), four(1, 1, 1, 1), 1.0, four(255, 255, 255, 255), four(0, 0, 0, 0))


def _refusals():
    """(io, w, h, c, batch) of every request snn_model_create14 refuses before it opens the model file."""
    out = [(None, W, H, 3, 1)]

    def add(io, w=W, h=H, c=3, batch=1):
        out.append((io, w, h, c, batch))

    for a in (0, R8, RGB8, RGBA8, RGB16, 0x601, -1):
        add(_io(a))  # unknown input formats
    for b in (NV12, I420, RGB16, 0x104, 0x101, 7, -1):
        add(_io(b=b))  # an output format that is neither float nor an 8-bit frame
    good = _io()
    add(good, c=1), add(good, c=2), add(good, c=5), add(good, c=0)  # in_c outside {3, 4}
    for sw, sh in ((63, 48), (64, 47), (0, 48), (64, 0), (-64, 48), (64, -2), (1, 1)):
        add(_io(sw=sw, sh=sh)), add(_io(I010, sw=sw, sh=sh, maxval=1023))  # odd or non-positive src_w / src_h
    add(good, w=0), add(good, h=0), add(good, w=-1), add(good, batch=0), add(good, batch=-1)
    add(_io(flt=2)), add(_io(flt=-1))
    # everything the plan refuses
    add(_io(siting=2)), add(_io(siting=-1)), add(_io(rng=2)), add(_io(rng=-1))
    add(_io(maxval=256)), add(_io(maxval=127)), add(_io(maxval=1023)), add(_io(shift=1)), add(_io(P010, maxval=65535)), add(_io(P010, maxval=1023, shift=7))
    add(_io(I010, maxval=1000)), add(_io(I010, maxval=8191)), add(_io(I420, shift=-1))
    for a in (NV12, I420):
        add(_io(a, kr=0.0)), add(_io(a, kb=-0.1)), add(_io(a, kr=0.7, kb=0.3))
    return out


def test_the_host_mirror_declares_binds_and_refuses_without_a_device(built):
    from shadernn_amd import host

    mirror = re.sub(r"/\*.*?\*/", "", _read("include/snn_c.h"), flags=re.S)
    assert re.search(r"\bsnn_model_create14\s*\(", mirror) and "snn_video_tensor_io" in mirror and re.search(r"\bsnn_model_download_input\s*\(", mirror)
    for name in ("snn_model_create14", "snn_model_download_input"):
        assert name in host.SIGNATURES and hasattr(host.lib(), name)
    assert C.sizeof(host.VideoTensorIO) == 28 * 4
    assert [n for n, _ in host.VideoTensorIO._fields_] == ["in_format", "out_format", "src_w", "src_h", "maxval", "shift", "siting", "range", "kr", "kb", "filter", "means", "norms",
                                                            "alpha", "out_scale", "out_offset"]
    assert C.sizeof(host.RgbFitIO) == 10 * 4 and C.sizeof(host.PlanarIO) == 10 * 4 and C.sizeof(host.VideoRgbIO) == 8 * 4 and C.sizeof(host.FrameIO) == 18 * 4  # the earlier structs keep their layout
    h = C.c_void_p()
    cases = _refusals()
    assert len(cases) > 50
    for io, w, hh, c, batch in cases:
        key = None if io is None else tuple(getattr(io, n) for n, _ in host.VideoTensorIO._fields_[:11])
        rc = host.lib().snn_model_create14(b"/nonexistent/model.json", 0, w, hh, c, 0, 1, 0, 0, 0, batch, None if io is None else C.byref(io), C.byref(h))
        assert rc == -1, (key, w, hh, c, batch)  # (-2 would be the model file: the request got past the resolver)
        assert host.frames_resolve(14, io, w, hh, c, batch) is None, (key, w, hh, c, batch)


def test_the_resolved_model_is_that_of_create4_and_create5(built):
    from shadernn_amd import host

    for a, mv, sh, planar in ((NV12, 255, 0, 0), (P010, 1023, 6, 0), (I420, 255, 0, 1), (I010, 1023, 0, 1), (P010, 4095, 0, 0)):
        for c in (3, 4):
            line = host.frames_resolve(14, _io(a, 0, 1920, 1080, mv, sh), 224, 224, c, 2)
            want = host.frames_resolve(5, None, 224, 224, c, 2)  # snn_model_create4 resolves as snn_model_create5 with a null struct
            assert line.split(" | ")[0] == want.split(" | ")[0]
            assert "source=yuv420_tensor sink=model channels=%d wide=%d maxval=%d shift=%d siting=1 range=0" % (c, 1 if a & 0x100 else 0, mv, sh) in line
            assert "planar=%d | entry=snn_model_create14 | src=1920x1080 filter=1 tensor_means=0,0,0 tensor_norms=1,1,1 alpha=1" % planar in line
    io = _io(NV12, RGB8)
    line = host.frames_resolve(14, io, W, H, 3)
    four = lambda *v: (C.c_float * 4)(*v)  # noqa: E731
    want = host.frames_resolve(5, host.FrameIO(0, RGB8, four(0, 0, 0, 0), four(1, 1, 1, 1), four(255, 255, 255, 255), four(0, 0, 0, 0)), W, H, 3)
    assert line.split(" | ")[0] == want.split(" | ")[0] and "out=0x3" in line


# one request through each earlier entry point and the line it resolved to before snn_model_create14 existed
EARLIER_LINES = {
    5: 'in=0x1 out=0x1 means=1,2,3,4 norms=0.5,0.25,2,1 scale=255,254,253,252 offset=0,1,2,3 in_shift=0 out_maxval=65535 out_shift=0 | source=model sink=model channels=0 wide=0 maxval=255 shift=0 siting=1 range=0 kr=0.298999995 kb=0.114 fit=0x0 planar=0 | entry=snn_model_create5',
    6: 'in=0x101 out=0x101 means=64,0,0,0 norms=0.00114155246,1,1,1 scale=876,1,1,1 offset=64,0,0,0 in_shift=6 out_maxval=1023 out_shift=6 | source=model sink=model channels=0 wide=0 maxval=255 shift=0 siting=1 range=0 kr=0.298999995 kb=0.114 fit=0x0 planar=0 | entry=snn_model_create6',
    7: 'in=0x1 out=0x1 means=0,0,0,0 norms=0.00392156886,0.00392156886,0.00392156886,0.00392156886 scale=255,255,255,255 offset=0,0,0,0 in_shift=0 out_maxval=65535 out_shift=0 | source=rgb sink=rgb_merged channels=4 wide=0 maxval=255 shift=0 siting=1 range=0 kr=0.212599993 kb=0.0722000003 fit=0x0 planar=0 | entry=snn_model_create7',
    8: 'in=0x1 out=0x1 means=16,16,16,16 norms=0.00456620986,0.00456620986,0.00456620986,0.00456620986 scale=219,219,219,219 offset=16,16,16,16 in_shift=0 out_maxval=65535 out_shift=0 | source=yuv420 sink=chroma_up channels=0 wide=0 maxval=255 shift=0 siting=1 range=0 kr=0.298999995 kb=0.114 fit=0x0 planar=0 | entry=snn_model_create8',
    9: 'in=0x101 out=0x101 means=0,0,0,0 norms=0.000977517106,0.000977517106,0.000977517106,0.000977517106 scale=1023,1023,1023,1023 offset=0,0,0,0 in_shift=6 out_maxval=1023 out_shift=6 | source=yuv420 sink=rgb_from_yuv channels=4 wide=1 maxval=1023 shift=6 siting=0 range=1 kr=0.212599993 kb=0.0722000003 fit=0x0 planar=0 | entry=snn_model_create9',
    10: 'in=0x1 out=0x1 means=0,0,0,0 norms=0.00392156886,0.00392156886,0.00392156886,0.00392156886 scale=219,219,219,219 offset=16,16,16,16 in_shift=0 out_maxval=65535 out_shift=0 | source=rgb sink=yuv420_from_rgb channels=3 wide=0 maxval=255 shift=0 siting=1 range=0 kr=0.298999995 kb=0.114 fit=0x0 planar=0 | entry=snn_model_create10',
    11: 'in=0x1 out=0x1 means=16,16,16,16 norms=0.00456620986,0.00456620986,0.00456620986,0.00456620986 scale=219,219,219,219 offset=16,16,16,16 in_shift=0 out_maxval=65535 out_shift=0 | source=yuv420 sink=fitted channels=0 wide=0 maxval=255 shift=0 siting=1 range=0 kr=0.298999995 kb=0.114 fit=48x36 planar=0 | entry=snn_model_create11',
    12: 'in=0x101 out=0x101 means=64,64,64,64 norms=0.00114155246,0.00114155246,0.00114155246,0.00114155246 scale=876,876,876,876 offset=64,64,64,64 in_shift=0 out_maxval=1023 out_shift=0 | source=yuv420 sink=fitted channels=0 wide=1 maxval=1023 shift=0 siting=1 range=0 kr=0.298999995 kb=0.114 fit=40x30 planar=1 | entry=snn_model_create12',
    13: 'in=0x1 out=0x1 means=0,0,0,0 norms=0.00392156886,0.00392156886,0.00392156886,0.00392156886 scale=255,255,255,255 offset=0,0,0,0 in_shift=0 out_maxval=65535 out_shift=0 | source=yuv420 sink=rgb_from_yuv_fitted channels=3 wide=0 maxval=255 shift=0 siting=1 range=1 kr=0.298999995 kb=0.114 fit=47x35 planar=1 | entry=snn_model_create13',
}


def _earlier_requests():
    from shadernn_amd import host

    four = lambda *v: (C.c_float * 4)(*v)  # noqa: E731
    video = host.VideoIO(NV12, 255, 0, 1, 16.0, 1 / 219.0, 219.0, 16.0)
    return {5: (host.FrameIO(R8, R8, four(1, 2, 3, 4), four(0.5, 0.25, 2, 1), four(255, 254, 253, 252), four(0, 1, 2, 3)), 1),
            6: (host.FrameIO2(0x101, 0x101, four(64, 0, 0, 0), four(1 / 876.0, 1, 1, 1), four(876, 1, 1, 1), four(64, 0, 0, 0), 6, 1023, 6), 1),
            7: (host.ColourIO(RGBA8, 0.2126, 0.0722, 0.0, 1 / 255.0, 255.0, 0.0), 1),
            8: (video, 1),
            9: (host.VideoRgbIO(P010, 0x104, 1023, 6, 0, 1, 0.2126, 0.0722), 1),
            10: (host.EncodeIO(RGB8, NV12, 1, 0, 0.299, 0.114), 1),
            11: (host.FitIO(video, 48, 36), 1),
            12: (host.PlanarIO(I010, I010, 1023, 0, 1, 0, 0.299, 0.114, 40, 30), 1),
            13: (host.RgbFitIO(I420, RGB8, 255, 0, 1, 1, 0.299, 0.114, 47, 35), 1)}


def test_the_resolved_lines_of_the_earlier_entry_points_are_unchanged(built):
    from shadernn_amd import host

    for entry, (io, c) in _earlier_requests().items():
        assert host.frames_resolve(entry, io, 32, 24, c, 2) == EARLIER_LINES[entry], entry


def test_host_model_argument_checks():
    from shadernn_amd import host

    ok = dict(video="NV12", frame_size=(64, 48))
    bad = [dict(frame_size=(64, 48)), dict(ok, video="RGB8"), dict(ok, video_out="RGB8"), dict(ok, colour="RGB8"), dict(ok, out_size=(32, 24)), dict(ok, rgb_size=(32, 24)),
           dict(ok, input_format="RGB8"), dict(ok, output_format="RGB16"), dict(ok, output_format="NV12"), dict(ok, frame_size=(63, 48)), dict(ok, frame_size=(64, 47)),
           dict(ok, frame_size=(0, 48)), dict(ok, frame_size=(64, -2)), dict(ok, video_range="tv"), dict(ok, siting="right"), dict(ok, video_filter="cubic"), dict(ok, kr=0.0),
           dict(ok, kr=0.7, kb=0.3)]
    for kw in bad:
        with pytest.raises(AssertionError, match="frame_size|8-bit frame|even extent|video_range|siting|video_filter|kr"):
            host.Model("/nonexistent/model.json", 16, 12, 3, **kw)
    for c in (1, 2, 5):
        with pytest.raises(AssertionError, match="3 \\(RGB\\) or 4"):
            host.Model("/nonexistent/model.json", 16, 12, c, **ok)
    with pytest.raises(AssertionError, match="rgb_size"):  # the earlier keywords keep their rules
        host.Model("/nonexistent/model.json", 32, 24, 1, video="NV12", rgb_size=(48, 36))
