"""Encoder frames behind RGB models, the CPU side: the entry points are declared, exported and bound and the structs have their sizes;
snnhip_tensor_yuv_coefficients against the formula in double, as the reciprocals of snnhip_yuv_rgb_coefficients' and its refusals; the float64
reference of tests/tensor_yuv_ref.py against a per-sample statement of the contract and, on a 2 x 2-replicated frame, against rgb_cbcr_ref; the
fp32-to-float64 distance and the near-tie share on exactly the frames of the GPU sweeps; every device-free snn_model_create15 refusal, the resolved
lines of the earlier entry points, host.Model's argument checks; the build list and the documents name the unit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rgb_cbcr_ref
import tensor_yuv_ref as R
import yuv_rgb_ref
from test_frame_yuv_tensor import EARLIER_LINES, _earlier_requests
from test_frame_yuv_tensor import _io as _video_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRICES = (R.BT601, R.BT709)


def _read(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi

    header = re.sub(r"/\*.*?\*/", "", _read("include/snnhip.h"), flags=re.S)
    lib = C.CDLL(snn.load_library())
    for name in ("snnhip_tensor_yuv_plan_create", "snnhip_tensor_yuv_planar_plan_create", "snnhip_tensor_yuv_coefficients", "snnhip_plan_run_io"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    assert "snnhip_tensor_yuv_desc" in header
    for f in (capi.tensor_yuv_plan, capi.tensor_yuv_coefficients, snn.tensor_yuv_plan, snn.tensor_yuv_coefficients, capi.Plan.run_io):
        assert callable(f)
    assert C.sizeof(capi.TensorYuvDesc) == 18 * 4
    assert [n for n, _ in capi.TensorYuvDesc._fields_] == ["N", "H", "W", "C", "in_dtype", "out_dtype", "maxval", "shift", "siting", "range", "kr", "kb", "scale", "offset"]
    assert C.sizeof(capi.YuvTensorDesc) == 22 * 4 and C.sizeof(capi.RgbFitDesc) == 14 * 4 and C.sizeof(capi.YuvRgbDesc) == 12 * 4  # the earlier structs keep their layout


def test_the_build_list_and_the_documents_name_the_unit():
    assert '"frame_tensor_yuv.hip"' in _read("__graft_entry__.py")
    assert "frame_tensor_yuv.hip" in _read("README.md") and "4.27" in _read("DESIGN.md") and "snn_model_create15" in _read("INTEGRATION.md")
    for header in ("include/snnhip.h", "include/snn_c.h"):
        assert "Not offered: resizing at this end" in _read(header), header


@pytest.mark.parametrize("maxval", [255, 1023, 4095])
def test_the_coefficients_are_the_formula_and_the_reciprocals_of_yuv_rgbs(built, maxval):
    from shadernn_amd import capi

    k = (maxval + 1) / 256.0
    for rng in ("limited", "full"):
        for kr, kb in MATRICES:
            got = capi.tensor_yuv_coefficients(maxval, rng, kr, kb)
            assert got.dtype == np.float32 and got.shape == (5,)
            kr32, kb32 = float(np.float32(kr)), float(np.float32(kb))
            yoff, yrange, crange = (16 * k, 219 * k, 224 * k) if rng == "limited" else (0.0, float(maxval), float(maxval))
            want = np.array([yoff, yrange / maxval, 128 * k, crange / (2 * (1 - kb32) * maxval), crange / (2 * (1 - kr32) * maxval)], np.float64).astype(np.float32)
            assert got.tobytes() == want.tobytes(), (got, want)
            assert got.tobytes() == R.coefficients(maxval, rng, kr, kb).tobytes()  # ... and the reference's own are the same five
            theirs = capi.yuv_rgb_coefficients(maxval, rng, kr, kb)  # Yoff, Coff, cy, crv, cbu, cgv, cgu
            assert got[0] == theirs[0] and got[2] == theirs[1]
            for mine, inverse in ((got[1], theirs[2]), (got[3], theirs[4]), (got[4], theirs[3])):  # ys = 1 / cy, cbs = 1 / cbu, crs = 1 / crv
                exact = 1.0 / float(inverse)
                assert abs(float(mine) - exact) <= float(np.spacing(np.float32(exact))), (mine, inverse)  # to one ulp
    if maxval == 255:  # at 8 bits the two chroma scales are rgb_cbcr's
        for rng in ("limited", "full"):
            assert capi.tensor_yuv_coefficients(255, rng)[2:].tobytes() == capi.rgb_cbcr_coefficients(rng).tobytes()


def test_the_coefficients_refuse_with_a_message(built):
    from shadernn_amd import capi

    lib = capi.lib()
    out = (C.c_float * 8)()
    op = C.cast(out, C.POINTER(C.c_float))
    for args, needle in (((255, 0, 0.299, 0.114, None, 5), "null"), ((255, 0, 0.299, 0.114, op, 4), "room for 4"), ((255, 0, 0.299, 0.114, op, -1), "room for -1"),
                         ((127, 0, 0.299, 0.114, op, 5), "maxval 127"), ((256, 0, 0.299, 0.114, op, 5), "maxval 256"), ((1000, 0, 0.299, 0.114, op, 5), "maxval 1000"),
                         ((0, 0, 0.299, 0.114, op, 5), "maxval 0"), ((65536, 0, 0.299, 0.114, op, 5), "maxval 65536"), ((255, 2, 0.299, 0.114, op, 5), "range 2"),
                         ((255, -1, 0.299, 0.114, op, 5), "range -1"), ((255, 0, 0.0, 0.114, op, 5), "kr"), ((255, 0, 0.299, -0.1, op, 5), "kb"), ((255, 0, 0.7, 0.3, op, 5), "kr + kb < 1")):
        assert lib.snnhip_tensor_yuv_coefficients(*args) == capi.E_INVALID, args
        msg = lib.snnhip_last_error().decode()
        assert msg.startswith("tensor_yuv_coefficients") and needle in msg, (args, msg)
    assert lib.snnhip_tensor_yuv_coefficients(255, 0, 0.299, 0.114, op, 5) == 0  # exactly enough room


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_the_reference_is_the_contract_sample_by_sample(depth):
    """Small frames, both sitings (column 0 of the left-sited filter among them), both ranges, every output map, fp32 and fp16 tensors: the vectorised
    reference against the statement with explicit loops.  Both are float64: they differ by the order of a few sums."""
    container, maxval, shift = depth
    for k, (n, h, w) in enumerate([(1, 2, 2), (2, 4, 6), (1, 6, 10)]):
        for siting in R.SITINGS:
            for rng, (kr, kb) in (("limited", R.BT601), ("full", R.BT709)):
                scale, offset = R.output_map(k, maxval)
                for half in (False, True):
                    x = R.tensor(n, h, w, 3 + k % 2, half, maxval, scale, offset, seed=10 * k + half)
                    got = R.values(x, scale, offset, siting, rng, maxval, kr, kb)
                    want = R.brute(x, scale, offset, siting, rng, maxval, kr, kb)
                    for a, b in zip(got, want):
                        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-9 * maxval
                    y, c = R.planes(x, scale, offset, siting, rng, maxval, shift, kr, kb)
                    assert y.dtype == c.dtype == (np.uint8 if container == "u8" else np.uint16) and y.shape == (n, h, w, 1) and c.shape == (n, h // 2, w // 2, 2)
                    assert not ((y | c.max()) & ((1 << shift) - 1)).any()


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_grey_and_constant_tensors(depth):
    container, maxval, shift = depth
    k = (maxval + 1) // 256
    g = np.random.default_rng(2)
    grey = np.repeat(g.uniform(-0.1 * maxval, 1.1 * maxval, size=(2, 6, 10, 1)), 3, axis=3).astype(np.float32)
    const = np.broadcast_to(g.uniform(0, maxval, size=(1, 1, 1, 3)), (2, 6, 10, 3)).astype(np.float32)
    for siting in R.SITINGS:
        for rng in R.RANGE_NAMES:
            yv, cv = R.values(grey, siting=siting, rng=rng, maxval=maxval)
            assert np.abs(cv - 128 * k).max() < 1e-7 * maxval  # Coff in every sample (kr + kg + kb is 1 to the float32 rounding of kg: 3e-8)
            assert (R.planes(grey, siting=siting, rng=rng, maxval=maxval, shift=shift)[1] == ((128 * k) << shift)).all()
            yv, cv = R.values(const, siting=siting, rng=rng, maxval=maxval)
            assert np.ptp(yv) < 1e-9 * maxval and np.ptp(cv[..., 0]) < 1e-9 * maxval and np.ptp(cv[..., 1]) < 1e-9 * maxval
    # on a 2 x 2-replicated tensor both sitings agree except in column 0 ... where they agree too once column -1 clamps to column 0's own value
    rep = np.repeat(np.repeat(R.tensor(1, 3, 5, 3, False, maxval, (1, 1, 1), (0, 0, 0), 7), 2, axis=1), 2, axis=2)
    a, b = R.values(rep, siting="centre", maxval=maxval)[1], R.values(rep, siting="left", maxval=maxval)[1]
    assert np.abs(a[:, :, 0] - b[:, :, 0]).max() < 1e-9 * maxval and np.abs(a[:, :, 1:] - b[:, :, 1:]).max() > 1e-3


def test_replicated_integer_frame_centre_is_rgb_cbcrs_r2():
    """A 2 x 2-replicated integer frame, centred: the decimation returns each block's own pixel, so the chroma values are rgb_cbcr_ref's at r = 2,
    centre (the identity resampling) of the unreplicated frame."""
    for k, (n, h, w) in enumerate([(1, 3, 5), (2, 4, 7)]):
        for rng in R.RANGE_NAMES:
            for kr, kb in MATRICES:
                for primaries in (False, True):
                    rgb = rgb_cbcr_ref.frame(20 + k, n, h, w, 3 + k, primaries=primaries)
                    x = np.repeat(np.repeat(rgb, 2, axis=1), 2, axis=2).astype(np.float32)
                    want = rgb_cbcr_ref.values(rgb, 2, "centre", rng, kr, kb)
                    got = R.values(x, siting="centre", rng=rng, kr=kr, kb=kb)[1]
                    assert got.shape == want.shape and np.abs(got - want).max() < 1e-9


@pytest.mark.parametrize("depth", R.DEPTHS, ids=R.DEPTH_IDS)
def test_the_measured_distance_and_the_tie_share_on_the_gpu_sweeps_frames(depth):
    """The reference in float32 against itself in float64 on exactly the frames of the GPU sweeps: at most a quarter of the family's near-tie
    half-width, so the family's eps stands; and the near ties of every sweep stay under the cap."""
    container, maxval, shift = depth
    d = R.measured_distance(container, maxval, shift)
    assert np.isfinite(d) and d > 0
    assert R.EPS is yuv_rgb_ref.EPS and R.MAX_TIE_FRACTION == 0.025
    assert 0.75 * R.MEASURED_DISTANCE[maxval] <= max(R.measured_distance(c, m, s) for c, m, s in R.DEPTHS if m == maxval) <= R.MEASURED_DISTANCE[maxval]
    assert 4.0 * R.MEASURED_DISTANCE[maxval] <= R.EPS[maxval]
    worst = 0.0
    for planar in (False, True):
        for half in (False, True):
            for C_ in (3, 4):
                ties = total = clamped = 0
                for case in R.sweep_cases(C_, half, container, maxval, shift, planar):
                    x = R.case_tensor(case, C_, half, maxval)
                    assert x.dtype == (np.float16 if half else np.float32) and (C_ == 3 or np.isnan(x[..., 3]).all())
                    for v in R.case_values(case, x, maxval):
                        ties, total = ties + int(R.near_tie(v, R.EPS[maxval]).sum()), total + v.size
                    p = x[..., :3].astype(np.float64) * np.asarray(case[4], np.float32)[:3] + np.asarray(case[5], np.float32)[:3]
                    clamped += int(((p < 0) | (p > maxval)).sum())
                assert ties <= R.MAX_TIE_FRACTION * total, (planar, half, C_, ties, total)
                assert clamped > 0  # both clamps are exercised
                worst = max(worst, ties / total)
    print("tensor_yuv reference, %s maxval=%d shift=%d: float32 to float64 distance %.3e (stated %.2e), eps %.0e, largest near-tie share of a sweep %.3f %% (cap %.1f %%)" % (
        container, maxval, shift, d, R.MEASURED_DISTANCE[maxval], R.EPS[maxval], 100 * worst, 100 * R.MAX_TIE_FRACTION))


def test_the_sweeps_hold_the_cases_the_contract_names():
    for (container, planar), tile in R.TILE.items():
        shapes = R.shapes(container, planar)
        assert {(1, 2, 2), (1, 2, 4), (1, 4, 2), (1, 2, 6), (1, 2, 10), (1, 6, 18)} <= set(shapes)
        pixels = [n * h * w for n, h, w in shapes]
        assert tile in pixels and tile - 4 in pixels and tile + 4 in pixels and 2 * tile + 4 in pixels  # the tile exactly, +- 2 columns of two rows, two tiles + 2 columns
        n, h, w = shapes[-1]
        assert n == 2 and (h * w) % tile != 0 and h * w > tile // 2  # the batch seam falls inside a block
        cases = list(R.sweep_cases(3, False, container, 255 if container == "u8" else 1023, 0, planar))
        assert {c[1] for c in cases} == set(R.SITINGS) and {c[2] for c in cases} == set(R.RANGE_NAMES) and {c[3] for c in cases} == {R.BT601, R.BT709}
        assert len({c[4] for c in cases}) == 3


# ---- the host mirror: snn_model_create15 and its resolver, device-free

W, H = 16, 12
NV12, P010, I420, I010 = 0x201, 0x301, 0x401, 0x501
R8, RGB8, RGBA8, RGB16 = 1, 3, 4, 0x103


def _io(a=0, b=NV12, maxval=255, shift=0, siting=1, rng=0, kr=0.299, kb=0.114, video_in=None):
    from shadernn_amd import host

    four = lambda *v: (C.c_float * 4)(*v)  # noqa: E731
    if video_in is None:
        video_in = _video_in(a, 0, 64, 48, 1023 if a & 0x100 else 255, 6 if a == P010 else 0) if a in (NV12, P010, I420, I010) else host.VideoTensorIO()
    return host.TensorVideoIO(a, b, maxval, shift, siting, rng, kr, kb, four(1, 1, 1, 1), four(0, 0, 0, 0), four(0, 0, 0, 0), four(1, 1, 1, 1), video_in)


def _refusals():
    """(io, w, h, c, batch) of every request snn_model_create15 refuses before it opens the model file."""
    out = [(None, W, H, 3, 1)]

    def add(io, w=W, h=H, c=3, batch=1):
        out.append((io, w, h, c, batch))

    for b in (0, R8, RGB8, RGBA8, RGB16, 0x601, -1):
        add(_io(b=b))  # out_format: none of the four
    for a in (0x101, RGB16, 0x104, 0x601, 7, -1):
        add(_io(a))  # in_format: neither float, an 8-bit frame nor a video format
    add(_io(RGB8), c=4), add(_io(RGBA8), c=3), add(_io(R8), c=3)  # an 8-bit in_format of another channel count than the model input's
    add(_io(NV12, video_in=_video_in(NV12, RGB8))), add(_io(NV12, video_in=_video_in(I420)))  # video_in: a float output, the same in_format
    good_video = _io(NV12)
    add(good_video, c=1), add(good_video, c=5)  # everything snn_model_create14 refuses about video_in
    for sw, sh in ((63, 48), (64, 47), (0, 48), (64, -2)):
        add(_io(I420, video_in=_video_in(I420, sw=sw, sh=sh)))
    add(_io(NV12, video_in=_video_in(flt=2))), add(_io(NV12, video_in=_video_in(siting=2))), add(_io(NV12, video_in=_video_in(rng=-1)))
    add(_io(NV12, video_in=_video_in(maxval=1023))), add(_io(P010, video_in=_video_in(P010, maxval=1023, shift=7))), add(_io(NV12, video_in=_video_in(kr=0.0)))
    good = _io()
    add(good, w=0), add(good, h=0), add(good, w=-1), add(good, batch=0), add(good, batch=-1)
    add(_io(siting=2)), add(_io(siting=-1)), add(_io(rng=2)), add(_io(rng=-1))
    add(_io(maxval=256)), add(_io(maxval=127)), add(_io(maxval=1023)), add(_io(shift=1)), add(_io(b=P010, maxval=65535)), add(_io(b=P010, maxval=1023, shift=7))
    add(_io(b=I010, maxval=1000)), add(_io(b=I010, maxval=8191)), add(_io(b=I420, shift=-1)), add(_io(b=I010, maxval=1023, shift=16))
    for b in (NV12, I420):
        add(_io(b=b, kr=0.0)), add(_io(b=b, kb=-0.1)), add(_io(b=b, kr=0.7, kb=0.3))
    return out


def test_the_host_mirror_declares_binds_and_refuses_without_a_device(built):
    from shadernn_amd import host

    mirror = re.sub(r"/\*.*?\*/", "", _read("include/snn_c.h"), flags=re.S)
    assert re.search(r"\bsnn_model_create15\s*\(", mirror) and "snn_tensor_video_io" in mirror
    assert "snn_model_create15" in host.SIGNATURES and hasattr(host.lib(), "snn_model_create15")
    assert C.sizeof(host.TensorVideoIO) == 52 * 4
    assert [n for n, _ in host.TensorVideoIO._fields_] == ["in_format", "out_format", "maxval", "shift", "siting", "range", "kr", "kb", "out_scale", "out_offset", "in_means",
                                                            "in_norms", "video_in"]
    assert C.sizeof(host.VideoTensorIO) == 28 * 4 and C.sizeof(host.RgbFitIO) == 10 * 4 and C.sizeof(host.FrameIO) == 18 * 4  # the earlier structs keep their layout
    h = C.c_void_p()
    cases = _refusals()
    assert len(cases) > 50
    for io, w, hh, c, batch in cases:
        key = None if io is None else tuple(getattr(io, n) for n, _ in host.TensorVideoIO._fields_[:8])
        rc = host.lib().snn_model_create15(b"/nonexistent/model.json", 0, w, hh, c, 0, 1, 0, 0, 0, batch, None if io is None else C.byref(io), C.byref(h))
        assert rc == -1, (key, w, hh, c, batch)  # (-2 would be the model file: the request got past the resolver)
        assert host.frames_resolve(15, io, w, hh, c, batch) is None, (key, w, hh, c, batch)
    for io, c in ((_io(), 3), (_io(), 1), (_io(RGB8, I010, 1023), 3), (_io(RGBA8, P010, 1023, 6), 4), (_io(NV12, I420), 3), (_io(I010, NV12), 4)):  # ... and these resolve
        assert host.frames_resolve(15, io, W, H, c, 1) is not None


def test_the_resolved_model_is_that_of_create4_create5_and_create14(built):
    from shadernn_amd import host

    four = lambda *v: (C.c_float * 4)(*v)  # noqa: E731
    for b, mv, sh, planar in ((NV12, 255, 0, 0), (P010, 1023, 6, 0), (I420, 255, 0, 1), (I010, 1023, 0, 1), (P010, 4095, 0, 0)):
        for c in (1, 3, 4):
            line = host.frames_resolve(15, _io(0, b, mv, sh, 0, 1, 0.2126, 0.0722), 224, 224, c, 2)
            want = host.frames_resolve(5, None, 224, 224, c, 2)  # snn_model_create4 resolves as snn_model_create5 with a null struct
            assert line.split(" | ")[0] == want.split(" | ")[0]
            assert " | source=model sink=yuv420_from_tensor channels=0 wide=0 maxval=255 shift=0 siting=1 range=0 " in line  # the input end's fields keep their defaults
            assert line.endswith("| entry=snn_model_create15 | encode wide=%d planar=%d maxval=%d shift=%d siting=0 range=1 kr=0.212599993 kb=0.0722000003 "
                                 "enc_scale=1,1,1 enc_offset=0,0,0" % (1 if b & 0x100 else 0, planar, mv, sh)), line
    io = _io(RGB8)
    io.in_means, io.in_norms = four(1, 2, 3, 4), four(0.5, 0.25, 2, 1)
    want = host.frames_resolve(5, host.FrameIO(RGB8, 0, four(1, 2, 3, 4), four(0.5, 0.25, 2, 1), four(1, 1, 1, 1), four(0, 0, 0, 0)), W, H, 3)
    assert host.frames_resolve(15, io, W, H, 3).split(" | ")[0] == want.split(" | ")[0] and "in=0x3 out=0x0" in want
    for a in (NV12, P010, I420, I010):  # a video frame in front: snn_model_create14's line, whole, with this entry's sink, name and tail
        io = _io(a, I420)
        line, front = host.frames_resolve(15, io, W, H, 3), host.frames_resolve(14, io.video_in, W, H, 3)
        assert "encode" not in front
        assert line.startswith(front.replace("sink=model", "sink=yuv420_from_tensor").replace("entry=snn_model_create14", "entry=snn_model_create15") + " | encode wide=0 planar=1 ")


def test_the_resolved_lines_of_the_earlier_entry_points_are_unchanged(built):
    from shadernn_amd import host

    for entry, (io, c) in _earlier_requests().items():
        assert host.frames_resolve(entry, io, 32, 24, c, 2) == EARLIER_LINES[entry], entry
    line = host.frames_resolve(14, _video_in(NV12, 0, 1920, 1080), 224, 224, 3, 2)  # entry 14's, as tests/test_frame_yuv_tensor.py states it
    assert line.endswith("planar=0 | entry=snn_model_create14 | src=1920x1080 filter=1 tensor_means=0,0,0 tensor_norms=1,1,1 alpha=1")


def test_host_model_argument_checks():
    from shadernn_amd import host

    path = "/nonexistent/model.json"
    bad = [dict(encode="YUY2"), dict(encode="RGB8"), dict(encode="NV12", video_out="RGB8"), dict(encode="NV12", colour="RGB8"), dict(encode="NV12", out_size=(32, 24)),
           dict(encode="NV12", rgb_size=(32, 24)), dict(encode="NV12", output_format="RGB8"), dict(encode="NV12", input_format="RGB16"), dict(encode="NV12", input_format="R16"),
           dict(encode="NV12", video="NV12"), dict(encode="I420", video_range="tv"), dict(encode="I420", siting="right"), dict(encode="P010", kr=0.0), dict(encode="P010", kr=0.7, kb=0.3),
           dict(encode="NV12", video="NV12", frame_size=(64, 48), input_format="RGB8")]
    for kw in bad:
        with pytest.raises(AssertionError, match="encode|video_range|siting|kr|frame_size|video frames replace"):
            host.Model(path, 16, 12, 3, **kw)
    # the older keywords keep their rules and assertions
    with pytest.raises(AssertionError, match="frame_size"):
        host.Model(path, 16, 12, 3, video="NV12", frame_size=(64, 48), video_out="RGB8")
    with pytest.raises(AssertionError, match="video_out needs video"):
        host.Model(path, 16, 12, 1, video_out="RGB8")
    with pytest.raises(AssertionError, match="8-bit frame"):
        host.Model(path, 16, 12, 3, video="NV12", frame_size=(64, 48), output_format="NV12")
    with pytest.raises(AssertionError, match="rgb_size"):
        host.Model(path, 32, 24, 1, video="NV12", rgb_size=(48, 36))
