"""The frame description behind snn_model_create5 .. 12 (shadernn_amd/host/snn/frames.h), without a device: snn_frames_resolve is declared, exported
and bound; every request include/snn_c.h describes as "built exactly as" another entry point's resolves to that entry point's model line; every
snn_model_create12 path resolves to its NV12 counterpart's line but for the planar flag and the entry name; the hook refuses every struct that the
device-free refusal tests of the tests/test_frame_*.py files and the tools/*_host_check.cpp programs feed to the real entry points."""
import ctypes as C
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R8, RGB8, RGBA8, R16, RGB16, RGBA16 = 1, 3, 4, 0x101, 0x103, 0x104
NV12, P010, I420, I010 = 0x201, 0x301, 0x401, 0x501
W, H = 32, 24
BT709 = (0.2126, 0.0722)


def _f32(x):
    return C.c_float(x).value


def _parts(line):
    model, frames, entry = line.split(" | ")
    return model, frames, entry


def _resolve(entry, io, w=W, h=H, c=1, batch=1):
    from shadernn_amd import host

    return host.frames_resolve(entry, io, w, h, c, batch)


def _model(entry, io, **kw):
    line = _resolve(entry, io, **kw)
    assert line is not None, (entry, kw)
    return _parts(line)[0]


def _io5(fmt_in, fmt_out, mean, norm, scale, offset):
    from shadernn_amd import host

    four = lambda v: (C.c_float * 4)(v, v, v, v)
    return host.FrameIO(fmt_in, fmt_out, four(mean), four(norm), four(scale), four(offset))


def _io6(fmt_in, fmt_out, mean, norm, scale, offset, in_shift, out_maxval, out_shift):
    from shadernn_amd import host

    four = lambda v: (C.c_float * 4)(v, v, v, v)
    return host.FrameIO2(fmt_in, fmt_out, four(mean), four(norm), four(scale), four(offset), in_shift, out_maxval, out_shift)


def _range_maps(maxval, rng):
    """the luma maps include/snn_c.h states for snn_model_create9: k = (maxval + 1) / 256"""
    k = (maxval + 1) / 256.0
    off, span = (16.0 * k, 219.0 * k) if rng == 0 else (0.0, float(maxval))
    return off, 1.0 / span, span, off


def _as_create8(fmt, maxval, shift, maps):
    """the model snn_model_create8 names: snn_model_create5 with R8 (NV12), snn_model_create6 with R16 and the container's layout (NV12_16)"""
    if fmt == NV12:
        return _model(5, _io5(R8, R8, *maps))
    return _model(6, _io6(R16, R16, *maps, shift, maxval, shift))


def test_the_hook_is_declared_exported_and_bound(built):
    from shadernn_amd import host

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snn_c.h"), encoding="utf-8").read(), flags=re.S)
    assert re.search(r"\bint\s+snn_frames_resolve\s*\(\s*int entry,\s*const void\*\s*io,\s*int in_w,\s*int in_h,\s*int in_c,\s*int batch,\s*char\*\s*buf,\s*int buflen\)", header)
    assert "snn_frames_resolve" in host.SIGNATURES and hasattr(host.lib(), "snn_frames_resolve")
    for entry in (4, 13, 0, -1):  # 5 .. 12 only
        assert _resolve(entry, None) is None
    assert host.lib().snn_frames_resolve(5, None, W, H, 1, 1, None, 0) == 0  # no buffer: the answer alone
    line = _resolve(5, None)
    model, frames, entry = _parts(line)
    assert "in=0x0 out=0x0" in model and "source=model sink=model" in frames and entry == "entry=snn_model_create5"
    assert _model(6, None) == model  # a null struct is the float model through either
    small = C.create_string_buffer(16)  # a short buffer is filled, terminated and not overrun
    assert host.lib().snn_frames_resolve(5, None, W, H, 1, 1, small, len(small)) == 0 and small.value == line[:15].encode()


@pytest.mark.parametrize("fmt", [RGB8, RGBA8])
def test_create7_builds_create5s_r8_model(built, fmt):
    from shadernn_amd import host

    for maps in ((0.0, 1 / 255.0, 255.0, 0.0), (16.0, 1 / 219.0, 219.0, 16.0)):
        for kr, kb in ((0.299, 0.114), BT709):
            line = _resolve(7, host.ColourIO(fmt, kr, kb, *maps))
            model, frames, entry = _parts(line)
            assert model == _model(5, _io5(R8, R8, *maps))
            assert "source=rgb sink=rgb_merged channels=%d " % fmt in frames and "kr=%.9g kb=%.9g" % (_f32(kr), _f32(kb)) in frames
            assert entry == "entry=snn_model_create7"


VIDEO_DEPTHS = [(NV12, 255, 0), (NV12, 200, 0), (P010, 1023, 6), (P010, 1023, 0), (P010, 4095, 0), (P010, 4095, 4), (P010, 1000, 2)]


@pytest.mark.parametrize("fmt,maxval,shift", VIDEO_DEPTHS)
def test_create8_builds_create5s_or_create6s_model(built, fmt, maxval, shift):
    from shadernn_amd import host

    for siting in (0, 1):
        maps = (16.0, 1 / 219.0, 219.0, 16.0) if fmt == NV12 else (64.0, 1 / 876.0, 876.0, 64.0)
        model, frames, entry = _parts(_resolve(8, host.VideoIO(fmt, maxval, shift, siting, *maps)))
        assert model == _as_create8(fmt, maxval, shift, maps)
        assert "source=yuv420 sink=chroma_up" in frames and "wide=%d maxval=%d shift=%d siting=%d " % (fmt == P010, maxval, shift, siting) in frames
        assert entry == "entry=snn_model_create8"


RANGED_DEPTHS = [(NV12, 255, 0), (P010, 1023, 6), (P010, 1023, 0), (P010, 4095, 0), (P010, 255, 0)]


@pytest.mark.parametrize("fmt,maxval,shift", RANGED_DEPTHS)
def test_create9_builds_create8s_model_with_the_ranges_maps(built, fmt, maxval, shift):
    from shadernn_amd import host

    for siting, rng, out_c in itertools.product((0, 1), (0, 1), (3, 4)):
        out = (RGB16 if out_c == 3 else RGBA16) if fmt == P010 else out_c
        model, frames, entry = _parts(_resolve(9, host.VideoRgbIO(fmt, out, maxval, shift, siting, rng, *BT709)))
        maps = _range_maps(maxval, rng)
        assert model == _model(8, host.VideoIO(fmt, maxval, shift, siting, *maps)) == _as_create8(fmt, maxval, shift, maps)
        assert "source=yuv420 sink=rgb_from_yuv channels=%d " % out_c in frames and "siting=%d range=%d " % (siting, rng) in frames
        assert entry == "entry=snn_model_create9"


@pytest.mark.parametrize("fmt", [RGB8, RGBA8])
def test_create10_builds_create5s_r8_model_with_the_ranges_output_map(built, fmt):
    from shadernn_amd import host

    for siting, rng in itertools.product((0, 1), (0, 1)):
        for w, h in ((W, H), (31, 23)):  # the input extent may be odd: only r * extent must be even, decided once the model file gives r
            model, frames, entry = _parts(_resolve(10, host.EncodeIO(fmt, NV12, siting, rng, 0.299, 0.114), w=w, h=h))
            assert model == _model(5, _io5(R8, R8, 0.0, 1 / 255.0, 219.0 if rng == 0 else 255.0, 16.0 if rng == 0 else 0.0), w=w, h=h)
            assert "source=rgb sink=yuv420_from_rgb channels=%d " % fmt in frames and "siting=%d range=%d " % (siting, rng) in frames
            assert entry == "entry=snn_model_create10"


@pytest.mark.parametrize("fmt,maxval,shift", VIDEO_DEPTHS)
def test_create11_builds_create8s_model(built, fmt, maxval, shift):
    from shadernn_amd import host

    maps = (16.0, 1 / 219.0, 219.0, 16.0)
    for ow, oh in ((48, 36), (16, 12), (128, 96), (40, 36)):
        video = host.VideoIO(fmt, maxval, shift, 1, *maps)
        line8, line11 = _resolve(8, video), _resolve(11, host.FitIO(video, ow, oh))
        assert _parts(line11)[0] == _parts(line8)[0]
        assert _parts(line11)[1] == _parts(line8)[1].replace("sink=chroma_up", "sink=fitted").replace("fit=0x0", "fit=%dx%d" % (ow, oh))
        assert _parts(line11)[2] == "entry=snn_model_create11"


def _planar_twin(line):
    """an NV12 path's line as snn_model_create12 must resolve its planar twin: the planar flag and the entry name differ, nothing else"""
    assert " planar=0 | entry=" in line
    return re.sub(r" planar=0 \| entry=\w+$", " planar=1 | entry=snn_model_create12", line)


@pytest.mark.parametrize("wide", [False, True], ids=["8bit", "10bit"])
@pytest.mark.parametrize("siting", [0, 1], ids=["centre", "left"])
@pytest.mark.parametrize("rng", [0, 1], ids=["limited", "full"])
def test_every_create12_path_resolves_to_its_nv12_counterpart(built, wide, siting, rng):
    from shadernn_amd import host

    planar, nv, maxval = (I010, P010, 1023) if wide else (I420, NV12, 255)
    maps = _range_maps(maxval, rng)
    for shift in ((0, 6) if wide else (0,)):
        video = host.VideoIO(nv, maxval, shift, siting, *maps)
        # planar -> the same planar format: snn_model_create8's path with the range's maps (the matrix is not looked at: any kr, kb)
        for kr, kb in ((0.299, 0.114), (0.0, 2.0)):
            assert _resolve(12, host.PlanarIO(planar, planar, maxval, shift, siting, rng, kr, kb, 0, 0)) == _planar_twin(_resolve(8, video))
        # ... at a fitted size: snn_model_create11's
        assert _resolve(12, host.PlanarIO(planar, planar, maxval, shift, siting, rng, 0.299, 0.114, 48, 36)) == _planar_twin(_resolve(11, host.FitIO(video, 48, 36)))
        # planar -> RGB: snn_model_create9's
        for out in ((RGB16, RGBA16) if wide else (RGB8, RGBA8)):
            assert _resolve(12, host.PlanarIO(planar, out, maxval, shift, siting, rng, *BT709, 0, 0)) == \
                _planar_twin(_resolve(9, host.VideoRgbIO(nv, out, maxval, shift, siting, rng, *BT709)))
    if not wide:  # RGB -> I420: snn_model_create10's (8-bit only)
        for fmt in (RGB8, RGBA8):
            assert _resolve(12, host.PlanarIO(fmt, I420, 255, 0, siting, rng, *BT709, 0, 0)) == _planar_twin(_resolve(10, host.EncodeIO(fmt, NV12, siting, rng, *BT709)))


def _refusals():
    """(entry, struct or None, w, h, in_c, batch) of every request the device-free refusal tests (tests/test_frame_chroma.py, _yuv_rgb.py, _rgb_cbcr.py,
    _fit.py, _planar.py) and the host-check programs (tools/chroma_, video_rgb_, rgb_nv12_, fit_, planar_host_check.cpp) feed to the entry points"""
    from shadernn_amd import host

    out = []

    def add(entry, io, w=W, h=H, c=1, batch=1):
        out.append((entry, io, w, h, c, batch))

    def v8(fmt=NV12, maxval=255, shift=0, siting=1):
        return host.VideoIO(fmt, maxval, shift, siting, 0.0, 1.0 / max(maxval, 1), float(maxval), 0.0)

    add(8, None)
    for fmt in (0, 1, 3, 4, 0x101, 0x202):
        add(8, v8(fmt=fmt))
    add(8, v8(), c=3), add(8, v8(), w=31), add(8, v8(), h=23), add(8, v8(), batch=0)
    for io in (v8(P010, 65535), v8(P010, 4096), v8(P010, 1023, 7), v8(NV12, 1023), v8(NV12, 127, 1), v8(NV12, 255, 0, 2), v8(NV12, 0), v8(P010, 1023, -1), v8(shift=1)):
        add(8, io)

    def v9(fmt=NV12, out=RGB8, maxval=255, shift=0, siting=1, rng=0, kr=0.299, kb=0.114):
        return host.VideoRgbIO(fmt, out, maxval, shift, siting, rng, kr, kb)

    add(9, None)
    for fmt in (0, 1, 3, 4, 0x101, 0x202):
        add(9, v9(fmt=fmt))
    for o in (0, 1, RGB16, RGBA16, NV12):
        add(9, v9(out=o))
    for o in (3, 4, R16, P010):
        add(9, v9(P010, o, 1023, 6))
    add(9, v9(), c=3), add(9, v9(), w=31), add(9, v9(), h=23), add(9, v9(), batch=0)
    for io in (v9(P010, RGB16, 65535), v9(P010, RGB16, 8191), v9(P010, RGB16, 1023, 7), v9(maxval=1023), v9(maxval=127), v9(P010, RGB16, 1000), v9(shift=1),
               v9(P010, RGB16, 1023, -1), v9(siting=2), v9(rng=2), v9(rng=-1), v9(kr=0.0), v9(kb=0.0), v9(kr=0.7, kb=0.3)):
        add(9, io)

    def v10(fmt=RGB8, out=NV12, siting=1, rng=0, kr=0.299, kb=0.114):
        return host.EncodeIO(fmt, out, siting, rng, kr, kb)

    add(10, None)
    for fmt in (0, 1, 5, RGB16, RGBA16, NV12, P010):
        add(10, v10(fmt=fmt))
    for o in (0, 1, 3, 4, RGB16, P010):
        add(10, v10(out=o))
    add(10, v10(), c=3), add(10, v10(RGBA8), c=4), add(10, v10(), batch=0), add(10, v10(), batch=-1)
    for io in (v10(siting=2), v10(siting=-1), v10(rng=2), v10(rng=-1), v10(kr=0.0), v10(kb=0.0), v10(kr=0.7, kb=0.3), v10(RGBA8, NV12, 0, 1, -0.1, 0.114)):
        add(10, io)

    def v11(ow, oh, fmt=NV12, maxval=255, shift=0, siting=1):
        return host.FitIO(host.VideoIO(fmt, maxval, shift, siting, 127.5, 1 / 127.5, 127.5, 127.5), ow, oh)

    add(11, None)
    for ow, oh in ((47, 36), (48, 35), (0, 36), (48, 0), (1, 1), (-2, 36), (48, -2), (14, 36), (130, 36), (48, 10), (48, 98)):
        add(11, v11(ow, oh))
    good = v11(48, 36)
    add(11, good, w=31), add(11, good, h=23), add(11, good, w=0), add(11, good, c=3), add(11, good, batch=0), add(11, good, batch=-1)
    for io in (v11(48, 36, 0), v11(48, 36, R8), v11(48, 36, R16), v11(48, 36, RGB8), v11(48, 36, NV12, 256), v11(48, 36, NV12, 0), v11(48, 36, NV12, 255, 1),
               v11(48, 36, P010, 65535), v11(48, 36, P010, 1023, 7), v11(48, 36, P010, 1023, 16), v11(48, 36, NV12, 255, 0, 2), v11(48, 36, NV12, 255, 0, -1)):
        add(11, io)

    def v12(a=I420, b=I420, maxval=255, shift=0, siting=1, rng=0, kr=0.299, kb=0.114, ow=0, oh=0):
        return host.PlanarIO(a, b, maxval, shift, siting, rng, kr, kb, ow, oh)

    add(12, None)
    add(12, v12(), w=31), add(12, v12(), h=23), add(12, v12(), w=0), add(12, v12(), h=0), add(12, v12(), c=3), add(12, v12(), batch=0), add(12, v12(), batch=-1)
    for a, b in ((0, I420), (1, I420), (NV12, NV12), (NV12, I420), (I420, NV12), (I420, I010), (I010, I420), (I420, RGB16), (I420, RGBA16), (I010, RGB8), (I010, RGBA8),
                 (I420, 1), (I420, 0), (RGB8, NV12), (RGB8, I010), (RGBA8, RGBA8), (RGB8, RGB8), (RGB16, I010), (RGB16, I420)):
        add(12, v12(a, b, 1023 if a in (I010, RGB16) else 255))
    for fmt, maxval, shift in ((I420, 256, 0), (I420, 0, 0), (I420, 127, 0), (I420, 1023, 0), (I420, 255, 1), (I420, 255, -1), (I010, 65535, 0), (I010, 8191, 0),
                               (I010, 1000, 0), (I010, 254, 0), (I010, 1023, 7), (I010, 1023, 16), (I010, 4095, 5)):
        add(12, v12(fmt, fmt, maxval, shift)), add(12, v12(fmt, RGB8 if fmt == I420 else RGB16, maxval, shift))
    for a, b in ((I420, I420), (I420, RGB8), (I010, RGBA16), (RGB8, I420), (RGBA8, I420)):
        mv = 1023 if a == I010 else 255
        add(12, v12(a, b, mv, siting=2)), add(12, v12(a, b, mv, siting=-1)), add(12, v12(a, b, mv, rng=2)), add(12, v12(a, b, mv, rng=-1))
    for a, b in ((I420, RGB8), (I420, RGBA8), (RGB8, I420), (RGBA8, I420)):
        add(12, v12(a, b, kr=0.0)), add(12, v12(a, b, kb=-0.1)), add(12, v12(a, b, kr=0.7, kb=0.3))
    for a, b, mv in ((I420, RGB8, 255), (I420, RGBA8, 255), (I010, RGB16, 1023), (RGB8, I420, 255)):
        add(12, v12(a, b, mv, ow=48, oh=36)), add(12, v12(a, b, mv, ow=48)), add(12, v12(a, b, mv, oh=36))
    for ow, oh in ((47, 36), (48, 35), (0, 36), (48, 0), (1, 1), (-2, 36), (14, 36), (130, 36), (48, 10), (48, 98)):
        add(12, v12(ow=ow, oh=oh)), add(12, v12(I010, I010, 1023, ow=ow, oh=oh))
    return out


def test_the_hook_refuses_what_the_entry_points_refuse_without_a_device(built):
    from shadernn_amd import host

    handle = C.c_void_p()
    cases = _refusals()
    assert len(cases) == 227  # (a guard against a list that silently came out short)
    for entry, io, w, h, c, batch in cases:
        what = (entry, None if io is None else [getattr(io, n) if not isinstance(getattr(io, n), C.Structure) else "..." for n, _ in io._fields_], w, h, c, batch)
        assert _resolve(entry, io, w, h, c, batch) is None, what
        create = getattr(host.lib(), "snn_model_create%d" % entry)  # ... and the entry point itself agrees (the model file does not exist)
        assert create(b"/nonexistent/model.json", 0, w, h, c, 0, 1, 0, 0, 0, batch, None if io is None else C.byref(io), C.byref(handle)) == -1, what
        assert not handle.value


def test_create5_create6_and_create7_rules(built):
    """their own rules (include/snn_c.h): snn_model_create5 refuses the 16-bit formats, the input format's channel count is the model input's, shifts
    are 0..15, out_maxval << out_shift fits 16 bits; the layout fields are not looked at on an end that is not 16-bit"""
    from shadernn_amd import host

    assert _resolve(5, _io5(R8, R8, 0, 1, 1, 0)) is not None and _resolve(5, _io5(0, R8, 0, 1, 1, 0)) is not None and _resolve(5, _io5(RGBA8, 0, 0, 1, 1, 0), c=4) is not None
    for a, b in ((R16, R8), (R8, R16), (RGB16, 0), (2, R8), (R8, 5), (NV12, NV12), (-1, 0)):
        assert _resolve(5, _io5(a, b, 0, 1, 1, 0)) is None, (a, b)
    assert _resolve(5, _io5(RGB8, RGB8, 0, 1, 1, 0)) is None and _resolve(5, _io5(RGB8, RGB8, 0, 1, 1, 0), c=3) is not None  # RGB8 on a one-channel model
    assert _resolve(6, _io6(R16, R16, 0, 1, 1, 0, 6, 1023, 6)) is not None and _resolve(6, _io6(R8, R16, 0, 1, 1, 0, 99, 65535, 0)) is not None
    assert _resolve(6, _io6(RGB16, 0, 0, 1, 1, 0, 0, 0, 99), c=3) is not None  # a float output: out_maxval / out_shift are not looked at
    for in_shift, out_maxval, out_shift in ((-1, 1023, 0), (16, 1023, 0), (0, 0, 0), (0, 65536, 0), (0, 1023, -1), (0, 1023, 16), (0, 1023, 7), (0, 65535, 1)):
        assert _resolve(6, _io6(R16, R16, 0, 1, 1, 0, in_shift, out_maxval, out_shift)) is None, (in_shift, out_maxval, out_shift)
    assert _resolve(6, _io6(RGB16, RGB16, 0, 1, 1, 0, 0, 1023, 0)) is None and _resolve(6, _io6(2, R16, 0, 1, 1, 0, 0, 1023, 0)) is None
    assert _resolve(7, None) is None
    for fmt in (0, R8, R16, RGB16, NV12):
        assert _resolve(7, host.ColourIO(fmt, 0.299, 0.114, 0, 1, 1, 0)) is None, fmt
    good = host.ColourIO(RGB8, 0.299, 0.114, 0, 1, 1, 0)
    assert _resolve(7, good) is not None and _resolve(7, good, w=31, h=23) is not None  # (any extent)
    assert _resolve(7, good, c=3) is None and _resolve(7, good, batch=0) is None and _resolve(7, good, w=0) is None
    for kr, kb in ((0.0, 0.114), (0.299, 0.0), (0.7, 0.3), (-0.1, 0.5)):
        assert _resolve(7, host.ColourIO(RGB8, kr, kb, 0, 1, 1, 0)) is None, (kr, kb)
    for entry in range(5, 13):  # the model input's own extent, channels and batch, through every entry point
        assert _resolve(entry, None, batch=0) is None and _resolve(entry, None, w=0) is None and _resolve(entry, None, h=-1) is None and _resolve(entry, None, c=0) is None


def test_the_build_and_the_documents_name_the_unit():
    def read(path):
        with open(os.path.join(ROOT, path), encoding="utf-8") as f:
            return f.read()

    assert os.path.exists(os.path.join(ROOT, "shadernn_amd", "host", "frames.cpp"))  # build_host compiles every .cpp of the directory
    header = read("shadernn_amd/host/snn/frames.h")
    assert "hip" not in re.sub(r"//.*", "", header).lower()  # device-free: nothing from HIP
    design, readme = read("DESIGN.md"), read("README.md")
    assert "4.20" in design and "FrameSpec" in design and "initFrames" in design and "snn_frames_resolve" in design
    assert "tools/frames_host_check.cpp" in readme and "tests/test_frame_paths.py" in readme
    assert "snn_frames_resolve" in read("tools/frames_host_check.cpp")
