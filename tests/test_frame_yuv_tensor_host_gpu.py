"""Video frames in front of an RGB(A) model through the C++ host mirror (snn_model_create14, host.Model(..., video=..., frame_size=(w, h))): a
one-convolution model of 3 and of 4 input channels at 16 x 12 behind a 64 x 48 frame.  The tensor the [yuv tensor] launch writes is held to
tests/yuv_tensor_ref.py under the tolerance of tests/test_frame_yuv_tensor_gpu.py; the model's output must be BYTE-IDENTICAL to that of a twin
snn_model_create4 model fed the downloaded tensor (the launch writes the model's own input tensor and changes nothing behind it); the launch count,
from the description and from the trace, is the twin's + 1."""
import ctypes as C

import numpy as np
import pytest

import yuv_tensor_ref as R

pytestmark = pytest.mark.gpu
W, H = 16, 12      # the model's input
SW, SH = 64, 48    # the frame
# what host.Model takes, the frame's depth, planar planes
SOURCES = {
    "NV12": dict(video="NV12", maxval=255, shift=0, dtype=np.uint8, unit="u8", planar=False),
    "P010": dict(video="P010", maxval=1023, shift=6, dtype=np.uint16, unit="u16", planar=False),
    "I420": dict(video="I420", maxval=255, shift=0, dtype=np.uint8, unit="u8", planar=True),
}


def _json(tmp_path, ic, oc=8):
    from shadernn_amd import models

    net = models.single_conv(seed=3, ic=ic, oc=oc)
    return models.write_json(net, W, H, str(tmp_path / ("single_conv_%d_%d.json" % (ic, oc))))


def _frame(source, batch, seed, sw=SW, sh=SH):
    s = SOURCES[source]
    return R.frame(batch, sh, sw, s["maxval"], s["shift"], s["dtype"], seed, whole_range=bool(seed % 2))


def _first(a, batch):
    return a if batch > 1 else a[0]


def _upload(m, source, frame, batch):
    y, cbcr = frame
    if SOURCES[source]["planar"]:
        m.upload_frame((_first(y[..., 0], batch), _first(cbcr[..., 0], batch), _first(cbcr[..., 1], batch)))
    else:
        m.upload_frame((_first(y[..., 0], batch), _first(cbcr, batch)))


def _maps(source, c):
    means, norms = R.normalisation(1, SOURCES[source]["maxval"])
    return dict(in_means=tuple(means) + (0.0,), in_norms=tuple(norms) + (1.0,), alpha=R.ALPHA), means, norms


def _extra_lines(desc):
    return [line for line in desc.split("\n") if line.startswith("[") and not line[1:line.index("]")].strip().isdigit()]  # (the stages are "[0] ...")


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("source", list(SOURCES))
def test_video_frames_in_front_of_a_model(ctx, tmp_path, monkeypatch, source, c, half):
    from shadernn_amd import capi, host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the two-launch inference
    s = SOURCES[source]
    path = _json(tmp_path, c)
    siting, rng, flt = ("left", "limited", "linear") if c == 3 else ("centre", "full", "nearest" if half else "linear")
    kw, means, norms = _maps(source, c)
    for batch in (1, 2):
        twin = host.Model(path, W, H, c, batch=batch, prefer_half=half)  # snn_model_create4
        frame = _frame(source, batch, 10 * c + batch)
        want = R.tensor(frame[0], frame[1], H, W, c, flt, siting, rng, s["maxval"], s["shift"], means=means, norms=norms, alpha=R.ALPHA)
        outs = []
        for capture in (False, True):
            m = host.Model(path, W, H, c, batch=batch, prefer_half=half, capture_graph=capture, video=s["video"], frame_size=(SW, SH), siting=siting, video_range=rng,
                           video_filter=flt, **kw)
            desc = m.describe()
            extra = _extra_lines(desc)
            assert len(extra) == 1 and extra[0].startswith("[yuv tensor] yuv_tensor%s_%s c=%d %s %s siting=%s range=%s %dx%d->%dx%d " % (
                "_planar" if s["planar"] else "", s["unit"], c, "f16" if half else "f32", flt, siting, rng, SH, SW, H, W)), desc
            assert _extra_lines(twin.describe()) == []
            steps = [d for _, _, d, _, _ in m.plan_steps()]
            assert steps == [d for _, _, d, _, _ in twin.plan_steps()]  # the model behind the launch is the twin's
            _upload(m, source, frame, batch)
            m.run()
            t = m.input_tensor().reshape(batch, H, W, c)
            worst = R.compare(t, want, norms, s["maxval"], half)
            if c == 4:
                assert (t[..., 3] == np.float32(R.ALPHA)).all()
            out = m.output()
            twin.upload(_first(t, batch))
            twin.run()
            assert out.tobytes() == twin.output().tobytes()  # byte-identical
            print("%s c=%d %s batch=%d capture=%s: the input tensor is at %.3f of the tolerance" % (source, c, "f16" if half else "f32", batch, capture, worst))
            if capture:  # replayed on a new frame, then on the first again
                other = _frame(source, batch, 99)
                _upload(m, source, other, batch)
                m.run()
                R.compare(m.input_tensor().reshape(batch, H, W, c), R.tensor(other[0], other[1], H, W, c, flt, siting, rng, s["maxval"], s["shift"], means=means, norms=norms,
                                                                               alpha=R.ALPHA), norms, s["maxval"], half)
                _upload(m, source, frame, batch)
                m.run()
                assert m.output().tobytes() == out.tobytes()
            else:
                capi.trace_begin()
                twin.run()
                base = capi.trace_end()["launches"]
                _upload(m, source, frame, batch)
                capi.trace_begin()
                m.run()
                tr = capi.trace_end()
                fns = sorted(k["function"] for k in tr["kernels"])
                assert tr["launches"] == base + 1 == len(steps) + 1, fns
                assert sum("yuv_tensor%s_kernel" % ("_planar" if s["planar"] else "") in f for f in fns) == 1, fns
            outs.append(out)
            m.close()
        assert outs[0].tobytes() == outs[1].tobytes()  # direct and recorded: the same bytes
        twin.close()


def test_pitched_planes_in(ctx, tmp_path):
    from shadernn_amd import host

    path = _json(tmp_path, 3)
    for source in SOURCES:
        s = SOURCES[source]
        m = host.Model(path, W, H, 3, video=s["video"], frame_size=(SW, SH))
        y, cbcr = _frame(source, 1, 5)
        _upload(m, source, (y, cbcr), 1)
        m.run()
        tight = m.input_tensor()
        planes = [y[0, ..., 0], cbcr[0, ..., 0], cbcr[0, ..., 1]] if s["planar"] else [y[0, ..., 0], cbcr[0].reshape(SH // 2, SW)]
        views = []
        for p in planes:
            wide = np.full((p.shape[0], p.shape[1] + 13), 0xEE, p.dtype)
            wide[:, :p.shape[1]] = p
            views.append(wide[:, :p.shape[1]])
        m.upload_planes(views)
        m.run()
        np.testing.assert_array_equal(m.input_tensor(), tight)  # no padding element was taken for a sample
        m.close()


def test_an_eight_bit_output_frame(ctx, tmp_path):
    """out_format RGB8 (Candy's case: video in, RGB8 out): the model is snn_model_create5's with a float input and that output frame."""
    from shadernn_amd import host

    path = _json(tmp_path, 4, oc=3)
    kw, means, norms = _maps("NV12", 4)
    m = host.Model(path, W, H, 4, video="NV12", frame_size=(SW, SH), output_format="RGB8", out_scale=(64.0,) * 4, out_offset=(16.0,) * 4, **kw)
    twin = host.Model(path, W, H, 4, output_format="RGB8", out_scale=(64.0,) * 4, out_offset=(16.0,) * 4)
    frame = _frame("NV12", 1, 7)
    _upload(m, "NV12", frame, 1)
    m.run()
    t = m.input_tensor()
    R.compare(t.reshape(1, H, W, 4), R.tensor(frame[0], frame[1], H, W, 4, means=means, norms=norms, alpha=R.ALPHA), norms, 255, False)
    got = m.output_frame()
    assert got.dtype == np.uint8 and got.shape == (H, W, 3)
    twin.upload(t)
    twin.run()
    np.testing.assert_array_equal(got, twin.output_frame())
    assert len(_extra_lines(m.describe())) == 1
    m.close()
    twin.close()


def test_float_and_byte_uploads_are_refused(ctx, tmp_path):
    from shadernn_amd import host

    m = host.Model(_json(tmp_path, 4), W, H, 4, video="NV12", frame_size=(SW, SH))
    x = np.zeros((H, W, 4), np.float32)
    img = np.zeros((SH, SW, 4), np.uint8)
    one = np.ones(4, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    assert host.lib().snn_model_upload_input(m.h, fp(x)) == -1
    assert host.lib().snn_model_upload_input_u8(m.h, img.ctypes.data_as(C.c_void_p), SW, SH, 4, fp(one), fp(one), fp(one), fp(one)) == -1
    frame = np.zeros(SH * SW, np.uint8)
    assert host.lib().snn_model_upload_frame_u8(m.h, frame.ctypes.data_as(C.c_void_p)) == -1  # frames go in as planes
    _upload(m, "NV12", _frame("NV12", 1, 2), 1)  # ... and the model still runs
    m.run()
    assert np.isfinite(m.output()).all()
    m.close()
    twin = host.Model(_json(tmp_path, 4), W, H, 4)  # a float model takes floats as before
    assert host.lib().snn_model_upload_input(twin.h, fp(x)) == 0
    twin.close()
