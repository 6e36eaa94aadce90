"""Encoder frames behind an RGB(A) model through the C++ host mirror (snn_model_create15, host.Model(..., encode=...)): a one-convolution model of
3 and of 4 output channels at 24 x 16.  The planes the [tensor yuv] launch writes are held to tests/tensor_yuv_ref.py on the float output of a twin
model with the same weights and input (snn_model_create4; snn_model_create5 with an RGB8 input; snn_model_create14 with a video frame in front), under
the rule of tests/test_frame_tensor_yuv_gpu.py; the launch count, from the description and from the trace, is the twin's + 1."""
import ctypes as C

import numpy as np
import pytest

import tensor_yuv_ref as R
import yuv_tensor_ref

pytestmark = pytest.mark.gpu
W, H = 24, 16      # the model's input and output extent (the chroma plane holds an 8 x 8 window of the frame metrics)
SW, SH = 64, 48    # a video frame in front
# what encode= takes: the output's depth, the planes' dtype, planar planes
ENCODES = {
    "NV12": dict(maxval=255, shift=0, dtype=np.uint8, unit="u8", planar=False),
    "P010": dict(maxval=1023, shift=6, dtype=np.uint16, unit="u16", planar=False),
    "I420": dict(maxval=255, shift=0, dtype=np.uint8, unit="u8", planar=True),
}


def _json(tmp_path, ic, oc, w=W, h=H):
    from shadernn_amd import models

    net = models.single_conv(seed=3, ic=ic, oc=oc)
    return models.write_json(net, w, h, str(tmp_path / ("single_conv_%d_%d_%dx%d.json" % (ic, oc, w, h))))


def _extra_lines(desc):
    return [line for line in desc.split("\n") if line.startswith("[") and not line[1:line.index("]")].strip().isdigit()]  # (the stages are "[0] ...")


def _maps(maxval):
    """an output map that spreads the convolution's output (about -2 .. 2) over and past the code range, one per channel"""
    return dict(out_scale=(0.3 * maxval, 0.25 * maxval, 0.35 * maxval, 1.0), out_offset=(0.5 * maxval, 0.45 * maxval, 0.55 * maxval, 0.0))


def _planes(got, batch, planar):
    """output_frame()'s pair / triple as (luma [N][H][W][1], cbcr [N][H/2][W/2][2])"""
    y = np.asarray(got[0]).reshape(batch, H, W, 1)
    if planar:
        cbcr = np.stack([np.asarray(got[1]).reshape(batch, H // 2, W // 2), np.asarray(got[2]).reshape(batch, H // 2, W // 2)], axis=-1)
    else:
        cbcr = np.asarray(got[1]).reshape(batch, H // 2, W // 2, 2)
    return y, cbcr


def _check(m, twin, batch, enc, half, kw, siting, rng, items):
    e = ENCODES[enc]
    t = twin.output().reshape(batch, H, W, -1)
    x = t.astype(np.float16) if half else t  # the tensor as the launch reads it: the twin's fp16 values widened are exact halves
    yv, cv = R.values(x, kw["out_scale"][:3], kw["out_offset"][:3], siting, rng, e["maxval"])
    y, cbcr = _planes(m.output_frame(), batch, e["planar"])
    assert y.dtype == e["dtype"] and y.shape == (batch, H, W, 1) and cbcr.shape == (batch, H // 2, W // 2, 2)
    items += [(y, yv, e["maxval"], e["shift"]), (cbcr, cv, e["maxval"], e["shift"])]
    return y, cbcr


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("oc", [3, 4])
@pytest.mark.parametrize("enc", list(ENCODES))
def test_encoder_frames_behind_a_float_model(ctx, tmp_path, monkeypatch, enc, oc, half):
    from shadernn_amd import capi, host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the two-launch inference
    e = ENCODES[enc]
    path = _json(tmp_path, 3, oc)
    siting, rng = ("left", "limited") if oc == 3 else ("centre", "full")
    kw = _maps(e["maxval"])
    items = []
    for batch in (1, 2):
        twin = host.Model(path, W, H, 3, batch=batch, prefer_half=half)  # snn_model_create4
        x = np.random.default_rng(10 * oc + batch).uniform(-1, 1, size=(batch, H, W, 3)).astype(np.float32)
        twin.upload(x if batch > 1 else x[0])
        twin.run()
        outs = []
        for capture in (False, True):
            m = host.Model(path, W, H, 3, batch=batch, prefer_half=half, capture_graph=capture, encode=enc, siting=siting, video_range=rng, **kw)
            extra = _extra_lines(m.describe())
            assert len(extra) == 1 and extra[0].startswith("[tensor yuv] tensor_yuv%s_%s c=%d %s siting=%s range=%s %dx%d " % (
                "_planar" if e["planar"] else "", e["unit"], oc, "f16" if half else "f32", siting, rng, H, W)), m.describe()
            assert _extra_lines(twin.describe()) == []
            steps = [d for _, _, d, _, _ in m.plan_steps()]
            assert steps == [d for _, _, d, _, _ in twin.plan_steps()]  # the model in front of the launch is the twin's
            m.upload(x if batch > 1 else x[0])
            m.run()
            y, cbcr = _check(m, twin, batch, enc, half, kw, siting, rng, items)
            if capture:  # replayed on another input, then on the first again
                m.upload(-x if batch > 1 else -x[0])
                m.run()
                m.upload(x if batch > 1 else x[0])
                m.run()
                y2, c2 = _planes(m.output_frame(), batch, e["planar"])
                assert y2.tobytes() == y.tobytes() and c2.tobytes() == cbcr.tobytes()
            else:
                capi.trace_begin()
                twin.run()
                base = capi.trace_end()["launches"]
                capi.trace_begin()
                m.run()
                tr = capi.trace_end()
                fns = sorted(k["function"] for k in tr["kernels"])
                assert tr["launches"] == base + 1 == len(steps) + 1, fns
                assert sum("tensor_yuv%s_kernel" % ("_planar" if e["planar"] else "") in f for f in fns) == 1, fns
            outs.append((y, cbcr))
            m.close()
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()  # direct and recorded: the same bytes
        twin.close()
    frac, ndiff = R.compare_all(items)
    print("encode=%s oc=%d %s: near ties %.3f %%, %d values differ" % (enc, oc, "f16" if half else "f32", 100 * frac, ndiff))


def test_rgb8_frames_in_and_encoder_frames_out(ctx, tmp_path):
    from shadernn_amd import host

    path = _json(tmp_path, 3, 3)
    maps = dict(in_means=(127.5, 127.5, 127.5, 0.0), in_norms=(1 / 127.5, 1 / 127.5, 1 / 127.5, 1.0))
    items = []
    for enc, half, batch in (("NV12", False, 2), ("I420", True, 1), ("P010", False, 1)):
        kw = _maps(ENCODES[enc]["maxval"])
        img = np.random.default_rng(5 + batch).integers(0, 256, size=(batch, H, W, 3)).astype(np.uint8)
        twin = host.Model(path, W, H, 3, batch=batch, prefer_half=half, input_format="RGB8", **maps)  # snn_model_create5, a float output
        m = host.Model(path, W, H, 3, batch=batch, prefer_half=half, input_format="RGB8", encode=enc, kr=R.BT709[0], kb=R.BT709[1], **maps, **kw)
        assert len(_extra_lines(m.describe())) == len(_extra_lines(twin.describe())) + 1
        for mod in (twin, m):
            mod.upload_frame(img if batch > 1 else img[0])
            mod.run()
        e = ENCODES[enc]
        t = twin.output().reshape(batch, H, W, 3)
        yv, cv = R.values(t.astype(np.float16) if half else t, kw["out_scale"][:3], kw["out_offset"][:3], "left", "limited", e["maxval"], *R.BT709)
        y, cbcr = _planes(m.output_frame(), batch, e["planar"])
        items += [(y, yv, e["maxval"], e["shift"]), (cbcr, cv, e["maxval"], e["shift"])]
        m.close()
        twin.close()
    frac, ndiff = R.compare_all(items)
    print("RGB8 in, encoder frames out: near ties %.3f %%, %d values differ" % (100 * frac, ndiff))


def test_video_frames_in_and_out(ctx, tmp_path, monkeypatch):
    """decoder -> RGB model -> encoder: snn_model_create14's frame in front, [tensor yuv] behind; two launches more than the float model"""
    from shadernn_amd import capi, host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")
    path = _json(tmp_path, 3, 3)
    means, norms = yuv_tensor_ref.normalisation(1, 255)
    front = dict(video="NV12", frame_size=(SW, SH), in_means=tuple(means) + (0.0,), in_norms=tuple(norms) + (1.0,))
    kw = _maps(255)
    items = []
    for capture in (False, True):
        twin = host.Model(path, W, H, 3, capture_graph=capture, **front)  # snn_model_create14, a float output
        m = host.Model(path, W, H, 3, capture_graph=capture, encode="NV12", **front, **kw)
        extra = _extra_lines(m.describe())
        assert [line.split(" ")[0] + " " + line.split(" ")[1] for line in extra] == ["[yuv tensor]", "[tensor yuv]"], m.describe()
        assert len(_extra_lines(twin.describe())) == 1
        frame = yuv_tensor_ref.frame(1, SH, SW, 255, 0, np.uint8, seed=4)
        for mod in (twin, m):
            mod.upload_frame((frame[0][0, ..., 0], frame[1][0]))
            mod.run()
        assert m.input_tensor().tobytes() == twin.input_tensor().tobytes()
        _check(m, twin, 1, "NV12", False, kw, "left", "limited", items)
        if not capture:
            capi.trace_begin()
            twin.run()
            base = capi.trace_end()["launches"]
            capi.trace_begin()
            m.run()
            tr = capi.trace_end()
            assert tr["launches"] == base + 1, tr
        m.close()
        twin.close()
    R.compare_all(items)


def test_pitched_planes_out_and_the_frame_metrics(ctx, tmp_path):
    from shadernn_amd import host

    path = _json(tmp_path, 3, 4)
    for enc in ENCODES:
        e = ENCODES[enc]
        batch = 2
        m = host.Model(path, W, H, 3, batch=batch, encode=enc, **_maps(e["maxval"]))
        x = np.random.default_rng(8).uniform(-1, 1, size=(batch, H, W, 3)).astype(np.float32)
        m.upload(x)
        m.run()
        got = m.output_frame()
        y, cbcr = _planes(got, batch, e["planar"])
        shapes = [(H, W), (H // 2, W // 2), (H // 2, W // 2)] if e["planar"] else [(H, W), (H // 2, W)]
        fill = 0xEE if e["dtype"] == np.uint8 else 0xEEEE
        wide = [np.full((s[0], s[1] + 13), fill, e["dtype"]) for _ in range(batch) for s in shapes]
        m.download_planes([a[:, :s[1]] for a, s in zip(wide, shapes * batch)])
        k = len(shapes)
        for n in range(batch):
            want = [y[n, ..., 0], cbcr[n, ..., 0], cbcr[n, ..., 1]] if e["planar"] else [y[n, ..., 0], cbcr[n].reshape(H // 2, W)]
            for p in range(k):
                a, s = wide[n * k + p], shapes[p]
                np.testing.assert_array_equal(a[:, :s[1]], want[p])
                assert (a[:, s[1]:] == fill).all()  # the padding is untouched
        # the frame against its own download: one luma row and two chroma rows per image, PSNR +inf
        m.set_reference(got)
        rows = m.metrics()
        assert len(rows) == 3 * batch
        assert [(r["image"], r["plane"], r["channel"]) for r in rows] == [(n, pl, ch) for n in range(batch) for pl, ch in (((0, 0), (1, 0), (2, 0)) if e["planar"] else ((0, 0), (1, 0), (1, 1)))]
        assert all(r["sse"] == 0 and np.isinf(r["psnr_db"]) and r["psnr_db"] > 0 for r in rows)
        # the float and the packed-frame downloads are refused: the frame comes back as planes
        buf = np.zeros(batch * H * W * 4, np.float32)
        assert host.lib().snn_model_download_output(m.h, buf.ctypes.data_as(C.POINTER(C.c_float))) == -1
        assert host.lib().snn_model_download_frame_u8(m.h, buf.ctypes.data_as(C.c_void_p)) == -1
        assert host.lib().snn_model_download_frame_u16(m.h, buf.ctypes.data_as(C.c_void_p)) == -1
        m.close()


def test_refusals_that_need_the_model(ctx, tmp_path):
    """1 or 2 output channels and an odd output extent are known once the model file gives the output: -1, nothing built on the device"""
    from shadernn_amd import host

    for oc in (1, 2):
        with pytest.raises(AssertionError):
            host.Model(_json(tmp_path, 3, oc), W, H, 3, encode="NV12")
    for w, h in ((23, 16), (24, 15)):
        with pytest.raises(AssertionError):
            host.Model(_json(tmp_path, 3, 3, w, h), w, h, 3, encode="I420")
    m = host.Model(_json(tmp_path, 3, 3), W, H, 3, encode="NV12")  # ... and the even three-channel model is taken
    m.close()
