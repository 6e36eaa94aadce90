"""NV12 / P010 frames through the C++ host mirror (snn_model_create8, host.Model(video=...)): ESPCN at x2 / x3 / x4.  The luma plane that comes back
is byte for byte what the same build's R8 / R16 model (snn_model_create5 / 6) returns for the same luma plane -- it runs the same kernels; the chroma
plane is compared with the float64 reference of tests/chroma_ref.py under its rule (equal off the near ties, within 1 << shift on them, near ties at
most 2.5 % of the values)."""
import ctypes as C

import numpy as np
import pytest

import chroma_ref as R

pytestmark = pytest.mark.gpu
H, W = 38, 30  # the luma plane; the chroma plane is 19 x 15: odd rows


def _maps(maxval):
    half = maxval / 2.0
    return dict(in_means=(half, half, half, 0), in_norms=(1 / half, 1 / half, 1 / half, 1), out_scale=(half, half, half, 1), out_offset=(half, half, half, 0))


VIDEO = {
    "NV12": dict(maxval=255, shift=0, dtype=np.uint8, ref=dict(input_format="R8", output_format="R8")),
    "P010": dict(maxval=1023, shift=6, dtype=np.uint16, ref=dict(input_format="R16", output_format="R16", frame_in_shift=6, frame_out_maxval=1023, frame_out_shift=6)),
}


def _json(tmp_path, r):
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r)
    return models.write_json(net, W, H, str(tmp_path / (net["name"] + ".json")))


def _frame(video, batch, seed):
    v = VIDEO[video]
    rng = np.random.default_rng(seed)
    y = (rng.integers(0, v["maxval"] + 1, size=(batch, H, W)) << v["shift"]).astype(v["dtype"])
    cbcr = (rng.integers(0, v["maxval"] + 1, size=(batch, H // 2, W // 2, 2)) << v["shift"]).astype(v["dtype"])
    return y, cbcr


def _models(path, video, batch=1, siting="left", **kw):
    from shadernn_amd import host

    v = VIDEO[video]
    m = host.Model(path, W, H, 1, batch=batch, video=video, siting=siting, **_maps(v["maxval"]), **kw)
    ref = host.Model(path, W, H, 1, batch=batch, **v["ref"], **_maps(v["maxval"]), **kw)
    return m, ref


def _check(m, ref, video, frame, batch, r, siting):
    v = VIDEO[video]
    y, cbcr = frame
    m.upload_frame((y, cbcr) if batch > 1 else (y[0], cbcr[0]))
    m.run()
    got_y, got_c = m.download_frame()
    got_y, got_c = got_y.reshape(batch, r * H, r * W), got_c.reshape(batch, r * H // 2, r * W // 2, 2)
    ref.upload_frame(y[..., None] if batch > 1 else y[0][..., None])
    ref.run()
    want_y = ref.output_frame().reshape(batch, r * H, r * W)
    np.testing.assert_array_equal(got_y, want_y)  # the same kernels: byte for byte
    frac, ndiff = R.compare_all([(got_c, R.up_values(cbcr, r, siting, v["shift"]), v["maxval"], v["shift"])])
    print("%s r=%d batch=%d siting=%s: chroma near ties %.3f %%, %d values differ" % (video, r, batch, siting, 100 * frac, ndiff))
    return got_y, got_c


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("video", ["NV12", "P010"])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_video_frames_around_espcn(ctx, tmp_path, r, video, batch):
    path = _json(tmp_path, r)
    for siting in ("left", "centre"):
        m, ref = _models(path, video, batch, siting)
        desc = m.describe()
        assert "[chroma out] chroma_up_%s r=%d c=2 siting=%s" % ("u8" if video == "NV12" else "u16", r, siting) in desc, desc
        steps = [d for _, _, d, _, _ in m.plan_steps()]  # the ESPCN steps are what the grey model launches: two fused kernels, the frame ends folded in
        assert steps == [d for _, _, d, _, _ in ref.plan_steps()] and len(steps) == 2, steps
        _check(m, ref, video, _frame(video, batch, 10 * r + batch), batch, r, siting)
        m.close()
        ref.close()


@pytest.mark.parametrize("video", ["NV12", "P010"])
def test_a_captured_graph_reads_each_new_frame(ctx, tmp_path, monkeypatch, video):
    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the three-launch inference
    r = 2
    from shadernn_amd import host

    v = VIDEO[video]
    path = _json(tmp_path, r)
    m = host.Model(path, W, H, 1, video=video, capture_graph=True, **_maps(v["maxval"]))
    ref = host.Model(path, W, H, 1, **v["ref"], **_maps(v["maxval"]))
    outs = []
    for seed in (1, 2, 3):  # the first run records, the others replay: every frame must give its own result
        outs.append(_check(m, ref, video, _frame(video, 1, seed), 1, r, "left"))
    for a, b in ((0, 1), (1, 2)):
        assert not np.array_equal(outs[a][0], outs[b][0]) and not np.array_equal(outs[a][1], outs[b][1])
    m.close()
    ref.close()


@pytest.mark.parametrize("video", ["NV12", "P010"])
def test_prefer_half(ctx, tmp_path, video):
    r = 2
    m, ref = _models(_json(tmp_path, r), video, prefer_half=True)
    _check(m, ref, video, _frame(video, 1, 8), 1, r, "left")
    m.close()
    ref.close()


def test_what_is_refused(ctx, tmp_path):
    from shadernn_amd import host, models

    path = _json(tmp_path, 2)
    h = C.c_void_p()

    def create8(p, in_c=1, fmt=0x201, maxval=255, shift=0, siting=1, w=W, hh=H, batch=1):
        io = host.VideoIO(fmt, maxval, shift, siting, 127.5, 1 / 127.5, 127.5, 127.5)
        return host.lib().snn_model_create8(p.encode(), 0, w, hh, in_c, 0, 1, 0, 0, 0, batch, C.byref(io), C.byref(h))

    three = models.write_json(models.single_conv(seed=1, ic=3, oc=3), W, H, str(tmp_path / "three.json"))
    assert create8(three, 3) == -1                                  # a three-channel model
    wide = models.write_json(models.single_conv(seed=1, ic=1, oc=16), W, H, str(tmp_path / "wide.json"))
    assert create8(wide, 1) == -1                                   # one channel in, sixteen out
    assert create8(path, fmt=1) == -1 and create8(path, fmt=0x101) == -1  # R8 / R16 are not video formats
    assert create8(path, w=W - 1) == -1 and create8(path, hh=H - 1) == -1  # odd extents
    assert create8(path, fmt=0x301, maxval=65535) == -1             # P016 chroma is not built
    assert create8(path, batch=0) == -1
    assert host.lib().snn_model_create8(path.encode(), 0, W, H, 1, 0, 1, 0, 0, 0, 1, None, C.byref(h)) == -1
    assert create8(path) == 0                                       # the process and the device are fine
    frame = np.zeros(H * W * 3 // 2, np.uint8)
    assert host.lib().snn_model_upload_frame_nv12(h, frame.ctypes.data_as(C.c_void_p)) == 0
    assert host.lib().snn_model_destroy(h) == 0
    grey = host.Model(path, W, H, 1, input_format="R8", output_format="R8")  # not a video model: the NV12 calls refuse it
    assert host.lib().snn_model_upload_frame_nv12(grey.h, frame.ctypes.data_as(C.c_void_p)) == -1
    assert host.lib().snn_model_download_frame_nv12(grey.h, frame.ctypes.data_as(C.c_void_p)) == -1
    grey.close()
