"""NV12 / P010 frames to any output size through the C++ host mirror (snn_model_create11, host.Model(video=..., out_size=(w, h))): ESPCN at x2 / x3,
then two plane_fit launches.  The luma plane that comes back is tests/fit_ref.py applied to the luma plane a snn_model_create8 model of the same
file and input returns, the chroma plane is fit_ref applied to the ORIGINAL chroma plane at ratio out / in; both under fit_ref's rule (equal off
the near ties, within 1 << shift on them, near ties at most 2.5 % of a case's values).  At ratio 1 the luma is snn_model_create8's byte for byte."""
import ctypes as C

import numpy as np
import pytest

import fit_ref as R

pytestmark = pytest.mark.gpu
H, W = 24, 32  # the luma plane; the chroma plane is 12 x 16
TARGETS = [(2, 48, 36), (3, 48, 36), (2, 64, 48), (2, 40, 36)]  # (r, out_w, out_h): 3/4, exactly 1/2, ratio 1, two ratios in one frame
TARGET_IDS = ["x2to48x36", "x3to48x36", "x2to64x48", "x2to40x36"]


def _maps(maxval):
    half = maxval / 2.0
    return dict(in_means=(half, half, half, 0), in_norms=(1 / half, 1 / half, 1 / half, 1), out_scale=(half, half, half, 1), out_offset=(half, half, half, 0))


VIDEO = {"NV12": dict(maxval=255, shift=0, dtype=np.uint8), "P010": dict(maxval=1023, shift=6, dtype=np.uint16)}


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


def _run(m, frame, batch):
    y, cbcr = frame
    m.upload_frame((y, cbcr) if batch > 1 else (y[0], cbcr[0]))
    m.run()
    return m.download_frame()


def _check(m, ref, video, frame, batch, r, ow, oh, siting):
    v = VIDEO[video]
    got_y, got_c = _run(m, frame, batch)
    assert got_y.size == batch * oh * ow and got_c.size == batch * (oh // 2) * ow  # out_h*out_w + (out_h/2)*out_w elements per frame
    got_y, got_c = got_y.reshape(batch, oh, ow, 1), got_c.reshape(batch, oh // 2, ow // 2, 2)
    full_y = _run(ref, frame, batch)[0].reshape(batch, r * H, r * W, 1)  # the r-fold luma plane of snn_model_create8
    items = [(got_y, R.fit_values(full_y, oh, ow, "centre", v["shift"]), v["maxval"], v["shift"]),
             (got_c, R.fit_values(frame[1], oh // 2, ow // 2, siting, v["shift"]), v["maxval"], v["shift"])]
    frac, ndiff = R.compare_all(items)
    if (ow, oh) == (r * W, r * H):
        np.testing.assert_array_equal(got_y, full_y)  # ratio 1: a copy
    print("%s x%d -> %dx%d batch=%d siting=%s: near ties %.3f %%, %d values differ" % (video, r, ow, oh, batch, siting, 100 * frac, ndiff))
    return got_y, got_c


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("video", ["NV12", "P010"])
@pytest.mark.parametrize("target", TARGETS, ids=TARGET_IDS)
def test_fitted_video_frames_behind_espcn(ctx, tmp_path, monkeypatch, target, video, batch):
    from shadernn_amd import host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the four-launch inference
    r, ow, oh = target
    v = VIDEO[video]
    path = _json(tmp_path, r)
    ref = host.Model(path, W, H, 1, batch=batch, video=video, **_maps(v["maxval"]))
    unit = "u8" if video == "NV12" else "u16"
    for siting in ("left", "centre"):
        for capture in (False, True):
            m = host.Model(path, W, H, 1, batch=batch, video=video, siting=siting, out_size=(ow, oh), capture_graph=capture, **_maps(v["maxval"]))
            desc = m.describe()
            assert "[luma fit] plane_fit_%s c=1 %dx%d->%dx%d siting=centre" % (unit, r * H, r * W, oh, ow) in desc, desc
            assert "[chroma fit] plane_fit_%s c=2 %dx%d->%dx%d siting=%s" % (unit, H // 2, W // 2, oh // 2, ow // 2, siting) in desc, desc
            assert desc.count("plane_fit_kernel") == 2 and "chroma_up" not in desc, desc
            steps = [d for _, _, d, _, _ in m.plan_steps()]  # the ESPCN steps are what the plain video model launches: two fused kernels
            assert steps == [d for _, _, d, _, _ in ref.plan_steps()] and len(steps) == 2, steps
            _check(m, ref, video, _frame(video, batch, 10 * r + batch), batch, r, ow, oh, siting)
            m.close()
    ref.close()


@pytest.mark.parametrize("video", ["NV12", "P010"])
def test_a_captured_graph_replays_and_reads_each_new_frame(ctx, tmp_path, monkeypatch, video):
    from shadernn_amd import host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")
    r, ow, oh = 2, 48, 36
    v = VIDEO[video]
    path = _json(tmp_path, r)
    m = host.Model(path, W, H, 1, video=video, out_size=(ow, oh), capture_graph=True, **_maps(v["maxval"]))
    ref = host.Model(path, W, H, 1, video=video, **_maps(v["maxval"]))
    first = _check(m, ref, video, _frame(video, 1, 1), 1, r, ow, oh, "left")   # records
    again = _check(m, ref, video, _frame(video, 1, 1), 1, r, ow, oh, "left")   # replays
    third = _check(m, ref, video, _frame(video, 1, 1), 1, r, ow, oh, "left")   # replays again
    for a in (again, third):
        np.testing.assert_array_equal(a[0], first[0])
        np.testing.assert_array_equal(a[1], first[1])
    other = _check(m, ref, video, _frame(video, 1, 2), 1, r, ow, oh, "left")   # a new frame gives its own result
    assert not np.array_equal(other[0], first[0]) and not np.array_equal(other[1], first[1])
    m.close()
    ref.close()


def test_prefer_half(ctx, tmp_path):
    from shadernn_amd import host

    r, ow, oh = 2, 48, 36
    v = VIDEO["NV12"]
    path = _json(tmp_path, r)
    m = host.Model(path, W, H, 1, video="NV12", out_size=(ow, oh), prefer_half=True, **_maps(v["maxval"]))
    ref = host.Model(path, W, H, 1, video="NV12", prefer_half=True, **_maps(v["maxval"]))
    _check(m, ref, "NV12", _frame("NV12", 1, 8), 1, r, ow, oh, "left")
    m.close()
    ref.close()


def test_what_is_refused(ctx, tmp_path):
    from shadernn_amd import host

    h = C.c_void_p()

    def create11(p, ow, oh, w=W, hh=H, fmt=0x201, maxval=255, siting=1):
        io = host.FitIO(host.VideoIO(fmt, maxval, 0, siting, 127.5, 1 / 127.5, 127.5, 127.5), ow, oh)
        return host.lib().snn_model_create11(p.encode(), 0, w, hh, 1, 0, 1, 0, 0, 0, 1, C.byref(io), C.byref(h))

    x2, x3 = _json(tmp_path, 2), _json(tmp_path, 3)
    assert create11(x2, 72, 48) == -1   # above r: x2 gives 64 x 48
    assert create11(x2, 64, 50) == -1
    assert create11(x3, 30, 22) == -1   # below r / 2: x3 gives 96 x 72
    assert create11(x3, 48, 34) == -1
    assert create11(x2, 47, 36) == -1 and create11(x2, 48, 35) == -1  # an odd target
    assert create11(x2, 14, 36) == -1 and create11(x2, 130, 36) == -1 and create11(x2, 48, 10) == -1 and create11(x2, 48, 98) == -1  # outside [1/2, 4] of the input
    assert create11(x2, 48, 36, fmt=1) == -1 and create11(x2, 48, 36, siting=2) == -1 and create11(x2, 48, 36, w=W - 1) == -1  # what snn_model_create8 refuses
    assert host.lib().snn_model_create11(x2.encode(), 0, W, H, 1, 0, 1, 0, 0, 0, 1, None, C.byref(h)) == -1
    assert create11(x2, 48, 36) == 0    # the process and the device are fine
    frame = np.zeros(H * W * 3 // 2, np.uint8)
    assert host.lib().snn_model_upload_frame_nv12(h, frame.ctypes.data_as(C.c_void_p)) == 0
    assert host.lib().snn_model_destroy(h) == 0
    with pytest.raises(AssertionError, match="out_size"):
        host.Model(x2, W, H, 1, video="NV12", video_out="RGB8", out_size=(48, 36))
    with pytest.raises(AssertionError, match="out_size"):
        host.Model(x2, W, H, 1, colour="RGB8", out_size=(48, 36))
    with pytest.raises(AssertionError, match="out_size"):
        host.Model(x2, W, H, 1, input_format="R8", output_format="R8", out_size=(48, 36))
