"""RGB frames at any output size through the C++ host mirror (snn_model_create13, host.Model(..., rgb_size=(w, h))): ESPCN at x2 / x3, then the luma
fit and the rgb_fit launch.  The frame that comes back is tests/rgb_fit_ref.py applied to tests/fit_ref.py's fit of the r-fold luma plane that a
snn_model_create8 / snn_model_create5 model of the same file and input returns, and to the ORIGINAL chroma planes (or the colour frame that went
in), under rgb_fit_ref's rule: equal off the near ties, within 1 << shift on them, near ties at most 3 % (1 % for colour frames) of a case's
values.  Where the fitted luma value itself is a near tie of fit_ref the device's luma sample may be the other neighbour: such a pixel is also
accepted against the reference evaluated on that neighbour.  Colour frames are chosen so that no luma value is a near tie of rgb_luma's rounding, as
tests/test_frame_colour_host_gpu.py chooses them.  Launch counts (4 from video, 5 from colour frames) come from the description and
from the launch trace."""
import ctypes as C

import numpy as np
import pytest

import colour_ref
import fit_ref
import metrics_ref
import rgb_fit_ref as R
from test_frame_metrics_host_gpu import _check as _check_rows

pytestmark = pytest.mark.gpu
H, W = 24, 32  # the model's input; the chroma planes are 12 x 16
# (r, out_w, out_h): 3/4 of the x2 frame, exactly 1/2 of the x3 frame, ratio 1 (x2) and 2/3 (x3), two ratios in one frame, an odd size
TARGETS = [(2, 48, 36), (3, 48, 36), (2, 64, 48), (3, 64, 48), (2, 40, 36), (2, 47, 35)]
TARGET_IDS = ["x%dto%dx%d" % t for t in TARGETS]
# source: what host.Model takes, the frame's depth, the kind of chroma source, the counterpart whose luma plane is the reference's input
SOURCES = {
    "NV12": dict(kw=dict(video="NV12", video_out="RGB8"), maxval=255, shift=0, dtype=np.uint8, unit="u8", src="cbcr", c=3, nv="NV12", nv_kw={}),
    "P010": dict(kw=dict(video="P010", video_out="RGBA16"), maxval=1023, shift=6, dtype=np.uint16, unit="u16", src="cbcr", c=4, nv="P010", nv_kw={}),
    "I420": dict(kw=dict(video="I420", video_out="RGBA8"), maxval=255, shift=0, dtype=np.uint8, unit="u8", src="planar", c=4, nv="NV12", nv_kw={}),
    "RGB8": dict(kw=dict(colour="RGB8"), maxval=255, shift=0, dtype=np.uint8, unit="u8", src="rgb", c=3),
    "RGBA8": dict(kw=dict(colour="RGBA8"), maxval=255, shift=0, dtype=np.uint8, unit="u8", src="rgb", c=4),
}


def _luma_maps(maxval, rng):
    """the luma plane's maps as include/snn_c.h states them for snn_model_create9"""
    k = (maxval + 1) / 256.0
    off, span = (16.0 * k, 219.0 * k) if rng == "limited" else (0.0, float(maxval))
    return dict(in_means=(off,) * 4, in_norms=(1.0 / span,) * 4, out_scale=(span,) * 4, out_offset=(off,) * 4)


def _json(tmp_path, r):
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r)
    return models.write_json(net, W, H, str(tmp_path / (net["name"] + ".json")))


def _frame(source, batch, seed):
    """video: (y [n][H][W], cbcr [n][H/2][W/2][2]) of tests/yuv_rgb_ref.py's recipe; colour: the frame [n][H][W][C], whole-range random bytes"""
    s = SOURCES[source]
    g = np.random.default_rng(seed)
    if s["src"] == "rgb":
        # as tests/test_frame_colour_host_gpu.py: no pixel's luma is a near tie of the rounding (the low bit of G is flipped where it is: the luma moves
        # by kg), so that the model's input plane is colour_ref.luma(frame) byte for byte -- one luma byte off would change the r-fold luma frame over
        # the network's whole receptive field
        u = g.integers(0, 256, size=(batch, H, W, s["c"])).astype(np.uint8)
        tie = colour_ref.near_tie(colour_ref.luma_values(u))[..., 0]
        u[..., 1][tie] ^= 1
        assert not colour_ref.near_tie(colour_ref.luma_values(u)).any()
        return u
    k = (s["maxval"] + 1) // 256
    y = (g.integers(40 * k, 200 * k, size=(batch, H, W)) << s["shift"]).astype(s["dtype"])
    cbcr = (g.integers(96 * k, 160 * k, size=(batch, H // 2, W // 2, 2)) << s["shift"]).astype(s["dtype"])
    return y, cbcr


def _first(a, batch):
    return a if batch > 1 else a[0]


def _upload(m, source, frame, batch):
    s = SOURCES[source]
    if s["src"] == "rgb":
        m.upload_frame(_first(frame, batch))
    elif s["src"] == "planar":
        m.upload_frame((_first(frame[0], batch), _first(frame[1][..., 0], batch), _first(frame[1][..., 1], batch)))
    else:
        m.upload_frame((_first(frame[0], batch), _first(frame[1], batch)))


def _run(m, source, frame, batch, ow, oh):
    _upload(m, source, frame, batch)
    m.run()
    out = m.download_frame()
    s = SOURCES[source]
    assert out.dtype == s["dtype"] and out.size == batch * oh * ow * s["c"]
    return out.reshape(batch, oh, ow, s["c"])


def _reference_model(path, source, batch, rng, prefer_half=False):
    from shadernn_amd import host

    s = SOURCES[source]
    if s["src"] == "rgb":  # snn_model_create5: R8 at both ends with the full-range luma maps
        return host.Model(path, W, H, 1, batch=batch, input_format="R8", output_format="R8", in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4, prefer_half=prefer_half)
    return host.Model(path, W, H, 1, batch=batch, video=s["nv"], prefer_half=prefer_half, **s["nv_kw"], **_luma_maps(s["maxval"], rng))  # snn_model_create8


def _full_luma(ref, source, frame, batch, r):
    """the r-fold luma plane [n][rH][rW][1] of the counterpart model on the same input"""
    s = SOURCES[source]
    if s["src"] == "rgb":
        ref.upload_frame(_first(colour_ref.luma(frame), batch))
        ref.run()
        return ref.download_frame().reshape(batch, r * H, r * W, 1)
    ref.upload_frame((_first(frame[0], batch), _first(frame[1], batch)))
    ref.run()
    return ref.download_frame()[0].reshape(batch, r * H, r * W, 1)


def _compare(got, full_y, source, frame, ow, oh, siting, rng):
    """rgb_fit_ref on fit_ref.fit of the r-fold luma; returns (near-tie share, values that differ from the reference frame)."""
    s = SOURCES[source]
    maxval, shift = s["maxval"], s["shift"]
    lv = fit_ref.fit_values(full_y, oh, ow, "centre", shift)
    yfit = fit_ref.quantise(lv, maxval, shift, full_y.dtype)
    luma_tie = fit_ref.near_tie(lv, fit_ref.EPS[maxval])[..., 0]
    if s["src"] == "rgb":
        values = lambda y: R.rgb_values(y, frame)  # noqa: E731
        if s["c"] == 4:
            np.testing.assert_array_equal(got[..., 3:], R.alpha_of(frame, oh, ow))
    else:
        values = lambda y: R.video_values(y, frame[1], siting, rng, maxval, shift)  # noqa: E731
        if s["c"] == 4:
            assert (got[..., 3] == maxval << shift).all()
    assert not (got.astype(np.int64) & ((1 << shift) - 1)).any(), "bits below the shift are set"
    ok = ties = ndiff = None
    for d in (0, -1, 1):
        y = np.clip(yfit.astype(np.int64) + (d << shift), 0, maxval << shift).astype(yfit.dtype)
        v = values(y)
        tie = R.near_tie(v, R.EPS[maxval])
        diff = (got[..., :3].astype(np.int64) >> shift) - (R.quantise(v, maxval, shift, got.dtype).astype(np.int64) >> shift)
        good = ((diff == 0) | (tie & (np.abs(diff) <= 1))).all(axis=-1)
        if d == 0:
            ok, ties, ndiff = good, float(tie.mean()), int((diff != 0).sum())
        else:
            ok = ok | (good & luma_tie)
    assert ok.all(), "%d pixels differ off the near ties, first at %s" % (int((~ok).sum()), tuple(np.argwhere(~ok)[0]))
    assert ties <= R.MAX_TIE_FRACTION["rgb" if s["src"] == "rgb" else "video"], "near ties are %.2f %% of the reference values: change the seed" % (100 * ties)
    return ties, ndiff


def _describe_checks(m, ref, source, r, ow, oh, siting, rng):
    s = SOURCES[source]
    desc = m.describe()
    steps = [d for _, _, d, _, _ in m.plan_steps()]  # the ESPCN steps are what the counterpart launches: two fused kernels
    assert steps == [d for _, _, d, _, _ in ref.plan_steps()] and len(steps) == 2, steps
    extra = [line for line in desc.split("\n") if line.startswith("[") and not line[1:line.index("]")].strip().isdigit()]  # (the stages are "[0] ...")
    labels = [line.split("]")[0] + "]" for line in extra]
    assert labels == (["[colour in]"] if s["src"] == "rgb" else []) + ["[luma fit]", "[rgb fit]"], desc  # 5 / 4 launches, in this order
    assert "[luma fit] plane_fit_%s c=1 %dx%d->%dx%d siting=centre" % (s["unit"], r * H, r * W, oh, ow) in desc, desc
    sh, sw = (H, W) if s["src"] == "rgb" else (H // 2, W // 2)
    want = "[rgb fit] rgb_fit_%s src=%s c=%d %dx%d->%dx%d siting=%s range=%s" % (s["unit"], s["src"], s["c"], sh, sw, oh, ow, "centre" if s["src"] == "rgb" else siting,
                                                                             "full" if s["src"] == "rgb" else rng)
    assert want in desc and "kernel=rgb_fit_kernel" in desc, desc
    for absent in ("chroma_up", "yuv_rgb", "ycc_merge", "[chroma fit]"):
        assert absent not in desc, desc
    return len(steps) + len(extra)


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("target", TARGETS, ids=TARGET_IDS)
def test_fitted_rgb_frames_behind_espcn(ctx, tmp_path, monkeypatch, target, source):
    from shadernn_amd import capi, host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the four-launch inference
    r, ow, oh = target
    s = SOURCES[source]
    path = _json(tmp_path, r)
    rng = "limited" if r == 2 else "full"
    siting = "left" if (ow + r) % 2 == 0 else "centre"
    for batch in (1, 2):
        ref = _reference_model(path, source, batch, rng)
        frame = _frame(source, batch, 10 * r + batch + ow)
        full_y = _full_luma(ref, source, frame, batch, r)
        outs = []
        for capture in (False, True):
            kw = dict(s["kw"], rgb_size=(ow, oh), batch=batch, capture_graph=capture)
            if s["src"] != "rgb":
                kw.update(siting=siting, video_range=rng)
            m = host.Model(path, W, H, 1, **kw)
            launches = _describe_checks(m, ref, source, r, ow, oh, siting, rng)
            assert launches == (5 if s["src"] == "rgb" else 4)
            got = _run(m, source, frame, batch, ow, oh)
            ties, ndiff = _compare(got, full_y, source, frame, ow, oh, siting, rng)
            print("%s x%d -> %dx%d batch=%d capture=%s: near ties %.3f %%, %d values differ" % (source, r, ow, oh, batch, capture, 100 * ties, ndiff))
            if capture:  # replayed on a new frame, then on the first again
                other = _frame(source, batch, 99)
                _compare(_run(m, source, other, batch, ow, oh), _full_luma(ref, source, other, batch, r), source, other, ow, oh, siting, rng)
                np.testing.assert_array_equal(_run(m, source, frame, batch, ow, oh), got)
            else:
                _upload(m, source, frame, batch)
                capi.trace_begin()
                m.run()
                t = capi.trace_end()
                fns = sorted(k["function"] for k in t["kernels"])
                assert t["launches"] == launches, fns
                assert any("plane_fit_kernel" in f for f in fns) and any("rgb_fit_kernel" in f for f in fns), fns
                assert not any(n in f for f in fns for n in ("yuv_rgb", "ycc_merge", "chroma_up")), fns
            outs.append(got)
            m.close()
        np.testing.assert_array_equal(outs[0], outs[1])  # direct and recorded: the same bytes
        ref.close()


def test_pitched_planes_in(ctx, tmp_path):
    from shadernn_amd import host

    r, ow, oh = 2, 47, 35
    path = _json(tmp_path, r)
    for source in ("NV12", "I420"):
        s = SOURCES[source]
        m = host.Model(path, W, H, 1, rgb_size=(ow, oh), **s["kw"])
        y, cbcr = _frame(source, 1, 5)
        tight = _run(m, source, (y, cbcr), 1, ow, oh)
        planes = [y[0], cbcr[0].reshape(H // 2, W)] if source == "NV12" else [y[0], cbcr[0, ..., 0], cbcr[0, ..., 1]]
        views = []
        for p in planes:
            wide = np.full((p.shape[0], p.shape[1] + 13), 0xEE, p.dtype)
            wide[:, :p.shape[1]] = p
            views.append(wide[:, :p.shape[1]])
        m.upload_planes(views)
        m.run()
        np.testing.assert_array_equal(m.download_frame().reshape(tight.shape), tight)  # no padding byte was taken for a sample
        m.close()


@pytest.mark.parametrize("source", ["NV12", "P010", "RGBA8"])
def test_metrics_of_the_fitted_frame(ctx, tmp_path, source):
    from shadernn_amd import host

    r, ow, oh, batch = 2, 48, 36, 2
    s = SOURCES[source]
    m = host.Model(_json(tmp_path, r), W, H, 1, batch=batch, rgb_size=(ow, oh), **s["kw"])
    out = _run(m, source, _frame(source, batch, 3), batch, ow, oh)
    g = np.random.default_rng(4)
    v = (out.astype(np.int64) >> s["shift"]) + g.integers(-6, 7, out.shape) * (s["maxval"] + 1) // 256
    ref = (np.clip(v, 0, s["maxval"]) << s["shift"]).astype(out.dtype)
    m.set_reference(ref)
    want = []
    for n in range(batch):
        for c, row in enumerate(metrics_ref.frame_metrics(out[n:n + 1], ref[n:n + 1], s["maxval"], s["shift"])):
            want.append(dict(row, image=n, plane=0, channel=c))
    _check_rows(m.metrics(), want, "%s -> %dx%d" % (source, ow, oh))  # one packed plan at the fitted size
    m.close()


def test_prefer_half(ctx, tmp_path):
    from shadernn_amd import host

    r, ow, oh = 2, 48, 36
    path = _json(tmp_path, r)
    for source in ("NV12", "RGB8"):
        m = host.Model(path, W, H, 1, rgb_size=(ow, oh), prefer_half=True, **SOURCES[source]["kw"])
        ref = _reference_model(path, source, 1, "limited", prefer_half=True)
        frame = _frame(source, 1, 8)
        _compare(_run(m, source, frame, 1, ow, oh), _full_luma(ref, source, frame, 1, r), source, frame, ow, oh, "left", "limited")
        m.close()
        ref.close()


def test_the_earlier_models_launch_what_they_launched(ctx, tmp_path):
    """snn_model_create9 and snn_model_create7 on the same file: three and four launches, none of them the new kernel."""
    from shadernn_amd import capi, host

    path = _json(tmp_path, 2)
    for source, kw, want, kernel in (("NV12", dict(video="NV12", video_out="RGB8"), 3, "yuv_rgb_kernel"), ("RGB8", dict(colour="RGB8", in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4), 4, "ycc_merge_u8_kernel")):
        m = host.Model(path, W, H, 1, **kw)
        _upload(m, source, _frame(source, 1, 2), 1)
        capi.trace_begin()
        m.run()
        t = capi.trace_end()
        fns = sorted(k["function"] for k in t["kernels"])
        assert t["launches"] == want and any(kernel in f for f in fns), fns
        assert not any("rgb_fit" in f or "plane_fit" in f for f in fns) and "rgb fit" not in m.describe(), fns
        m.close()


def test_what_is_refused_once_r_is_known(ctx, tmp_path, capfd):
    from shadernn_amd import host

    h = C.c_void_p()

    def create13(p, ow, oh, a=0x201, b=3):
        io = host.RgbFitIO(a, b, 255, 0, 1, 0, 0.299, 0.114, ow, oh)
        return host.lib().snn_model_create13(p.encode(), 0, W, H, 1, 0, 1, 0, 0, 0, 1, C.byref(io), C.byref(h))

    def refused(p, ow, oh, *needles, **kw):
        capfd.readouterr()
        assert create13(p, ow, oh, **kw) == -1, (ow, oh)
        log = "".join(capfd.readouterr())
        assert "snn_model_create13" in log and all(n in log for n in needles), log

    x1, x2, x3 = _json(tmp_path, 1), _json(tmp_path, 2), _json(tmp_path, 3)
    refused(x2, 72, 48, "r = 2", "larger than that", "a model of r = 3")      # above r: x2 gives 64 x 48
    refused(x2, 64, 50, "r = 2", "larger than that")
    refused(x3, 47, 36, "r = 3", "less than half of that", "a model of r = 2")  # below r / 2: x3 gives 96 x 72
    refused(x3, 48, 35, "r = 3", "less than half of that")
    refused(x2, 31, 24, "r = 2", "less than half of that", "a model of r = 1")
    refused(x1, 33, 24, "r = 1", "larger than that", a=3, b=3)                  # a colour frame at r = 1: out = in alone
    refused(x1, 32, 25, "r = 1", "larger than that", a=4, b=4)
    assert create13(x1, 32, 24, a=3, b=3) == 0 and host.lib().snn_model_destroy(h) == 0
    assert create13(x1, 20, 16) == 0 and host.lib().snn_model_destroy(h) == 0   # video at r = 1: down to a half
    assert create13(x2, 47, 35) == 0                                            # the process and the device are fine; an odd size
    frame = np.zeros(H * W * 3 // 2, np.uint8)
    assert host.lib().snn_model_upload_frame_nv12(h, frame.ctypes.data_as(C.c_void_p)) == 0
    assert host.lib().snn_model_download_frame_nv12(h, frame.ctypes.data_as(C.c_void_p)) == -1  # an RGB end
    assert host.lib().snn_model_destroy(h) == 0
