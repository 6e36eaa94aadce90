"""Planar 4:2:0 frames (I420 / I010) through the C++ host mirror (snn_model_create12, host.Model(video="I420" | "I010", ...) and
host.Model(colour=..., video_out="I420")): ESPCN at x2 / x3 on a 32 x 24 luma frame, the four paths of include/snn_c.h.  The luma plane that comes back
is byte for byte that of the NV12 / P010 model built with the same maps (the same kernels on the same bytes); chroma and RGB are held against the
float64 references of the interleaved units on the (de)interleaved samples (tests/planar_ref.py) under those references' near-tie rule.  Launch counts
come from the description and from the launch trace; pitched planes go in and out through snn_model_upload_frame_planes / _download_frame_planes."""
import ctypes as C

import numpy as np
import pytest

import chroma_ref
import fit_ref
import planar_ref as P
import rgb_cbcr_ref as RC
import yuv_rgb_ref as RY

pytestmark = pytest.mark.gpu
H, W = 24, 32  # the luma plane; the chroma planes are 12 x 16

# planar format: its depth, the interleaved counterpart and how host.Model spells the counterpart's depth
VIDEO = {
    "I420": dict(maxval=255, shift=0, dtype=np.uint8, unit="u8", nv="NV12", nv_kw={}, outs=("RGB8", "RGBA8")),
    "I010": dict(maxval=1023, shift=0, dtype=np.uint16, unit="u16", nv="P010", nv_kw=dict(video_maxval=1023, video_shift=0), outs=("RGB16", "RGBA16")),
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


def _frame(video, batch, seed):
    """(y [n][H][W], cb, cr [n][H/2][W/2]) over the limited-range codes"""
    v = VIDEO[video]
    k = (v["maxval"] + 1) // 256
    rng = np.random.default_rng(seed)
    y = (rng.integers(16 * k, 236 * k, size=(batch, H, W)) << v["shift"]).astype(v["dtype"])
    cb = (rng.integers(16 * k, 241 * k, size=(batch, H // 2, W // 2)) << v["shift"]).astype(v["dtype"])
    cr = (rng.integers(16 * k, 241 * k, size=(batch, H // 2, W // 2)) << v["shift"]).astype(v["dtype"])
    return y, cb, cr


def _planes(cb, cr):
    """(cb, cr) [n][h][w] each -> the planar tensor [2n][h][w][1]"""
    return P.deinterleave(np.stack([cb, cr], axis=-1))


def _batched(arrays, batch):
    return tuple(a if batch > 1 else a[0] for a in arrays)


def _run(m, frame, batch):
    m.upload_frame(_batched(frame, batch))
    m.run()
    return m.download_frame()


def _run_nv(m, frame, batch):
    """the same samples through the interleaved counterpart"""
    y, cb, cr = frame
    m.upload_frame(_batched((y, np.stack([cb, cr], axis=-1)), batch))
    m.run()
    return m.download_frame()


def _launches(m, frame, batch):
    """(launches, kernel functions) of one inference, from the launch trace"""
    from shadernn_amd import capi

    m.upload_frame(_batched(frame, batch))
    capi.trace_begin()
    m.run()
    t = capi.trace_end()
    return t["launches"], sorted(k["function"] for k in t["kernels"])


def _extra(desc):
    return [line for line in desc.split("\n") if line.startswith("[") and ("chroma" in line.split("]")[0] or "rgb out" in line or "luma fit" in line or "colour in" in line)]


def _no_interleaving(fns, desc):
    assert not any("interleave" in f or "split" in f or "pack" in f for f in fns), fns
    assert "interleave" not in desc, desc


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("video", ["I420", "I010"])
@pytest.mark.parametrize("r", [2, 3])
def test_planar_in_planar_out(ctx, tmp_path, monkeypatch, r, video, batch):
    from shadernn_amd import host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the three-launch inference
    v = VIDEO[video]
    path = _json(tmp_path, r)
    rng = "limited" if r == 2 else "full"
    ref = host.Model(path, W, H, 1, batch=batch, video=v["nv"], **v["nv_kw"], **_luma_maps(v["maxval"], rng))
    frame = _frame(video, batch, 10 * r + batch)
    want_y = _run_nv(ref, frame, batch)[0]
    for siting in ("left", "centre"):
        for capture in (False, True):
            m = host.Model(path, W, H, 1, batch=batch, video=video, video_range=rng, siting=siting, capture_graph=capture)
            desc = m.describe()
            steps = [d for _, _, d, _, _ in m.plan_steps()]
            assert steps == [d for _, _, d, _, _ in ref.plan_steps()] and len(steps) == 2, steps
            extra = _extra(desc)
            assert len(extra) == 1 and "[chroma out] chroma_up_%s" % v["unit"] in extra[0] and " c=1 " in extra[0], desc  # 3 launches: C = 1 over 2N planes
            y, cb, cr = _run(m, frame, batch)
            assert y.dtype == v["dtype"] and y.shape == want_y.shape and cb.shape == cr.shape == ((r * H // 2, r * W // 2) if batch == 1 else (batch, r * H // 2, r * W // 2))
            np.testing.assert_array_equal(y, want_y)  # byte for byte
            got = _planes(cb.reshape(batch, r * H // 2, r * W // 2), cr.reshape(batch, r * H // 2, r * W // 2))
            frac, ndiff = chroma_ref.compare_all([(got, P.up_values(_planes(frame[1], frame[2]), r, siting, v["shift"]), v["maxval"], v["shift"])])
            print("%s x%d batch=%d siting=%s capture=%s: near ties %.3f %%, %d values differ" % (video, r, batch, siting, capture, 100 * frac, ndiff))
            if not capture:
                n, fns = _launches(m, frame, batch)
                assert n == 3 and len(fns) == 3, fns
                _no_interleaving(fns, desc)
            m.close()
    ref.close()


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("video", ["I420", "I010"])
@pytest.mark.parametrize("target", [(2, 48, 36), (3, 48, 36), (2, 40, 36)], ids=["x2to48x36", "x3to48x36", "x2to40x36"])
def test_planar_in_planar_out_at_a_fitted_size(ctx, tmp_path, monkeypatch, target, video, batch):
    from shadernn_amd import host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")
    r, ow, oh = target
    v = VIDEO[video]
    path = _json(tmp_path, r)
    ref = host.Model(path, W, H, 1, batch=batch, video=v["nv"], out_size=(ow, oh), **v["nv_kw"], **_luma_maps(v["maxval"], "limited"))
    frame = _frame(video, batch, 20 * r + batch)
    want_y = _run_nv(ref, frame, batch)[0]
    for siting, capture in (("left", False), ("centre", True)):
        m = host.Model(path, W, H, 1, batch=batch, video=video, siting=siting, out_size=(ow, oh), capture_graph=capture)
        desc = m.describe()
        assert len([d for _, _, d, _, _ in m.plan_steps()]) == 2
        assert "[luma fit] plane_fit_%s c=1 %dx%d->%dx%d siting=centre" % (v["unit"], r * H, r * W, oh, ow) in desc, desc
        assert "[chroma fit] plane_fit_%s c=1 %dx%d->%dx%d siting=%s" % (v["unit"], H // 2, W // 2, oh // 2, ow // 2, siting) in desc, desc
        assert desc.count("plane_fit_kernel") == 2 and "chroma_up" not in desc, desc  # 4 launches
        y, cb, cr = _run(m, frame, batch)
        np.testing.assert_array_equal(y, want_y)  # byte for byte
        got = _planes(cb.reshape(batch, oh // 2, ow // 2), cr.reshape(batch, oh // 2, ow // 2))
        frac, ndiff = fit_ref.compare_all([(got, P.fit_values(_planes(frame[1], frame[2]), oh // 2, ow // 2, siting, v["shift"]), v["maxval"], v["shift"])])
        print("%s x%d -> %dx%d batch=%d siting=%s: near ties %.3f %%, %d values differ" % (video, r, ow, oh, batch, siting, 100 * frac, ndiff))
        if not capture:
            n, fns = _launches(m, frame, batch)
            assert n == 4, fns
            _no_interleaving(fns, desc)
        m.close()
    ref.close()


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("video", ["I420", "I010"])
@pytest.mark.parametrize("r", [2, 3])
def test_planar_in_rgb_out(ctx, tmp_path, monkeypatch, r, video, batch):
    from shadernn_amd import host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")
    v = VIDEO[video]
    path = _json(tmp_path, r)
    frame = _frame(video, batch, 30 * r + batch)
    for rng, siting, video_out, capture in (("limited", "left", v["outs"][0], False), ("full", "centre", v["outs"][1], True)):
        channels = 4 if "A" in video_out else 3
        ref = host.Model(path, W, H, 1, batch=batch, video=v["nv"], siting=siting, **v["nv_kw"], **_luma_maps(v["maxval"], rng))
        yhi = _run_nv(ref, frame, batch)[0].reshape(batch, r * H, r * W, 1)  # the luma plane the RGB launch reads: the same two fused kernels
        m = host.Model(path, W, H, 1, batch=batch, video=video, video_out=video_out, video_range=rng, siting=siting, capture_graph=capture)
        desc = m.describe()
        steps = [d for _, _, d, _, _ in m.plan_steps()]
        assert steps == [d for _, _, d, _, _ in ref.plan_steps()] and len(steps) == 2, steps
        extra = _extra(desc)
        assert len(extra) == 1 and extra[0].startswith("[rgb out] yuv_rgb_planar_%s r=%d c=%d siting=%s range=%s" % (v["unit"], r, channels, siting, rng)), desc
        assert "kernel=yuv_rgb_planar_kernel" in extra[0] and "chroma_up" not in desc, desc  # 3 launches
        got = _run(m, frame, batch).reshape(batch, r * H, r * W, channels)
        assert got.dtype == v["dtype"]
        frac, ndiff = RY.compare_all([(got, P.yuv_values(yhi, _planes(frame[1], frame[2]), r, siting, rng, v["maxval"], v["shift"]), v["maxval"], v["shift"])])
        print("%s -> %s x%d batch=%d: near ties %.3f %%, %d values differ" % (video, video_out, r, batch, 100 * frac, ndiff))
        if not capture:
            n, fns = _launches(m, frame, batch)
            assert n == 3 and "yuv_rgb_planar_kernel" in fns, fns
            _no_interleaving(fns, desc)
        m.close()
        ref.close()


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("r", [2, 3])
def test_rgb_in_planar_out(ctx, tmp_path, monkeypatch, r, batch):
    from shadernn_amd import host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")
    path = _json(tmp_path, r)
    for colour, rng, siting, capture in (("RGB8", "limited", "left", False), ("RGBA8", "full", "centre", True)):
        rgb = RC.frame(40 * r + batch, batch, H, W, 4 if colour == "RGBA8" else 3)
        ref = host.Model(path, W, H, 1, batch=batch, colour=colour, video_out="NV12", video_range=rng, siting=siting)
        ref.upload_frame(rgb if batch > 1 else rgb[0])
        ref.run()
        want_y = ref.download_frame()[0]
        m = host.Model(path, W, H, 1, batch=batch, colour=colour, video_out="I420", video_range=rng, siting=siting, capture_graph=capture)
        desc = m.describe()
        steps = [d for _, _, d, _, _ in m.plan_steps()]
        assert steps == [d for _, _, d, _, _ in ref.plan_steps()] and len(steps) == 2, steps
        assert "[colour in] rgb_luma" in desc and "[chroma out] rgb_cbcr_planar_u8 r=%d c=%d siting=%s range=%s" % (r, rgb.shape[-1], siting, rng) in desc, desc
        assert "kernel=rgb_cbcr_planar_kernel" in desc and "ycc_merge" not in desc, desc  # 4 launches
        m.upload_frame(rgb if batch > 1 else rgb[0])
        m.run()
        y, cb, cr = m.download_frame()
        np.testing.assert_array_equal(y, want_y)  # byte for byte
        got = np.stack([cb.reshape(batch, r * H // 2, r * W // 2), cr.reshape(batch, r * H // 2, r * W // 2)], axis=-1)
        frac, ndiff = RC.compare_all([(got, RC.values(rgb, r, siting, rng))])
        print("%s -> I420 x%d batch=%d: near ties %.3f %%, %d bytes differ" % (colour, r, batch, 100 * frac, ndiff))
        if not capture:
            from shadernn_amd import capi

            capi.trace_begin()
            m.run()
            t = capi.trace_end()
            fns = sorted(k["function"] for k in t["kernels"])
            assert t["launches"] == 4 and "rgb_cbcr_planar_kernel" in fns, fns
            _no_interleaving(fns, desc)
        m.close()
        ref.close()


def test_prefer_half(ctx, tmp_path):
    from shadernn_amd import host

    path = _json(tmp_path, 2)
    frame = _frame("I420", 1, 8)
    for kw in (dict(video="I420"), dict(video="I420", out_size=(48, 36)), dict(video="I420", video_out="RGB8")):
        m = host.Model(path, W, H, 1, prefer_half=True, **kw)
        out = _run(m, frame, 1)
        assert all(a.size > 0 for a in (out if isinstance(out, tuple) else (out,)))
        m.close()
    m = host.Model(path, W, H, 1, prefer_half=True, colour="RGB8", video_out="I420")
    m.upload_frame(RC.frame(3, 1, H, W, 3)[0])
    m.run()
    y, cb, cr = m.download_frame()
    assert y.shape == (2 * H, 2 * W) and cb.shape == cr.shape == (H, W)
    m.close()


def _pitched(a, pad, poison):
    """a copy of the 2-D array `a` as a view into a buffer whose rows are `pad` elements longer, the padding holding `poison`"""
    buf = np.full((a.shape[0], a.shape[1] + pad), poison, a.dtype)
    buf[:, :a.shape[1]] = a
    return buf, buf[:, :a.shape[1]]


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("video", ["I420", "I010", "NV12"])
def test_pitched_planes_in_and_out(ctx, tmp_path, video, batch):
    """pitch = width + 13 elements, the padding poisoned on the way in and pre-filled with 0xA5 on the way out; n_planes = 3 on a planar model and 2
    on an NV12 model (Y, CbCr: the interleaved plane as rows of W elements)"""
    from shadernn_amd import host

    r = 2
    path = _json(tmp_path, r)
    planar = video in VIDEO
    v = VIDEO[video] if planar else dict(maxval=255, shift=0, dtype=np.uint8)
    kw = dict(video_range="limited") if planar else _luma_maps(255, "limited")
    m = host.Model(path, W, H, 1, batch=batch, video=video, **kw)
    y, cb, cr = _frame(video if planar else "I420", batch, 50 + batch)
    chroma = [cb, cr] if planar else [np.stack([cb, cr], axis=-1).reshape(batch, H // 2, W)]
    m.upload_frame(_batched((y, cb, cr), batch) if planar else _batched((y, np.stack([cb, cr], axis=-1)), batch))
    m.run()
    tight = m.download_frame()
    tight = [np.asarray(a).reshape((batch,) + np.asarray(a).shape[-2 if planar or i == 0 else -3:]) for i, a in enumerate(tight)]
    if not planar:
        tight[1] = tight[1].reshape(batch, r * H // 2, r * W)

    poison = 0x5A if v["dtype"] == np.uint8 else 0x5A5A
    keep, views = [], []
    for n in range(batch):
        for a in [y] + chroma:
            buf, view = _pitched(a[n], 13, poison)
            keep.append(buf)
            views.append(view)
    assert views[0].strides[0] == (W + 13) * y.itemsize
    m.upload_planes(views)
    m.run()
    again = m.download_frame()
    for a, b in zip(again, m.download_frame()):
        np.testing.assert_array_equal(a, b)
    for i, a in enumerate(again):  # the pitched upload gives the bytes of the tight one: no padding byte was taken for a sample
        np.testing.assert_array_equal(np.asarray(a).reshape(tight[i].shape), tight[i])

    fill = 0xA5 if v["dtype"] == np.uint8 else 0xA5A5
    outs, oviews = [], []
    for n in range(batch):
        for t in tight:
            buf = np.full((t.shape[1], t.shape[2] + 13), fill, v["dtype"])
            outs.append(buf)
            oviews.append(buf[:, :t.shape[2]])
    m.download_planes(oviews)
    k = len(tight)
    for n in range(batch):
        for p in range(k):
            np.testing.assert_array_equal(oviews[n * k + p], tight[p][n])                     # the payload
            assert (outs[n * k + p][:, tight[p].shape[2]:] == fill).all()                      # the padding still reads 0xA5
    # a plane count that does not match this end, and a pitch below the row's bytes
    lib = host.lib()
    ptrs = (C.c_void_p * len(views))(*[a.ctypes.data for a in views])
    good = (C.c_int * k)(*[views[p].strides[0] for p in range(k)])
    assert lib.snn_model_upload_frame_planes(m.h, ptrs, good, k) == 0
    assert lib.snn_model_upload_frame_planes(m.h, ptrs, good, 5 - k) == -1 and lib.snn_model_download_frame_planes(m.h, ptrs, good, 5 - k) == -1
    short = (C.c_int * k)(*[W * y.itemsize - 1] + [views[p].strides[0] for p in range(1, k)])
    assert lib.snn_model_upload_frame_planes(m.h, ptrs, short, k) == -1
    short_c = (C.c_int * k)(*[views[0].strides[0]] + [chroma[0].shape[2] * y.itemsize - 1] * (k - 1))
    assert lib.snn_model_upload_frame_planes(m.h, ptrs, short_c, k) == -1
    assert lib.snn_model_upload_frame_planes(m.h, None, good, k) == -1 and lib.snn_model_upload_frame_planes(m.h, ptrs, None, k) == -1
    flat = np.zeros(batch * H * W * 3 // 2, v["dtype"])
    rc = lib.snn_model_upload_frame_nv12(m.h, flat.ctypes.data_as(C.c_void_p))
    assert rc == (-1 if planar else 0)  # the NV12 functions keep their behaviour and refuse planar ends
    m.close()


def test_the_plane_functions_refuse_rgb_ends(ctx, tmp_path):
    from shadernn_amd import host

    path = _json(tmp_path, 2)
    lib = host.lib()
    y, c = np.zeros((2 * H, 2 * W), np.uint8), np.zeros((H, W), np.uint8)
    ptrs = (C.c_void_p * 3)(y.ctypes.data, c.ctypes.data, c.ctypes.data)
    m = host.Model(path, W, H, 1, video="I420", video_out="RGB8")
    assert lib.snn_model_download_frame_planes(m.h, ptrs, (C.c_int * 3)(2 * W, W, W), 3) == -1      # an RGB output
    assert lib.snn_model_upload_frame_planes(m.h, ptrs, (C.c_int * 3)(W, W // 2, W // 2), 3) == 0  # its input end is planar
    m.close()
    m = host.Model(path, W, H, 1, colour="RGB8", video_out="I420")
    assert lib.snn_model_upload_frame_planes(m.h, ptrs, (C.c_int * 3)(W, W // 2, W // 2), 3) == -1  # an RGB input
    assert lib.snn_model_download_frame_planes(m.h, ptrs, (C.c_int * 3)(2 * W, W, W), 3) == 0
    nv = np.zeros(2 * H * 2 * W * 3 // 2, np.uint8)
    assert lib.snn_model_download_frame_nv12(m.h, nv.ctypes.data_as(C.c_void_p)) == -1               # a planar end
    m.close()
    m = host.Model(path, W, H, 1, input_format="R8", output_format="R8")
    assert lib.snn_model_upload_frame_planes(m.h, ptrs, (C.c_int * 3)(W, W // 2, W // 2), 3) == -1  # no video frames at all
    m.close()


def test_what_needs_the_models_r_is_refused(ctx, tmp_path):
    from shadernn_amd import host, models

    handle = C.c_void_p()

    def create12(p, in_format=0x401, out_format=0x401, ow=0, oh=0, w=W, hh=H):
        io = host.PlanarIO(in_format, out_format, 255, 0, 1, 0, 0.299, 0.114, ow, oh)
        return host.lib().snn_model_create12(p.encode(), 0, w, hh, 1, 0, 1, 0, 0, 0, 1, C.byref(io), C.byref(handle))

    x2, x3 = _json(tmp_path, 2), _json(tmp_path, 3)
    assert create12(x2, ow=72, oh=48) == -1 and create12(x2, ow=64, oh=50) == -1   # above r: x2 gives 64 x 48
    assert create12(x3, ow=30, oh=22) == -1 and create12(x3, ow=48, oh=34) == -1   # below r / 2: x3 gives 96 x 72
    one = models.write_json(models.single_conv(seed=1, ic=1, oc=1), W, H, str(tmp_path / "one.json"))
    assert create12(one, in_format=3) == -1                                        # r = 1 with RGB in: the chroma grid would be decimated
    wide = models.write_json(models.single_conv(seed=1, ic=1, oc=16), W, H, str(tmp_path / "wide.json"))
    assert create12(wide) == -1 and create12(wide, out_format=3) == -1             # one channel in, sixteen out
    x3odd = models.write_json(models.espcn_weights(seed=1, scale=3), 47, H, str(tmp_path / "x3odd.json"))
    assert create12(x3odd, in_format=3, w=47) == -1                                # r * in_w is odd: no 4:2:0 planes
    assert create12(x2, ow=48, oh=36) == 0                                         # the process and the device are fine
    assert host.lib().snn_model_destroy(handle) == 0
    with pytest.raises(AssertionError, match="out_size"):
        host.Model(x2, W, H, 1, video="I420", video_out="RGB8", out_size=(48, 36))
    with pytest.raises(AssertionError, match="out_size"):
        host.Model(x2, W, H, 1, colour="RGB8", video_out="I420", out_size=(48, 36))
