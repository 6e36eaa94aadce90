"""Colour frames through the C++ host mirror (snn_model_create7, host.Model(colour=...)): ESPCN at x2 / x3 / x4 on RGB8 / RGBA8 frames.  The expected
bytes are colour_ref.merge(Yhi, rgb, r) with Yhi what the same build's R8 -> R8 model (snn_model_create5) returns for colour_ref.luma(rgb), so the
network's own rounding never enters the comparison; colour_ref.compare is the rule (equal off the near ties, within 1 on them).  The frames are
chosen so that no luma value is a near tie: one luma byte off would change Yhi over the network's whole receptive field."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as R

pytestmark = pytest.mark.gpu
H, W = 37, 29
DEMO = dict(in_means=(127.5, 127.5, 127.5, 0), in_norms=(1 / 127.5, 1 / 127.5, 1 / 127.5, 1), out_scale=(127.5, 127.5, 127.5, 1), out_offset=(127.5, 127.5, 127.5, 0))


def _json(tmp_path, r):
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r)
    return models.write_json(net, W, H, str(tmp_path / (net["name"] + ".json")))


def _frame(batch, c, seed, coeff=R.BT601):
    """Random bytes, except that no pixel's luma is a near tie of the rounding (the low bit of G is flipped where it is: the luma moves by kg): the
    model's input plane then is colour_ref.luma(rgb) byte for byte, and Yhi from the R8 model is what the colour model merges."""
    u = np.random.default_rng(seed).integers(0, 256, size=(batch, H, W, c), dtype=np.uint8)
    if c >= 3:
        tie = R.near_tie(R.luma_values(u, *coeff))[..., 0]
        u[..., 1][tie] ^= 1
        assert not R.near_tie(R.luma_values(u, *coeff)).any()
    return u


def _run(m, frame, batch, r, c):
    m.upload_frame(frame if batch > 1 else frame[0])
    m.run()
    return m.output_frame().reshape(batch, r * H, r * W, c)


def _check(colour_model, r8_model, rgb, batch, r, kw=None):
    c = rgb.shape[-1]
    got = _run(colour_model, rgb, batch, r, c)
    yhi = _run(r8_model, R.luma(rgb, **(kw or {})), batch, r, 1)
    ties, total, ndiff = R.compare(got[..., :3], R.merge_values(yhi, rgb, r, **(kw or {})))
    print("r=%d batch=%d c=%d: near ties %.3f %%, %d bytes differ" % (r, batch, c, 100.0 * ties / total, ndiff))
    if c == 4:
        np.testing.assert_array_equal(got[..., 3], R.merge(yhi, rgb, r)[..., 3])
    return got, yhi


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_rgb8_frames_around_espcn(ctx, tmp_path, r, batch):
    from shadernn_amd import host

    path = _json(tmp_path, r)
    m = host.Model(path, W, H, 1, batch=batch, colour="RGB8", **DEMO)
    ref = host.Model(path, W, H, 1, batch=batch, input_format="R8", output_format="R8", **DEMO)
    desc = m.describe()
    assert "rgb_luma_u8" in desc and "ycc_merge_u8 r=%d" % r in desc, desc
    steps = [d for _, _, d, _, _ in m.plan_steps()]  # the ESPCN steps are still the two fused 8-bit launches
    assert len(steps) == 2 and "conv_kxk_c1o16_wino3x3_c16o16_u8_kernel" in steps[0] and "d2s_tanh_u8_kernel" in steps[1], steps
    _check(m, ref, _frame(batch, 3, 10 * r + batch), batch, r)
    # a grey frame: the R8 model's output in every channel, byte for byte
    g = _frame(batch, 1, 5)
    got = _run(m, np.repeat(g, 3, axis=-1), batch, r, 3)
    yhi = _run(ref, g, batch, r, 1)
    np.testing.assert_array_equal(got, np.repeat(yhi, 3, axis=-1))
    m.close()
    ref.close()


def test_rgba8_carries_alpha_and_bt709(ctx, tmp_path):
    from shadernn_amd import host

    r, batch = 3, 2
    path = _json(tmp_path, r)
    kw = dict(kr=R.BT709[0], kb=R.BT709[1])
    m = host.Model(path, W, H, 1, batch=batch, colour="RGBA8", **kw, **DEMO)
    ref = host.Model(path, W, H, 1, batch=batch, input_format="R8", output_format="R8", **DEMO)
    rgba = _frame(batch, 4, 3, R.BT709)
    got, _ = _check(m, ref, rgba, batch, r, kw)
    np.testing.assert_array_equal(got[..., 3], np.repeat(np.repeat(rgba[..., 3], r, axis=1), r, axis=2))
    m.close()
    ref.close()


def test_a_captured_graph_reads_each_new_frame(ctx, tmp_path, monkeypatch):
    from shadernn_amd import host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even the four-launch inference
    r = 2
    path = _json(tmp_path, r)
    m = host.Model(path, W, H, 1, capture_graph=True, colour="RGB8", **DEMO)
    ref = host.Model(path, W, H, 1, input_format="R8", output_format="R8", **DEMO)
    outs = []
    for seed in (1, 2, 3):  # the first run records, the others replay: every frame must give its own result
        got, _ = _check(m, ref, _frame(1, 3, seed), 1, r)
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    m.close()
    ref.close()


def test_prefer_half(ctx, tmp_path):
    from shadernn_amd import host

    r = 2
    path = _json(tmp_path, r)
    m = host.Model(path, W, H, 1, prefer_half=True, colour="RGB8", **DEMO)
    ref = host.Model(path, W, H, 1, prefer_half=True, input_format="R8", output_format="R8", **DEMO)
    _check(m, ref, _frame(1, 3, 8), 1, r)
    m.close()
    ref.close()


def test_what_is_refused(ctx, tmp_path):
    from shadernn_amd import host, models

    path = _json(tmp_path, 2)
    h = C.c_void_p()
    one = (C.c_float * 4)(1, 1, 1, 1)
    zero = (C.c_float * 4)(0, 0, 0, 0)
    io5 = host.FrameIO(host.FRAME_FORMATS["RGB8"], host.FRAME_FORMATS["RGB8"], zero, one, one, zero)
    assert host.lib().snn_model_create5(path.encode(), 0, W, H, 1, 0, 1, 0, 0, 0, 1, C.byref(io5), C.byref(h)) == -1  # RGB8 on a one-channel model: as before

    def create7(p, in_c, fmt="RGB8", kr=0.299, kb=0.114):
        io = host.ColourIO(host.FRAME_FORMATS[fmt], kr, kb, 127.5, 1 / 127.5, 127.5, 127.5)
        return host.lib().snn_model_create7(p.encode(), 0, W, H, in_c, 0, 1, 0, 0, 0, 1, C.byref(io), C.byref(h))

    three = models.write_json(models.single_conv(seed=1, ic=3, oc=3), W, H, str(tmp_path / "three.json"))
    assert create7(three, 3) == -1                                  # a three-channel model
    wide = models.write_json(models.single_conv(seed=1, ic=1, oc=16), W, H, str(tmp_path / "wide.json"))
    assert create7(wide, 1) == -1                                   # one channel in, sixteen out
    assert create7(path, 1, fmt="R8") == -1                         # not a colour format
    assert create7(path, 1, kr=0.7, kb=0.4) == -1                   # kr + kb >= 1
    assert create7(path, 1) == 0                                    # the process and the device are fine
    assert host.lib().snn_model_destroy(h) == 0
