"""Every frame path of the C++ host mirror once, through host.Model: ESPCN x2 on the 32 x 24 luma frame of the other host tests, batch 2, launched
directly and as a recorded graph.  One description (shadernn_amd/host/snn/frames.h) drives all thirteen, so each is held to the same three things:
the extra launches describe() lists, in order; the launch trace counts the model's plan steps plus exactly those; and upload -> run -> download
returns the shapes and dtypes host.Model's docstring states.  What the bytes must be is the per-path files' business (tests/test_frame_*_host_gpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
H, W, R, N = 24, 32, 2, 2
OH, OW = R * H, R * W
U8, U16 = np.uint8, np.uint16


def _yuv(dt, planar=False, h=OH, w=OW):
    chroma = [((N, h // 2, w // 2), dt)] * 2 if planar else [((N, h // 2, w // 2, 2), dt)]
    return [((N, h, w), dt)] + chroma


# id: (host.Model keywords, what upload_frame takes (None: upload() of floats), what comes back as [(shape, dtype)], the labels of describe())
PATHS = {
    "float": (dict(), None, [((N, OH, OW, 1), np.float32)], []),
    "R8": (dict(input_format="R8", output_format="R8", in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4), [((N, H, W, 1), U8)], [((N, OH, OW, 1), U8)], []),
    "R16": (dict(input_format="R16", output_format="R16", in_norms=(1 / 1023.0,) * 4, out_scale=(1023.0,) * 4, frame_out_maxval=1023), [((N, H, W, 1), U16)],
            [((N, OH, OW, 1), U16)], []),
    "RGB8": (dict(colour="RGB8", in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4), [((N, H, W, 3), U8)], [((N, OH, OW, 3), U8)], ["[colour in]", "[colour out]"]),
    "NV12": (dict(video="NV12", in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4), _yuv(U8, h=H, w=W), _yuv(U8), ["[chroma out]"]),
    "P010": (dict(video="P010", in_norms=(1 / 1023.0,) * 4, out_scale=(1023.0,) * 4), _yuv(U16, h=H, w=W), _yuv(U16), ["[chroma out]"]),
    "I420": (dict(video="I420"), _yuv(U8, True, H, W), _yuv(U8, True), ["[chroma out]"]),
    "I010": (dict(video="I010"), _yuv(U16, True, H, W), _yuv(U16, True), ["[chroma out]"]),
    "NV12-RGB8": (dict(video="NV12", video_out="RGB8"), _yuv(U8, h=H, w=W), [((N, OH, OW, 3), U8)], ["[rgb out]"]),
    "I420-RGBA8": (dict(video="I420", video_out="RGBA8"), _yuv(U8, True, H, W), [((N, OH, OW, 4), U8)], ["[rgb out]"]),
    "RGB8-NV12": (dict(colour="RGB8", video_out="NV12"), [((N, H, W, 3), U8)], _yuv(U8), ["[colour in]", "[chroma out]"]),
    "RGB8-I420": (dict(colour="RGB8", video_out="I420"), [((N, H, W, 3), U8)], _yuv(U8, True), ["[colour in]", "[chroma out]"]),
    "NV12-48x36": (dict(video="NV12", out_size=(48, 36), in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4), _yuv(U8, h=H, w=W), _yuv(U8, h=36, w=48),
                   ["[luma fit]", "[chroma fit]"]),
}


@pytest.fixture(scope="module")
def espcn_x2(tmp_path_factory):
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=R)
    return models.write_json(net, W, H, str(tmp_path_factory.mktemp("frame_paths") / (net["name"] + ".json")))


def _arrays(spec, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(16, 236, size=shape).astype(dt) for shape, dt in spec]


def _labels(desc):
    return [line[:line.index("]") + 1] for line in desc.split("\n") if line.startswith("[") and not line[1:2].isdigit()]


def _round_trip(m, takes, frames):
    if takes is None:
        m.upload(frames[0])
        m.run()
        return [m.output()]
    m.upload_frame(frames[0] if len(frames) == 1 else tuple(frames))
    m.run()
    out = m.download_frame()
    return list(out) if isinstance(out, tuple) else [out]


@pytest.mark.parametrize("capture", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("path", list(PATHS))
def test_every_frame_path(ctx, espcn_x2, monkeypatch, path, capture):
    from shadernn_amd import capi, host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")  # record / replay even a two-launch inference
    kw, takes, gives, labels = PATHS[path]
    m = host.Model(espcn_x2, W, H, 1, batch=N, capture_graph=capture, **kw)
    desc = m.describe()
    assert _labels(desc) == labels, desc
    frames = [np.random.default_rng(5).random((N, H, W, 1), dtype=np.float32)] if takes is None else _arrays(takes, 5)
    got = _round_trip(m, takes, frames)  # (with capture: records, then launches the recording)
    assert [(a.shape, a.dtype) for a in got] == [(shape, np.dtype(dt)) for shape, dt in gives], path
    again = _round_trip(m, takes, frames)  # (with capture: a replay)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)
    m.suspend_replay(True)  # a replayed graph never calls the plans: the trace wants them launched one by one
    capi.trace_begin()
    m.run()
    trace = capi.trace_end()
    assert trace["launches"] == len(m.plan_steps()) + len(labels), (trace["launches"], m.plan_steps(), labels)
    m.close()
