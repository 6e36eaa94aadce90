"""Frame metrics through the C++ host mirror (snn_model_reference_frame / _reference_frame_planes / _frame_metrics; host.Model.set_reference /
metrics) on ESPCN x2 over a 32 x 24 frame: packed R8 / RGB8 / RGBA8 output frames, NV12, P010, I420 and NV12 at a fitted out_size, each run directly
and from its recorded graph.  The reference handed in is a perturbed copy of the model's own downloaded output; what metrics() returns is held
against tests/metrics_ref.py on the downloaded planes: sse exactly, ssim to 1e-9 (the bound of tests/test_frame_metrics_gpu.py), psnr_db as the
formula gives it from that sse, the rows in the stated order and number."""
import numpy as np
import pytest

import metrics_ref as R

pytestmark = pytest.mark.gpu
H, W = 24, 32

# name -> (host.Model keywords, (maxval, shift) of the output, what output_frame returns)
MODELS = {
    "R8": (dict(input_format="R8", output_format="R8", in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4), (255, 0), "frame"),
    "RGB8": (dict(colour="RGB8", in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4), (255, 0), "frame"),
    "RGBA8": (dict(colour="RGBA8", in_norms=(1 / 255.0,) * 4, out_scale=(255.0,) * 4), (255, 0), "frame"),
    "NV12": (dict(video="NV12", in_means=(16.0,) * 4, in_norms=(1 / 219.0,) * 4, out_scale=(219.0,) * 4, out_offset=(16.0,) * 4), (255, 0), "nv"),
    "P010": (dict(video="P010", in_means=(64.0,) * 4, in_norms=(1 / 876.0,) * 4, out_scale=(876.0,) * 4, out_offset=(64.0,) * 4), (1023, 6), "nv"),
    "I420": (dict(video="I420"), (255, 0), "planar"),
    "NV12-fitted": (dict(video="NV12", out_size=(48, 36), in_means=(16.0,) * 4, in_norms=(1 / 219.0,) * 4, out_scale=(219.0,) * 4, out_offset=(16.0,) * 4), (255, 0), "nv"),
}


def _json(tmp_path, r=2):
    from shadernn_amd import models

    net = models.espcn_weights(seed=1, scale=r)
    return models.write_json(net, W, H, str(tmp_path / (net["name"] + ".json")))


def _input(name, batch, seed):
    kw, (maxval, shift), kind = MODELS[name]
    rng = np.random.default_rng(seed)
    dt = np.uint16 if maxval > 255 else np.uint8
    lead = (batch,) if batch > 1 else ()
    if kind == "frame":
        c = {"R8": 1, "RGB8": 3, "RGBA8": 4}[name]
        return rng.integers(0, 256, lead + (H, W, c)).astype(np.uint8)
    y = (rng.integers(maxval // 16, maxval - maxval // 12, lead + (H, W)) << shift).astype(dt)
    if kind == "nv":
        return y, (rng.integers(maxval // 16, maxval - maxval // 16, lead + (H // 2, W // 2, 2)) << shift).astype(dt)
    return y, (rng.integers(16, 240, lead + (H // 2, W // 2))).astype(dt), (rng.integers(16, 240, lead + (H // 2, W // 2))).astype(dt)


def _perturb(a, maxval, shift, seed):
    """a copy of a downloaded plane some grey levels away, in the same container"""
    rng = np.random.default_rng(seed)
    v = (a.astype(np.int64) >> shift) + rng.integers(-6, 7, a.shape) * (maxval + 1) // 256
    return (np.clip(v, 0, maxval) << shift).astype(a.dtype)


def _parts(out):
    return list(out) if isinstance(out, tuple) else [out]


def _expected(name, batch, out, ref):
    """the rows metrics() must return, from the downloaded output `out` and the reference `ref` (both as output_frame returns them)"""
    _, (maxval, shift), kind = MODELS[name]
    rows = []

    def plane_rows(a, b, plane):  # a, b: [H][W][C] of one image
        for c, m in enumerate(R.frame_metrics(a[None], b[None], maxval, shift)):
            rows.append(dict(m, plane=plane, channel=c))

    outs = [p.reshape((batch,) + p.shape[(1 if batch > 1 else 0):]) for p in _parts(out)]
    refs = [p.reshape(o.shape) for p, o in zip(_parts(ref), outs)]
    for n in range(batch):
        first = len(rows)
        if kind == "frame":
            plane_rows(outs[0][n], refs[0][n], 0)
        elif kind == "nv":
            plane_rows(outs[0][n][..., None], refs[0][n][..., None], 0)
            plane_rows(outs[1][n], refs[1][n], 1)
        else:
            for p in range(3):
                plane_rows(outs[p][n][..., None], refs[p][n][..., None], p)
        for r in rows[first:]:
            r["image"] = n
    return rows


def _check(got, want, label):
    assert len(got) == len(want), (label, len(got), len(want))
    for g, w in zip(got, want):
        print("%s image %d plane %d channel %d: sse %d (ref %d) psnr %.4f ssim %.12f (ref %.12f)" %
              (label, g["image"], g["plane"], g["channel"], g["sse"], w["sse"], g["psnr_db"], g["ssim"], w["ssim"]))
        assert (g["image"], g["plane"], g["channel"]) == (w["image"], w["plane"], w["channel"]), (label, g, w)
        assert g["sse"] == w["sse"] and g["pixels"] == w["pixels"], (label, g, w)
        assert abs(g["ssim"] - w["ssim"]) <= 1e-9, (label, g, w)
        assert g["psnr_db"] == w["psnr_db"] or abs(g["psnr_db"] - w["psnr_db"]) <= 1e-12 * abs(w["psnr_db"]), (label, g, w)


def _trace(fn):
    from shadernn_amd import capi

    capi.trace_begin()
    fn()
    t = capi.trace_end()
    return t["launches"], sorted(k["function"] for k in t["kernels"])


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_metrics_match_the_reference_on_the_downloaded_planes(ctx, tmp_path, monkeypatch, name, batch):
    from shadernn_amd import host

    monkeypatch.setenv("SNN_GRAPH_MIN_LAUNCHES", "1")
    kw, (maxval, shift), kind = MODELS[name]
    path = _json(tmp_path)
    x = _input(name, batch, seed=len(name) + batch)
    rows_by_capture = []
    for capture in (False, True):
        m = host.Model(path, W, H, 1, batch=batch, capture_graph=capture, **kw)
        m.upload_frame(x)
        if not capture:
            before = _trace(m.run)
        m.run()
        m.run()  # with capture_graph the second run replays the recording
        out = m.output_frame()
        ref = tuple(_perturb(p, maxval, shift, 7 + i) for i, p in enumerate(out)) if isinstance(out, tuple) else _perturb(out, maxval, shift, 7)
        m.set_reference(ref)
        got = m.metrics()
        _check(got, _expected(name, batch, out, ref), "%s batch=%d capture=%s" % (name, batch, capture))
        n_planes = {"frame": 1, "nv": 2, "planar": 3}[kind]
        channels = sum(p.shape[-1] if (kind == "frame" or (kind == "nv" and i == 1)) else 1 for i, p in enumerate(_parts(out)))
        assert len(got) == batch * channels and {r["plane"] for r in got} == set(range(n_planes))
        assert all(0 < r["sse"] and r["ssim"] < 1.0 and np.isfinite(r["psnr_db"]) for r in got)
        if not capture:
            # run() launches what it launched before a reference existed; the metrics launches appear under metrics() only
            assert _trace(m.run) == before, (before,)
            n, fns = _trace(m.metrics)
            assert n == (2 if kind == "frame" else 4), (n, fns)
            assert fns and all("frame_metrics_tile_kernel" in f or "frame_metrics_fold_kernel" in f for f in fns), fns
            assert not any("frame_metrics" in f for f in before[1]), before
        m.run()
        assert m.metrics() == got  # the same output against the same reference: bit for bit
        # the reference a second time: the output itself
        m.set_reference(out)
        same = m.metrics()
        assert len(same) == len(got) and all(r["sse"] == 0 and r["psnr_db"] == float("inf") and r["ssim"] == 1.0 for r in same), same
        rows_by_capture.append(got)
        m.close()
    assert rows_by_capture[0] == rows_by_capture[1]  # a replayed graph produces the frame the launches produce


@pytest.mark.parametrize("name", ["NV12", "P010", "I420"])
def test_pitched_reference_planes(ctx, tmp_path, name):
    from shadernn_amd import host

    kw, (maxval, shift), kind = MODELS[name]
    batch = 2
    m = host.Model(_json(tmp_path), W, H, 1, batch=batch, **kw)
    m.upload_frame(_input(name, batch, seed=3))
    m.run()
    out = m.output_frame()
    ref = tuple(_perturb(p, maxval, shift, 20 + i) for i, p in enumerate(out))
    m.set_reference(ref)
    dense = m.metrics()
    _check(dense, _expected(name, batch, out, ref), name + " dense")
    views = []
    for n in range(batch):
        for i, p in enumerate(ref):
            rows = p[n].reshape(p.shape[1], -1)  # an interleaved CbCr plane as rows of W elements
            wide = np.full((rows.shape[0], rows.shape[1] + 5 + 2 * i), 0xA5, rows.dtype)  # padding that must never be read as samples
            wide[:, :rows.shape[1]] = rows
            views.append(wide[:, :rows.shape[1]])
    m.set_reference([np.zeros_like(v) for v in views])  # something else in between, through the same call
    assert m.metrics() != dense
    m.set_reference(views)
    assert m.metrics() == dense
    m.close()


def test_refusals(ctx, tmp_path):
    from shadernn_amd import host

    path = _json(tmp_path)
    m = host.Model(path, W, H, 1)  # float tensors in and out
    m.upload(np.random.default_rng(1).random((H, W, 1), dtype=np.float32))
    m.run()
    with pytest.raises(AssertionError, match="snn_model_reference_frame refused"):
        m.set_reference(np.zeros((2 * H, 2 * W, 1), np.uint8))
    with pytest.raises(AssertionError, match="snn_model_frame_metrics refused"):
        m.metrics()
    ptrs = (host.C.c_void_p * 3)()
    assert host.lib().snn_model_reference_frame_planes(m.h, ptrs, (host.C.c_int * 3)(8, 4, 4), 3) == -1
    m.close()
    kw = MODELS["R8"][0]
    m = host.Model(path, W, H, 1, **kw)
    m.upload_frame(np.zeros((H, W, 1), np.uint8))
    m.run()
    with pytest.raises(AssertionError, match="snn_model_frame_metrics refused"):  # no reference set
        m.metrics()
    with pytest.raises(AssertionError, match="extent"):
        m.set_reference(np.zeros((H, W, 1), np.uint8))  # the input's extent, not the output's
    assert host.lib().snn_model_reference_frame_planes(m.h, ptrs, (host.C.c_int * 3)(8, 4, 4), 3) == -1  # a packed output has no planes
    with pytest.raises(AssertionError, match="snn_model_frame_metrics refused"):  # still none
        m.metrics()
    m.set_reference(m.output_frame())
    assert [r["sse"] for r in m.metrics()] == [0]
    m.close()
