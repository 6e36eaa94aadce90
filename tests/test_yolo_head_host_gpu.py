"""The YOLO head inside host.Model: the device head at batch 2 against the C-ABI plan on the downloaded heads, the batch-1 default on the CPU stage,
SNNHIP_YOLO_HEAD=device at batch 1 against the CPU stage's list; direct and recorded."""
import numpy as np
import pytest


pytestmark = pytest.mark.gpu


def _yolo_net(seed=12):
    """416 x 416 x 3 -> strided convs -> a 26 x 26 and a 13 x 13 head of 3 x 6 channels -> the YOLO layer (tests/test_host.py's model, rebuilt here)"""
    from shadernn_amd import models

    rng = np.random.default_rng(seed)
    L, c = [], 3
    for i, oc in enumerate([8, 8, 16, 16]):
        L.append(dict(models._conv(rng, "c%d" % i, c, oc, 3, "leakyRelu", stride=2), alpha=0.1))
        c = oc
    fine = models._conv(rng, "fine", c, 18, 1, "linear")
    coarse_f = dict(models._conv(rng, "c4", c, 32, 3, "leakyRelu", stride=2), inputs=["c3"], alpha=0.1)
    coarse = models._conv(rng, "coarse", 32, 18, 1, "linear")
    for hd in (fine, coarse):
        hd["w"] *= 20.0 / 6.0
        hd["b"] = rng.uniform(-1.0, 1.0, 18).astype(np.float32)
    return {"name": "yolo_mini", "input_channels": 3, "layers": L + [fine, coarse_f, coarse, models._op("YOLO", "yolo", 18, inputs=["coarse", "fine"])]}


def _json(tmp_path, net, w, h):
    from shadernn_amd import models

    return models.write_json(net, w, h, str(tmp_path / (net["name"] + ".json")))


def _run(tmp_path, x, **kw):
    from shadernn_amd import host

    m = host.Model(_json(tmp_path, _yolo_net(), 416, 416), 416, 416, 3, batch=len(x), **kw)
    m.set_type("detection")
    m.upload(x if len(x) > 1 else x[0:1])
    m.run()
    m.run()  # (capture_graph: the second run replays the recording)
    return m


@pytest.mark.parametrize("capture_graph", [False, True], ids=["direct", "recorded"])
def test_batch_2_detections_are_the_plans_on_each_images_heads(ctx, tmp_path, monkeypatch, capture_graph):
    from shadernn_amd import capi, host

    monkeypatch.delenv("SNNHIP_YOLO_HEAD", raising=False)
    x = np.random.default_rng(8).random((2, 416, 416, 3), dtype=np.float32)
    x[1] = x[1, ::-1] * 0.7  # two different images
    m = _run(tmp_path, x, capture_graph=capture_graph)
    steps = m.plan_steps()
    assert "yolo_head" in steps[-1][2] and steps[-1][0] == len(m.stages()) - 1, steps[-1]  # the last stage is a GPU stage with one launch
    path = _json(tmp_path, _yolo_net(), 416, 416)
    heads = [m.stage_output(i) for i in host.graph_summary(path, 416, 416, 3)[-1]["inputs"]]  # the YOLO stage's producers: coarse, fine
    plan = capi.yolo_head_plan(ctx, 2)
    outs = [capi.Tensor(ctx, 2, 100, 1, 6), capi.Tensor(ctx, 2, 1, 1, 2)]
    plan.run_io([capi.Tensor.from_numpy(ctx, h) for h in heads], outs)
    ctx.sync()
    rows, counts = outs[0].numpy().reshape(2, 100, 6), outs[1].numpy().reshape(2, 2)
    got = [m.detections(image=i) for i in range(2)]
    for i in range(2):
        assert len(got[i]) == counts[i, 0] > 10 and got[i].tobytes() == rows[i, :len(got[i])].tobytes()
    assert got[0].tobytes() != got[1].tobytes()
    if not capture_graph:  # the launches of run(): the body's and one more
        capi.trace_begin()
        m.run()
        assert capi.trace_end()["launches"] == len(steps) == len([s for s in steps if "yolo_head" not in s[2]]) + 1
    m.close()


def test_batch_1_keeps_the_cpu_stage_and_the_switch_gives_its_first_100_rows(ctx, tmp_path, monkeypatch):
    monkeypatch.delenv("SNNHIP_YOLO_HEAD", raising=False)
    x = np.random.default_rng(8).random((1, 416, 416, 3), dtype=np.float32)
    cpu = _run(tmp_path, x)
    assert not any("yolo_head" in s[2] for s in cpu.plan_steps())  # the CPU stage launches nothing
    want = cpu.detections(max_rows=8192)
    cpu.close()
    monkeypatch.setenv("SNNHIP_YOLO_HEAD", "device")
    dev = _run(tmp_path, x)
    assert "yolo_head" in dev.plan_steps()[-1][2]
    got = dev.detections(max_rows=8192)
    dev.close()
    # the same device-computed heads feed both: no decision should flip, but the CPU's expf may differ in its last bits, so values get a tolerance
    assert len(want) > 100 and len(got) == 100 and np.array_equal(got[:, 0], want[:100, 0])
    np.testing.assert_allclose(got, want[:100], rtol=1e-5, atol=1e-6)


def test_the_yolo_op_runs_through_the_graph_runner(ctx):
    import shadernn_amd as snn
    from shadernn_amd import capi

    x = np.random.default_rng(8).random((2, 416, 416, 3), dtype=np.float32)
    x[1] = x[1, ::-1] * 0.7
    r = snn.GraphRunner(ctx, _yolo_net(), 2, 416, 416)
    r(x)
    plan = capi.yolo_head_plan(ctx, 2)
    outs = [capi.Tensor(ctx, 2, 100, 1, 6), capi.Tensor(ctx, 2, 1, 1, 2)]
    plan.run_io([capi.Tensor.from_numpy(ctx, r.output_of(n)) for n in ("coarse", "fine")], outs)
    ctx.sync()
    for i in range(2):
        got = r.detections(image=i)
        assert len(got) == outs[1].numpy()[i, 0, 0, 0] > 10 and got.tobytes() == outs[0].numpy()[i, :len(got), 0].tobytes()
