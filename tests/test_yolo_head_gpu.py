"""The YOLO head plan through the C-ABI into NaN-filled outputs against tests/yolo_ref.py's float64 list, on inputs whose decisions all have margins."""
import numpy as np
import pytest

import yolo_ref as R

pytestmark = pytest.mark.gpu


def run_case(ctx, name, record=False):
    # the rows [N][max_boxes][6] and counts [N][2] of a case, run directly or (record) replayed twice from a graph, the replays bit-identical
    from shadernn_amd import capi

    p, _, dtype, max_boxes = R.CASES[name]
    images = R.case_images(name)
    n, cands = len(images), sum(h.size for h in images[0]) // (5 + p["classes"])
    max_boxes = max_boxes or cands
    plan = capi.yolo_head_plan(ctx, n, net_size=p["net"], n_heads=p["n_heads"], classes=p["classes"], max_boxes=max_boxes)
    heads = [capi.Tensor.from_numpy(ctx, np.stack([im[h] for im in images]).astype(np.float32), dtype=capi.F16 if dtype == np.float16 else capi.F32) for h in range(p["n_heads"])]
    outs = [capi.Tensor(ctx, n, max_boxes, 1, 6), capi.Tensor(ctx, n, 1, 1, 2)]
    got = []
    if record:
        with capi.Graph.capture(ctx) as g:
            plan.run_io(heads, outs)
    for _ in range(2 if record else 1):
        for t in outs:
            t.fill(np.nan)
        g.launch() if record else plan.run_io(heads, outs)
        ctx.sync()
        got.append([t.numpy().copy() for t in outs])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], got[-1]))
    plan.destroy()
    return got[0][0].reshape(n, max_boxes, 6), got[0][1].reshape(n, 2), images, max_boxes


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_kept_list_is_the_references(ctx, name):
    rows, counts, images, max_boxes = run_case(ctx, name)
    for i, image in enumerate(images):
        want, passed, _, _ = R.decode(image, R.CASES[name][0])
        want = want[:max_boxes]  # max_boxes keeps a prefix
        k = len(want)
        print(name, i, "rows", counts[i], "want", k, passed, "max err", np.abs(rows[i, :k] - want).max(initial=0))
        assert counts[i].tolist() == [k, passed] and not rows[i, k:].any()  # every row past the count is zeros (no NaN left anywhere)
        assert np.array_equal(rows[i, :k, 0], want[:, 0])  # (equal scores: the reference's candidate order shows in x, y, cells apart)
        assert np.all(np.abs(rows[i, :k, 1:4] - want[:, 1:4]) <= R.EPS) and np.all(np.abs(rows[i, :k, 4:] - want[:, 4:]) <= R.EPS * want[:, 4:])


def test_a_recorded_graph_replays_bit_identically_and_equals_the_direct_run(ctx):
    direct, recorded = run_case(ctx, "net96_three_images"), run_case(ctx, "net96_three_images", record=True)
    assert direct[0].tobytes() == recorded[0].tobytes() and direct[1].tobytes() == recorded[1].tobytes()


def test_the_run_functions_refuse_the_wrong_plans(ctx):
    from shadernn_amd import capi

    plan = capi.yolo_head_plan(ctx, 1, net_size=32, max_boxes=4)
    heads = [capi.Tensor(ctx, 1, 1, 1, 18), capi.Tensor(ctx, 1, 2, 2, 18)]
    rows, counts = capi.Tensor(ctx, 1, 4, 1, 6), capi.Tensor(ctx, 1, 1, 1, 2)
    for call in (lambda: plan.run(heads[0], rows), lambda: plan.run(heads, rows)):
        with pytest.raises(capi.SnnHipError, match="yolo_head.*snnhip_plan_run_io"):
            call()
    conv = capi.conv2d_plan(ctx, 1, 4, 4, np.zeros((2, 2, 3, 3), np.float32), np.zeros(2, np.float32))
    with pytest.raises(capi.SnnHipError, match="plan_run_io: only"):
        conv.run_io([capi.Tensor(ctx, 1, 4, 4, 2)], [capi.Tensor(ctx, 1, 4, 4, 2), counts])
