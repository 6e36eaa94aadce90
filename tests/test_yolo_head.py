"""The YOLO head plan, CPU side: declared / exported / bound, the refusals, yolo_ref against the oracle, the margins and fp32 distance of the GPU inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import yolo_ref as R


def test_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(__file__), "..", "include", "snnhip.h"), encoding="utf-8").read(), flags=re.S)
    assert re.search(r"\bsnnhip_yolo_head_plan_create\s*\(", header) and "snnhip_yolo_head_desc" in header
    assert hasattr(C.CDLL(snn.load_library()), "snnhip_yolo_head_plan_create") and "snnhip_yolo_head_plan_create" in capi.SIGNATURES
    assert callable(snn.yolo_head_plan) and C.sizeof(capi.YoloHeadDesc) == 28 * 4


@pytest.mark.parametrize("change, needle", [
    ({}, "null"), ({"N": 0}, "N = 0"), ({"n_heads": 3}, "n_heads = 3"), ({"net_size": 100}, "net_size 100"), ({"net_size": 544}, "net_size 544"),
    ({"grid_scale": (32, 24)}, "not a multiple of grid_scale[1] = 24"), ({"grid_scale": (32, 0)}, "grid_scale[1] = 0"), ({"grid_scale": (8, 16)}, "more than 4096 candidates"),
    ({"anchors_per_cell": 4}, "anchors_per_cell = 4"), ({"classes": 0}, "classes = 0"), ({"masks": (3, 4, 6, 1, 2, 3)}, "masks[2] = 6"), ({"masks": (3, 4, 5, 1, -1, 3)}, "masks[4] = -1"),
    ({"max_boxes": 0}, "max_boxes = 0"), ({"max_boxes": 2536}, "max_boxes = 2536"), ({"conf": 0.0}, "conf_threshold = 0"), ({"conf": 1.0}, "conf_threshold = 1"),
    ({"iou": 0.0}, "iou_threshold = 0"), ({"iou": 1.5}, "iou_threshold = 1.5")])
def test_plan_creation_refuses_with_a_message(built, change, needle):
    from shadernn_amd import capi

    d = capi.yolo_head_desc(change.pop("N", 2), **change)
    ctx, out = C.create_string_buffer(64), C.c_void_p()  # never read: every check comes before the context is used
    args = (None, C.byref(d), C.byref(out)) if needle == "null" else (C.cast(ctx, C.c_void_p), C.byref(d), C.byref(out))
    assert capi.lib().snnhip_yolo_head_plan_create(*args) == capi.E_INVALID
    msg = capi.lib().snnhip_last_error().decode()
    assert msg.startswith("yolo_head") and needle in msg, msg


def test_the_reference_is_the_oracles_decode():
    rng = np.random.default_rng(3)
    heads = [rng.normal(-2.0, 2.5, (13, 13, 18)).astype(np.float32), rng.normal(-2.0, 2.5, (26, 26, 18)).astype(np.float32)]
    want = np.array(O.yolo_decode([h[None] for h in heads]), np.float64).reshape(-1, 6)
    got = R.decode(heads, R.params(416))[0]
    assert len(want) > 20 and abs(len(want) - len(got)) <= 0.01 * len(want)  # float32 there, float64 here: a box right at a threshold may flip
    d = np.abs(want[:, None, 2:6] - got[None, :, 2:6]).max(axis=2)
    j = d.argmin(axis=1)
    ok = (d[np.arange(len(want)), j] < 1e-5) & (np.abs(want[:, 1] - got[j, 1]) < 1e-5) & (want[:, 0] == got[j, 0])
    assert ok.mean() >= 0.99, ok.mean()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_gpu_input_has_its_margins_and_stays_within_D(name):
    p = R.CASES[name][0]
    for image in R.case_images(name):
        margins = R.decode(image, p)[2]
        assert min(margins) >= R.EPS, margins  # confidence, score order, IoU: no decision of this input is a near tie
        assert R.distance(image, p) <= R.D
    if p["classes"] > 1:  # a kept box lies on an earlier kept box of another class (IoU over the threshold): dropping the class test would lose it
        rows = R.decode(R.case_images(name)[0], p)[0]
        assert any(r[0] != q[0] and R._iou(q[2:], r[None, 2:], np.float64)[0] > p["iou"] for i, r in enumerate(rows) for q in rows[:i])
