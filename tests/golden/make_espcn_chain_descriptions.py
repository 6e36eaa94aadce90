#!/usr/bin/env python
"""Writes tests/golden/espcn_chain_descriptions.json: plan.describe() and the per-step descriptions of the ESPCN chain plan, with and without 8- /
16-bit frame ends, for every kernel family the chain planner can select.  The descriptions name the kernel each step launches (tests and launch traces
read them), so the fixture pins which kernel a frame end folds into, its spelling, and where a conversion stays a step of its own.  It was generated
on an MI355X at the commit before FrameIn / FrameOut replaced the per-family frame-end plumbing (tests/test_espcn_frame_ends_gpu.py compares).
Plan creation only: nothing is launched.   python tests/golden/make_espcn_chain_descriptions.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, H, W = 2, 19, 71  # more than one tile across, a ragged edge, two images (one of tests/test_frame_u16_gpu.py's shapes)
SWITCHES = ("SNNHIP_ESPCN_A", "SNNHIP_ESPCN_B", "SNNHIP_ESPCN_F16", "SNNHIP_ESPCN_FUSION")
# family -> (environment, fp16 tensors, widths)
FAMILIES = {
    "fp32": ({}, False, (16, 16)),
    "a_direct": ({"SNNHIP_ESPCN_A": "direct"}, False, (16, 16)),
    "b_wino": ({"SNNHIP_ESPCN_B": "wino"}, False, (16, 16)),
    "f16": ({"SNNHIP_ESPCN_F16": "1"}, True, (16, 16)),
    "f16_wide": ({"SNNHIP_ESPCN_F16": "1"}, True, (64, 32)),
    "stream": ({"SNNHIP_ESPCN_FUSION": "stream"}, False, (16, 16)),
}
STREAM_LINE = "<stream kernel>"  # rule C's own line carries the compute-unit count: only its place is recorded


def _net(r, k1, widths):
    from shadernn_amd import models

    net = models.espcn_weights(seed=3, scale=r, widths=widths)
    if k1 != 5:
        first = net["layers"][0]
        first["w"] = first["w"][:, :, :k1, :k1].copy()
        first["kernel"] = k1
    return net


def _plans(ctx, net, bits, ends, dtype):
    from shadernn_amd import capi
    from shadernn_amd.runner import _layer_plan

    plans, shape = [], (N, H, W, 1)
    if ends in ("in", "both"):
        if bits == 8:
            plans.append(capi.u8_in_plan(ctx, N, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1), dtype=dtype))
        else:
            plans.append(capi.u16_in_plan(ctx, N, H, W, 1, (511.5, 0, 0, 0), (1 / 511.5, 1, 1, 1), shift=6, dtype=dtype))
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape, dtype)
        plans.append(p)
        shape = p.out_shape()
    if ends in ("out", "both"):
        if bits == 8:
            plans.append(capi.u8_out_plan(ctx, *shape, (127.5, 0, 0, 0), (127.5, 0, 0, 0), dtype=dtype))
        else:
            plans.append(capi.u16_out_plan(ctx, *shape, (511.5, 0, 0, 0), (511.5, 0, 0, 0), maxval=1023, shift=6, dtype=dtype))
    return plans


def chain_descriptions(ctx):
    """{"family/r/k1/ends/bits": {"describe": ..., "steps": [...]}}; the planner's switches are set per family and put back."""
    from shadernn_amd import capi

    saved = {k: os.environ.get(k) for k in SWITCHES}
    out = {}
    try:
        for family, (env, half, widths) in FAMILIES.items():
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(env)
            dtype = capi.F16 if half else capi.F32
            for r in (2, 3, 4):
                for k1 in (3, 5):
                    net = _net(r, k1, widths)
                    for ends in ("none", "in", "out", "both"):
                        for bits in (8, 16):
                            chain = capi.chain_plan(ctx, _plans(ctx, net, bits, ends, dtype))
                            steps = [chain.step_describe(i) for i in range(chain.num_steps())]
                            rec = {"describe": chain.describe(), "steps": steps}
                            if family == "stream":  # the step count and the other steps' descriptions only
                                rec = {"steps": [STREAM_LINE if "] stream " in s else s for s in steps]}
                            out["%s/r%d/k%d/%s/%d" % (family, r, k1, ends, bits)] = rec
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


if __name__ == "__main__":
    import shadernn_amd as snn

    snn.load_library()
    ctx = snn.Context(0)
    path = os.environ.get("ESPCN_CHAIN_DESCRIPTIONS_OUT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "espcn_chain_descriptions.json")
    with open(path, "w") as f:
        json.dump(chain_descriptions(ctx), f, indent=0, sort_keys=True)
        f.write("\n")
    print("written", path)
