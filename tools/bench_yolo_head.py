#!/usr/bin/env python3
"""Times the YOLO head on the device (snnhip_yolo_head_plan_create, one launch) on YOLOv3-tiny-shaped heads (416: 13 x 13 and 26 x 26 cells, 18 channels)
and, beside it, what the CPU stage does per image with the same heads: download both, then snn_yolo_decode.  Device times are event pairs around
`reps` back-to-back launches, the configurations alternated over `rounds` rounds in one process; the spread is over the rounds.

    python tools/bench_yolo_head.py [--reps 200] [--rounds 5] [--json profiles/yolo_head.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import shadernn_amd as snn
    from shadernn_amd import capi, host
    import yolo_ref as R

    ctx = snn.Context(0)
    p = R.params(416)
    rng = np.random.default_rng(3)
    natural = lambda n: [rng.normal(-2.0, 2.5, (n, g, g, 18)).astype(np.float32) for g in (13, 26)]  # the heads tests/test_host.py decodes: ~10 % pass
    ladder = lambda count, mode: [h[None] for h in R.make_image(p, count, mode, 5)]
    configs = [("natural_n1", natural(1), 100), ("natural_n8", natural(8), 100), ("natural_n8_fp16", natural(8), 100), ("kept_0", ladder(0, "small"), 100),
               ("kept_10", ladder(10, "small"), 100), ("kept_100", ladder(100, "small"), 100), ("kept_100_of_2535", ladder("all", "small"), 100),
               ("worst_all_pass_none_overlap", ladder("all", "small"), 2535)]
    runs = []
    for name, heads, max_boxes in configs:
        n = heads[0].shape[0]
        plan = capi.yolo_head_plan(ctx, n, max_boxes=max_boxes)
        ts = [capi.Tensor.from_numpy(ctx, h, dtype=capi.F16 if name.endswith("fp16") else capi.F32) for h in heads]
        outs = [capi.Tensor(ctx, n, max_boxes, 1, 6), capi.Tensor(ctx, n, 1, 1, 2)]
        for _ in range(10):
            plan.run_io(ts, outs)
        ctx.sync()
        runs.append((name, plan, ts, outs, heads))
    timer = capi.Timer(ctx)
    us = {name: [] for name, *_ in runs}
    cpu = []
    for _ in range(a.rounds):
        for name, plan, ts, outs, _ in runs:
            timer.start()
            for _ in range(a.reps):
                plan.run_io(ts, outs)
            timer.stop()
            us[name].append(1e3 * timer.elapsed_ms() / a.reps)
        t0 = time.perf_counter()  # the CPU stage's work on one image: both heads to the host, decode + NMS there
        for _ in range(20):
            h0, h1 = runs[0][2][0].numpy(), runs[0][2][1].numpy()
            host.yolo_decode(h0[0], h1[0], 416, max_rows=4096)
        cpu.append(1e6 * (time.perf_counter() - t0) / 20)
    out = {"device": ctx.info()["name"] if hasattr(ctx, "info") else "", "reps": a.reps, "rounds": a.rounds, "launch_us": {}, "unit": "microseconds per launch, median [min, max] over the rounds"}
    for name, plan, ts, outs, _ in runs:
        counts = outs[1].numpy().reshape(-1, 2)
        out["launch_us"][name] = {"median": float(np.median(us[name])), "min": float(min(us[name])), "max": float(max(us[name])), "images": int(counts.shape[0]),
                                  "rows_per_image": float(counts[:, 0].mean()), "passed_per_image": float(counts[:, 1].mean()), "plan": plan.describe()}
    out["cpu_stage_per_image_us"] = {"median": float(np.median(cpu)), "min": float(min(cpu)), "max": float(max(cpu)),
                                     "what": "download of both fp32 heads (two synchronising copies) + snn_yolo_decode on natural_n1's heads, host clock"}
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
