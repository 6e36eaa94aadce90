#!/usr/bin/env python3
"""Times the four up-convolutions of the zoo U-Net (nearest UpSampling2D x2 -> Conv2D 2x2 "same", batch 8, fp32 and fp16) as the chain planner builds them:
conv2d_upconv2 (SNNHIP_CONV=upconv2: nine pre-summed GEMMs on the low-resolution tensor) against the direct kernel with the upsampling resolved in its
staging (SNNHIP_UPCONV2=0), both plans in one process.  Device times are event pairs around `reps` back-to-back launches; per round the two plans run in
mirrored order (new, old, old, new), the figure is the median over the rounds with [min, max].  A (precision, shape class) is routed to the new kernel by
default only where it won by more than the run's own spread: new max < old min.

    python tools/bench_upconv2.py [--reps 50] [--rounds 7] [--batch 8] [--json profiles/upconv2_layers.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS = [(1024, 512, 16), (512, 256, 32), (256, 128, 64), (128, 64, 128)]  # IC, OC, low-resolution extent (the output is twice that)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import shadernn_amd as snn
    from shadernn_amd import capi

    ctx = snn.Context(0)
    timer = capi.Timer(ctx)
    rows = []
    for f16 in (False, True):
        dt = capi.F16 if f16 else capi.F32
        for ic, oc, s in LAYERS:
            rng = np.random.default_rng(ic)
            x = rng.standard_normal((a.batch, s, s, ic)).astype(np.float32)
            w = (rng.standard_normal((oc, ic, 2, 2)) / np.sqrt(4 * ic)).astype(np.float32)
            b = rng.standard_normal(oc).astype(np.float32) * 0.1
            plans = {}
            for name, env in (("upconv2", {"SNNHIP_CONV": "upconv2"}), ("direct", {"SNNHIP_UPCONV2": "0"})):
                per_layer = [capi.upsample_plan(ctx, a.batch, s, s, ic, 2.0, "nearest"), capi.conv2d_plan(ctx, a.batch, 2 * s, 2 * s, w, b, stride=1, act="relu", dtype=dt)]
                for k, v in env.items():
                    capi.set_option(k, v)
                plans[name] = capi.chain_plan(ctx, per_layer)
                for k in env:
                    capi.set_option(k, None)
            assert "upconv2" in plans["upconv2"].describe() and "upconv2" not in plans["direct"].describe(), [p.describe() for p in plans.values()]
            xt = capi.Tensor.from_numpy(ctx, x, dtype=dt)
            ys = {k: capi.Tensor(ctx, a.batch, 2 * s, 2 * s, oc, dtype=dt) for k in plans}
            for k, p in plans.items():  # warm-up
                for _ in range(5):
                    p.run(xt, ys[k])
            ctx.sync()
            diff = float(np.abs(ys["upconv2"].numpy().astype(np.float64) - ys["direct"].numpy()).max())
            us = {k: [] for k in plans}
            for _ in range(a.rounds):
                pair = {k: [] for k in plans}
                for k in ("upconv2", "direct", "direct", "upconv2"):
                    timer.start()
                    for _ in range(a.reps):
                        plans[k].run(xt, ys[k])
                    timer.stop()
                    pair[k].append(1e3 * timer.elapsed_ms() / a.reps)
                for k in plans:
                    us[k].append(float(np.mean(pair[k])))
            st = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in us.items()}
            flops, issued = plans["upconv2"].cost()[0], 9.0 / 16.0 * plans["upconv2"].cost()[0]
            rows.append({"precision": "fp16" if f16 else "fp32", "layer": "%d->%d @%dx%d -> %dx%d b%d" % (ic, oc, s, s, 2 * s, 2 * s, a.batch),
                         "class": "deep (flushing, 32 channels a block)" if 4 * ic > 1152 else "shallow (64 channels a block)",
                         "upconv2_us": st["upconv2"], "direct_us": st["direct"], "speedup_median": st["direct"]["median"] / st["upconv2"]["median"],
                         "wins_beyond_spread": st["upconv2"]["max"] < st["direct"]["min"], "max_abs_difference": diff,
                         "nominal_tflops_upconv2": flops / st["upconv2"]["median"] * 1e-6, "issued_mfma_tflops_upconv2": issued / st["upconv2"]["median"] * 1e-6,
                         "plans": {k: p.describe() for k, p in plans.items()}})
            for t in [xt] + list(ys.values()):
                t.free()
            for p in plans.values():
                p.destroy()
    routing = {}
    for r in rows:
        key = r["precision"] + ", " + r["class"]
        routing[key] = routing.get(key, True) and r["wins_beyond_spread"]
    out = {"device": ctx.info()["name"] if hasattr(ctx, "info") else "", "reps": a.reps, "rounds": a.rounds, "unit": "microseconds per launch, median [min, max] over the rounds",
           "layers": rows, "default_routing_to_upconv2": routing}
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
