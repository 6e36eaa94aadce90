#!/usr/bin/env python3
"""Times the four Conv2D -> MaxPooling2D 2x2 places of YOLOv3-tiny's backbone whose full-resolution tensor has no other reader (conv2d .. conv2d_3; batch
8, fp32 and fp16): chain rule L's one launch (SNNHIP_POOL_FUSE=1, the POOL instances of conv2d_mfma) against what runs without it -- the layer's own
convolution plan as the default routing builds it and the pooling launch -- in one process.  Device times are event pairs around `reps` back-to-back
runs; per round the two forms run in mirrored order (new, old, old, new), the figure is the median over the rounds with [min, max].  A (precision, layer)
wins only where it won by more than the run's own spread: new max < old min.  --models adds the tools/bench_models.py lines of the graph with the switch
on and off.

    python tools/bench_pool.py [--reps 50] [--rounds 7] [--batch 8] [--models] [--json profiles/pool_layers.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# layer, IC, OC, extent of the convolution (3x3 "same", BN + leakyRelu(0.1), MaxPooling2D 2x2 stride 2 "same" behind it)
LAYERS = [("conv2d", 3, 16, 416), ("conv2d_1", 16, 32, 208), ("conv2d_2", 32, 64, 104), ("conv2d_3", 64, 128, 52)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import shadernn_amd as snn
    from shadernn_amd import capi

    ctx = snn.Context(0)
    timer = capi.Timer(ctx)
    rows = []
    for f16 in (False, True):
        dt = capi.F16 if f16 else capi.F32
        for name, ic, oc, s in LAYERS:
            rng = np.random.default_rng(ic + s)
            x = rng.standard_normal((a.batch, s, s, ic)).astype(np.float32)
            w = (rng.standard_normal((oc, ic, 3, 3)) / np.sqrt(9 * ic)).astype(np.float32)
            b = rng.standard_normal(oc).astype(np.float32) * 0.1
            bn = {"beta": rng.uniform(-0.1, 0.1, oc).astype(np.float32), "gamma": rng.uniform(0.5, 1.5, oc).astype(np.float32),
                  "mean": rng.uniform(-0.1, 0.1, oc).astype(np.float32), "var": rng.uniform(0.5, 1.5, oc).astype(np.float32)}
            per_layer = [capi.conv2d_plan(ctx, a.batch, s, s, w, b, stride=1, act="leakyRelu", leaky=0.1, bn=bn, dtype=dt), capi.pool2d_plan(ctx, a.batch, s, s, oc, 2, 2, kind="max", same=True)]
            capi.set_option("SNNHIP_POOL_FUSE", "1")
            fused = capi.chain_plan(ctx, per_layer)
            capi.set_option("SNNHIP_POOL_FUSE", None)
            assert fused.num_steps() == 1 and "+maxpool(2x2)" in fused.describe(), fused.describe()
            tx = capi.Tensor.from_numpy(ctx, x, dtype=dt)
            tm = capi.Tensor(ctx, a.batch, s, s, oc, dtype=dt)
            ys = {k: capi.Tensor(ctx, a.batch, s // 2, s // 2, oc, dtype=dt) for k in ("pool", "separate")}

            def separate():
                per_layer[0].run(tx, tm)
                per_layer[1].run(tm, ys["separate"])

            run = {"pool": lambda: fused.run(tx, ys["pool"]), "separate": separate}
            for k in run:  # warm-up
                for _ in range(5):
                    run[k]()
            ctx.sync()
            diff = float(np.abs(ys["pool"].numpy().astype(np.float64) - ys["separate"].numpy()).max())
            us = {k: [] for k in run}
            for _ in range(a.rounds):
                pair = {k: [] for k in run}
                for k in ("pool", "separate", "separate", "pool"):
                    timer.start()
                    for _ in range(a.reps):
                        run[k]()
                    timer.stop()
                    pair[k].append(1e3 * timer.elapsed_ms() / a.reps)
                for k in run:
                    us[k].append(float(np.mean(pair[k])))
            st = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in us.items()}
            rows.append({"precision": "fp16" if f16 else "fp32", "layer": "%s: %d -> %d @%dx%d b%d" % (name, ic, oc, s, s, a.batch),
                         "pool_us": st["pool"], "separate_us": st["separate"], "speedup_median": st["separate"]["median"] / st["pool"]["median"],
                         "wins_beyond_spread": st["pool"]["max"] < st["separate"]["min"], "loses_beyond_spread": st["separate"]["max"] < st["pool"]["min"], "max_abs_difference": diff,
                         "nominal_gbps_pool": fused.cost()[1] / st["pool"]["median"] * 1e-3,
                         "plans": {"pool": fused.describe(), "separate": [p.describe() for p in per_layer]}})
            for t in [tx, tm] + list(ys.values()):
                t.free()
            for p in [fused] + per_layer:
                p.destroy()
    out = {"reps": a.reps, "rounds": a.rounds, "unit": "microseconds per run of the layer, median [min, max] over the rounds", "layers": rows}
    if a.models:  # the whole graph, each configuration in a process of its own
        out["models"] = {}
        for fp16 in (False, True):
            for label, env in (("default", {}), ("SNNHIP_POOL_FUSE=1", {"SNNHIP_POOL_FUSE": "1"})):
                cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_models.py"), "--model", "yolov3-tiny", "--batch", str(a.batch)] + (["--fp16"] if fp16 else [])
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, **env), timeout=600)
                line = [ln for ln in r.stdout.splitlines() if "ms/batch" in ln]
                out["models"]["yolov3-tiny %s, %s" % ("fp16" if fp16 else "fp32", label)] = line[0].strip() if line else "failed: " + r.stdout[-300:]
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
