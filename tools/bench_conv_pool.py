#!/usr/bin/env python3
"""Times the four Conv2D -> MaxPooling2D 2x2 places of YOLOv3-tiny's backbone whose full-resolution tensor has no other reader (conv2d .. conv2d_3; batch
8, fp32 and fp16) in three forms in one process: chain rule L's one launch on conv2d_mfma's POOL instances (SNNHIP_POOL_FUSE=1), what runs without the
rule -- the layer's own convolution plan as the default routing builds it and the pooling launch -- and the rule's launch on the layer's own kernel
(SNNHIP_POOL_FUSE=1 SNNHIP_POOL_KERNEL=auto: conv2d_wino_pool_kernel in fp32, conv2d_wide_pool_kernel in fp16, each where the layer's own plan is that
kernel; where auto leaves conv2d_mfma's form the row says so and times the other two).  Device times are event pairs around `reps` back-to-back runs;
per round the forms run in mirrored order (kernel, pool, separate, separate, pool, kernel), the figure is the median over the rounds with [min, max].
A form wins on a (precision, layer) only where it won by more than the run's own spread: its max < the other's min.  --models adds the
tools/bench_models.py lines of the graph by default, with SNNHIP_POOL_FUSE=1, and with SNNHIP_POOL_KERNEL=auto beside it.

    python tools/bench_conv_pool.py [--reps 50] [--rounds 7] [--batch 8] [--models] [--json profiles/pool_kernel_layers.json]
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
            capi.set_option("SNNHIP_POOL_KERNEL", "auto")
            own = capi.chain_plan(ctx, per_layer)
            capi.set_option("SNNHIP_POOL_KERNEL", None)
            capi.set_option("SNNHIP_POOL_FUSE", None)
            assert fused.num_steps() == 1 and "+maxpool(2x2)" in fused.describe(), fused.describe()
            assert own.num_steps() == 1 and "+maxpool(2x2)" in own.describe(), own.describe()
            third = own.describe() != fused.describe()  # auto took the layer's own kernel
            tx = capi.Tensor.from_numpy(ctx, x, dtype=dt)
            tm = capi.Tensor(ctx, a.batch, s, s, oc, dtype=dt)
            ys = {k: capi.Tensor(ctx, a.batch, s // 2, s // 2, oc, dtype=dt) for k in ("pool", "separate", "kernel")}

            def separate():
                per_layer[0].run(tx, tm)
                per_layer[1].run(tm, ys["separate"])

            run = {"pool": lambda: fused.run(tx, ys["pool"]), "separate": separate}
            if third:
                run["kernel"] = lambda: own.run(tx, ys["kernel"])
            for k in run:  # warm-up
                for _ in range(5):
                    run[k]()
            ctx.sync()
            diff = float(np.abs(ys["pool"].numpy().astype(np.float64) - ys["separate"].numpy()).max())
            kdiff = float(np.abs(ys["kernel"].numpy().astype(np.float64) - ys["separate"].numpy()).max()) if third else None
            us = {k: [] for k in run}
            for _ in range(a.rounds):
                pair = {k: [] for k in run}
                for k in [k for k in ("kernel", "pool", "separate", "separate", "pool", "kernel") if k in run]:
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
                         "plans": {"pool": fused.describe(), "separate": [p.describe() for p in per_layer], "kernel": own.describe() if third else "as pool: auto leaves conv2d_mfma's form"}})
            if third:  # against the separate launches (the layer's own kernel + pool2d_kernel) and against conv2d_mfma's form
                rows[-1].update({"kernel_us": st["kernel"], "kernel_speedup_median": st["separate"]["median"] / st["kernel"]["median"],
                                 "kernel_wins_beyond_spread": st["kernel"]["max"] < st["separate"]["min"], "kernel_loses_beyond_spread": st["separate"]["max"] < st["kernel"]["min"],
                                 "kernel_vs_pool_median": st["pool"]["median"] / st["kernel"]["median"], "kernel_beats_pool_beyond_spread": st["kernel"]["max"] < st["pool"]["min"],
                                 "kernel_max_abs_difference": kdiff})
            for t in [tx, tm] + list(ys.values()):
                t.free()
            for p in [fused, own] + per_layer:
                p.destroy()
    out = {"reps": a.reps, "rounds": a.rounds, "unit": "microseconds per run of the layer, median [min, max] over the rounds", "layers": rows}
    if a.models:  # the whole graph, each configuration in a process of its own
        out["models"] = {}
        for fp16 in (False, True):
            for label, env in (("default", {}), ("SNNHIP_POOL_FUSE=1", {"SNNHIP_POOL_FUSE": "1"}),
                               ("SNNHIP_POOL_FUSE=1 SNNHIP_POOL_KERNEL=auto", {"SNNHIP_POOL_FUSE": "1", "SNNHIP_POOL_KERNEL": "auto"})):
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
