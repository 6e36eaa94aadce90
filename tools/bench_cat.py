#!/usr/bin/env python3
"""Times the five Concatenate -> Conv2D places of the zoo (U-Net's four decoder concats, YOLOv3-tiny's second head with its nearest x2 UpSampling2D on
input 0; batch 8, fp32 and fp16): chain rule K's one two-source convolution launch (SNNHIP_CONV=cat) against what runs without it -- [the upsampling's
launch,] the Concatenate launch and the layer's own convolution plan as the default routing builds it (conv2d_wino in fp32, conv2d_wide_f16 / conv2d_mfma
in fp16) -- in one process.  Device times are event pairs around `reps` back-to-back runs; per round the two forms run in mirrored order (new, old, old,
new), the figure is the median over the rounds with [min, max].  A (precision, layer class) is routed to the rule by default only where it won by more
than the run's own spread: new max < old min.  A third form runs in the same rounds where it exists: the rule on the layer's own kernel
(SNNHIP_CAT_KERNEL=auto: conv2d_wino's two-source instances in fp32, conv2d_wide_f16's in fp16; profiles/cat_kernel_layers.json).  --models adds the tools/bench_models.py lines of
the two graphs with and without SNNHIP_CAT=0 and under SNNHIP_CAT_KERNEL=auto.

    python tools/bench_cat.py [--reps 50] [--rounds 7] [--batch 8] [--models] [--json profiles/cat_kernel_layers.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# model, layer, C0, C1, OC, extent of the convolution, upsampling on input 0
LAYERS = [("unet", "concatenate_4", 512, 512, 512, 32, False), ("unet", "concatenate_5", 256, 256, 256, 64, False), ("unet", "concatenate_6", 128, 128, 128, 128, False),
          ("unet", "concatenate_7", 64, 64, 64, 256, False), ("yolov3-tiny", "concatenate", 128, 256, 256, 26, True)]


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
        for model, name, c0, c1, oc, s, up in LAYERS:
            rng = np.random.default_rng(c0 + s)
            s0 = s // 2 if up else s
            xa = rng.standard_normal((a.batch, s0, s0, c0)).astype(np.float32)
            xb = rng.standard_normal((a.batch, s, s, c1)).astype(np.float32)
            w = (rng.standard_normal((oc, c0 + c1, 3, 3)) / np.sqrt(9 * (c0 + c1))).astype(np.float32)
            b = rng.standard_normal(oc).astype(np.float32) * 0.1
            act = "leakyRelu" if up else "relu"
            per_layer = ([capi.upsample_plan(ctx, a.batch, s0, s0, c0, 2.0, "nearest")] if up else []) + [
                capi.concat_plan(ctx, a.batch, s, s, c0, c1), capi.conv2d_plan(ctx, a.batch, s, s, w, b, stride=1, act=act, leaky=0.1, dtype=dt)]
            capi.set_option("SNNHIP_CONV", "cat")
            fused = capi.chain_plan(ctx, per_layer)
            capi.set_option("SNNHIP_CONV", None)
            assert "+concat" in fused.describe(), fused.describe()
            # third form: the rule on the layer's own kernel (SNNHIP_CAT_KERNEL=auto: conv2d_wino's two-source instances in fp32, conv2d_wide_f16's in fp16); None where auto keeps today's decision
            capi.set_option("SNNHIP_CAT_KERNEL", "auto")
            try:
                own = capi.chain_plan(ctx, per_layer)
            except capi.SnnHipError:
                own = None
            capi.set_option("SNNHIP_CAT_KERNEL", None)
            if own is not None and ("+concat" not in own.describe() or own.describe() == fused.describe()):
                own.destroy()
                own = None
            ta, tb = capi.Tensor.from_numpy(ctx, xa, dtype=dt), capi.Tensor.from_numpy(ctx, xb, dtype=dt)
            tu = capi.Tensor(ctx, a.batch, s, s, c0, dtype=dt) if up else ta
            tc = capi.Tensor(ctx, a.batch, s, s, c0 + c1, dtype=dt)
            ys = {k: capi.Tensor(ctx, a.batch, s, s, oc, dtype=dt) for k in ("cat", "separate") + (("own",) if own else ())}

            def separate():
                if up:
                    per_layer[0].run(ta, tu)
                per_layer[-2].run([tu, tb], tc)
                per_layer[-1].run(tc, ys["separate"])

            run = {"cat": lambda: fused.run([ta, tb], ys["cat"]), "separate": separate}
            if own:
                run["own"] = lambda: own.run([ta, tb], ys["own"])
            for k in run:  # warm-up
                for _ in range(5):
                    run[k]()
            ctx.sync()
            diff = float(np.abs(ys["cat"].numpy().astype(np.float64) - ys["separate"].numpy()).max())
            us = {k: [] for k in run}
            for _ in range(a.rounds):
                pair = {k: [] for k in run}
                for k in ("cat", "own", "separate", "separate", "own", "cat") if own else ("cat", "separate", "separate", "cat"):
                    timer.start()
                    for _ in range(a.reps):
                        run[k]()
                    timer.stop()
                    pair[k].append(1e3 * timer.elapsed_ms() / a.reps)
                for k in run:
                    us[k].append(float(np.mean(pair[k])))
            st = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in us.items()}
            rows.append({"precision": "fp16" if f16 else "fp32", "model": model, "layer": "%s: %d+%d -> %d @%dx%d b%d%s" % (name, c0, c1, oc, s, s, a.batch, ", x2 upsampling on input 0" if up else ""),
                         "class": "upsampling on input 0" if up else "plain concat",
                         "cat_us": st["cat"], "separate_us": st["separate"], "speedup_median": st["separate"]["median"] / st["cat"]["median"],
                         "wins_beyond_spread": st["cat"]["max"] < st["separate"]["min"], "max_abs_difference": diff,
                         "nominal_tflops_cat": fused.cost()[0] / st["cat"]["median"] * 1e-6,
                         "plans": {"cat": fused.describe(), "separate": [p.describe() for p in per_layer]}})
            if own:
                rows[-1].update({"own_kernel_us": st["own"], "own_kernel_speedup_median": st["separate"]["median"] / st["own"]["median"],
                                 "own_kernel_wins_beyond_spread": st["own"]["max"] < st["separate"]["min"],
                                 "own_kernel_max_abs_difference": float(np.abs(ys["own"].numpy().astype(np.float64) - ys["separate"].numpy()).max())})
                rows[-1]["plans"]["own_kernel"] = own.describe()
            for t in {ta, tb, tu, tc} | set(ys.values()):
                t.free()
            for p in [fused] + ([own] if own else []) + per_layer:
                p.destroy()
    routing = {}
    for r in rows:
        key = r["precision"] + ", " + r["class"]
        routing[key] = routing.get(key, True) and r["wins_beyond_spread"]
    out = {"reps": a.reps, "rounds": a.rounds, "unit": "microseconds per run of the layer, median [min, max] over the rounds", "layers": rows, "default_routing_to_rule_k": routing}
    if a.models:  # whole graphs, each configuration in a process of its own: SNNHIP_CONV=cat takes the rule (and keeps every 3x3 layer on conv2d_mfma), SNNHIP_CAT=0 switches it off
        out["models"] = {}
        for model in ("unet", "yolov3-tiny"):
            for fp16 in (False, True):
                for label, env in (("default", {}), ("SNNHIP_CAT=0", {"SNNHIP_CAT": "0"}), ("SNNHIP_CONV=cat", {"SNNHIP_CONV": "cat"}), ("SNNHIP_CAT_KERNEL=auto", {"SNNHIP_CAT_KERNEL": "auto"})):
                    cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_models.py"), "--model", model, "--batch", str(a.batch)] + (["--fp16"] if fp16 else [])
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, **env), timeout=600)
                    line = [ln for ln in r.stdout.splitlines() if "ms/batch" in ln]
                    out["models"]["%s %s, %s" % (model, "fp16" if fp16 else "fp32", label)] = line[0].strip() if line else "failed: " + r.stdout[-300:]
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
