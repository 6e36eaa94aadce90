#!/usr/bin/env python
"""bench_irb.py -- MobileNetV2's inverted-residual blocks (BASELINE configs[3]) one at a time: the fused kernel (irb_fused.hip, chain rule G)
against the three / four separate layers, at --batch images.   python tools/bench_irb.py [--batch 64] [--only b02] [--reps 20]
--half: the same blocks on half tensors, irb_f16.hip's fused plan (SNNHIP_IRB_F16=1) against the per-layer fp16 plans of the same chain, both in this
process, per round in mirrored order (fused, separate, separate, fused); median [min, max] over the rounds -> --json (profiles/irb_f16_blocks.json).
    python tools/bench_irb.py --half [--batch 256] [--reps 20] [--rounds 7] [--json profiles/irb_f16_blocks.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, H, C, Ch, Co, stride, residual
BLOCKS = [("b01", 112, 16, 96, 24, 2, False), ("b02", 56, 24, 144, 24, 1, True), ("b03", 56, 24, 144, 32, 2, False), ("b04", 28, 32, 192, 32, 1, True),
          ("b06", 28, 32, 192, 64, 2, False), ("b07", 14, 64, 384, 64, 1, True), ("b10", 14, 64, 384, 96, 1, False), ("b11", 14, 96, 576, 96, 1, True),
          ("b13", 14, 96, 576, 160, 2, False), ("b14", 7, 160, 960, 160, 1, True), ("b16", 7, 160, 960, 320, 1, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--half", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import shadernn_amd as snn

    snn.load_library()
    ctx = snn.Context(0)
    rng = np.random.default_rng(1)
    N = args.batch
    if args.half:
        return half(snn, ctx, rng, args)

    def timeit(fn):
        for _ in range(3):
            fn()
        ctx.sync()
        t = snn.Timer(ctx)
        t.start()
        for _ in range(args.reps):
            fn()
        t.stop()
        ctx.sync()
        us = 1e3 * t.elapsed_ms() / args.reps
        t.destroy()
        return us

    for name, H, C, Ch, Co, s, res in BLOCKS:
        if args.only and args.only != name:
            continue
        r = lambda *sh, sc=1.0: (rng.standard_normal(sh) * sc).astype(np.float32)
        bn = lambda c: {"beta": r(c, sc=0.1), "gamma": (1 + r(c, sc=0.1)), "mean": r(c, sc=0.1), "var": (1 + np.abs(r(c, sc=0.1))).astype(np.float32)}
        pe = snn.conv2d_plan(ctx, N, H, H, r(Ch, C, 1, 1, sc=C ** -0.5), r(Ch, sc=0.1), act="relu6", bn=bn(Ch))
        pd = snn.conv2d_plan(ctx, N, H, H, r(Ch, 3, 3, sc=1 / 3), r(Ch, sc=0.1), stride=s, pads=(1, 1, 1, 1), act="relu6", bn=bn(Ch), depthwise=True)
        _, OH, OW, _ = pd.out_shape()
        pp = snn.conv2d_plan(ctx, N, OH, OW, r(Co, Ch, 1, 1, sc=Ch ** -0.5), r(Co, sc=0.1), bn=bn(Co))
        x = snn.Tensor.from_numpy(ctx, rng.random((N, H, H, C), dtype=np.float32))
        th, td, tp, ty = (snn.Tensor(ctx, N, H, H, Ch), snn.Tensor(ctx, N, OH, OW, Ch), snn.Tensor(ctx, N, OH, OW, Co), snn.Tensor(ctx, N, OH, OW, Co))
        if res:
            pa = snn.add_plan(ctx, N, OH, OW, Co)
            fused = snn.graph_fuse(ctx, [(pe, [-1], False), (pd, [0], False), (pp, [1], False), (pa, [2, -1], True)])[3][0]
        else:
            pa = None
            try:
                fused = snn.chain_plan(ctx, [pe, pd, pp])
            except snn.SnnHipError:
                fused = None

        def separate():
            pe.run(x, th)
            pd.run(th, td)
            pp.run(td, tp)
            if pa:
                pa.run([tp, x], ty)

        fl = pe.cost()[0] + pd.cost()[0] + pp.cost()[0]
        t_sep = None if args.fused_only else timeit(separate)
        t_f = timeit(lambda: fused.run(x, ty)) if fused is not None and "irb_fused" in fused.describe() else None
        d = fused.describe() if t_f else ""
        tile = d.split("tile=")[1].split(" ")[0] if "tile=" in d else ("band " + d.split("band per block (")[1].split(")")[0]) if "band per block" in d else "image" if "image per block" in d else "-"
        print("%s %dx%d %d->%d->%d s%d%s b%d: separate %s us, fused[%s per wave] %s us (%.1f TF/s)" % (
            name, H, H, C, Ch, Co, s, " +add" if res else "", N, "%.1f" % t_sep if t_sep else "-", tile, "%.1f" % t_f if t_f else "n/a",
            fl / t_f / 1e6 if t_f else 0.0), flush=True)
        for t in (x, th, td, tp, ty):
            t.free()


def half(snn, ctx, rng, args):
    N, rows = args.batch, []

    def timeit(fn):
        fn()
        ctx.sync()
        t = snn.Timer(ctx)
        t.start()
        for _ in range(args.reps):
            fn()
        t.stop()
        ctx.sync()
        us = 1e3 * t.elapsed_ms() / args.reps
        t.destroy()
        return us

    for name, H, C, Ch, Co, s, res in BLOCKS:
        if args.only and args.only != name:
            continue
        r = lambda *sh, sc=1.0: (rng.standard_normal(sh) * sc).astype(np.float32)
        bn = lambda c: {"beta": r(c, sc=0.1), "gamma": (1 + r(c, sc=0.1)), "mean": r(c, sc=0.1), "var": (1 + np.abs(r(c, sc=0.1))).astype(np.float32)}
        kw = dict(dtype=snn.F16)
        pe = snn.conv2d_plan(ctx, N, H, H, r(Ch, C, 1, 1, sc=C ** -0.5), r(Ch, sc=0.1), act="relu6", bn=bn(Ch), **kw)
        pd = snn.conv2d_plan(ctx, N, H, H, r(Ch, 3, 3, sc=1 / 3), r(Ch, sc=0.1), stride=s, pads=(1, 1, 1, 1), act="relu6", bn=bn(Ch), depthwise=True, **kw)
        _, OH, OW, _ = pd.out_shape()
        pp = snn.conv2d_plan(ctx, N, OH, OW, r(Co, Ch, 1, 1, sc=Ch ** -0.5), r(Co, sc=0.1), bn=bn(Co), **kw)
        pa = snn.add_plan(ctx, N, OH, OW, Co) if res else None
        x = snn.Tensor.from_numpy(ctx, rng.random((N, H, H, C), dtype=np.float32), dtype=snn.F16)
        th, td, tp, ty = (snn.Tensor(ctx, N, H, H, Ch, **kw), snn.Tensor(ctx, N, OH, OW, Ch, **kw), snn.Tensor(ctx, N, OH, OW, Co, **kw), snn.Tensor(ctx, N, OH, OW, Co, **kw))
        os.environ["SNNHIP_IRB_F16"] = "1"
        try:
            fused = snn.graph_fuse(ctx, [(pe, [-1], False), (pd, [0], False), (pp, [1], False), (pa, [2, -1], True)])[3][0] if res else snn.chain_plan(ctx, [pe, pd, pp])
        except snn.SnnHipError:
            fused = None
        del os.environ["SNNHIP_IRB_F16"]
        if fused is None or "irb_f16" not in fused.describe():
            print("%s: declined by irb_f16" % name, flush=True)
            rows.append({"block": name, "declined": True})
            continue

        def separate():
            pe.run(x, th)
            pd.run(th, td)
            pp.run(td, tp if pa else ty)
            if pa:
                pa.run([tp, x], ty)

        us = {"fused": [], "separate": []}
        for _ in range(args.rounds):
            for k in ("fused", "separate", "separate", "fused"):
                us[k].append(timeit((lambda: fused.run(x, ty)) if k == "fused" else separate))
        st = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in us.items()}
        verdict = "wins" if st["fused"]["max"] < st["separate"]["min"] else "loses" if st["fused"]["min"] > st["separate"]["max"] else "inside the spreads"
        rows.append({"block": name, "H": H, "C": C, "Ch": Ch, "Co": Co, "stride": s, "add": res, "batch": N, "fused_us": st["fused"], "separate_us": st["separate"],
                     "speedup_median": st["separate"]["median"] / st["fused"]["median"], "fused_beyond_both_spreads": verdict, "plan": fused.describe(),
                     "separate_plans": [p.describe() for p in (pe, pd, pp)]})
        print("%s %dx%d %d->%d->%d s%d%s b%d fp16: separate %.1f [%.1f, %.1f] us, irb_f16 %.1f [%.1f, %.1f] us: %.2fx (%s)" % (
            name, H, H, C, Ch, Co, s, " +add" if res else "", N, st["separate"]["median"], st["separate"]["min"], st["separate"]["max"], st["fused"]["median"],
            st["fused"]["min"], st["fused"]["max"], st["separate"]["median"] / st["fused"]["median"], verdict), flush=True)
        for t in (x, th, td, tp, ty):
            t.free()
    if args.json:
        out = {"reps": args.reps, "rounds": args.rounds, "batch": N, "unit": "microseconds per run of the block, median [min, max] over 2 x rounds samples of `reps` runs each",
               "blocks": rows}
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
