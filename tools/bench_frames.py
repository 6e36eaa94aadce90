#!/usr/bin/env python
"""ESPCN 2x at 1080p with fp32 I/O against 8-bit I/O (chain rules A8 / B8), in one process.

Three forms: f32 (the fused two-kernel chain), u8 (the conversions folded into it: two launches) and u8_sep (the u8_in launch, the same fp32
chain, the u8_out launch: four launches).  The forms are alternated in mirrored order (A B C C B A per round): per round, a timed region of
--iters device steps each (hipEvent pair), the median over --rounds is reported; the end-to-end loops run in rounds of their own.  End to end
adds the H2D upload of one input frame and the D2H download of one output frame to every step (synchronous copies, as a caller does them).
Then one launch-trace pass (snnhip_trace_begin / _end) lists the kernels of each form with their per-launch times.

    python tools/bench_frames.py [--h 1080 --w 1920 --rounds 7 --iters 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    net = models.espcn_weights(seed=1)
    H, W = a.h, a.w
    rng = np.random.default_rng(1)
    u8 = rng.integers(0, 256, size=(1, H, W, 1), dtype=np.uint8)
    f32 = ((u8.astype(np.float32) - 127.5) * np.float32(1 / 127.5))

    layers, shape = [], (1, H, W, 1)
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape)
        layers.append(p)
        shape = p.out_shape()
    uin = capi.u8_in_plan(ctx, 1, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1))
    uout = capi.u8_out_plan(ctx, *shape, (127.5, 0, 0, 0), (127.5, 0, 0, 0))
    class Seq:  # u8_in, the fp32 chain, u8_out as separate launches (what rules A8 / B8 replace)
        def __init__(self, plans, shapes):
            self.plans, self.mids = plans, [capi.Tensor(ctx, *sh) for sh in shapes]

        def run(self, x, y):
            src = x
            for p, dst in zip(self.plans, self.mids + [y]):
                p.run(src, dst)
                src = dst

        def num_steps(self):
            return sum(p.num_steps() for p in self.plans)

        def step_describe(self, i):
            return [p.step_describe(k) for p in self.plans for k in range(p.num_steps())][i]

    fchain = capi.chain_plan(ctx, layers)
    forms = {
        "f32": dict(plan=fchain, x=capi.Tensor(ctx, 1, H, W, 1), y=capi.Tensor(ctx, *shape),
                    xh=f32, yh=np.empty(shape, np.float32)),
        "u8": dict(plan=capi.chain_plan(ctx, [uin] + layers + [uout]), x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U8),
                   y=capi.Tensor(ctx, *shape, dtype=capi.U8), xh=u8, yh=np.empty(shape, np.uint8)),
        "u8_sep": dict(plan=Seq([uin, fchain, uout], [(1, H, W, 1), shape]), x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U8),
                       y=capi.Tensor(ctx, *shape, dtype=capi.U8), xh=u8, yh=np.empty(shape, np.uint8)),
    }
    for f in forms.values():
        if f["x"].dtype == capi.U8:
            f["x"].upload_u8(f["xh"])
        else:
            f["x"].upload(f["xh"])

    def upload(f):
        if f["x"].dtype == capi.U8:
            capi.check(capi.lib().snnhip_tensor_upload_raw(f["x"].h, f["xh"].ctypes.data_as(capi._P), f["xh"].nbytes))
        else:
            capi.check(capi.lib().snnhip_tensor_upload(f["x"].h, capi._fptr(f["xh"])))

    def download(f):
        capi.check(capi.lib().snnhip_tensor_download_raw(f["y"].h, f["yh"].ctypes.data_as(capi._P), f["yh"].nbytes))

    timer = capi.Timer(ctx)
    dev = {k: [] for k in forms}
    e2e = {k: [] for k in forms}
    for k, f in forms.items():
        for _ in range(a.warmup):
            f["plan"].run(f["x"], f["y"])
        ctx.sync()
    order = list(forms) + list(forms)[::-1]  # mirrored: A B C C B A
    for _ in range(a.rounds):
        for k in order:
            f = forms[k]
            timer.start()
            for _ in range(a.iters):
                f["plan"].run(f["x"], f["y"])
            timer.stop()
            dev[k].append(timer.elapsed_ms() / a.iters)
    for _ in range(a.rounds):
        for k in order:
            f = forms[k]
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                upload(f)
                f["plan"].run(f["x"], f["y"])
                download(f)
            e2e[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"frame": "%dx%d -> %dx%d" % (H, W, 2 * H, 2 * W), "rounds": a.rounds, "iters": a.iters}
    for k, f in forms.items():
        d, e = statistics.median(dev[k]), statistics.median(e2e[k])
        out[k] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[k]), 4), "device_ms_max": round(max(dev[k]), 4),
                  "e2e_ms_median": round(e, 4), "e2e_frames_per_s": round(1e3 / e, 1),
                  "io_bytes_per_frame": int(f["xh"].nbytes + f["yh"].nbytes),
                  "steps": [f["plan"].step_describe(i) for i in range(f["plan"].num_steps())]}
    out["device_u8_over_f32"] = round(out["u8"]["device_ms_median"] / out["f32"]["device_ms_median"], 4)
    out["device_u8_over_u8_sep"] = round(out["u8"]["device_ms_median"] / out["u8_sep"]["device_ms_median"], 4)
    out["e2e_fps_u8_over_f32"] = round(out["u8"]["e2e_frames_per_s"] / out["f32"]["e2e_frames_per_s"], 4)
    print(json.dumps(out, indent=1))
    for k, f in forms.items():
        capi.trace_begin()
        for _ in range(a.iters):
            f["plan"].run(f["x"], f["y"])
        ctx.sync()
        rep = capi.trace_end()
        print("launches (%s I/O), per-kernel time over %d steps:" % (k, a.iters))
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        for item in kernels:
            name = item.get("function")
            n, ms = item.get("launches", 0), item.get("total_ms", item.get("ms", 0.0))
            print("  %-48s launches=%-4d us/launch=%.2f" % (name, n, 1e3 * ms / max(n, 1)))
    ctx.close()


if __name__ == "__main__":
    main()
