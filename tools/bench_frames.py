#!/usr/bin/env python
"""ESPCN 2x at 1080p with fp32 I/O against 8-bit I/O (chain rules A8 / B8), in one process.

Three forms: f32 (the fused two-kernel chain), u8 (the conversions folded into it: two launches) and u8_sep (the u8_in launch, the same fp32
chain, the u8_out launch: four launches).  The forms are alternated in mirrored order (A B C C B A per round): per round, a timed region of
--iters device steps each (hipEvent pair), the median over --rounds is reported; the end-to-end loops run in rounds of their own.  End to end
adds the H2D upload of one input frame and the D2H download of one output frame to every step (synchronous copies, as a caller does them).
Then one launch-trace pass (snnhip_trace_begin / _end) lists the kernels of each form with their per-launch times.

    python tools/bench_frames.py [--h 1080 --w 1920 --rounds 7 --iters 20]

--scale 3 / 4: the ESPCN of that upscale factor on the input size that keeps the output at 3840 x 2160 (1280 x 720, 960 x 540), and two more
forms in the same alternation, f32_layers and u8_layers: one plan per layer (the generic convolutions, the stand-alone Subpixel launch and the
stand-alone 8-bit conversions) -- the baseline rule B's kernel for that factor has to beat.  The report then also carries, per form, the traced
kernels with their time per launch and, for the chain's fused steps, the fraction of the HBM roofline on the step's own bytes and of the fp32
matrix peak on the MFMA flops it executes.  --per-layer adds the two forms at scale 2 as well.

    python tools/bench_frames.py --scale 3

--half: the fp16 forms instead, in the same alternation: f32 (the fused fp32 chain), f16_layers (one fp16 plan per layer, what prefer_half runs by
default), f16 (the fused fp16 chain, chain rules A16 / B16, SNNHIP_ESPCN_F16=1) and f16_u8 (the same with the 8-bit conversions folded in).  Device
step per form with the spread over the rounds, the kernels of the launch trace, and the bytes each form's launches move per frame.

    python tools/bench_frames.py --half --scale 2

--half --widths 64,32 (with any --scale): the net at the published widths 1 -> 64 -> 32 -> r*r.  No fused fp32 form exists
for it, so the forms are f16_layers, f16 (the two launches of espcn_f16_wide.hip) and f16_u8; each fused form also reports its issued MFMA flops and
its two floors (its own bytes at --hbm-tbs, those flops at --f16-mfma-tflops).  --out FILE merges the record into a JSON file under the key
half_64_32_scale<r>: profiles/espcn_wide_frames.json holds the runs at 1080p x2, 720p x3 and 540p x4.

    python tools/bench_frames.py --half --widths 64,32 --scale 3 --out profiles/espcn_wide_frames.json

--bits 10 | 12 | 16 (with any --scale): two more forms in the same alternation and the same
end-to-end rounds, u16 (16-bit frames, the conversions folded into the fp32 kernels: two launches) and u16_sep (u16_in, the fp32 chain, u16_out:
four launches), on low-aligned frames of that bit depth normalised symmetrically ((2^bits - 1) / 2).  The f32 and u8 forms of the same run are the
yardstick; the report carries every form's spread over its timed regions and its traced kernels.  With --half the two forms are f16_u16 and
f16_u16_sep around the fused fp16 chain (device step only, as the other --half forms).  One run prints one scale; profiles/espcn_u16_frames.json
holds the JSON objects of six runs (--bits 10 at --scale 2, 3, 4, each without and with --half) under the keys scale<r> / half_scale<r>, next to
the line of `python bench.py --gpus 1 --steps 20 --warmup 5` taken in the same session.

    python tools/bench_frames.py --bits 10 --scale 3
    python tools/bench_frames.py --bits 10 --half

--colour RGB8 | RGBA8 (with any --scale): colour frames around the luma chain.  Four forms in the same mirrored alternation:
r8 (the 8-bit chain on a luma plane: two launches), colour (the luma plan, the same chain, the chroma-merge plan: four launches, on the context's
stream in a straight line), merge (the merge launch alone) and copy (one hipMemcpyDtoDAsync that moves as many bytes through HBM as the merge
kernel has to: half of them read, half written).  Device step per form with the spread over the rounds, frames/s including one frame's H2D + D2H
for r8 and colour, the kernels of the launch trace, and the merge kernel's bytes/s beside the copy's.  profiles/espcn_colour_frames.json holds the
runs at --scale 2 and --scale 3 under the keys scale<r>.

    python tools/bench_frames.py --colour RGB8 --scale 3

--video NV12 | P010 (with any --scale): a decoder's 4:2:0 frames around the luma chain.  Five forms in the same mirrored
alternation: grey (the 8-bit / 16-bit chain on the luma plane: two launches), video (the same chain plus the chroma launch on the half-resolution
CbCr plane: three launches in a straight line), chroma (that launch alone), copy (one hipMemcpyDtoDAsync that moves as many bytes through HBM as
the chroma kernel has to) and rgb8 (the RGB8 colour step of --colour: four launches), so that the video step stands beside the grey step and the
RGB8 step of the same run.  Device step per form with the spread over the rounds, frames/s including one frame's H2D + D2H for grey, video and
rgb8 (an NV12 frame moves 1.5 bytes per pixel over the link, an RGB8 frame 3), the kernels of the launch trace, and the chroma kernel's bytes/s
beside the copy's.  profiles/espcn_video_frames.json holds the runs under the keys <format>_scale<r>.

    python tools/bench_frames.py --video P010 --scale 2

--video NV12 | P010 --video-out RGB8 | RGBA8 (with any --scale): video in, display out.  Five forms in the same mirrored
alternation: nv12 (the NV12 -> NV12 step of --video: the chain plus the chroma launch, three launches), nv12_rgb (the chain with the range's luma
maps plus the yuv_rgb launch on its output and the ORIGINAL chroma plane: three launches, packed RGB out; a P010 frame comes back in 16-bit
containers), yuv_rgb (that launch alone), copy (one hipMemcpyDtoDAsync that moves as many bytes through HBM as the yuv_rgb kernel has to) and rgb8
(the RGB8 colour step of --colour: four launches).  Device step per form with the spread over the rounds, frames/s including one frame's H2D + D2H
for nv12, nv12_rgb and rgb8, the kernels of the launch trace, and the yuv_rgb kernel's bytes/s beside the copy's.
profiles/espcn_video_rgb_frames.json holds the runs under the keys <format>_<out>_scale<r>.

    python tools/bench_frames.py --video NV12 --video-out RGB8 --scale 2

--colour RGB8 | RGBA8 --video-out NV12 (with any --scale): capture in, encoder out.  Five forms in the same mirrored
alternation: grey (the 8-bit chain on a luma plane: two launches), rgb_nv12 (the luma plan, the chain with the range's output map, the rgb_cbcr
launch from the RGB frame to the chroma plane of the upscaled frame: four launches, an NV12 frame out), rgb_cbcr (that launch alone), copy (one
hipMemcpyDtoDAsync that moves as many bytes through HBM as the rgb_cbcr kernel has to) and rgb8 (the RGB8 -> RGB8 colour step of --colour: four
launches).  Device step per form with the spread over the rounds, frames/s including one frame's H2D + D2H for grey, rgb_nv12 and rgb8 (an NV12
frame comes back as 1.5 bytes per pixel, an RGB8 frame as 3), the kernels of the launch trace, and the rgb_cbcr kernel's bytes/s beside the copy's.
profiles/espcn_rgb_nv12_frames.json holds the runs under the keys <format>_nv12_scale<r>.

    python tools/bench_frames.py --colour RGB8 --video-out NV12 --scale 2

--video NV12 | P010 --fit WxH (with any --scale, --h / --w the input): the frame at any output size.  Four forms in the same
mirrored alternation: nv12 (the NV12 -> NV12 step of --video at the same r: the chain plus the chroma launch, three launches), fitted (the chain plus
the two plane_fit launches, the model's luma frame to H x W and the ORIGINAL chroma plane to H/2 x W/2: four launches), fit (those two launches
alone) and copy (one hipMemcpyDtoDAsync that moves as many bytes through HBM as the two have to).  Device step per form with the spread over the
rounds, frames/s including one frame's H2D + D2H for nv12 and fitted, the kernels of the launch trace, and the two launches' bytes/s beside the
copy's.  profiles/espcn_fit_frames.json holds the runs under the keys <format>_<in>_x<r>_<out>.

    python tools/bench_frames.py --video NV12 --scale 2 --h 720 --w 1280 --fit 1920x1080

--video I420 | I010 [--video-out RGB8 | RGBA8] [--fit WxH], and --colour RGB8 | RGBA8 --video-out I420 (with any --scale): planar 4:2:0 frames
(DESIGN.md section 4.19).  Each of the four paths beside its NV12 / P010 counterpart at the same depth, in the same process, in the same mirrored
alternation: planar (the chain plus the launches behind / in front of it on planar chroma), nv12 (the same step on the interleaved plane),
planar_kernels and nv12_kernels (the launches around the chain alone: chroma_up / plane_fit with C = 1 over two planes against C = 2 over one,
yuv_rgb_planar against yuv_rgb, rgb_cbcr_planar against rgb_cbcr) and copy (one hipMemcpyDtoDAsync that moves as many bytes through HBM as those
launches have to).  Device step per form as the median of the timed regions with their min - max spread, frames/s including one frame's H2D + D2H
for planar and nv12, the kernels of the launch trace, and the planar launches' bytes/s beside the copy's.  --out FILE merges the record into a JSON
file under the key <format>[_<out>]_<in>_x<r>[_<fit>]: profiles/espcn_planar_frames.json holds the runs at 1080p x2, 720p x3, 540p x4 and 720p ->
1080p.

    python tools/bench_frames.py --video I420 --video-out RGB8 --scale 2 --out profiles/espcn_planar_frames.json

--metrics [--half]: frame metrics on the device.  For the 4K U8 luma plane (x2 from 1080p), an NV12 frame and an RGB8
frame of that size, in one process and mirrored: metrics (the frame_metrics launches alone, device events), copy (one hipMemcpyDtoDAsync of the
frame's bytes: it moves through HBM what the launches read), d2h (the download of the frame, what a user without the plan has to do; host clock)
and metrics_read (launches plus the read of the rows; host clock).  The condition recorded with them: the metrics launches take less time than the
download measured in the same run.  With --half also PSNR and SSIM of the fused fp16 chain's 8-bit output against the fused fp32 chain's on the
seeded input.  --out FILE merges the record under the key metrics_<H>x<W>[_half]: profiles/espcn_metrics_frames.json.

    python tools/bench_frames.py --metrics --half --out profiles/espcn_metrics_frames.json
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


def main_half(a):
    """--half: f32 / f16_layers / f16 / f16_u8, device step only."""
    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R = a.scale
    widths = tuple(int(c) for c in a.widths.split(","))
    wide = widths != (16, 16)  # no fused fp32 form at other widths: the f32 arm is left out
    net = models.espcn_weights(seed=1, scale=R, widths=widths)
    H, W = a.h or 2160 // R, a.w or 3840 // R
    u8 = np.random.default_rng(1).integers(0, 256, size=(1, H, W, 1), dtype=np.uint8)
    f32 = ((u8.astype(np.float32) - 127.5) * np.float32(1 / 127.5))

    def layer_plans(dtype):
        plans, shape = [], (1, H, W, 1)
        for layer in net["layers"]:
            p = _layer_plan(ctx, layer, shape, dtype)
            plans.append(p)
            shape = p.out_shape()
        return plans, shape

    class Seq:  # plans run one by one, each into a tensor of its own
        def __init__(self, plans, dtype):
            self.plans, self.mids = plans, [capi.Tensor(ctx, *p.out_shape(), dtype=dtype) for p in plans[:-1]]

        def run(self, x, y):
            src = x
            for p, dst in zip(self.plans, self.mids + [y]):
                p.run(src, dst)
                src = dst

        def num_steps(self):
            return len(self.plans)

        def step_describe(self, i):
            return self.plans[i].describe()

        def step_cost(self, i):
            f, b = self.plans[i].cost()
            return f, b * (0.5 if "subpixel" in self.plans[i].describe() else 1.0)  # (the dtype-agnostic Subpixel plan reports fp32 bytes)

    l32, shape = layer_plans(capi.F32)
    l16, _ = layer_plans(capi.F16)
    uin = capi.u8_in_plan(ctx, 1, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1), dtype=capi.F16)
    uout = capi.u8_out_plan(ctx, *shape, (127.5, 0, 0, 0), (127.5, 0, 0, 0), dtype=capi.F16)
    capi.set_option("SNNHIP_ESPCN_F16", "1")
    try:
        c16, c16u8 = capi.chain_plan(ctx, l16), capi.chain_plan(ctx, [uin] + l16 + [uout])
    finally:
        capi.set_option("SNNHIP_ESPCN_F16", None)
    assert c16.num_steps() == 2 and c16u8.num_steps() == 2, (c16.describe(), c16u8.describe())
    if a.bits:  # 16-bit frames of that depth around the fused fp16 chain: folded (two launches) and as launches of their own (four)
        maxval = (1 << a.bits) - 1
        halfv = maxval / 2.0
        u16 = np.random.default_rng(2).integers(0, maxval + 1, size=(1, H, W, 1)).astype(np.uint16)
        win = capi.u16_in_plan(ctx, 1, H, W, 1, (halfv, 0, 0, 0), (1 / halfv, 1, 1, 1), dtype=capi.F16)
        wout = capi.u16_out_plan(ctx, *shape, (halfv, 0, 0, 0), (halfv, 0, 0, 0), maxval=maxval, dtype=capi.F16)
        capi.set_option("SNNHIP_ESPCN_F16", "1")
        try:
            c16u16 = capi.chain_plan(ctx, [win] + l16 + [wout])
        finally:
            capi.set_option("SNNHIP_ESPCN_F16", None)
        assert c16u16.num_steps() == 2, c16u16.describe()
    forms = {} if wide else {"f32": dict(plan=capi.chain_plan(ctx, l32), x=capi.Tensor(ctx, 1, H, W, 1), y=capi.Tensor(ctx, *shape))}
    forms.update({
        "f16_layers": dict(plan=Seq(l16, capi.F16), x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.F16), y=capi.Tensor(ctx, *shape, dtype=capi.F16)),
        "f16": dict(plan=c16, x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.F16), y=capi.Tensor(ctx, *shape, dtype=capi.F16)),
        "f16_u8": dict(plan=c16u8, x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U8), y=capi.Tensor(ctx, *shape, dtype=capi.U8)),
    })
    if a.bits:
        forms["f16_u16"] = dict(plan=c16u16, x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U16), y=capi.Tensor(ctx, *shape, dtype=capi.U16))
        forms["f16_u16_sep"] = dict(plan=Seq([win, c16, wout], capi.F16), x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U16), y=capi.Tensor(ctx, *shape, dtype=capi.U16))
    for f in forms.values():
        if f["x"].dtype == capi.U8:
            f["x"].upload_u8(u8)
        elif f["x"].dtype == capi.U16:
            f["x"].upload_u16(u16)
        else:
            f["x"].upload(f32)
    timer = capi.Timer(ctx)
    dev = {k: [] for k in forms}
    for f in forms.values():
        for _ in range(a.warmup):
            f["plan"].run(f["x"], f["y"])
        ctx.sync()
    order = list(forms) + list(forms)[::-1]  # mirrored: A B C D D C B A
    for _ in range(a.rounds):
        for k in order:
            f = forms[k]
            timer.start()
            for _ in range(a.iters):
                f["plan"].run(f["x"], f["y"])
            timer.stop()
            dev[k].append(timer.elapsed_ms() / a.iters)
    y16 = forms["f16"]["y"].numpy()
    out = {"frame": "%dx%d -> %dx%d" % (H, W, R * H, R * W), "scale": R, "widths": list(widths), "rounds": a.rounds, "iters": a.iters,
           "max_abs_f16_minus_f16_layers": float(np.abs(y16 - forms["f16_layers"]["y"].numpy()).max())}
    if not wide:
        out["max_abs_f16_minus_f32"] = float(np.abs(y16 - forms["f32"]["y"].numpy()).max())
    for k, f in forms.items():
        plan, d = f["plan"], statistics.median(dev[k])
        capi.trace_begin()
        for _ in range(a.iters):
            plan.run(f["x"], f["y"])
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        nbytes = sum(plan.step_cost(i)[1] for i in range(plan.num_steps()))
        out[k] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[k]), 4), "device_ms_max": round(max(dev[k]), 4),
                  "spread": round((max(dev[k]) - min(dev[k])) / d, 4), "hbm_bytes_per_frame": int(nbytes),
                  "hbm_tbs_at_median": round(nbytes / (d * 1e-3) / 1e12, 3),
                  "steps": [plan.step_describe(i) for i in range(plan.num_steps())],
                  "kernels": [{"function": it.get("function"), "launches": it.get("launches", 0),
                               "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]}
        # the fused forms against their two floors: the steps' own bytes at the HBM rate, the MFMA flops they issue at the f16 matrix peak
        issued = [float(s.split("mfma_flops=")[1].split()[0]) for s in out[k]["steps"] if "mfma_flops=" in s]
        if k != "f16_layers" and len(issued) == plan.num_steps():
            out[k]["mfma_flops_issued"] = sum(issued)
            out[k]["floor_ms_hbm"] = round(nbytes / (a.hbm_tbs * 1e12) * 1e3, 4)
            out[k]["floor_ms_mfma_f16"] = round(sum(issued) / (a.f16_mfma_tflops * 1e12) * 1e3, 4)
            out[k]["hbm_floor_over_median"] = round(out[k]["floor_ms_hbm"] / d, 4)
            out[k]["mfma_floor_over_median"] = round(out[k]["floor_ms_mfma_f16"] / d, 4)
    if not wide:
        out["device_f16_over_f32"] = round(out["f16"]["device_ms_median"] / out["f32"]["device_ms_median"], 4)
    out["device_f16_over_f16_layers"] = round(out["f16"]["device_ms_median"] / out["f16_layers"]["device_ms_median"], 4)
    out["device_f16_u8_over_f16"] = round(out["f16_u8"]["device_ms_median"] / out["f16"]["device_ms_median"], 4)
    if a.bits:
        out["bits"] = a.bits
        out["device_f16_u16_over_f16"] = round(out["f16_u16"]["device_ms_median"] / out["f16"]["device_ms_median"], 4)
        out["device_f16_u16_over_f16_u8"] = round(out["f16_u16"]["device_ms_median"] / out["f16_u8"]["device_ms_median"], 4)
        out["device_f16_u16_over_f16_u16_sep"] = round(out["f16_u16"]["device_ms_median"] / out["f16_u16_sep"]["device_ms_median"], 4)
    out["spread_max"] = max(out[k]["spread"] for k in forms)
    print(json.dumps(out, indent=1))
    if a.out:  # merge the record into a JSON file under half[_<c1>_<c2>]_scale<r>
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        rec["half_%sscale%d" % ("%d_%d_" % widths if wide else "", R)] = out
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    ctx.close()


def _hip_runtime():
    """the HIP runtime this process already has mapped (torch's), for the one call the C-ABI does not wrap: hipMemcpyDtoDAsync"""
    import ctypes

    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is mapped into this process")


def main_colour(a):
    """--colour: r8 / colour / merge / copy."""
    import ctypes

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R, Cc = a.scale, {"RGB8": 3, "RGBA8": 4}[a.colour]
    net = models.espcn_weights(seed=1, scale=R)
    H, W = a.h or 2160 // R, a.w or 3840 // R
    rgb = np.random.default_rng(1).integers(0, 256, size=(1, H, W, Cc), dtype=np.uint8)
    luma_h = np.random.default_rng(2).integers(0, 256, size=(1, H, W, 1), dtype=np.uint8)
    layers, shape = [], (1, H, W, 1)
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape)
        layers.append(p)
        shape = p.out_shape()
    uin = capi.u8_in_plan(ctx, 1, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1))
    uout = capi.u8_out_plan(ctx, *shape, (127.5, 0, 0, 0), (127.5, 0, 0, 0))
    chain = capi.chain_plan(ctx, [uin] + layers + [uout])
    assert chain.num_steps() == 2, chain.describe()
    luma, merge = capi.rgb_luma_plan(ctx, 1, H, W, Cc), capi.ycc_merge_plan(ctx, 1, H, W, Cc, R)
    oshape = (1, R * H, R * W, Cc)
    t_rgb = capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8)
    t_luma = capi.Tensor.from_numpy(ctx, luma_h, dtype=capi.U8)
    t_yhi = capi.Tensor(ctx, *shape, dtype=capi.U8)
    t_out = capi.Tensor(ctx, *oshape, dtype=capi.U8)
    merge_bytes = int(merge.cost()[1])
    half = merge_bytes // 2
    t_src, t_dst = capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8)
    t_src.upload_u8(np.random.default_rng(3).integers(0, 256, size=half, dtype=np.uint8))
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()

    def run_r8():
        chain.run(t_luma, t_yhi)

    def run_colour():
        luma.run(t_rgb, t_luma)
        chain.run(t_luma, t_yhi)
        merge.run([t_yhi, t_rgb], t_out)

    def run_merge():
        merge.run([t_yhi, t_rgb], t_out)

    def run_copy():
        rc = hip.hipMemcpyDtoDAsync(t_dst.data_ptr(), t_src.data_ptr(), half, stream)
        assert rc == 0, rc

    forms = {"r8": run_r8, "colour": run_colour, "merge": run_merge, "copy": run_copy}
    yhi_h, out_h = np.empty(shape, np.uint8), np.empty(oshape, np.uint8)
    io = {"r8": (t_luma, luma_h, t_yhi, yhi_h), "colour": (t_rgb, rgb, t_out, out_h)}
    for f in forms.values():
        for _ in range(a.warmup):
            f()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {k: [] for k in forms}
    e2e = {k: [] for k in io}
    order = list(forms) + list(forms)[::-1]  # mirrored: A B C D D C B A
    for _ in range(a.rounds):
        for k in order:
            timer.start()
            for _ in range(a.iters):
                forms[k]()
            timer.stop()
            dev[k].append(timer.elapsed_ms() / a.iters)
    for _ in range(a.rounds):
        for k in list(io) + list(io)[::-1]:
            x, xh, y, yh = io[k]
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                capi.check(capi.lib().snnhip_tensor_upload_raw(x.h, xh.ctypes.data_as(capi._P), xh.nbytes))
                forms[k]()
                capi.check(capi.lib().snnhip_tensor_download_raw(y.h, yh.ctypes.data_as(capi._P), yh.nbytes))
            e2e[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"frame": "%dx%d -> %dx%d" % (H, W, R * H, R * W), "scale": R, "colour": a.colour, "rounds": a.rounds, "iters": a.iters}
    for k in forms:
        d = statistics.median(dev[k])
        out[k] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[k]), 4), "device_ms_max": round(max(dev[k]), 4),
                  "device_spread": round((max(dev[k]) - min(dev[k])) / d, 4)}
        if k in io:
            e = statistics.median(e2e[k])
            out[k].update({"e2e_ms_median": round(e, 4), "e2e_frames_per_s": round(1e3 / e, 1), "io_bytes_per_frame": int(io[k][1].nbytes + io[k][3].nbytes)})
    out["r8"]["steps"] = [chain.step_describe(i) for i in range(2)]
    out["colour"]["steps"] = [luma.describe()] + out["r8"]["steps"] + [merge.describe()]
    for k in ("r8", "colour", "merge"):  # the launch trace: per-kernel times of each form (a copy is no kernel of the library)
        capi.trace_begin()
        for _ in range(a.iters):
            forms[k]()
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        out[k]["kernels"] = [{"function": it.get("function"), "launches": it.get("launches", 0),
                              "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]
    out["device_colour_over_r8"] = round(out["colour"]["device_ms_median"] / out["r8"]["device_ms_median"], 4)
    out["e2e_fps_colour_over_r8"] = round(out["colour"]["e2e_frames_per_s"] / out["r8"]["e2e_frames_per_s"], 4)
    traced = [it for it in out["merge"]["kernels"] if it["function"] and "ycc_merge" in it["function"]]
    merge_us = traced[0]["us_per_launch"] if traced else 1e3 * out["merge"]["device_ms_median"]
    copy_us = 1e3 * out["copy"]["device_ms_median"]
    out["merge_vs_copy"] = {"merge_hbm_bytes": merge_bytes, "merge_us_per_launch_traced": merge_us, "merge_tbs": round(merge_bytes / (merge_us * 1e-6) / 1e12, 3),
                            "merge_tbs_event_timed_loop": round(merge_bytes / (out["merge"]["device_ms_median"] * 1e-3) / 1e12, 3),
                            "copy_bytes_each_way": half, "copy_hbm_bytes": 2 * half, "copy_us": round(copy_us, 2),
                            "copy_tbs": round(2 * half / (copy_us * 1e-6) / 1e12, 3)}
    out["merge_vs_copy"]["merge_over_copy_rate"] = round(out["merge_vs_copy"]["merge_tbs_event_timed_loop"] / out["merge_vs_copy"]["copy_tbs"], 4)
    print(json.dumps(out, indent=1))
    ctx.close()


def main_video(a):
    """--video: grey / video / chroma / copy / rgb8."""
    import ctypes

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R = a.scale
    wide = a.video == "P010"
    maxval, shift, dt, npdt = (1023, 6, capi.U16, np.uint16) if wide else (255, 0, capi.U8, np.uint8)
    half_range = maxval / 2.0
    net = models.espcn_weights(seed=1, scale=R)
    H, W = a.h or 2160 // R, a.w or 3840 // R
    assert H % 2 == 0 and W % 2 == 0, "4:2:0 frames have even extents"
    rng = np.random.default_rng(1)
    y_h = (rng.integers(0, maxval + 1, size=(1, H, W, 1)) << shift).astype(npdt)
    c_h = (rng.integers(0, maxval + 1, size=(1, H // 2, W // 2, 2)) << shift).astype(npdt)
    rgb = rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)

    def chain_for(first, last_of):
        layers, shape = [], (1, H, W, 1)
        for layer in net["layers"]:
            p = _layer_plan(ctx, layer, shape)
            layers.append(p)
            shape = p.out_shape()
        chain = capi.chain_plan(ctx, [first] + layers + [last_of(shape)])
        assert chain.num_steps() == 2, chain.describe()
        return chain, shape

    if wide:
        grey, shape = chain_for(capi.u16_in_plan(ctx, 1, H, W, 1, (half_range, 0, 0, 0), (1 / half_range, 1, 1, 1), shift),
                                lambda sh: capi.u16_out_plan(ctx, *sh, (half_range, 0, 0, 0), (half_range, 0, 0, 0), maxval, shift))
    else:
        grey, shape = chain_for(capi.u8_in_plan(ctx, 1, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1)), lambda sh: capi.u8_out_plan(ctx, *sh, (127.5, 0, 0, 0), (127.5, 0, 0, 0)))
    chain8, _ = chain_for(capi.u8_in_plan(ctx, 1, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1)), lambda sh: capi.u8_out_plan(ctx, *sh, (127.5, 0, 0, 0), (127.5, 0, 0, 0)))
    chroma = capi.chroma_up_plan(ctx, 1, H // 2, W // 2, 2, R, dt, maxval, shift, a.siting)
    luma, merge = capi.rgb_luma_plan(ctx, 1, H, W, 3), capi.ycc_merge_plan(ctx, 1, H, W, 3, R)
    cshape, oshape = (1, R * H // 2, R * W // 2, 2), (1, R * H, R * W, 3)
    t_y, t_c = capi.Tensor.from_numpy(ctx, y_h, dtype=dt), capi.Tensor.from_numpy(ctx, c_h, dtype=dt)
    t_yhi, t_chi = capi.Tensor(ctx, *shape, dtype=dt), capi.Tensor(ctx, *cshape, dtype=dt)
    t_rgb, t_luma = capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8), capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U8)
    t_yhi8, t_out = capi.Tensor(ctx, *shape, dtype=capi.U8), capi.Tensor(ctx, *oshape, dtype=capi.U8)
    chroma_bytes = int(chroma.cost()[1])
    half = chroma_bytes // 2
    t_src, t_dst = capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8)
    t_src.upload_u8(np.random.default_rng(3).integers(0, 256, size=half, dtype=np.uint8))
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()

    def run_grey():
        grey.run(t_y, t_yhi)

    def run_video():
        grey.run(t_y, t_yhi)
        chroma.run(t_c, t_chi)

    def run_chroma():
        chroma.run(t_c, t_chi)

    def run_copy():
        rc = hip.hipMemcpyDtoDAsync(t_dst.data_ptr(), t_src.data_ptr(), half, stream)
        assert rc == 0, rc

    def run_rgb8():
        luma.run(t_rgb, t_luma)
        chain8.run(t_luma, t_yhi8)
        merge.run([t_yhi8, t_rgb], t_out)

    forms = {"grey": run_grey, "video": run_video, "chroma": run_chroma, "copy": run_copy, "rgb8": run_rgb8}
    yhi_h, chi_h, out_h = np.empty(shape, npdt), np.empty(cshape, npdt), np.empty(oshape, np.uint8)
    io = {"grey": ([(t_y, y_h)], [(t_yhi, yhi_h)]), "video": ([(t_y, y_h), (t_c, c_h)], [(t_yhi, yhi_h), (t_chi, chi_h)]), "rgb8": ([(t_rgb, rgb)], [(t_out, out_h)])}
    for f in forms.values():
        for _ in range(a.warmup):
            f()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {k: [] for k in forms}
    e2e = {k: [] for k in io}
    order = list(forms) + list(forms)[::-1]  # mirrored: A B C D E E D C B A
    for _ in range(a.rounds):
        for k in order:
            timer.start()
            for _ in range(a.iters):
                forms[k]()
            timer.stop()
            dev[k].append(timer.elapsed_ms() / a.iters)
    for _ in range(a.rounds):
        for k in list(io) + list(io)[::-1]:
            ups, downs = io[k]
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                for t, h in ups:
                    capi.check(capi.lib().snnhip_tensor_upload_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
                forms[k]()
                for t, h in downs:
                    capi.check(capi.lib().snnhip_tensor_download_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
            e2e[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"frame": "%dx%d -> %dx%d" % (H, W, R * H, R * W), "scale": R, "video": a.video, "siting": a.siting, "rounds": a.rounds, "iters": a.iters}
    for k in forms:
        d = statistics.median(dev[k])
        out[k] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[k]), 4), "device_ms_max": round(max(dev[k]), 4),
                  "device_spread": round((max(dev[k]) - min(dev[k])) / d, 4)}
        if k in io:
            e = statistics.median(e2e[k])
            out[k].update({"e2e_ms_median": round(e, 4), "e2e_ms_min": round(min(e2e[k]), 4), "e2e_ms_max": round(max(e2e[k]), 4), "e2e_frames_per_s": round(1e3 / e, 1),
                           "io_bytes_per_frame": int(sum(h.nbytes for _, h in io[k][0]) + sum(h.nbytes for _, h in io[k][1]))})
    out["grey"]["steps"] = [grey.step_describe(i) for i in range(2)]
    out["video"]["steps"] = out["grey"]["steps"] + [chroma.describe()]
    out["rgb8"]["steps"] = [luma.describe()] + [chain8.step_describe(i) for i in range(2)] + [merge.describe()]
    for k in ("grey", "video", "chroma", "rgb8"):  # the launch trace: per-kernel times of each form (a copy is no kernel of the library)
        capi.trace_begin()
        for _ in range(a.iters):
            forms[k]()
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        out[k]["kernels"] = [{"function": it.get("function"), "launches": it.get("launches", 0),
                              "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]
    out["device_video_over_grey"] = round(out["video"]["device_ms_median"] / out["grey"]["device_ms_median"], 4)
    out["device_video_over_rgb8"] = round(out["video"]["device_ms_median"] / out["rgb8"]["device_ms_median"], 4)
    out["e2e_fps_video_over_grey"] = round(out["video"]["e2e_frames_per_s"] / out["grey"]["e2e_frames_per_s"], 4)
    out["e2e_fps_video_over_rgb8"] = round(out["video"]["e2e_frames_per_s"] / out["rgb8"]["e2e_frames_per_s"], 4)
    traced = [it for it in out["chroma"]["kernels"] if it["function"] and "chroma_up" in it["function"]]
    chroma_us = traced[0]["us_per_launch"] if traced else 1e3 * out["chroma"]["device_ms_median"]
    copy_us = 1e3 * out["copy"]["device_ms_median"]
    out["chroma_vs_copy"] = {"chroma_hbm_bytes": chroma_bytes, "chroma_us_per_launch_traced": chroma_us, "chroma_tbs_traced": round(chroma_bytes / (chroma_us * 1e-6) / 1e12, 3),
                             "chroma_tbs_event_timed_loop": round(chroma_bytes / (out["chroma"]["device_ms_median"] * 1e-3) / 1e12, 3),
                             "copy_bytes_each_way": half, "copy_hbm_bytes": 2 * half, "copy_us": round(copy_us, 2),
                             "copy_tbs": round(2 * half / (copy_us * 1e-6) / 1e12, 3)}
    out["chroma_vs_copy"]["chroma_over_copy_rate"] = round(out["chroma_vs_copy"]["chroma_tbs_event_timed_loop"] / out["chroma_vs_copy"]["copy_tbs"], 4)
    print(json.dumps(out, indent=1))
    ctx.close()


def main_fit(a):
    """--video ... --fit WxH: nv12 / fitted / fit / copy."""
    import ctypes

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R = a.scale
    OW, OH = (int(v) for v in a.fit.lower().split("x"))
    wide = a.video == "P010"
    maxval, shift, dt, npdt = (1023, 6, capi.U16, np.uint16) if wide else (255, 0, capi.U8, np.uint8)
    half_range = maxval / 2.0
    net = models.espcn_weights(seed=1, scale=R)
    H, W = a.h or 2160 // R, a.w or 3840 // R
    assert H % 2 == 0 and W % 2 == 0 and OH % 2 == 0 and OW % 2 == 0, "4:2:0 frames have even extents"
    assert R * H >= OH >= R * H / 2 and R * W >= OW >= R * W / 2, "the target lies between half and all of the x%d frame %dx%d" % (R, R * W, R * H)
    rng = np.random.default_rng(1)
    y_h = (rng.integers(0, maxval + 1, size=(1, H, W, 1)) << shift).astype(npdt)
    c_h = (rng.integers(0, maxval + 1, size=(1, H // 2, W // 2, 2)) << shift).astype(npdt)
    layers, shape = [], (1, H, W, 1)
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape)
        layers.append(p)
        shape = p.out_shape()
    if wide:
        ends = (capi.u16_in_plan(ctx, 1, H, W, 1, (half_range, 0, 0, 0), (1 / half_range, 1, 1, 1), shift), capi.u16_out_plan(ctx, *shape, (half_range, 0, 0, 0), (half_range, 0, 0, 0), maxval, shift))
    else:
        ends = (capi.u8_in_plan(ctx, 1, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1)), capi.u8_out_plan(ctx, *shape, (127.5, 0, 0, 0), (127.5, 0, 0, 0)))
    grey = capi.chain_plan(ctx, [ends[0]] + layers + [ends[1]])
    assert grey.num_steps() == 2, grey.describe()
    chroma = capi.chroma_up_plan(ctx, 1, H // 2, W // 2, 2, R, dt, maxval, shift, a.siting)
    fit_y = capi.plane_fit_plan(ctx, 1, R * H, R * W, 1, OH, OW, dt, maxval, shift, "centre")
    fit_c = capi.plane_fit_plan(ctx, 1, H // 2, W // 2, 2, OH // 2, OW // 2, dt, maxval, shift, a.siting)
    cshape, fyshape, fcshape = (1, R * H // 2, R * W // 2, 2), (1, OH, OW, 1), (1, OH // 2, OW // 2, 2)
    t_y, t_c = capi.Tensor.from_numpy(ctx, y_h, dtype=dt), capi.Tensor.from_numpy(ctx, c_h, dtype=dt)
    t_yhi, t_chi = capi.Tensor(ctx, *shape, dtype=dt), capi.Tensor(ctx, *cshape, dtype=dt)
    t_fy, t_fc = capi.Tensor(ctx, *fyshape, dtype=dt), capi.Tensor(ctx, *fcshape, dtype=dt)
    fit_bytes = int(fit_y.cost()[1] + fit_c.cost()[1])
    half = fit_bytes // 2
    t_src, t_dst = capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8)
    t_src.upload_u8(np.random.default_rng(3).integers(0, 256, size=half, dtype=np.uint8))
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()

    def run_nv12():
        grey.run(t_y, t_yhi)
        chroma.run(t_c, t_chi)

    def run_fit():
        fit_y.run(t_yhi, t_fy)
        fit_c.run(t_c, t_fc)

    def run_fitted():
        grey.run(t_y, t_yhi)
        run_fit()

    def run_copy():
        rc = hip.hipMemcpyDtoDAsync(t_dst.data_ptr(), t_src.data_ptr(), half, stream)
        assert rc == 0, rc

    forms = {"nv12": run_nv12, "fitted": run_fitted, "fit": run_fit, "copy": run_copy}
    yhi_h, chi_h, fy_h, fc_h = np.empty(shape, npdt), np.empty(cshape, npdt), np.empty(fyshape, npdt), np.empty(fcshape, npdt)
    io = {"nv12": ([(t_y, y_h), (t_c, c_h)], [(t_yhi, yhi_h), (t_chi, chi_h)]), "fitted": ([(t_y, y_h), (t_c, c_h)], [(t_fy, fy_h), (t_fc, fc_h)])}
    for f in forms.values():
        for _ in range(a.warmup):
            f()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {k: [] for k in forms}
    e2e = {k: [] for k in io}
    order = list(forms) + list(forms)[::-1]  # mirrored: A B C D D C B A
    for _ in range(a.rounds):
        for k in order:
            timer.start()
            for _ in range(a.iters):
                forms[k]()
            timer.stop()
            dev[k].append(timer.elapsed_ms() / a.iters)
    for _ in range(a.rounds):
        for k in list(io) + list(io)[::-1]:
            ups, downs = io[k]
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                for t, h in ups:
                    capi.check(capi.lib().snnhip_tensor_upload_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
                forms[k]()
                for t, h in downs:
                    capi.check(capi.lib().snnhip_tensor_download_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
            e2e[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"frame": "%dx%d -> x%d %dx%d -> %dx%d" % (H, W, R, R * H, R * W, OH, OW), "scale": R, "video": a.video, "siting": a.siting, "ratio": round(OH / (R * H), 4),
           "rounds": a.rounds, "iters": a.iters}
    for k in forms:
        d = statistics.median(dev[k])
        out[k] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[k]), 4), "device_ms_max": round(max(dev[k]), 4),
                  "device_spread": round((max(dev[k]) - min(dev[k])) / d, 4)}
        if k in io:
            e = statistics.median(e2e[k])
            out[k].update({"e2e_ms_median": round(e, 4), "e2e_ms_min": round(min(e2e[k]), 4), "e2e_ms_max": round(max(e2e[k]), 4), "e2e_frames_per_s": round(1e3 / e, 1),
                           "io_bytes_per_frame": int(sum(h.nbytes for _, h in io[k][0]) + sum(h.nbytes for _, h in io[k][1]))})
    out["nv12"]["steps"] = [grey.step_describe(i) for i in range(2)] + [chroma.describe()]
    out["fitted"]["steps"] = [grey.step_describe(i) for i in range(2)] + [fit_y.describe(), fit_c.describe()]
    for k in ("nv12", "fitted", "fit"):  # the launch trace: per-kernel times of each form (a copy is no kernel of the library)
        capi.trace_begin()
        for _ in range(a.iters):
            forms[k]()
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        out[k]["kernels"] = [{"function": it.get("function"), "launches": it.get("launches", 0),
                              "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]
    out["fit"]["luma"] = {"plan": fit_y.describe(), "hbm_bytes": int(fit_y.cost()[1])}
    out["fit"]["chroma"] = {"plan": fit_c.describe(), "hbm_bytes": int(fit_c.cost()[1])}
    for k, plan in (("luma", fit_y), ("chroma", fit_c)):  # each launch alone, traced, so that the two have a time of their own
        capi.trace_begin()
        for _ in range(a.iters):
            plan.run(*((t_yhi, t_fy) if k == "luma" else (t_c, t_fc)))
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        hit = [it for it in kernels if it.get("function") and "plane_fit" in it["function"]]
        if hit:
            us = 1e3 * hit[0].get("total_ms", hit[0].get("ms", 0.0)) / max(hit[0].get("launches", 0), 1)
            out["fit"][k].update({"us_per_launch_traced": round(us, 2), "tbs_traced": round(out["fit"][k]["hbm_bytes"] / (us * 1e-6) / 1e12, 3)})
    out["device_fitted_over_nv12"] = round(out["fitted"]["device_ms_median"] / out["nv12"]["device_ms_median"], 4)
    out["e2e_fps_fitted_over_nv12"] = round(out["fitted"]["e2e_frames_per_s"] / out["nv12"]["e2e_frames_per_s"], 4)
    copy_us = 1e3 * out["copy"]["device_ms_median"]
    out["fit_vs_copy"] = {"fit_hbm_bytes": fit_bytes, "fit_us_event_timed_loop": round(1e3 * out["fit"]["device_ms_median"], 2),
                          "fit_tbs_event_timed_loop": round(fit_bytes / (out["fit"]["device_ms_median"] * 1e-3) / 1e12, 3),
                          "copy_bytes_each_way": half, "copy_hbm_bytes": 2 * half, "copy_us": round(copy_us, 2), "copy_tbs": round(2 * half / (copy_us * 1e-6) / 1e12, 3)}
    out["fit_vs_copy"]["fit_over_copy_rate"] = round(out["fit_vs_copy"]["fit_tbs_event_timed_loop"] / out["fit_vs_copy"]["copy_tbs"], 4)
    print(json.dumps(out, indent=1))
    ctx.close()


def main_rgb_fit(a):
    """--video NV12 | P010 | I420 --video-out RGB8 | RGBA8 --rgb-fit WxH, or --colour RGB8 | RGBA8 --rgb-fit WxH: the RGB frame at that size (the chain,
    the luma fit, rgb_fit; rgb_luma in front for a colour frame) beside the r-fold RGB step of the same r (yuv_rgb / ycc_merge), the fitted NV12
    step (video, even sizes), the plane_fit + rgb_fit launches alone, a device copy of their bytes, rgb_fit and the fixed-phase RGB launch alone
    from the trace, and end to end with one frame's H2D + D2H.  Alternated in one process in mirrored order."""
    import ctypes

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R = a.scale
    OW, OH = (int(v) for v in a.rgb_fit.lower().split("x"))
    colour = a.colour is not None
    Cc = {"RGB8": 3, "RGBA8": 4}[a.colour if colour else a.video_out]
    wide, planar = a.video == "P010", a.video == "I420"
    maxval, shift, dt, npdt = (1023, 6, capi.U16, np.uint16) if wide else (255, 0, capi.U8, np.uint8)
    k = (maxval + 1) / 256.0
    yoff, yspan = (0.0, 255.0) if colour else (16.0 * k, 219.0 * k) if a.range == "limited" else (0.0, float(maxval))  # the luma maps snn_model_create13 derives
    net = models.espcn_weights(seed=1, scale=R)
    H, W = a.h or 2160 // R, a.w or 3840 // R
    assert colour or (H % 2 == 0 and W % 2 == 0), "4:2:0 frames have even extents"
    assert R * H >= OH >= R * H / 2 and R * W >= OW >= R * W / 2, "the target lies between half and all of the x%d frame %dx%d" % (R, R * W, R * H)
    rng = np.random.default_rng(1)
    layers, shape = [], (1, H, W, 1)
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape)
        layers.append(p)
        shape = p.out_shape()
    if wide:
        ends = (capi.u16_in_plan(ctx, 1, H, W, 1, (yoff, 0, 0, 0), (1 / yspan, 1, 1, 1), shift), capi.u16_out_plan(ctx, *shape, (yspan, 0, 0, 0), (yoff, 0, 0, 0), maxval, shift))
    else:
        ends = (capi.u8_in_plan(ctx, 1, H, W, 1, (yoff, 0, 0, 0), (1 / yspan, 1, 1, 1)), capi.u8_out_plan(ctx, *shape, (yspan, 0, 0, 0), (yoff, 0, 0, 0)))
    grey = capi.chain_plan(ctx, [ends[0]] + layers + [ends[1]])
    assert grey.num_steps() == 2, grey.describe()
    fit_y = capi.plane_fit_plan(ctx, 1, R * H, R * W, 1, OH, OW, dt, maxval, shift, "centre")
    oshape, rshape = (1, OH, OW, Cc), (1, R * H, R * W, Cc)
    t_y = capi.Tensor(ctx, 1, H, W, 1, dtype=dt)
    t_yhi, t_fy = capi.Tensor(ctx, *shape, dtype=dt), capi.Tensor(ctx, 1, OH, OW, 1, dtype=dt)
    t_out, t_rout = capi.Tensor(ctx, *oshape, dtype=dt), capi.Tensor(ctx, *rshape, dtype=dt)
    front = None
    if colour:
        src_h = rng.integers(0, 256, size=(1, H, W, Cc), dtype=np.uint8)
        t_src_frame = capi.Tensor.from_numpy(ctx, src_h, dtype=capi.U8)
        front = capi.rgb_luma_plan(ctx, 1, H, W, Cc)
        rgb_fit = capi.rgb_fit_plan(ctx, 1, H, W, OH, OW, Cc, "rgb")
        fixed = capi.ycc_merge_plan(ctx, 1, H, W, Cc, R)
        ups = [(t_src_frame, src_h)]
    else:
        y_h = (rng.integers(int(16 * k), int(236 * k), size=(1, H, W, 1)) << shift).astype(npdt)
        c_h = (rng.integers(int(16 * k), int(241 * k), size=(2 if planar else 1, H // 2, W // 2, 1 if planar else 2)) << shift).astype(npdt)
        t_y.upload_u16(y_h) if wide else t_y.upload_u8(y_h)
        t_src_frame = capi.Tensor.from_numpy(ctx, c_h, dtype=dt)
        rgb_fit = capi.rgb_fit_plan(ctx, 1, H // 2, W // 2, OH, OW, Cc, "planar" if planar else "cbcr", dt, maxval, shift, a.siting, a.range)
        mk = capi.yuv_rgb_planar_plan if planar else capi.yuv_rgb_plan
        fixed = mk(ctx, 1, H // 2, W // 2, Cc, R, dt, maxval, shift, a.siting, a.range)
        ups = [(t_y, y_h), (t_src_frame, c_h)]
    nv12_fit = None
    if not colour and OH % 2 == 0 and OW % 2 == 0:  # the fitted NV12 / I420 step of the same target
        nv12_fit = capi.plane_fit_plan(ctx, 2 if planar else 1, H // 2, W // 2, 1 if planar else 2, OH // 2, OW // 2, dt, maxval, shift, a.siting)
        t_fc = capi.Tensor(ctx, 2 if planar else 1, OH // 2, OW // 2, 1 if planar else 2, dtype=dt)
    pair_bytes = int(fit_y.cost()[1] + rgb_fit.cost()[1])
    half = pair_bytes // 2
    t_csrc, t_cdst = capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8)
    t_csrc.upload_u8(np.random.default_rng(3).integers(0, 256, size=half, dtype=np.uint8))
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()

    def run_model():
        if front is not None:
            front.run(t_src_frame, t_y)
        grey.run(t_y, t_yhi)

    def run_pair():
        fit_y.run(t_yhi, t_fy)
        rgb_fit.run([t_fy, t_src_frame], t_out)

    def run_rgb_fitted():
        run_model()
        run_pair()

    def run_rgb_rfold():
        run_model()
        fixed.run([t_yhi, t_src_frame], t_rout)

    def run_nv12_fitted():
        grey.run(t_y, t_yhi)
        fit_y.run(t_yhi, t_fy)
        nv12_fit.run(t_src_frame, t_fc)

    def run_copy():
        rc = hip.hipMemcpyDtoDAsync(t_cdst.data_ptr(), t_csrc.data_ptr(), half, stream)
        assert rc == 0, rc

    forms = {"rgb_fitted": run_rgb_fitted, "rgb_rfold": run_rgb_rfold, "fit_pair": run_pair, "copy": run_copy}
    if nv12_fit is not None:
        forms["nv12_fitted"] = run_nv12_fitted
    out_h, rout_h = np.empty(oshape, npdt), np.empty(rshape, npdt)
    io = {"rgb_fitted": (ups, [(t_out, out_h)]), "rgb_rfold": (ups, [(t_rout, rout_h)])}
    for f in forms.values():
        for _ in range(a.warmup):
            f()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {n: [] for n in forms}
    e2e = {n: [] for n in io}
    order = list(forms) + list(forms)[::-1]  # mirrored: A B C D D C B A
    for _ in range(a.rounds):
        for n in order:
            timer.start()
            for _ in range(a.iters):
                forms[n]()
            timer.stop()
            dev[n].append(timer.elapsed_ms() / a.iters)
    for _ in range(a.rounds):
        for n in list(io) + list(io)[::-1]:
            up, downs = io[n]
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                for t, h in up:
                    capi.check(capi.lib().snnhip_tensor_upload_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
                forms[n]()
                for t, h in downs:
                    capi.check(capi.lib().snnhip_tensor_download_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
            e2e[n].append((time.perf_counter() - t0) * 1e3 / a.iters)
    source = a.colour if colour else a.video
    out = {"frame": "%dx%d -> x%d %dx%d -> %dx%d" % (H, W, R, R * H, R * W, OH, OW), "scale": R, "source": source, "channels": Cc, "siting": a.siting, "range": a.range,
           "ratio": round(OH / (R * H), 4), "rounds": a.rounds, "iters": a.iters}
    for n in forms:
        d = statistics.median(dev[n])
        out[n] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[n]), 4), "device_ms_max": round(max(dev[n]), 4),
                  "device_spread": round((max(dev[n]) - min(dev[n])) / d, 4)}
        if n in io:
            e = statistics.median(e2e[n])
            out[n].update({"e2e_ms_median": round(e, 4), "e2e_ms_min": round(min(e2e[n]), 4), "e2e_ms_max": round(max(e2e[n]), 4), "e2e_frames_per_s": round(1e3 / e, 1),
                           "io_bytes_per_frame": int(sum(h.nbytes for _, h in io[n][0]) + sum(h.nbytes for _, h in io[n][1]))})
    out["rgb_fitted"]["steps"] = ([front.describe()] if front is not None else []) + [grey.step_describe(i) for i in range(2)] + [fit_y.describe(), rgb_fit.describe()]
    out["rgb_rfold"]["steps"] = ([front.describe()] if front is not None else []) + [grey.step_describe(i) for i in range(2)] + [fixed.describe()]

    def traced(run, needle):
        """us per launch of the kernel whose function name holds `needle`, from the launch trace of `run` alone"""
        capi.trace_begin()
        for _ in range(a.iters):
            run()
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        hit = [it for it in kernels if it.get("function") and needle in it["function"]]
        return round(1e3 * hit[0].get("total_ms", hit[0].get("ms", 0.0)) / max(hit[0].get("launches", 0), 1), 2) if hit else None

    alone = {"luma_fit": (lambda: fit_y.run(t_yhi, t_fy), "plane_fit", fit_y), "rgb_fit": (lambda: rgb_fit.run([t_fy, t_src_frame], t_out), "rgb_fit_kernel", rgb_fit),
             "fixed_phase": (lambda: fixed.run([t_yhi, t_src_frame], t_rout), "ycc_merge" if colour else "yuv_rgb", fixed)}
    out["launches"] = {}
    for n, (run, needle, plan) in alone.items():
        us = traced(run, needle)
        rec = {"plan": plan.describe(), "hbm_bytes": int(plan.cost()[1]), "us_per_launch_traced": us}
        if us:
            rec["tbs_traced"] = round(rec["hbm_bytes"] / (us * 1e-6) / 1e12, 3)
        out["launches"][n] = rec
    copy_us = 1e3 * out["copy"]["device_ms_median"]
    out["device_fitted_over_rfold"] = round(out["rgb_fitted"]["device_ms_median"] / out["rgb_rfold"]["device_ms_median"], 4)
    out["e2e_fps_fitted_over_rfold"] = round(out["rgb_fitted"]["e2e_frames_per_s"] / out["rgb_rfold"]["e2e_frames_per_s"], 4)
    out["pair_vs_copy"] = {"pair_hbm_bytes": pair_bytes, "pair_us_event_timed_loop": round(1e3 * out["fit_pair"]["device_ms_median"], 2),
                           "pair_tbs_event_timed_loop": round(pair_bytes / (out["fit_pair"]["device_ms_median"] * 1e-3) / 1e12, 3), "copy_bytes_each_way": half,
                           "copy_hbm_bytes": 2 * half, "copy_us": round(copy_us, 2), "copy_tbs": round(2 * half / (copy_us * 1e-6) / 1e12, 3)}
    out["pair_vs_copy"]["pair_over_copy_rate"] = round(out["pair_vs_copy"]["pair_tbs_event_timed_loop"] / out["pair_vs_copy"]["copy_tbs"], 4)
    print(json.dumps(out, indent=1))
    if a.out:
        record = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                record = json.load(f)
        record["%s_%s_%dx%d_x%d_to_%dx%d" % (source, "RGB8" if Cc == 3 else "RGBA8", W, H, R, OW, OH)] = out
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    ctx.close()


def main_video_rgb(a):
    """--video ... --video-out ...: nv12 / nv12_rgb / yuv_rgb / copy / rgb8."""
    import ctypes

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R, Cc = a.scale, {"RGB8": 3, "RGBA8": 4}[a.video_out]
    wide = a.video == "P010"
    maxval, shift, dt, npdt = (1023, 6, capi.U16, np.uint16) if wide else (255, 0, capi.U8, np.uint8)
    k = (maxval + 1) / 256.0
    yoff, yspan = (16.0 * k, 219.0 * k) if a.range == "limited" else (0.0, float(maxval))  # the luma maps snn_model_create9 derives from the range
    net = models.espcn_weights(seed=1, scale=R)
    H, W = a.h or 2160 // R, a.w or 3840 // R
    assert H % 2 == 0 and W % 2 == 0, "4:2:0 frames have even extents"
    rng = np.random.default_rng(1)
    y_h = (rng.integers(int(16 * k), int(236 * k), size=(1, H, W, 1)) << shift).astype(npdt)
    c_h = (rng.integers(int(16 * k), int(241 * k), size=(1, H // 2, W // 2, 2)) << shift).astype(npdt)
    rgb = rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)

    def chain_for(first, last_of):
        layers, shape = [], (1, H, W, 1)
        for layer in net["layers"]:
            p = _layer_plan(ctx, layer, shape)
            layers.append(p)
            shape = p.out_shape()
        chain = capi.chain_plan(ctx, [first] + layers + [last_of(shape)])
        assert chain.num_steps() == 2, chain.describe()
        return chain, shape

    if wide:
        grey, shape = chain_for(capi.u16_in_plan(ctx, 1, H, W, 1, (yoff, 0, 0, 0), (1 / yspan, 1, 1, 1), shift),
                                lambda sh: capi.u16_out_plan(ctx, *sh, (yspan, 0, 0, 0), (yoff, 0, 0, 0), maxval, shift))
    else:
        grey, shape = chain_for(capi.u8_in_plan(ctx, 1, H, W, 1, (yoff, 0, 0, 0), (1 / yspan, 1, 1, 1)), lambda sh: capi.u8_out_plan(ctx, *sh, (yspan, 0, 0, 0), (yoff, 0, 0, 0)))
    chain8, _ = chain_for(capi.u8_in_plan(ctx, 1, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1)), lambda sh: capi.u8_out_plan(ctx, *sh, (127.5, 0, 0, 0), (127.5, 0, 0, 0)))
    chroma = capi.chroma_up_plan(ctx, 1, H // 2, W // 2, 2, R, dt, maxval, shift, a.siting)
    yuv = capi.yuv_rgb_plan(ctx, 1, H // 2, W // 2, Cc, R, dt, maxval, shift, a.siting, a.range)
    luma, merge = capi.rgb_luma_plan(ctx, 1, H, W, 3), capi.ycc_merge_plan(ctx, 1, H, W, 3, R)
    cshape, vshape, oshape = (1, R * H // 2, R * W // 2, 2), (1, R * H, R * W, Cc), (1, R * H, R * W, 3)
    t_y, t_c = capi.Tensor.from_numpy(ctx, y_h, dtype=dt), capi.Tensor.from_numpy(ctx, c_h, dtype=dt)
    t_yhi, t_chi, t_vout = capi.Tensor(ctx, *shape, dtype=dt), capi.Tensor(ctx, *cshape, dtype=dt), capi.Tensor(ctx, *vshape, dtype=dt)
    t_rgb, t_luma = capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8), capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U8)
    t_yhi8, t_out = capi.Tensor(ctx, *shape, dtype=capi.U8), capi.Tensor(ctx, *oshape, dtype=capi.U8)
    yuv_bytes = int(yuv.cost()[1])
    half = yuv_bytes // 2
    t_src, t_dst = capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8)
    t_src.upload_u8(np.random.default_rng(3).integers(0, 256, size=half, dtype=np.uint8))
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()

    def run_nv12():
        grey.run(t_y, t_yhi)
        chroma.run(t_c, t_chi)

    def run_nv12_rgb():
        grey.run(t_y, t_yhi)
        yuv.run([t_yhi, t_c], t_vout)

    def run_yuv_rgb():
        yuv.run([t_yhi, t_c], t_vout)

    def run_copy():
        rc = hip.hipMemcpyDtoDAsync(t_dst.data_ptr(), t_src.data_ptr(), half, stream)
        assert rc == 0, rc

    def run_rgb8():
        luma.run(t_rgb, t_luma)
        chain8.run(t_luma, t_yhi8)
        merge.run([t_yhi8, t_rgb], t_out)

    forms = {"nv12": run_nv12, "nv12_rgb": run_nv12_rgb, "yuv_rgb": run_yuv_rgb, "copy": run_copy, "rgb8": run_rgb8}
    yhi_h, chi_h, vout_h, out_h = np.empty(shape, npdt), np.empty(cshape, npdt), np.empty(vshape, npdt), np.empty(oshape, np.uint8)
    io = {"nv12": ([(t_y, y_h), (t_c, c_h)], [(t_yhi, yhi_h), (t_chi, chi_h)]), "nv12_rgb": ([(t_y, y_h), (t_c, c_h)], [(t_vout, vout_h)]), "rgb8": ([(t_rgb, rgb)], [(t_out, out_h)])}
    for f in forms.values():
        for _ in range(a.warmup):
            f()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {k_: [] for k_ in forms}
    e2e = {k_: [] for k_ in io}
    order = list(forms) + list(forms)[::-1]  # mirrored: A B C D E E D C B A
    for _ in range(a.rounds):
        for k_ in order:
            timer.start()
            for _ in range(a.iters):
                forms[k_]()
            timer.stop()
            dev[k_].append(timer.elapsed_ms() / a.iters)
    for _ in range(a.rounds):
        for k_ in list(io) + list(io)[::-1]:
            ups, downs = io[k_]
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                for t, h in ups:
                    capi.check(capi.lib().snnhip_tensor_upload_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
                forms[k_]()
                for t, h in downs:
                    capi.check(capi.lib().snnhip_tensor_download_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
            e2e[k_].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"frame": "%dx%d -> %dx%d" % (H, W, R * H, R * W), "scale": R, "video": a.video, "video_out": a.video_out, "siting": a.siting, "range": a.range,
           "rounds": a.rounds, "iters": a.iters}
    for k_ in forms:
        d = statistics.median(dev[k_])
        out[k_] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[k_]), 4), "device_ms_max": round(max(dev[k_]), 4),
                   "device_spread": round((max(dev[k_]) - min(dev[k_])) / d, 4)}
        if k_ in io:
            e = statistics.median(e2e[k_])
            out[k_].update({"e2e_ms_median": round(e, 4), "e2e_ms_min": round(min(e2e[k_]), 4), "e2e_ms_max": round(max(e2e[k_]), 4), "e2e_frames_per_s": round(1e3 / e, 1),
                            "io_bytes_per_frame": int(sum(h.nbytes for _, h in io[k_][0]) + sum(h.nbytes for _, h in io[k_][1]))})
    chain_steps = [grey.step_describe(i) for i in range(2)]
    out["nv12"]["steps"] = chain_steps + [chroma.describe()]
    out["nv12_rgb"]["steps"] = chain_steps + [yuv.describe()]
    out["rgb8"]["steps"] = [luma.describe()] + [chain8.step_describe(i) for i in range(2)] + [merge.describe()]
    for k_ in ("nv12", "nv12_rgb", "yuv_rgb", "rgb8"):  # the launch trace: per-kernel times of each form (a copy is no kernel of the library)
        capi.trace_begin()
        for _ in range(a.iters):
            forms[k_]()
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        out[k_]["kernels"] = [{"function": it.get("function"), "launches": it.get("launches", 0),
                               "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]
    out["device_nv12_rgb_over_nv12"] = round(out["nv12_rgb"]["device_ms_median"] / out["nv12"]["device_ms_median"], 4)
    out["device_nv12_rgb_over_rgb8"] = round(out["nv12_rgb"]["device_ms_median"] / out["rgb8"]["device_ms_median"], 4)
    out["e2e_fps_nv12_rgb_over_nv12"] = round(out["nv12_rgb"]["e2e_frames_per_s"] / out["nv12"]["e2e_frames_per_s"], 4)
    out["e2e_fps_nv12_rgb_over_rgb8"] = round(out["nv12_rgb"]["e2e_frames_per_s"] / out["rgb8"]["e2e_frames_per_s"], 4)
    traced = [it for it in out["yuv_rgb"]["kernels"] if it["function"] and "yuv_rgb" in it["function"]]
    yuv_us = traced[0]["us_per_launch"] if traced else 1e3 * out["yuv_rgb"]["device_ms_median"]
    copy_us = 1e3 * out["copy"]["device_ms_median"]
    out["yuv_rgb_vs_copy"] = {"yuv_rgb_hbm_bytes": yuv_bytes, "yuv_rgb_us_per_launch_traced": yuv_us, "yuv_rgb_tbs_traced": round(yuv_bytes / (yuv_us * 1e-6) / 1e12, 3),
                              "yuv_rgb_tbs_event_timed_loop": round(yuv_bytes / (out["yuv_rgb"]["device_ms_median"] * 1e-3) / 1e12, 3),
                              "copy_bytes_each_way": half, "copy_hbm_bytes": 2 * half, "copy_us": round(copy_us, 2),
                              "copy_tbs": round(2 * half / (copy_us * 1e-6) / 1e12, 3)}
    out["yuv_rgb_vs_copy"]["yuv_rgb_over_copy_rate"] = round(out["yuv_rgb_vs_copy"]["yuv_rgb_tbs_event_timed_loop"] / out["yuv_rgb_vs_copy"]["copy_tbs"], 4)
    print(json.dumps(out, indent=1))
    ctx.close()


def main_rgb_nv12(a):
    """--colour ... --video-out NV12: grey / rgb_nv12 / rgb_cbcr / copy / rgb8."""
    import ctypes

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R, Cc = a.scale, {"RGB8": 3, "RGBA8": 4}[a.colour]
    scale, off = (219.0, 16.0) if a.range == "limited" else (255.0, 0.0)  # the output map snn_model_create10 derives from the range
    net = models.espcn_weights(seed=1, scale=R)
    H, W = a.h or 2160 // R, a.w or 3840 // R
    assert (R * H) % 2 == 0 and (R * W) % 2 == 0, "the 4:2:0 output frame has even extents"
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, size=(1, H, W, Cc), dtype=np.uint8)
    y_h = rng.integers(0, 256, size=(1, H, W, 1), dtype=np.uint8)

    def chain_for(first, last_of):
        layers, shape = [], (1, H, W, 1)
        for layer in net["layers"]:
            p = _layer_plan(ctx, layer, shape)
            layers.append(p)
            shape = p.out_shape()
        chain = capi.chain_plan(ctx, [first] + layers + [last_of(shape)])
        assert chain.num_steps() == 2, chain.describe()
        return chain, shape

    enc, shape = chain_for(capi.u8_in_plan(ctx, 1, H, W, 1, (0, 0, 0, 0), (1 / 255.0, 1, 1, 1)), lambda sh: capi.u8_out_plan(ctx, *sh, (scale, 0, 0, 0), (off, 0, 0, 0)))
    chain8, _ = chain_for(capi.u8_in_plan(ctx, 1, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1)), lambda sh: capi.u8_out_plan(ctx, *sh, (127.5, 0, 0, 0), (127.5, 0, 0, 0)))
    luma, merge = capi.rgb_luma_plan(ctx, 1, H, W, Cc), capi.ycc_merge_plan(ctx, 1, H, W, Cc, R)
    cbcr = capi.rgb_cbcr_plan(ctx, 1, H, W, Cc, R, a.siting, a.range)
    cshape, oshape = (1, R * H // 2, R * W // 2, 2), (1, R * H, R * W, Cc)
    t_rgb, t_y = capi.Tensor.from_numpy(ctx, rgb, dtype=capi.U8), capi.Tensor.from_numpy(ctx, y_h, dtype=capi.U8)
    t_luma, t_yhi, t_chi = capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U8), capi.Tensor(ctx, *shape, dtype=capi.U8), capi.Tensor(ctx, *cshape, dtype=capi.U8)
    t_yhi8, t_out = capi.Tensor(ctx, *shape, dtype=capi.U8), capi.Tensor(ctx, *oshape, dtype=capi.U8)
    cbcr_bytes = int(cbcr.cost()[1])
    half = cbcr_bytes // 2
    t_src, t_dst = capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8)
    t_src.upload_u8(np.random.default_rng(3).integers(0, 256, size=half, dtype=np.uint8))
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()

    def run_grey():
        chain8.run(t_y, t_yhi8)

    def run_rgb_nv12():
        luma.run(t_rgb, t_luma)
        enc.run(t_luma, t_yhi)
        cbcr.run(t_rgb, t_chi)

    def run_rgb_cbcr():
        cbcr.run(t_rgb, t_chi)

    def run_copy():
        rc = hip.hipMemcpyDtoDAsync(t_dst.data_ptr(), t_src.data_ptr(), half, stream)
        assert rc == 0, rc

    def run_rgb8():
        luma.run(t_rgb, t_luma)
        chain8.run(t_luma, t_yhi8)
        merge.run([t_yhi8, t_rgb], t_out)

    forms = {"grey": run_grey, "rgb_nv12": run_rgb_nv12, "rgb_cbcr": run_rgb_cbcr, "copy": run_copy, "rgb8": run_rgb8}
    yhi_h, chi_h, out_h = np.empty(shape, np.uint8), np.empty(cshape, np.uint8), np.empty(oshape, np.uint8)
    io = {"grey": ([(t_y, y_h)], [(t_yhi8, yhi_h)]), "rgb_nv12": ([(t_rgb, rgb)], [(t_yhi, yhi_h), (t_chi, chi_h)]), "rgb8": ([(t_rgb, rgb)], [(t_out, out_h)])}
    for f in forms.values():
        for _ in range(a.warmup):
            f()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {k_: [] for k_ in forms}
    e2e = {k_: [] for k_ in io}
    order = list(forms) + list(forms)[::-1]  # mirrored: A B C D E E D C B A
    for _ in range(a.rounds):
        for k_ in order:
            timer.start()
            for _ in range(a.iters):
                forms[k_]()
            timer.stop()
            dev[k_].append(timer.elapsed_ms() / a.iters)
    for _ in range(a.rounds):
        for k_ in list(io) + list(io)[::-1]:
            ups, downs = io[k_]
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                for t, h in ups:
                    capi.check(capi.lib().snnhip_tensor_upload_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
                forms[k_]()
                for t, h in downs:
                    capi.check(capi.lib().snnhip_tensor_download_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
            e2e[k_].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"frame": "%dx%d -> %dx%d" % (H, W, R * H, R * W), "scale": R, "colour": a.colour, "video_out": a.video_out, "siting": a.siting, "range": a.range,
           "rounds": a.rounds, "iters": a.iters}
    for k_ in forms:
        d = statistics.median(dev[k_])
        out[k_] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[k_]), 4), "device_ms_max": round(max(dev[k_]), 4),
                   "device_spread": round((max(dev[k_]) - min(dev[k_])) / d, 4)}
        if k_ in io:
            e = statistics.median(e2e[k_])
            out[k_].update({"e2e_ms_median": round(e, 4), "e2e_ms_min": round(min(e2e[k_]), 4), "e2e_ms_max": round(max(e2e[k_]), 4), "e2e_frames_per_s": round(1e3 / e, 1),
                            "io_bytes_per_frame": int(sum(h.nbytes for _, h in io[k_][0]) + sum(h.nbytes for _, h in io[k_][1]))})
    out["grey"]["steps"] = [chain8.step_describe(i) for i in range(2)]
    out["rgb_nv12"]["steps"] = [luma.describe()] + [enc.step_describe(i) for i in range(2)] + [cbcr.describe()]
    out["rgb8"]["steps"] = [luma.describe()] + [chain8.step_describe(i) for i in range(2)] + [merge.describe()]
    for k_ in ("grey", "rgb_nv12", "rgb_cbcr", "rgb8"):  # the launch trace: per-kernel times of each form (a copy is no kernel of the library)
        capi.trace_begin()
        for _ in range(a.iters):
            forms[k_]()
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        out[k_]["kernels"] = [{"function": it.get("function"), "launches": it.get("launches", 0),
                               "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]
    out["device_rgb_nv12_over_grey"] = round(out["rgb_nv12"]["device_ms_median"] / out["grey"]["device_ms_median"], 4)
    out["device_rgb_nv12_over_rgb8"] = round(out["rgb_nv12"]["device_ms_median"] / out["rgb8"]["device_ms_median"], 4)
    out["e2e_fps_rgb_nv12_over_rgb8"] = round(out["rgb_nv12"]["e2e_frames_per_s"] / out["rgb8"]["e2e_frames_per_s"], 4)
    traced = [it for it in out["rgb_cbcr"]["kernels"] if it["function"] and "rgb_cbcr" in it["function"]]
    cbcr_us = traced[0]["us_per_launch"] if traced else 1e3 * out["rgb_cbcr"]["device_ms_median"]
    copy_us = 1e3 * out["copy"]["device_ms_median"]
    out["rgb_cbcr_vs_copy"] = {"rgb_cbcr_hbm_bytes": cbcr_bytes, "rgb_cbcr_us_per_launch_traced": cbcr_us, "rgb_cbcr_tbs_traced": round(cbcr_bytes / (cbcr_us * 1e-6) / 1e12, 3),
                               "rgb_cbcr_tbs_event_timed_loop": round(cbcr_bytes / (out["rgb_cbcr"]["device_ms_median"] * 1e-3) / 1e12, 3),
                               "copy_bytes_each_way": half, "copy_hbm_bytes": 2 * half, "copy_us": round(copy_us, 2),
                               "copy_tbs": round(2 * half / (copy_us * 1e-6) / 1e12, 3)}
    out["rgb_cbcr_vs_copy"]["rgb_cbcr_over_copy_rate"] = round(out["rgb_cbcr_vs_copy"]["rgb_cbcr_tbs_event_timed_loop"] / out["rgb_cbcr_vs_copy"]["copy_tbs"], 4)
    print(json.dumps(out, indent=1))
    ctx.close()


def main_planar(a):
    """--video I420 | I010 ..., --colour ... --video-out I420: planar / nv12 / planar_kernels / nv12_kernels / copy."""
    import ctypes

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R = a.scale
    encode = a.video_out == "I420"
    wide = a.video == "I010"
    maxval, shift, dt, npdt = (1023, 0, capi.U16, np.uint16) if wide else (255, 0, capi.U8, np.uint8)  # I010: 10 bits in the low end of 2 bytes
    k = (maxval + 1) / 256.0
    yoff, yspan = (16.0 * k, 219.0 * k) if a.range == "limited" else (0.0, float(maxval))  # the luma maps snn_model_create12 derives from the range
    net = models.espcn_weights(seed=1, scale=R)
    H, W = a.h or 2160 // R, a.w or 3840 // R
    assert (R * H) % 2 == 0 and (R * W) % 2 == 0 and (encode or (H % 2 == 0 and W % 2 == 0)), "4:2:0 frames have even extents"
    rng = np.random.default_rng(1)
    layers, shape = [], (1, H, W, 1)
    for layer in net["layers"]:
        p = _layer_plan(ctx, layer, shape)
        layers.append(p)
        shape = p.out_shape()
    if encode:
        ends = (capi.u8_in_plan(ctx, 1, H, W, 1, (0, 0, 0, 0), (1 / 255.0, 1, 1, 1)), capi.u8_out_plan(ctx, *shape, (yspan, 0, 0, 0), (yoff, 0, 0, 0)))
    elif wide:
        ends = (capi.u16_in_plan(ctx, 1, H, W, 1, (yoff, 0, 0, 0), (1 / yspan, 1, 1, 1), shift), capi.u16_out_plan(ctx, *shape, (yspan, 0, 0, 0), (yoff, 0, 0, 0), maxval, shift))
    else:
        ends = (capi.u8_in_plan(ctx, 1, H, W, 1, (yoff, 0, 0, 0), (1 / yspan, 1, 1, 1)), capi.u8_out_plan(ctx, *shape, (yspan, 0, 0, 0), (yoff, 0, 0, 0)))
    chain = capi.chain_plan(ctx, [ends[0]] + layers + [ends[1]])
    assert chain.num_steps() == 2, chain.describe()
    t_yhi = capi.Tensor(ctx, *shape, dtype=dt)
    ch, cw = H // 2, W // 2
    front = None  # a launch in front of the chain (RGB in), shared by both forms
    if encode:
        Cc = {"RGB8": 3, "RGBA8": 4}[a.colour]
        rgb_h = rng.integers(0, 256, size=(1, H, W, Cc), dtype=np.uint8)
        t_rgb, t_y = capi.Tensor.from_numpy(ctx, rgb_h, dtype=capi.U8), capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U8)
        front = capi.rgb_luma_plan(ctx, 1, H, W, Cc)
        pl, nv = capi.rgb_cbcr_planar_plan(ctx, 1, H, W, Cc, R, a.siting, a.range), capi.rgb_cbcr_plan(ctx, 1, H, W, Cc, R, a.siting, a.range)
        t_pc, t_nc = capi.Tensor(ctx, 2, R * H // 2, R * W // 2, 1, dtype=capi.U8), capi.Tensor(ctx, 1, R * H // 2, R * W // 2, 2, dtype=capi.U8)
        behind = {"planar": [(pl, [t_rgb], t_pc)], "nv12": [(nv, [t_rgb], t_nc)]}
        ups = {"planar": [(t_rgb, rgb_h)], "nv12": [(t_rgb, rgb_h)]}
        downs = {"planar": [t_yhi, t_pc], "nv12": [t_yhi, t_nc]}
        key = "%s_I420_%dx%d_x%d" % (a.colour, W, H, R)
    else:
        y_h = (rng.integers(int(16 * k), int(236 * k), size=(1, H, W, 1)) << shift).astype(npdt)
        c_h = (rng.integers(int(16 * k), int(241 * k), size=(1, ch, cw, 2)) << shift).astype(npdt)
        p_h = np.ascontiguousarray(np.moveaxis(c_h, 3, 1).reshape(2, ch, cw, 1))  # the same samples as two planes
        t_y, t_nc_in, t_pc_in = capi.Tensor.from_numpy(ctx, y_h, dtype=dt), capi.Tensor.from_numpy(ctx, c_h, dtype=dt), capi.Tensor.from_numpy(ctx, p_h, dtype=dt)
        ups = {"planar": [(t_y, y_h), (t_pc_in, p_h)], "nv12": [(t_y, y_h), (t_nc_in, c_h)]}
        if a.video_out:
            Cc = {"RGB8": 3, "RGBA8": 4}[a.video_out]
            pl = capi.yuv_rgb_planar_plan(ctx, 1, ch, cw, Cc, R, dt, maxval, shift, a.siting, a.range)
            nv = capi.yuv_rgb_plan(ctx, 1, ch, cw, Cc, R, dt, maxval, shift, a.siting, a.range)
            t_po, t_no = capi.Tensor(ctx, 1, R * H, R * W, Cc, dtype=dt), capi.Tensor(ctx, 1, R * H, R * W, Cc, dtype=dt)
            behind = {"planar": [(pl, [t_yhi, t_pc_in], t_po)], "nv12": [(nv, [t_yhi, t_nc_in], t_no)]}
            downs = {"planar": [t_po], "nv12": [t_no]}
            key = "%s_%s_%dx%d_x%d" % (a.video, a.video_out, W, H, R)
        elif a.fit:
            OW, OH = (int(v) for v in a.fit.lower().split("x"))
            assert OH % 2 == 0 and OW % 2 == 0 and R * H >= OH >= R * H / 2 and R * W >= OW >= R * W / 2, "the target is even and lies between half and all of the x%d frame" % R
            fit_y = capi.plane_fit_plan(ctx, 1, R * H, R * W, 1, OH, OW, dt, maxval, shift, "centre")
            pl = capi.plane_fit_plan(ctx, 2, ch, cw, 1, OH // 2, OW // 2, dt, maxval, shift, a.siting)
            nv = capi.plane_fit_plan(ctx, 1, ch, cw, 2, OH // 2, OW // 2, dt, maxval, shift, a.siting)
            t_fy = capi.Tensor(ctx, 1, OH, OW, 1, dtype=dt)
            t_po, t_no = capi.Tensor(ctx, 2, OH // 2, OW // 2, 1, dtype=dt), capi.Tensor(ctx, 1, OH // 2, OW // 2, 2, dtype=dt)
            behind = {"planar": [(fit_y, [t_yhi], t_fy), (pl, [t_pc_in], t_po)], "nv12": [(fit_y, [t_yhi], t_fy), (nv, [t_nc_in], t_no)]}
            downs = {"planar": [t_fy, t_po], "nv12": [t_fy, t_no]}
            key = "%s_%dx%d_x%d_%dx%d" % (a.video, W, H, R, OW, OH)
        else:
            pl = capi.chroma_up_plan(ctx, 2, ch, cw, 1, R, dt, maxval, shift, a.siting)
            nv = capi.chroma_up_plan(ctx, 1, ch, cw, 2, R, dt, maxval, shift, a.siting)
            t_po, t_no = capi.Tensor(ctx, 2, R * ch, R * cw, 1, dtype=dt), capi.Tensor(ctx, 1, R * ch, R * cw, 2, dtype=dt)
            behind = {"planar": [(pl, [t_pc_in], t_po)], "nv12": [(nv, [t_nc_in], t_no)]}
            downs = {"planar": [t_yhi, t_po], "nv12": [t_yhi, t_no]}
            key = "%s_%dx%d_x%d" % (a.video, W, H, R)
    kernel_bytes = int(sum(plan.cost()[1] for plan, _, _ in behind["planar"]))
    assert kernel_bytes == int(sum(plan.cost()[1] for plan, _, _ in behind["nv12"])), "the two forms move the same bytes"
    half = kernel_bytes // 2
    t_src, t_dst = capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, half, 1, dtype=capi.U8)
    t_src.upload_u8(np.random.default_rng(3).integers(0, 256, size=half, dtype=np.uint8))
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()

    def run_kernels(form):
        for plan, ins, out_t in behind[form]:
            plan.run(ins if len(ins) > 1 else ins[0], out_t)

    def run_step(form):
        if front is not None:
            front.run(t_rgb, t_y)
        chain.run(t_y, t_yhi)
        run_kernels(form)

    def run_copy():
        rc = hip.hipMemcpyDtoDAsync(t_dst.data_ptr(), t_src.data_ptr(), half, stream)
        assert rc == 0, rc

    forms = {"planar": lambda: run_step("planar"), "nv12": lambda: run_step("nv12"), "planar_kernels": lambda: run_kernels("planar"),
             "nv12_kernels": lambda: run_kernels("nv12"), "copy": run_copy}
    for f in forms.values():
        for _ in range(a.warmup):
            f()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {k_: [] for k_ in forms}
    order = list(forms) + list(forms)[::-1]  # mirrored: A B C D E E D C B A
    for _ in range(a.rounds):
        for k_ in order:
            timer.start()
            for _ in range(a.iters):
                forms[k_]()
            timer.stop()
            dev[k_].append(timer.elapsed_ms() / a.iters)
    host_out = {form: [np.empty(t.shape, npdt if t.dtype == capi.U16 else np.uint8) for t in downs[form]] for form in downs}
    e2e = {form: [] for form in downs}
    for _ in range(a.rounds):
        for form in ("planar", "nv12", "nv12", "planar"):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                for t, h in ups[form]:
                    capi.check(capi.lib().snnhip_tensor_upload_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
                forms[form]()
                for t, h in zip(downs[form], host_out[form]):
                    capi.check(capi.lib().snnhip_tensor_download_raw(t.h, h.ctypes.data_as(capi._P), h.nbytes))
            e2e[form].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = {"frame": "%dx%d x%d" % (W, H, R), "scale": R, "video": a.video, "colour": a.colour, "video_out": a.video_out, "fit": a.fit, "siting": a.siting, "range": a.range,
           "rounds": a.rounds, "iters": a.iters}
    for k_ in forms:
        d = statistics.median(dev[k_])
        out[k_] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[k_]), 4), "device_ms_max": round(max(dev[k_]), 4),
                   "device_spread": round((max(dev[k_]) - min(dev[k_])) / d, 4)}
        if k_ in e2e:
            e = statistics.median(e2e[k_])
            out[k_].update({"e2e_ms_median": round(e, 4), "e2e_ms_min": round(min(e2e[k_]), 4), "e2e_ms_max": round(max(e2e[k_]), 4), "e2e_frames_per_s": round(1e3 / e, 1),
                            "io_bytes_per_frame": int(sum(h.nbytes for _, h in ups[k_]) + sum(h.nbytes for h in host_out[k_]))})
    for form in ("planar", "nv12"):
        out[form]["steps"] = ([front.describe()] if front is not None else []) + [chain.step_describe(i) for i in range(2)] + [plan.describe() for plan, _, _ in behind[form]]
    for k_ in ("planar", "nv12", "planar_kernels", "nv12_kernels"):  # the launch trace: per-kernel times of each form (a copy is no kernel of the library)
        capi.trace_begin()
        for _ in range(a.iters):
            forms[k_]()
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        out[k_]["kernels"] = [{"function": it.get("function"), "launches": it.get("launches", 0),
                               "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]
    # the planar step against its counterpart; the margin is this run's own spread (min - max of the repeated regions, the wider of the two forms)
    out["device_planar_over_nv12"] = round(out["planar"]["device_ms_median"] / out["nv12"]["device_ms_median"], 4)
    out["device_kernels_planar_over_nv12"] = round(out["planar_kernels"]["device_ms_median"] / out["nv12_kernels"]["device_ms_median"], 4)
    out["spread_of_the_two_steps"] = max(out["planar"]["device_spread"], out["nv12"]["device_spread"])
    out["planar_within_spread"] = bool(out["device_planar_over_nv12"] <= 1.0 + out["spread_of_the_two_steps"])
    out["e2e_fps_planar_over_nv12"] = round(out["planar"]["e2e_frames_per_s"] / out["nv12"]["e2e_frames_per_s"], 4)
    copy_us = 1e3 * out["copy"]["device_ms_median"]
    pk = out["planar_kernels"]["device_ms_median"]
    out["kernels_vs_copy"] = {"hbm_bytes": kernel_bytes, "planar_us_event_timed_loop": round(1e3 * pk, 2), "planar_tbs": round(kernel_bytes / (pk * 1e-3) / 1e12, 3),
                              "nv12_us_event_timed_loop": round(1e3 * out["nv12_kernels"]["device_ms_median"], 2),
                              "nv12_tbs": round(kernel_bytes / (out["nv12_kernels"]["device_ms_median"] * 1e-3) / 1e12, 3),
                              "copy_bytes_each_way": half, "copy_hbm_bytes": 2 * half, "copy_us": round(copy_us, 2), "copy_tbs": round(2 * half / (copy_us * 1e-6) / 1e12, 3)}
    out["kernels_vs_copy"]["planar_over_copy_rate"] = round(out["kernels_vs_copy"]["planar_tbs"] / out["kernels_vs_copy"]["copy_tbs"], 4)
    print(json.dumps(out, indent=1))
    if a.out:
        record = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                record = json.load(f)
        record[key] = out
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    ctx.close()


def main_metrics(a):
    """--metrics: frame metrics (PSNR / SSIM on the device) against what a user without them has to do, a download of the frame.  For the 4K U8 luma
    plane, an NV12 frame and an RGB8 frame: the metrics launches alone, a device copy of the same bytes and the device-to-host copy of the frame, in
    one process, mirrored; with --half also the quality of the fused fp16 chain's 8-bit output against the fused fp32 chain's."""
    import ctypes

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R = a.scale
    H, W = a.h or 2160 // R, a.w or 3840 // R
    OH, OW = R * H, R * W
    assert OH % 2 == 0 and OW % 2 == 0, "4:2:0 frames have even extents"
    rng = np.random.default_rng(1)
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()

    def noisy(shape):  # a frame and a copy a few grey levels away: what is measured does not depend on the values
        ref = rng.integers(0, 256, size=shape, dtype=np.uint8)
        return np.clip(ref.astype(np.int16) + rng.integers(-3, 4, size=shape), 0, 255).astype(np.uint8), ref

    planes = {"luma": [(1, OH, OW, 1)], "nv12": [(1, OH, OW, 1), (1, OH // 2, OW // 2, 2)], "rgb8": [(1, OH, OW, 3)]}
    forms, recs, d2h = {}, {}, {}
    for fmt, shapes in planes.items():
        parts = []
        for shp in shapes:
            t, r = noisy(shp)
            parts.append(dict(plan=capi.frame_metrics_plan(ctx, *shp), a=capi.Tensor.from_numpy(ctx, t, dtype=capi.U8), b=capi.Tensor.from_numpy(ctx, r, dtype=capi.U8),
                              out=capi.Tensor(ctx, shp[0], 1, shp[3], 2), host=np.empty(shp, np.uint8), bytes=int(np.prod(shp))))
        frame_bytes = sum(p["bytes"] for p in parts)
        src, dst = capi.Tensor(ctx, 1, 1, frame_bytes, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, frame_bytes, 1, dtype=capi.U8)
        src.upload_u8(rng.integers(0, 256, size=frame_bytes, dtype=np.uint8))

        def run_metrics(parts=parts):
            for p in parts:
                p["plan"].run([p["a"], p["b"]], p["out"])

        def run_copy(src=src, dst=dst, n=frame_bytes):  # reads n bytes and writes n: the 2 n bytes the metrics launches read
            rc = hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), n, stream)
            assert rc == 0, rc

        def run_d2h(parts=parts):  # what a user without the plan does: the output frame over the host link
            for p in parts:
                capi.check(capi.lib().snnhip_tensor_download_raw(p["a"].h, p["host"].ctypes.data_as(capi._P), p["host"].nbytes))

        def run_read(parts=parts):  # the metrics launches and the read of their rows (a sync and N * C * 32 bytes)
            for p in parts:
                p["plan"].run([p["a"], p["b"]], p["out"])
            return [capi.frame_metrics_read(p["plan"]) for p in parts]

        forms[fmt + ":metrics"], forms[fmt + ":copy"] = run_metrics, run_copy
        d2h[fmt + ":d2h"], d2h[fmt + ":metrics_read"] = run_d2h, run_read
        recs[fmt] = dict(parts=parts, frame_bytes=frame_bytes, read=run_read)
    for f in list(forms.values()) + list(d2h.values()):
        for _ in range(a.warmup):
            f()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {k: [] for k in forms}
    host = {k: [] for k in d2h}
    for _ in range(a.rounds):
        for k in list(forms) + list(forms)[::-1]:  # mirrored, device events around `iters` enqueued runs
            timer.start()
            for _ in range(a.iters):
                forms[k]()
            timer.stop()
            dev[k].append(timer.elapsed_ms() / a.iters)
        for k in list(d2h) + list(d2h)[::-1]:  # host clock around work that ends in a synchronise (both forms wait for the device every frame)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                d2h[k]()
            host[k].append((time.perf_counter() - t0) * 1e3 / a.iters)

    def stat(v):
        m = statistics.median(v)
        return {"ms_median": round(m, 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5), "spread": round((max(v) - min(v)) / m, 4)}

    out = {"frame": "%dx%d" % (OH, OW), "rounds": a.rounds, "iters": a.iters, "timing": "metrics / copy: device events around iters enqueued runs; d2h / metrics_read: host clock, every frame ends in a synchronise"}
    for fmt, rec in recs.items():
        o = {"frame_bytes": rec["frame_bytes"], "metrics": stat(dev[fmt + ":metrics"]), "copy": stat(dev[fmt + ":copy"]), "d2h": stat(host[fmt + ":d2h"]),
             "metrics_read": stat(host[fmt + ":metrics_read"]), "steps": [p["plan"].describe() for p in rec["parts"]]}
        m, c, d = o["metrics"]["ms_median"], o["copy"]["ms_median"], o["d2h"]["ms_median"]
        o["metrics_hbm_bytes"] = int(sum(p["plan"].cost()[1] for p in rec["parts"]))
        o["metrics_tbs"] = round(o["metrics_hbm_bytes"] / (m * 1e-3) / 1e12, 3)
        o["copy_hbm_bytes"] = 2 * rec["frame_bytes"]
        o["copy_tbs"] = round(o["copy_hbm_bytes"] / (c * 1e-3) / 1e12, 3)
        o["d2h_gbs"] = round(rec["frame_bytes"] / (d * 1e-3) / 1e9, 2)
        o["metrics_over_copy"] = round(m / c, 3)         # a finding, not a gate
        o["metrics_over_d2h"] = round(m / d, 4)          # the condition: below 1
        o["metrics_read_over_d2h"] = round(o["metrics_read"]["ms_median"] / d, 4)
        o["condition_metrics_faster_than_d2h"] = bool(m < d and o["metrics"]["ms_max"] < o["d2h"]["ms_min"])
        capi.trace_begin()
        for _ in range(a.iters):
            forms[fmt + ":metrics"]()
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        o["kernels"] = [{"function": it.get("function"), "launches": it.get("launches", 0),
                         "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]
        rows = rec["read"]()
        o["rows"] = [{"psnr_db": round(capi.frame_metrics_psnr(r["sse"], r["pixels"], 255), 4), "ssim": round(r["ssim"], 6)} for part in rows for r in part]
        out[fmt] = o
    out["spread_max"] = max(out[f][k]["spread"] for f in recs for k in ("metrics", "copy", "d2h", "metrics_read"))
    out["condition_met"] = all(out[f]["condition_metrics_faster_than_d2h"] for f in recs)

    if a.half:  # what the fp16 opt-in costs in picture quality: its 8-bit output against the fused fp32 chain's, same weights, same seeded input
        net = models.espcn_weights(seed=1, scale=R)
        u8 = np.random.default_rng(1).integers(0, 256, size=(1, H, W, 1), dtype=np.uint8)

        def chain(dtype):
            layers, shape = [], (1, H, W, 1)
            for layer in net["layers"]:
                p = _layer_plan(ctx, layer, shape, dtype)
                layers.append(p)
                shape = p.out_shape()
            ends = [capi.u8_in_plan(ctx, 1, H, W, 1, (127.5, 0, 0, 0), (1 / 127.5, 1, 1, 1), dtype=dtype)] + layers + [capi.u8_out_plan(ctx, *shape, (127.5, 0, 0, 0), (127.5, 0, 0, 0), dtype=dtype)]
            c = capi.chain_plan(ctx, ends)
            assert c.num_steps() == 2, c.describe()
            return c, shape

        c32, shape = chain(capi.F32)
        capi.set_option("SNNHIP_ESPCN_F16", "1")
        try:
            c16, _ = chain(capi.F16)
        finally:
            capi.set_option("SNNHIP_ESPCN_F16", None)
        x = capi.Tensor.from_numpy(ctx, u8, dtype=capi.U8)
        y32, y16 = capi.Tensor(ctx, *shape, dtype=capi.U8), capi.Tensor(ctx, *shape, dtype=capi.U8)
        c32.run(x, y32)
        c16.run(x, y16)
        plan = capi.frame_metrics_plan(ctx, *shape)
        res = capi.Tensor(ctx, shape[0], 1, shape[3], 2)
        plan.run([y16, y32], res)  # test: fp16, reference: fp32
        row = capi.frame_metrics_read(plan)[0]
        h16, h32 = y16.numpy_u8().astype(np.int16), y32.numpy_u8().astype(np.int16)
        diff = np.abs(h16 - h32)
        out["f16_vs_f32"] = {"input": "seeded uniform noise, %dx%d, U8" % (H, W), "test": c16.describe(), "reference": c32.describe(), "sse": row["sse"], "pixels": row["pixels"],
                             "psnr_db": capi.frame_metrics_psnr(row["sse"], row["pixels"], 255), "ssim": row["ssim"],
                             "host_check_sse": int((diff.astype(np.int64) ** 2).sum()), "bytes_that_differ": int((diff > 0).sum()), "max_abs_difference": int(diff.max())}
        assert out["f16_vs_f32"]["host_check_sse"] == row["sse"]
    print(json.dumps(out, indent=1))
    if a.out:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        rec["metrics_%dx%d%s" % (OH, OW, "_half" if a.half else "")] = out
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    ctx.close()


def main_yuv_tensor(a):
    """--video NV12 | P010 | I420 --tensor WxH [--half] [--batch N]: video frames in front of an RGB(A) model.  The yuv_tensor launch alone (frame of
    --h x --w, 1080p by default, to the WxH x 4 input tensor), the three launches it replaces (yuv_rgb at r = 1, image_u8, resize: 8-bit frames only)
    and a device copy of the launch's own bytes, in one process, alternated in mirrored order: medians with spreads."""
    import ctypes

    import shadernn_amd as snn
    from shadernn_amd import capi

    snn.load_library()
    ctx = capi.Context(0)
    OW, OH = (int(v) for v in a.tensor.lower().split("x"))
    H, W, N, Cc = a.h or 1080, a.w or 1920, a.batch, 4
    assert H % 2 == 0 and W % 2 == 0, "4:2:0 frames have even extents"
    planar, wide = a.video == "I420", a.video == "P010"
    dt, npdt, maxval, shift = (capi.U16, np.uint16, 1023, 6) if wide else (capi.U8, np.uint8, 255, 0)
    odt = capi.F16 if a.half else capi.F32
    rng = np.random.default_rng(1)
    k = (maxval + 1) // 256
    means, norms = (123.675 * k, 116.28 * k, 103.53 * k), (1 / (58.395 * k), 1 / (57.12 * k), 1 / (57.375 * k))
    y = capi.Tensor.from_numpy(ctx, (rng.integers(16 * k, 236 * k, size=(N, H, W, 1)) << shift).astype(npdt), dtype=dt)
    cshape = (2 * N, H // 2, W // 2, 1) if planar else (N, H // 2, W // 2, 2)
    c = capi.Tensor.from_numpy(ctx, (rng.integers(16 * k, 241 * k, size=cshape) << shift).astype(npdt), dtype=dt)
    t_new = capi.Tensor(ctx, N, OH, OW, Cc, dtype=odt)
    plan = capi.yuv_tensor_plan(ctx, N, H, W, OH, OW, Cc, dt, odt, maxval, shift, a.siting, a.range, filter="linear", means=means, norms=norms, alpha=1.0, planar=planar)
    forms = {"yuv_tensor": lambda: plan.run([y, c], t_new)}
    steps = {"yuv_tensor": [plan.describe()]}
    new_bytes = int(plan.cost()[1])
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()
    half_bytes = new_bytes // 2  # a copy of n bytes reads n and writes n: the launch's bytes, read + written, are 2 n
    src, dst = capi.Tensor(ctx, 1, 1, half_bytes, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, half_bytes, 1, dtype=capi.U8)

    def run_copy():
        rc = hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), half_bytes, stream)
        assert rc == 0, rc

    forms["copy"] = run_copy
    three_bytes = None
    if not wide:  # the composition of existing plans: an RGBA8 frame and a 4-channel float frame at the source size in between
        p1 = (capi.yuv_rgb_planar_plan if planar else capi.yuv_rgb_plan)(ctx, N, H // 2, W // 2, 4, 1, capi.U8, 255, 0, a.siting, a.range)
        p2 = capi.image_u8_plan(ctx, N, H, W, 4)
        p3 = capi.resize_plan(ctx, N, H, W, 4, OH, OW, means + (0.0,), norms + (1.0,), linear=True)
        rgba, f, t_old = capi.Tensor(ctx, N, H, W, 4, dtype=capi.U8), capi.Tensor(ctx, N, H, W, 4, dtype=odt), capi.Tensor(ctx, N, OH, OW, 4, dtype=odt)

        def run_three():
            p1.run([y, c], rgba)
            p2.run(rgba, f)
            p3.run(f, t_old)

        forms["three_launches"] = run_three
        steps["three_launches"] = [p.describe() for p in (p1, p2, p3)]
        three_bytes = int(sum(p.cost()[1] for p in (p1, p2, p3)))
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name in list(forms) + list(forms)[::-1]:  # mirrored, device events around `iters` enqueued runs
            timer.start()
            for _ in range(a.iters):
                forms[name]()
            timer.stop()
            dev[name].append(timer.elapsed_ms() / a.iters)

    def stat(v):
        m = statistics.median(v)
        return {"ms_median": round(m, 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5), "spread": round((max(v) - min(v)) / m, 4)}

    out = {"video": a.video, "frame": "%dx%d" % (H, W), "tensor": "%dx%dx%d %s" % (OH, OW, Cc, "f16" if a.half else "f32"), "batch": N, "rounds": a.rounds, "iters": a.iters,
           "timing": "device events around iters enqueued runs, the forms alternated in mirrored order", "steps": steps}
    for name in forms:
        out[name] = stat(dev[name])
    out["yuv_tensor"]["hbm_bytes"] = new_bytes
    out["yuv_tensor"]["tbs"] = round(new_bytes / (out["yuv_tensor"]["ms_median"] * 1e-3) / 1e12, 3)
    out["copy"]["hbm_bytes"] = 2 * half_bytes
    out["copy"]["tbs"] = round(2 * half_bytes / (out["copy"]["ms_median"] * 1e-3) / 1e12, 3)
    out["yuv_tensor_over_copy"] = round(out["yuv_tensor"]["ms_median"] / out["copy"]["ms_median"], 3)  # a finding, not a gate
    if three_bytes is not None:
        out["three_launches"]["hbm_bytes"] = three_bytes
        out["yuv_tensor_over_three_launches"] = round(out["yuv_tensor"]["ms_median"] / out["three_launches"]["ms_median"], 4)
        # the condition: the one launch takes no longer than the three, beyond the run's own spread
        out["condition_no_slower_than_three_launches"] = bool(out["yuv_tensor"]["ms_median"] <= out["three_launches"]["ms_median"] or
                                                              out["yuv_tensor"]["ms_min"] <= out["three_launches"]["ms_max"])
    capi.trace_begin()
    for _ in range(a.iters):
        forms["yuv_tensor"]()
    ctx.sync()
    rep = capi.trace_end()
    kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
    out["kernels"] = [{"function": it.get("function"), "launches": it.get("launches", 0),
                       "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]
    print(json.dumps(out, indent=1))
    if a.out:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        rec["%s_%dx%d_to_%dx%dx%d_%s_b%d" % (a.video.lower(), W, H, OW, OH, Cc, "f16" if a.half else "f32", N)] = out
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    ctx.close()


def main_tensor_yuv(a):
    """--encode NV12 | P010 | I420 [--half] [--batch N] [--h --w]: encoder frames behind an RGB model.  The tensor_yuv launch alone (a 0 .. 255 tensor of
    --h x --w x 3, 720p by default, to the frame's planes), a device copy of the launch's own bytes and the u8_out launch of the same tensor (the only
    device-side 8-bit end there was), in one process, alternated in mirrored order: device-event medians with spreads.  Then end to end with one
    frame's download, host clock: the launch + the planes (1.5 bytes per pixel, 3 for P010) against u8_out + the RGB8 frame and against the float
    tensor alone."""
    import ctypes
    import time

    import shadernn_amd as snn
    from shadernn_amd import capi

    snn.load_library()
    ctx = capi.Context(0)
    H, W, N, Cc = a.h or 720, a.w or 1280, a.batch, 3
    assert H % 2 == 0 and W % 2 == 0, "4:2:0 frames have even extents"
    planar, wide = a.encode == "I420", a.encode == "P010"
    dt, maxval, shift = (capi.U16, 1023, 6) if wide else (capi.U8, 255, 0)
    idt = capi.F16 if a.half else capi.F32
    rng = np.random.default_rng(1)
    src = capi.Tensor.from_numpy(ctx, rng.uniform(-10.0, 265.0, size=(N, H, W, Cc)).astype(np.float32), dtype=idt)
    scale = (maxval / 255.0,) * 3
    plan = capi.tensor_yuv_plan(ctx, N, H, W, Cc, idt, dt, maxval, shift, a.siting, a.range, scale=scale, planar=planar)
    luma = capi.Tensor(ctx, N, H, W, 1, dtype=dt)
    chroma = capi.Tensor(ctx, 2 * N if planar else N, H // 2, W // 2, 1 if planar else 2, dtype=dt)
    u8 = capi.u8_out_plan(ctx, N, H, W, Cc, dtype=idt)
    rgb8 = capi.Tensor(ctx, N, H, W, Cc, dtype=capi.U8)
    forms = {"tensor_yuv": lambda: plan.run_io([src], [luma, chroma]), "u8_out": lambda: u8.run(src, rgb8)}
    steps = {"tensor_yuv": [plan.describe()], "u8_out": [u8.describe()]}
    new_bytes = int(plan.cost()[1])
    hip = _hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctx.stream()
    half_bytes = new_bytes // 2  # a copy of n bytes reads n and writes n: the launch's bytes, read + written, are 2 n
    csrc, cdst = capi.Tensor(ctx, 1, 1, half_bytes, 1, dtype=capi.U8), capi.Tensor(ctx, 1, 1, half_bytes, 1, dtype=capi.U8)

    def run_copy():
        rc = hip.hipMemcpyDtoDAsync(cdst.data_ptr(), csrc.data_ptr(), half_bytes, stream)
        assert rc == 0, rc

    forms["copy"] = run_copy
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    ctx.sync()
    timer = capi.Timer(ctx)
    dev = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name in list(forms) + list(forms)[::-1]:  # mirrored, device events around `iters` enqueued runs
            timer.start()
            for _ in range(a.iters):
                forms[name]()
            timer.stop()
            dev[name].append(timer.elapsed_ms() / a.iters)

    def stat(v):
        m = statistics.median(v)
        return {"ms_median": round(m, 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5), "spread": round((max(v) - min(v)) / m, 4)}

    out = {"encode": a.encode, "tensor": "%dx%dx%d %s" % (H, W, Cc, "f16" if a.half else "f32"), "batch": N, "siting": a.siting, "range": a.range, "rounds": a.rounds, "iters": a.iters,
           "timing": "device events around iters enqueued runs, the forms alternated in mirrored order", "steps": steps}
    for name in forms:
        out[name] = stat(dev[name])
    out["tensor_yuv"]["hbm_bytes"] = new_bytes
    out["tensor_yuv"]["tbs"] = round(new_bytes / (out["tensor_yuv"]["ms_median"] * 1e-3) / 1e12, 3)
    out["copy"]["hbm_bytes"] = 2 * half_bytes
    out["copy"]["tbs"] = round(2 * half_bytes / (out["copy"]["ms_median"] * 1e-3) / 1e12, 3)
    out["u8_out"]["hbm_bytes"] = int(u8.cost()[1])
    out["u8_out"]["tbs"] = round(out["u8_out"]["hbm_bytes"] / (out["u8_out"]["ms_median"] * 1e-3) / 1e12, 3)
    out["tensor_yuv_rate_over_copy_rate"] = round(out["tensor_yuv"]["tbs"] / out["copy"]["tbs"], 3)  # a finding, not a gate: the launch's rate as a share of a device copy's
    out["tensor_yuv_over_u8_out"] = round(out["tensor_yuv"]["ms_median"] / out["u8_out"]["ms_median"], 3)

    # ---- end to end with one frame's download (pageable host memory, the host clock around launch + download; the download waits for the launch)
    def frame_yuv():
        plan.run_io([src], [luma, chroma])
        return (luma.numpy_u16(), chroma.numpy_u16()) if wide else (luma.numpy_u8(), chroma.numpy_u8())

    def frame_rgb8():
        u8.run(src, rgb8)
        return rgb8.numpy_u8()

    ends = {"tensor_yuv_and_planes": frame_yuv, "u8_out_and_rgb8": frame_rgb8, "float_tensor": src.numpy}
    for fn in ends.values():
        fn()
    host = {name: [] for name in ends}
    for _ in range(a.rounds):
        for name in list(ends) + list(ends)[::-1]:
            ctx.sync()
            t0 = time.perf_counter()
            ends[name]()
            host[name].append((time.perf_counter() - t0) * 1e3)
    es = np.dtype(np.uint16 if wide else np.uint8).itemsize
    d2h = {"tensor_yuv_and_planes": N * H * W * 3 // 2 * es, "u8_out_and_rgb8": N * H * W * Cc, "float_tensor": N * H * W * Cc * 4}  # (a half tensor downloads as floats)
    out["end_to_end"] = {"timing": "host clock around the launch and one download into pageable memory, alternated in mirrored order"}
    for name in ends:
        out["end_to_end"][name] = dict(stat(host[name]), d2h_bytes=d2h[name])
    out["end_to_end"]["planes_over_rgb8"] = round(out["end_to_end"]["tensor_yuv_and_planes"]["ms_median"] / out["end_to_end"]["u8_out_and_rgb8"]["ms_median"], 3)
    out["end_to_end"]["planes_over_float"] = round(out["end_to_end"]["tensor_yuv_and_planes"]["ms_median"] / out["end_to_end"]["float_tensor"]["ms_median"], 3)
    capi.trace_begin()
    for _ in range(a.iters):
        forms["tensor_yuv"]()
    ctx.sync()
    rep = capi.trace_end()
    kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
    out["kernels"] = [{"function": it.get("function"), "launches": it.get("launches", 0),
                       "us_per_launch": round(1e3 * it.get("total_ms", it.get("ms", 0.0)) / max(it.get("launches", 0), 1), 2)} for it in kernels]
    print(json.dumps(out, indent=1))
    if a.out:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
        rec["%s_%dx%dx%d_%s_b%d" % (a.encode.lower(), W, H, Cc, "f16" if a.half else "f32", N)] = out
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--half", action="store_true", help="the fp16 forms: fused fp32, per-layer fp16, fused fp16 (SNNHIP_ESPCN_F16=1), fused fp16 with 8-bit ends")
    ap.add_argument("--metrics", action="store_true", help="frame metrics on the device against a device copy and a download of the same frame (4K luma, NV12, RGB8); with --half also PSNR / SSIM of the fused fp16 chain's 8-bit output against the fused fp32 chain's")
    ap.add_argument("--widths", default="16,16", metavar="C1,C2", help="with --half: the ESPCN's channel widths; 64,32 is the net as published (per-layer fp16, fused fp16, fused fp16 with 8-bit ends)")
    ap.add_argument("--f16-mfma-tflops", type=float, default=2500.0, help="with --half: the f16 matrix peak the fused steps' issued MFMA flops are held against, TFLOP/s")
    ap.add_argument("--scale", type=int, default=2, choices=[2, 3, 4], help="upscale factor; the input size follows it (output 3840 x 2160) unless --h / --w are given")
    ap.add_argument("--bits", type=int, default=0, choices=[0, 10, 12, 16], help="also time 16-bit frames of this bit depth, folded and as separate launches")
    ap.add_argument("--colour", choices=["RGB8", "RGBA8"], default=None, help="colour frames around the luma chain: r8, colour, the merge launch alone and a device copy of its bytes")
    ap.add_argument("--video", choices=["NV12", "P010", "I420", "I010"], default=None, help="4:2:0 video frames around the luma chain: grey, video, the chroma launch alone, a device copy of its bytes and the RGB8 colour step")
    ap.add_argument("--out", default=None, metavar="FILE", help="with the planar forms: merge the record into this JSON file")
    ap.add_argument("--video-out", choices=["RGB8", "RGBA8", "NV12", "I420"], default=None,
                    help="with --video: packed RGB / RGBA out of the yuv_rgb launch (16-bit containers for P010) beside the NV12 step; NV12 with --colour: an NV12 frame out of the rgb_cbcr launch")
    ap.add_argument("--fit", default=None, metavar="WxH", help="with --video: the NV12 / P010 frame at this output size (the chain, then two plane_fit launches) beside the plain step of the same r")
    ap.add_argument("--rgb-fit", default=None, metavar="WxH", help="with --video NV12 | P010 | I420 --video-out RGB8 | RGBA8, or with --colour alone: the RGB frame at this output size "
                    "(the chain, the luma fit, rgb_fit) beside the r-fold RGB step of the same r; --out merges the record into a JSON file")
    ap.add_argument("--tensor", default=None, metavar="WxH", help="with --video NV12 | P010 | I420 alone: video in front of an RGB(A) model -- the yuv_tensor launch from a frame of "
                    "--h x --w (1080p by default) to the WxH x 4 input tensor (fp16 with --half), the three launches it replaces and a device copy of its bytes")
    ap.add_argument("--encode", choices=["NV12", "P010", "I420"], default=None, help="alone: encoder frames behind an RGB model -- the tensor_yuv launch from a --h x --w x 3 tensor "
                    "(720p by default, fp16 with --half), a device copy of its bytes, the u8_out launch of the same tensor, and end to end with one frame's download")
    ap.add_argument("--batch", type=int, default=1, help="with --tensor / --encode: frames per launch")
    ap.add_argument("--range", choices=["limited", "full"], default="limited", help="the stream's range with --video-out")
    ap.add_argument("--siting", choices=["left", "centre"], default="left", help="horizontal chroma siting of --video")
    ap.add_argument("--per-layer", action="store_true", help="also time the per-layer forms (always on for --scale 3 / 4)")
    ap.add_argument("--h", type=int, default=0)
    ap.add_argument("--w", type=int, default=0)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM roofline, TB/s")
    ap.add_argument("--mfma-tflops", type=float, default=157.3, help="fp32 matrix peak, TFLOP/s")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.metrics:
        return main_metrics(a)
    if a.encode:
        assert not a.video and not a.video_out and not a.colour and not a.fit and not a.rgb_fit and not a.tensor, "--encode goes alone (with --half, --batch, --h, --w, --siting, --range)"
        return main_tensor_yuv(a)
    if a.tensor:
        assert a.video in ("NV12", "P010", "I420") and not a.video_out and not a.colour and not a.fit and not a.rgb_fit, "--tensor goes with --video NV12 | P010 | I420 alone"
        return main_yuv_tensor(a)
    if a.rgb_fit:
        assert not a.fit and ((a.video in ("NV12", "P010", "I420") and a.video_out in ("RGB8", "RGBA8") and not a.colour) or (a.colour and not a.video and not a.video_out)), \
            "--rgb-fit goes with --video NV12 | P010 | I420 --video-out RGB8 | RGBA8, or with --colour RGB8 | RGBA8 alone"
        return main_rgb_fit(a)
    if a.video in ("I420", "I010") or a.video_out == "I420":
        assert (a.video_out == "I420") == bool(a.colour) and not (a.colour and a.video), "--video I420 | I010 [--video-out RGB8 | RGBA8] [--fit WxH], or --colour ... --video-out I420"
        assert not (a.fit and a.video_out), "--fit goes with --video alone"
        return main_planar(a)
    if a.video_out == "NV12":
        assert a.colour and not a.video, "--video-out NV12 goes with --colour RGB8 | RGBA8"
        return main_rgb_nv12(a)
    if a.fit:
        assert a.video and not a.video_out and not a.colour, "--fit goes with --video alone"
        return main_fit(a)
    if a.video and a.video_out:
        return main_video_rgb(a)
    if a.video:
        return main_video(a)
    if a.colour:
        return main_colour(a)
    if a.half:
        return main_half(a)

    import shadernn_amd as snn
    from shadernn_amd import capi, models
    from shadernn_amd.runner import _layer_plan

    snn.load_library()
    ctx = capi.Context(0)
    R = a.scale
    net = models.espcn_weights(seed=1, scale=R)
    H, W = a.h or 2160 // R, a.w or 3840 // R
    per_layer = a.per_layer or R != 2
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
    if per_layer:
        lshapes = [p.out_shape() for p in layers[:-1]]
        forms["f32_layers"] = dict(plan=Seq(layers, lshapes), x=capi.Tensor(ctx, 1, H, W, 1), y=capi.Tensor(ctx, *shape), xh=f32,
                                   yh=np.empty(shape, np.float32))
        forms["u8_layers"] = dict(plan=Seq([uin] + layers + [uout], [(1, H, W, 1)] + lshapes + [shape]), x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U8),
                                  y=capi.Tensor(ctx, *shape, dtype=capi.U8), xh=u8, yh=np.empty(shape, np.uint8))
    if a.bits:
        maxval = (1 << a.bits) - 1
        half = maxval / 2.0
        u16 = np.random.default_rng(2).integers(0, maxval + 1, size=(1, H, W, 1)).astype(np.uint16)
        win = capi.u16_in_plan(ctx, 1, H, W, 1, (half, 0, 0, 0), (1 / half, 1, 1, 1))
        wout = capi.u16_out_plan(ctx, *shape, (half, 0, 0, 0), (half, 0, 0, 0), maxval=maxval)
        forms["u16"] = dict(plan=capi.chain_plan(ctx, [win] + layers + [wout]), x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U16),
                            y=capi.Tensor(ctx, *shape, dtype=capi.U16), xh=u16, yh=np.empty(shape, np.uint16))
        forms["u16_sep"] = dict(plan=Seq([win, fchain, wout], [(1, H, W, 1), shape]), x=capi.Tensor(ctx, 1, H, W, 1, dtype=capi.U16),
                                y=capi.Tensor(ctx, *shape, dtype=capi.U16), xh=u16, yh=np.empty(shape, np.uint16))
        assert forms["u16"]["plan"].num_steps() == 2, forms["u16"]["plan"].describe()
    for f in forms.values():
        if f["x"].dtype == capi.U8:
            f["x"].upload_u8(f["xh"])
        elif f["x"].dtype == capi.U16:
            f["x"].upload_u16(f["xh"])
        else:
            f["x"].upload(f["xh"])

    def upload(f):
        if f["x"].dtype in (capi.U8, capi.U16):
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
    out = {"frame": "%dx%d -> %dx%d" % (H, W, R * H, R * W), "rounds": a.rounds, "iters": a.iters}
    for k, f in forms.items():
        d, e = statistics.median(dev[k]), statistics.median(e2e[k])
        out[k] = {"device_ms_median": round(d, 4), "device_ms_min": round(min(dev[k]), 4), "device_ms_max": round(max(dev[k]), 4),
                  "e2e_ms_median": round(e, 4), "e2e_frames_per_s": round(1e3 / e, 1),
                  "io_bytes_per_frame": int(f["xh"].nbytes + f["yh"].nbytes),
                  "steps": [f["plan"].step_describe(i) for i in range(f["plan"].num_steps())]}
    out["device_u8_over_f32"] = round(out["u8"]["device_ms_median"] / out["f32"]["device_ms_median"], 4)
    out["device_u8_over_u8_sep"] = round(out["u8"]["device_ms_median"] / out["u8_sep"]["device_ms_median"], 4)
    out["e2e_fps_u8_over_f32"] = round(out["u8"]["e2e_frames_per_s"] / out["f32"]["e2e_frames_per_s"], 4)
    if a.bits:
        out["scale"], out["bits"] = R, a.bits
        for k in forms:
            out[k]["device_spread"] = round((max(dev[k]) - min(dev[k])) / statistics.median(dev[k]), 4)
        out["device_u16_over_f32"] = round(out["u16"]["device_ms_median"] / out["f32"]["device_ms_median"], 4)
        out["device_u16_over_u8"] = round(out["u16"]["device_ms_median"] / out["u8"]["device_ms_median"], 4)
        out["device_u16_over_u16_sep"] = round(out["u16"]["device_ms_median"] / out["u16_sep"]["device_ms_median"], 4)
        out["e2e_fps_u16_over_f32"] = round(out["u16"]["e2e_frames_per_s"] / out["f32"]["e2e_frames_per_s"], 4)
        out["e2e_fps_u16_over_u8"] = round(out["u16"]["e2e_frames_per_s"] / out["u8"]["e2e_frames_per_s"], 4)
    if per_layer:
        out["scale"] = R
        for k in ("f32", "u8"):
            out["device_%s_fused_over_layers" % k] = round(out[k]["device_ms_median"] / out[k + "_layers"]["device_ms_median"], 4)
            # the spread between repeated regions of one form, as a fraction of its median: what a difference between forms has to exceed
            out["device_%s_spread" % k] = round(max((max(dev[j]) - min(dev[j])) / statistics.median(dev[j]) for j in (k, k + "_layers")), 4)
    traces = {}
    for k, f in forms.items():
        capi.trace_begin()
        for _ in range(a.iters):
            f["plan"].run(f["x"], f["y"])
        ctx.sync()
        rep = capi.trace_end()
        kernels = rep.get("kernels", rep) if isinstance(rep, dict) else rep
        traces[k] = [(item.get("function"), item.get("launches", 0), item.get("total_ms", item.get("ms", 0.0))) for item in kernels]
    if a.bits and not per_layer:
        for k in forms:
            out[k]["kernels"] = [{"function": name, "launches": n, "us_per_launch": round(1e3 * ms / max(n, 1), 2)} for name, n, ms in traces[k]]
    if per_layer:
        import re

        for k, f in forms.items():
            out[k]["kernels"] = [{"function": name, "launches": n, "us_per_launch": round(1e3 * ms / max(n, 1), 2)} for name, n, ms in traces[k]]
        for k in ("f32", "u8"):  # the fused chain: step i of the plan is kernel i of the trace's launch order; match by the kernel name in the description
            plan, roof = forms[k]["plan"], []
            for i in range(plan.num_steps()):
                desc = plan.step_describe(i)
                m = re.search(r"kernel=([A-Za-z0-9_]+)", desc)
                fl = re.search(r"mfma_flops=([0-9.e+]+)", desc)
                hit = [t for t in traces[k] if m and t[0] and t[0].split("<")[0].split("(")[0].strip().endswith(m.group(1))]
                if not hit:
                    continue
                us = 1e3 * hit[0][2] / max(hit[0][1], 1)
                _, nbytes = plan.step_cost(i)
                roof.append({"kernel": m.group(1), "us_per_launch": round(us, 2), "hbm_bytes": int(nbytes),
                             "hbm_fraction": round(nbytes / (us * 1e-6) / (a.hbm_tbs * 1e12), 4),
                             "mfma_fraction": round(float(fl.group(1)) / (us * 1e-6) / (a.mfma_tflops * 1e12), 4) if fl else None})
            out[k]["roofline"] = roof
    print(json.dumps(out, indent=1))
    for k in forms:
        print("launches (%s I/O), per-kernel time over %d steps:" % (k, a.iters))
        for name, n, ms in traces[k]:
            print("  %-48s launches=%-4d us/launch=%.2f" % (name, n, 1e3 * ms / max(n, 1)))
    ctx.close()


if __name__ == "__main__":
    main()
