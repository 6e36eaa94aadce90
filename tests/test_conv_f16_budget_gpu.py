"""The fp16 convolution kernels behind snnhip_conv2d_plan_create held to their contract -- half storage, products of half operands accumulated in fp32, an
fp32 epilogue, ONE round-to-nearest-even store: conv2d_mfma's f16 instances (three block widths, split-K, the LDS-transposed and the direct store),
conv2d_thin's f16 instance, conv2d_wide_f16, conv2d_widep_f16, conv2d_stem_f16, conv2d_rowfold's tile kernel and conv2d_rowmarch, conv2d_s2march and the
f16 form of conv1x1_stream, with the fused residual Add (chain rule E) and the fused reflect Pad (rule D) -- each pinned by its switch at the edges of its
own tile, against the float64 reference of tests/ref64.py on the half-rounded inputs and weights.  Two half operands multiply exactly in fp32, so such a
kernel stores the correctly rounded half of the exact result except within its fp32 accumulation error of a rounding tie: ref64.budget_half allows
ref64.M_F16 times the distance of a pairwise fp32 evaluation from float64 beyond half an ulp, about 1 % of an ulp, where the 4e-3 tests of these kernels
allow four ulps at unit scale and thirty at 0.1.  Output tensors start as NaN.  Every test prints one line
"BUDGET16 family | case | description | ratio mismatch% per-channel"."""
import functools
import re

import numpy as np
import pytest

import oracle_lib as O
import ref64
from test_conv_budget_gpu import LEAKY, _free
from test_ops_gpu import _bn, _rand

pytestmark = pytest.mark.gpu

MFMA, THIN, WIDE, WIDEP = "conv2d_mfma_f16_32x32x16 k=", "conv2d_thin_mfma_f16_4x4x4", "conv2d_mfma_wide_f16_32x32x16 k=3x3", "conv2d_mfma_wide_f16_32x32x16 persistent"
STEM, ROWFOLD, MARCH, STREAM = "conv2d_mfma_stem_f16_32x32x16 k=9x9", "conv2d_rowfold_mfma_f16_32x32x16", "row-marching", "stream: wave = 32px"
S2MARCH = re.compile(r"^conv2d_mfma_f16_32x32x16 k=3x3 s=2 ic=\d+ oc=\d+ row-marching strips=")
DIRECT = re.compile(r"^conv2d_mfma_f16_32x32x16 k=\S+ s=\d ic=\d+ oc=\d+ tile=\d+x\d+x\d+px x \d+oc (chunk=\d+|tap-pairs) lds=\d+B splitK=\d+")


def case(family, shape, act="", bn=False, mode="constant", padding="same", env=None, expect=(), add=False, prepad=0, tag=""):
    """One case, as in tests/test_conv_budget_gpu.py: the layer (N, H, W, IC, OC, k, stride), its epilogue, the switches that pin the kernel and what the
    plan's description must say ("!text": must not say).  prepad = p: a reflect Pad of p pixels in front of a "valid" convolution (chain rule D)."""
    layer = (tuple(shape), act, bool(bn), mode, "valid" if prepad else padding, bool(add), int(prepad))
    name = "x".join(map(str, shape)) + "".join("_" + t for t in (act, "bn" if bn else "", mode if mode != "constant" else "", padding if padding != "same" and not prepad else "",
                                                                  "add" if add else "", "pad%d" % prepad if prepad else "", tag) if t)
    return pytest.param(family, layer, dict(env or {}), tuple(expect), id=family + "-" + name)


M_, T_, W_, S2_ = ({"SNNHIP_CONV": v} for v in ("mfma", "thin", "wide", "s2march"))
W0 = dict(W_, SNNHIP_WIDE_PERSIST="0")  # the block-per-tile kernel also where IC = OC = 128
S1 = {"SNNHIP_CONV_1X1": "2"}           # the stream kernel also on few-tile deep-K layers
ST = {}                                 # the stem kernel has no switch that forces it on: it is the planner's choice for 9x9 stride 1, IC <= 4, OC % 32 == 0
RT = {"SNNHIP_ROWFOLD": "tile"}         # conv2d_rowfold's tile kernel where the row-marching form would take the layer (OC <= 4)
RM = {}                                 # ... and the row-marching form is the planner's choice for OC <= 4 at every size


def _mfma(bn=None, split=None, **more):
    e = dict(M_, **more)
    if bn:
        e["SNNHIP_CONV_BN"] = str(bn)
    if split:
        e["SNNHIP_CONV_SPLITK"] = str(split)
    return e


def _widep(grid, blocks):
    return (dict(W_, SNNHIP_WIDEP_GRID=str(grid)) if grid else dict(W_)), ([WIDEP, "blocks=%d " % blocks] if grid else [WIDEP])


def _widep_cases():
    out = []
    # (N, H, W), tiles of 8 x 32 pixels, epilogue (the persistent kernel implements none / relu; every other activation goes back to conv2d_wide_kernel)
    # the four shapes of the listing in the three pad modes, and the second one once more as "valid": no border offsets in the halo path, which is how the
    # style graphs reach this kernel (a "valid" convolution behind a reflect Pad); that Pad fused in front (chain rule D) follows the loop
    for (n, h, w), kw in (((1, 8, 32), dict(act="relu")), ((2, 19, 45), dict(act="relu", bn=True, mode="reflect")), ((4, 5, 7), dict(bn=True, mode="replicate")), ((1, 8, 300), dict()),
                          ((2, 19, 45), dict(act="relu", padding="valid"))):
        oh, ow = (h - 2, w - 2) if kw.get("padding") == "valid" else (h, w)
        tiles = n * ((oh + 7) // 8) * ((ow + 31) // 32)
        for grid in (0, 1, 3, 7):
            env, expect = _widep(grid, min(grid, tiles))
            out.append(case("widep", (n, h, w, 128, 128, 3, 1), env=env, expect=expect, tag="grid%s" % (grid or "auto"), **kw))
    env, expect = _widep(3, 3)
    out.append(case("widep", (2, 9, 33, 128, 128, 3, 1), "relu", prepad=1, env=env, expect=expect + ["+pad(reflect)"], tag="grid3"))
    return out


CASES = [
    # ---- conv2d_mfma, f16 instances: 128-pixel tiles x 32 / 64 / 128 output channels, 32-channel chunks (16 behind a stride-2 halo, 8 for IC <= 8)
    case("mfma", (2, 17, 23, 32, 48, 3, 1), env=_mfma(bn=32), expect=[MFMA, "px x 32oc"], tag="bn32"),                      # OC not a multiple of the block, at the three widths
    case("mfma", (2, 17, 23, 32, 48, 3, 1), env=_mfma(bn=64), expect=[MFMA, "px x 64oc"], tag="bn64"),
    case("mfma", (2, 17, 23, 32, 48, 3, 1), env=_mfma(bn=128), expect=[MFMA, "px x 128oc"], tag="bn128"),
    case("mfma", (1, 9, 9, 40, 40, 3, 1), "leakyRelu", bn=True, env=M_, expect=[MFMA, "ic=40 oc=40"]),                      # IC % 16 = 8, OC % 32 = 8
    case("mfma", (2, 9, 11, 20, 33, 3, 1), "tanh", mode="reflect", env=M_, expect=[MFMA, "ic=20 oc=33"]),                   # OC % 8 != 0: the direct store, IC % 8 = 4
    case("mfma", (1, 8, 8, 10, 16, 5, 1), "sigmoid", bn=True, mode="replicate", env=M_, expect=[MFMA, "k=5x5"]),            # below a tile
    case("mfma", (2, 15, 17, 64, 64, 3, 2), "relu", bn=True, mode="replicate", env=M_, expect=[MFMA, "s=2"]),               # stride 2, odd extents
    case("mfma", (3, 7, 7, 256, 96, 1, 1), "relu6", env=dict(M_, SNNHIP_CONV_1X1="0"), expect=[MFMA, "k=1x1"]),             # several images per pixel tile, the last one ragged
    case("mfma", (1, 16, 8, 32, 32, 3, 1), env=M_, expect=[MFMA, re.compile(r"tile=1x\d+x\d+px")]),                         # one exact 128-pixel tile
    case("mfma", (2, 12, 20, 64, 96, 3, 1), "sigmoid", padding="valid", env=M_, expect=[MFMA]),                             # Q20: pads 0, the unshrunk extent
    # K = 4608: the split over K must keep fp32 partials (workspace + reduce pass)
    case("mfma", (2, 7, 7, 512, 128, 3, 1), env=_mfma(split=1), expect=[MFMA, "splitK=1"], tag="split1"),
    case("mfma", (2, 7, 7, 512, 128, 3, 1), env=_mfma(split=2), expect=[MFMA, "splitK=2"], tag="split2"),
    case("mfma", (2, 7, 7, 512, 128, 3, 1), env=_mfma(split=4), expect=[MFMA, "splitK=4"], tag="split4"),
    case("mfma", (2, 7, 7, 512, 128, 3, 1), env=_mfma(split=8), expect=[MFMA, "splitK=8"], tag="split8"),
    case("mfma", (2, 19, 21, 64, 64, 3, 1), bn=True, add=True, env=M_, expect=[MFMA, "splitK=1", "+add"]),                  # the fused residual Add + relu (chain rule E)
    case("mfma", (2, 7, 7, 512, 128, 3, 1), bn=True, add=True, env=_mfma(split=4), expect=[MFMA, "splitK=4", "+add"], tag="split4"),  # ... and in the reduce pass
    case("mfma", (2, 19, 21, 64, 64, 3, 1), bn=True, add=True, env=_mfma(SNNHIP_CONV_DIRECT_STORE="1"), expect=[MFMA, "splitK=1", "+add"], tag="direct"),  # ... in the direct store, by its switch
    case("mfma", (2, 9, 11, 20, 33, 3, 1), add=True, env=M_, expect=[MFMA, "oc=33", "splitK=1", "+add"]),                   # ... and where OC % 8 != 0 takes it
    # ---- conv2d_thin, f16 instance (OC <= 4; the row-fold kernels take k >= 5 with 16 / 32 input channels first: pinned)
    case("thin", (1, 16, 32, 16, 4, 3, 1), env=T_, expect=[THIN, "tile=32x"]),                                              # an exact tile
    case("thin", (2, 17, 33, 24, 3, 5, 1), "leakyRelu", bn=True, mode="reflect", env=T_, expect=[THIN, "k=5x5"]),            # one pixel over on both axes
    case("thin", (1, 5, 7, 40, 1, 3, 1), "sigmoid", mode="replicate", env=T_, expect=[THIN, "ic=40 oc=1"]),                  # below a tile
    case("thin", (2, 9, 20, 16, 2, 3, 1), "relu", padding="valid", env=T_, expect=[THIN]),
    # ---- conv2d_wide_f16: 8 x 32 or 16 x 32 pixel tiles x 128 / 64 / 32 output channels
    case("wide", (1, 8, 32, 32, 128, 3, 1), "relu", env=W_, expect=[WIDE, "!persistent"]),                                  # one exact 8 x 32 tile
    case("wide", (2, 19, 45, 64, 128, 3, 1), "tanh", bn=True, mode="reflect", env=W_, expect=[WIDE, "x 128oc"]),
    case("wide", (1, 9, 33, 16, 128, 3, 1), "relu6", mode="replicate", env=W_, expect=[WIDE, "chunk=16"]),                   # one pixel over on both axes, a 16-channel chunk
    case("wide", (1, 33, 35, 48, 64, 3, 1), "leakyRelu", bn=True, env=W_, expect=[WIDE, "ic=48 oc=64"]),                     # IC % 32 = 16
    case("wide", (3, 7, 9, 16, 96, 3, 1), "sigmoid", env=W_, expect=[WIDE, "oc=96"]),                                       # below a tile, several images, OC = 3 x 32
    case("wide", (1, 21, 50, 32, 128, 3, 1), "relu", padding="valid", env=dict(W_, SNNHIP_WIDE_BN="128"), expect=[WIDE, "x 128oc"], tag="bn128"),
    case("wide", (1, 21, 50, 32, 128, 3, 1), "relu", padding="valid", env=dict(W_, SNNHIP_WIDE_BN="64"), expect=[WIDE, "x 64oc"], tag="bn64"),
    case("wide", (1, 21, 50, 32, 128, 3, 1), "relu", padding="valid", env=dict(W_, SNNHIP_WIDE_BN="32"), expect=[WIDE, "x 32oc"], tag="bn32"),
    case("wide", (1, 8, 32, 256, 256, 3, 1), bn=True, env=W_, expect=[WIDE, "ic=256 oc=256"]),                              # K = 2304, two output-channel blocks
    case("wide", (2, 9, 33, 128, 128, 3, 1), "relu", env=W0, expect=[WIDE, "!persistent"], tag="nopersist"),                 # the layer of the persistent kernel, block per tile
    case("wide", (2, 13, 21, 64, 64, 3, 1), add=True, env=W_, expect=[WIDE, "+add"]),                                       # the fused residual Add + relu (chain rule E)
    case("wide", (2, 13, 21, 32, 64, 3, 1), "relu", prepad=1, env=W_, expect=[WIDE, "+pad(reflect)"]),                      # the fused reflect Pad (chain rule D)
    # ---- conv2d_widep_f16 (128 -> 128): one tile, ragged in both directions, a map narrower than a tile over several images, a long row of tiles; grids
    # of 1, 3 and 7 resident blocks, whose runs of tiles cross image boundaries
    *_widep_cases(),
    # ---- conv2d_stem_f16 (9x9, IC <= 4): 8 x 32 pixel tiles, persistent blocks
    case("stem", (1, 40, 50, 3, 32, 9, 1), "relu", env=ST, expect=[STEM, "ic=3 oc=32"]),
    case("stem", (3, 5, 7, 3, 32, 9, 1), "tanh", bn=True, mode="reflect", env=ST, expect=[STEM]),                            # below a tile (and narrower than the kernel), several images
    case("stem", (1, 9, 70, 1, 32, 9, 1), mode="replicate", env=ST, expect=[STEM, "ic=1"]),                                 # one pixel over in the rows
    case("stem", (1, 64, 64, 4, 64, 9, 1), "leakyRelu", bn=True, env=ST, expect=[STEM, "ic=4 oc=64"]),                      # exact tiles, two output-channel blocks
    case("stem", (1, 8, 32, 3, 32, 9, 1), "sigmoid", padding="valid", env=ST, expect=[STEM]),                               # one exact tile
    # ---- conv2d_rowfold's tile kernel (k * OC <= 32, IC = 16 / 32) ...
    case("rowfold", (1, 33, 61, 32, 3, 9, 1), "tanh", bn=True, mode="reflect", env=RT, expect=[ROWFOLD, "tile=", "!" + MARCH]),
    case("rowfold", (2, 20, 130, 16, 4, 7, 1), "relu", bn=True, mode="replicate", env=RT, expect=[ROWFOLD, "tile=", "!" + MARCH]),
    case("rowfold", (1, 17, 19, 32, 6, 5, 1), "sigmoid", env=RT, expect=[ROWFOLD, "tile=", "!" + MARCH]),                    # OC = 6: the tile kernel is the only form
    case("rowfold", (3, 9, 9, 16, 1, 9, 1), env=RT, expect=[ROWFOLD, "tile=", "!" + MARCH]),
    case("rowfold", (1, 75, 57, 16, 4, 7, 1), "leakyRelu", bn=True, env=RT, expect=[ROWFOLD, "tile=", "!" + MARCH]),        # (SNNHIP_ROWFOLD_SEGS belongs to the marching form: not set)
    case("rowfold", (1, 9, 64, 32, 2, 5, 1), padding="valid", env=RT, expect=[ROWFOLD, "tile=", "k=5x5", "!" + MARCH]),
    case("rowfold", (1, 12, 30, 32, 3, 9, 1), "relu6", padding="valid", env=RT, expect=[ROWFOLD, "tile=", "!" + MARCH]),
    case("rowfold", (2, 14, 26, 32, 3, 9, 1), prepad=4, env=RT, expect=[ROWFOLD, "tile=", "+pad(reflect)", "!" + MARCH]),    # the fused reflect Pad (chain rule D)
    # ---- ... and conv2d_rowmarch (OC <= 4): strips of rows, several segments per strip
    case("rowmarch", (1, 33, 61, 32, 3, 9, 1), "tanh", bn=True, mode="reflect", env=RM, expect=[ROWFOLD, MARCH]),
    case("rowmarch", (2, 20, 130, 16, 4, 7, 1), "relu", bn=True, mode="replicate", env=RM, expect=[ROWFOLD, MARCH]),
    case("rowmarch", (3, 9, 9, 16, 1, 9, 1), env=RM, expect=[ROWFOLD, MARCH]),
    case("rowmarch", (1, 75, 57, 16, 4, 7, 1), "leakyRelu", bn=True, env={"SNNHIP_ROWFOLD_SEGS": "2"}, expect=[ROWFOLD, MARCH, "segments=2 x"], tag="segs2"),
    case("rowmarch", (1, 9, 64, 32, 2, 5, 1), padding="valid", env=RM, expect=[ROWFOLD, MARCH, "k=5x5"]),
    case("rowmarch", (2, 14, 26, 32, 3, 9, 1), prepad=4, env=RM, expect=[ROWFOLD, MARCH, "+pad(reflect)"]),
    # ---- conv2d_s2march (3x3 stride 2, IC = 32 / 64): strips of 32 columns, 64 / 128 output channels per block
    case("s2march", (2, 9, 9, 32, 64, 3, 2), env=S2_, expect=[S2MARCH]),
    case("s2march", (1, 21, 130, 32, 128, 3, 2), "leakyRelu", bn=True, mode="replicate", env=S2_, expect=[S2MARCH, "oc=128"]),
    case("s2march", (2, 33, 61, 64, 128, 3, 2), "relu", mode="reflect", env=dict(S2_, SNNHIP_S2MARCH_SEGS="2"), expect=[S2MARCH, "segments=2 x"], tag="segs2"),
    case("s2march", (1, 50, 37, 64, 256, 3, 2), "tanh", bn=True, env=dict(S2_, SNNHIP_S2MARCH_SEGS="3"), expect=[S2MARCH, "segments=3 x"], tag="segs3"),
    case("s2march", (1, 16, 64, 32, 64, 3, 2), "relu6", padding="valid", env=S2_, expect=[S2MARCH]),
    # ---- conv1x1_stream, f16 form: a wave = 32 pixels x 32 / 64 / 96 output channels, 16-channel chunks
    case("stream", (1, 9, 9, 8, 16, 1, 1), "leakyRelu", bn=True, env=S1, expect=[MFMA, STREAM]),                            # half a chunk, half a column
    case("stream", (1, 19, 21, 144, 32, 1, 1), bn=True, env=S1, expect=[MFMA, STREAM, "ic=144"]),
    case("stream", (2, 14, 14, 96, 24, 1, 1), "relu6", env=S1, expect=[MFMA, STREAM, "oc=24"]),
    case("stream", (2, 27, 31, 64, 128, 1, 2), "sigmoid", bn=True, env=S1, expect=[MFMA, STREAM, "k=1x1 s=2"]),
    case("stream", (1, 12, 12, 200, 64, 1, 1), "tanh", env=S1, expect=[MFMA, STREAM, "ic=200"]),                            # IC % 16 = 8
    case("stream", (1, 12, 12, 64, 96, 1, 1), "relu", env=dict(S1, SNNHIP_CONV_1X1_NT="1"), expect=[STREAM + " x 32oc"], tag="nt1"),
    case("stream", (1, 12, 12, 64, 96, 1, 1), "relu", env=dict(S1, SNNHIP_CONV_1X1_NT="2"), expect=[STREAM + " x 64oc"], tag="nt2"),
    case("stream", (1, 12, 12, 64, 96, 1, 1), "relu", env=dict(S1, SNNHIP_CONV_1X1_NT="3"), expect=[STREAM + " x 96oc"], tag="nt3"),
    case("stream", (2, 14, 14, 144, 24, 1, 1), bn=True, add=True, env=S1, expect=[STREAM, "+add"]),                          # the fused residual Add + relu (chain rule E)
]

# One deep case per family (the deepest reduction its shapes admit) for the second run.
DEEP = [
    case("mfma", (2, 7, 7, 512, 128, 3, 1), env=_mfma(split=4), expect=[MFMA, "splitK=4"], tag="split4"),
    case("thin", (1, 7, 9, 256, 4, 3, 1), env=T_, expect=[THIN]),
    case("wide", (1, 8, 32, 256, 256, 3, 1), bn=True, env=W_, expect=[WIDE, "ic=256 oc=256"]),
    case("widep", (2, 19, 45, 128, 128, 3, 1), "relu", bn=True, mode="reflect", env=_widep(3, 3)[0], expect=_widep(3, 3)[1], tag="grid3"),
    case("stem", (1, 64, 64, 4, 64, 9, 1), "leakyRelu", bn=True, env=ST, expect=[STEM, "ic=4 oc=64"]),
    case("rowfold", (1, 33, 61, 32, 3, 9, 1), "tanh", bn=True, mode="reflect", env=RT, expect=[ROWFOLD, "tile=", "!" + MARCH]),
    case("rowmarch", (1, 33, 61, 32, 3, 9, 1), "tanh", bn=True, mode="reflect", env=RM, expect=[ROWFOLD, MARCH]),
    case("s2march", (2, 33, 61, 64, 128, 3, 2), "relu", mode="reflect", env=dict(S2_, SNNHIP_S2MARCH_SEGS="2"), expect=[S2MARCH, "segments=2 x"], tag="segs2"),
    case("stream", (1, 12, 12, 200, 64, 1, 1), "tanh", env=S1, expect=[MFMA, STREAM, "ic=200"]),
]

# What the planner chooses with no switch set, one small shape per family.  conv2d_wide_f16, conv2d_widep_f16 and conv2d_s2march are its choice on large maps
# only (from about one tile per CU on: tests/test_conv_wide_gpu.py::test_wide_is_the_default_on_large_maps_only pins that with plans it does not run against a
# reference), conv2d_thin's f16 instance gets what the row-fold kernels decline, and conv2d_rowfold's tile kernel the row-fold layers with more than four
# output channels.
ROUTES = [
    case("mfma", (1, 12, 20, 32, 32, 5, 1), "relu", expect=[DIRECT]),
    case("thin", (1, 16, 32, 16, 4, 3, 1), expect=[THIN]),
    case("stem", (1, 9, 70, 3, 32, 9, 1), "relu", expect=[STEM]),
    case("rowfold", (1, 17, 19, 32, 6, 5, 1), "sigmoid", expect=[ROWFOLD, "tile=", "!" + MARCH]),
    case("rowmarch", (1, 16, 20, 32, 3, 9, 1), "tanh", expect=[ROWFOLD, MARCH]),
    case("stream", (2, 14, 14, 96, 24, 1, 1), "relu6", expect=[MFMA, STREAM]),
]

# conv2d_mfma's f16 switches that change how a result is stored or how the loop is compiled, never what is computed: bit-identical to the default.  The
# last two entries: what the default's description and the switched one must say.  The plan's description prints the staging geometry, so it shows
# SNNHIP_CONV_WIDE_CHUNKS; the store path and the loop form are not in it, and there the bit-identity is all that is asserted of the switch.
SWITCHES = [
    ("SNNHIP_CONV_DIRECT_STORE", case("mfma", (2, 17, 23, 32, 48, 3, 1), "relu", bn=True, env=M_, expect=[MFMA]), (), ()),  # no LDS transpose of the output tile
    ("SNNHIP_CONV_ROLLED", case("mfma", (1, 9, 9, 40, 40, 3, 1), "leakyRelu", bn=True, env=M_, expect=[MFMA]), (), ()),     # the run-time tap loop instead of the unrolled 3x3
    ("SNNHIP_CONV_WIDE_CHUNKS", case("mfma", (2, 15, 17, 64, 64, 3, 2), "relu", bn=True, mode="replicate", env=M_, expect=[MFMA, "s=2"]),  # 32-channel chunks behind a stride-2 halo, the K steps in the default's order
     ("chunk=16",), ("chunk=32",)),
]


def _h(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def _geometry(layer):
    """(pads, (OH, OW), the extent the convolution reads): behind a fused Pad the convolution is "valid" on the padded extent and keeps it (Q20)."""
    (n, h, w, ic, oc, k, s), act, bn, mode, padding, add, prepad = layer
    h, w = h + 2 * prepad, w + 2 * prepad
    pads = O.padding_offsets(padding, k)
    return pads, (O.out_dim(h, k, s, pads[0], pads[1]), O.out_dim(w, k, s, pads[0], pads[1])), (h, w)


@functools.lru_cache(maxsize=None)
def _refs(layer):
    """(x, w, bias, bn, residual, float64 reference, pairwise fp32) of one layer: x, w and the residual rounded to half before anything reads them, bias and BN
    fp32; computed once, shared by the cases that run it, read-only."""
    (n, h, w, ic, oc, k, s), act, bn, mode, padding, add, prepad = layer
    x, wt, b = _h(_rand((n, h, w, ic), 31)), _h(_rand((oc, ic, k, k), 32, 1.0 / np.sqrt(k * k * ic))), _rand((oc,), 33, 0.1)
    bnp = _bn(oc, 34) if bn else None
    pads, out_hw, _ = _geometry(layer)
    xin = np.pad(x, ((0, 0), (prepad, prepad), (prepad, prepad), (0, 0)), mode="reflect") if prepad else x  # (copies of halves: nothing rounded)
    y64 = ref64.conv_layer_general(xin, wt, b, s, pads, mode, out_hw, bnp, act, LEAKY)
    y32 = ref64.conv_layer_pairwise32(xin, wt, b, s, pads, mode, out_hw, bnp, act, LEAKY)
    res = None
    if add:  # conv -> Add(residual) -> relu in one launch with one store: nothing is rounded between the convolution and the sum
        res = _h(_rand(y32.shape, 35))
        y64, y32 = ref64.activation("relu", y64 + res.astype(np.float64)), ref64.activation32("relu", y32 + res)
    assert y64.dtype == np.float64 and y32.dtype == np.float32
    for a in (x, wt, b, res, y64, y32):
        if a is not None:
            a.setflags(write=False)
    return x, wt, b, bnp, res, y64, y32


def _plan(ctx, monkeypatch, layer, env):
    """The plan through the public binding, the switches set around plan creation only (a fused Pad / Add re-plans the convolution: inside too)."""
    import shadernn_amd as snn

    (n, h, w, ic, oc, k, s), act, bn, mode, padding, add, prepad = layer
    x, wt, b, bnp, res, y64, y32 = _refs(layer)
    pads, (oh, ow), (ch, cw) = _geometry(layer)
    with monkeypatch.context() as m:
        for name, value in env.items():
            m.setenv(name, value)
        plan = snn.conv2d_plan(ctx, n, ch, cw, wt, b, stride=s, pads=pads, pad_mode=mode, act=act, leaky=LEAKY, bn=bnp, dtype=snn.F16)
        assert plan.out_shape() == (n, oh, ow, oc), (plan.out_shape(), plan.describe())
        if prepad:
            plan = snn.chain_plan(ctx, [snn.pad_plan(ctx, n, h, w, ic, (prepad,) * 4, "reflect"), plan])
        if add:
            plan = snn.chain_plan(ctx, [plan, snn.add_plan(ctx, n, oh, ow, oc, act="relu")])
    assert plan.num_steps() <= 1, plan.describe()
    return plan


def _run(ctx, plan, layer):
    """One run on half tensors into an output that starts as NaN, so that an element no block writes cannot pass on stale data."""
    import shadernn_amd as snn

    x, wt, b, bnp, res, y64, y32 = _refs(layer)
    ins = [snn.Tensor.from_numpy(ctx, a, dtype=snn.F16) for a in ((x, res) if res is not None else (x,))]
    yt = snn.Tensor.from_numpy(ctx, np.full(y64.shape, np.nan, np.float32), dtype=snn.F16)
    assert np.isnan(yt.numpy()).all()
    plan.run(ins if len(ins) > 1 else ins[0], yt)
    y = yt.numpy()
    for t in ins + [yt]:
        t.free()
    return y


def _tile(desc):
    """(TH, TW) in output pixels where the description prints the pixel tile."""
    for pat, th, tw in ((r"tile=\d+x(\d+)x(\d+)px", 1, 2), (r"tile=(\d+)x(\d+)px", 1, 2), (r"conv2d_thin\S+ .* tile=(\d+)x(\d+) ", 2, 1)):
        m = re.search(pat, desc)
        if m:
            return int(m.group(th)), int(m.group(tw))
    return None


def _check_description(desc, expect, family):
    assert "f16" in desc, desc
    body = desc.replace("chain{", "")
    for e in expect:
        if hasattr(e, "search"):
            assert e.search(body), "%s: expected %r in %s" % (family, e.pattern, desc)
        elif e.startswith("!"):
            assert e[1:] not in desc, "%s: %r must not be in %s" % (family, e[1:], desc)
        else:
            assert e in desc, "%s: expected %r in %s" % (family, e, desc)
    if family == "mfma":  # the direct kernel, not one of the kernels that share its prefix
        assert DIRECT.search(body) and "stream" not in desc and MARCH not in desc, desc


def _report(family, request, desc, figures):
    print("BUDGET16 %s | %s | %s | %.2f %.3f%% %.4f" % (family, request.node.callspec.id, desc, figures[0], 100 * figures[1], figures[2]))


def _figures_then_assert(got, y64, y32, desc):
    """budget_half at M_F16; a run over it still prints its figures."""
    try:
        return ref64.budget_half(got, y64, y32, ref64.M_F16, what=desc, tile=_tile(desc))
    except AssertionError as e:
        print("BUDGET16-FAIL %s" % e)
        raise


def _one(ctx, monkeypatch, layer, env, expect, family, runs=1):
    plan = _plan(ctx, monkeypatch, layer, env)
    desc = plan.describe()
    try:
        _check_description(desc, expect, family)
        return desc, [_run(ctx, plan, layer) for _ in range(runs)]
    finally:
        _free(plan)


@pytest.mark.parametrize("family,layer,env,expect", CASES)
def test_f16_kernel_within_the_half_budget(ctx, monkeypatch, request, family, layer, env, expect):
    x, wt, b, bnp, res, y64, y32 = _refs(layer)
    desc, (got,) = _one(ctx, monkeypatch, layer, env, expect, family)
    _report(family, request, desc, _figures_then_assert(got, y64, y32, desc))


@pytest.mark.parametrize("family,layer,env,expect", DEEP)
def test_f16_deep_reduction_is_repeatable(ctx, monkeypatch, request, family, layer, env, expect):
    """A second run through the same plan is bit-identical: the split-K reduce pass, the persistent blocks' runs of tiles and the strips' row rings have a
    fixed order, and nothing is left over from the first run."""
    x, wt, b, bnp, res, y64, y32 = _refs(layer)
    desc, (got, again) = _one(ctx, monkeypatch, layer, env, expect, family, runs=2)
    _report(family, request, desc, _figures_then_assert(got, y64, y32, desc))
    np.testing.assert_array_equal(got, again, err_msg="second run differs: " + desc)


@pytest.mark.parametrize("family,layer,env,expect", ROUTES)
def test_the_planners_own_f16_choice_is_within_the_budget(ctx, monkeypatch, request, family, layer, env, expect):
    """No switch set: what users get.  The description names the family, the result is inside the same budget."""
    for name in ("SNNHIP_CONV", "SNNHIP_CONV_1X1", "SNNHIP_CONV_BN", "SNNHIP_CONV_SPLITK", "SNNHIP_CONV_STEM", "SNNHIP_CONV_WIDE", "SNNHIP_CONV_S2MARCH", "SNNHIP_ROWFOLD",
                 "SNNHIP_ROWFOLD_SEGS", "SNNHIP_WIDE_PERSIST", "SNNHIP_WIDE_BN", "SNNHIP_WIDEP_GRID"):
        monkeypatch.delenv(name, raising=False)
    assert env == {}
    x, wt, b, bnp, res, y64, y32 = _refs(layer)
    desc, (got,) = _one(ctx, monkeypatch, layer, env, expect, family)
    _report(family, request, desc, _figures_then_assert(got, y64, y32, desc))


@pytest.mark.parametrize("switch,param,says0,says1", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_f16_mfma_switch_is_bit_identical_and_within_the_budget(ctx, monkeypatch, request, switch, param, says0, says1):
    """Each switch on a layer where it changes the kernel that runs, inside the budget and bit-identical to the default.  SNNHIP_CONV_WIDE_CHUNKS keeps
    32-channel chunks behind a stride-2 halo, where the default stages 16-channel ones (chunk=32 lds=88264B against chunk=16 lds=44232B here): its K steps
    run half by half, every tap of a 16-channel half, which is the default's (chunk, tap) order -- the same MFMAs in the same order."""
    family, layer, env, expect = param.values
    x, wt, b, bnp, res, y64, y32 = _refs(layer)
    desc0, (base,) = _one(ctx, monkeypatch, layer, env, expect, family)
    desc, (got,) = _one(ctx, monkeypatch, layer, dict(env, **{switch: "1"}), expect, family)
    print("BUDGET16-SWITCH %s | %s | %s" % (switch, desc0, desc))
    for text in says0:
        assert text in desc0 and text not in desc, "%s=1: %r belongs to the default only: %s vs %s" % (switch, text, desc0, desc)
    for text in says1:
        assert text in desc and text not in desc0, "%s=1 did not change the kernel: expected %r in %s only (default %s)" % (switch, text, desc, desc0)
    _report(family, request, desc, _figures_then_assert(got, y64, y32, desc))
    np.testing.assert_array_equal(got, base, err_msg="%s=1 changes the result: %s vs %s" % (switch, desc, desc0))
