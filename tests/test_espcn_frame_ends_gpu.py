"""The chain planner's descriptions of the ESPCN chain, with and without 8- / 16-bit frame ends, against tests/golden/espcn_chain_descriptions.json,
which was written on an MI355X at the commit before one FrameIn / FrameOut description replaced the per-family frame-end plumbing
(tests/golden/make_espcn_chain_descriptions.py: r in {2, 3, 4}, k1 in {3, 5}, ends in {none, in, out, both}, bits in {8, 16}, the fp32 default, the
direct kernel A, the Winograd kernel B, the narrow and the wide fp16 kernels, and rule C for its step count and the conversion steps).  The kernel
names in these strings are what tests and launch traces read, so they stay byte for byte.  Plan creation only; the bit-identical runs are
tests/test_frame_u8_gpu.py, tests/test_frame_u16_gpu.py and tests/test_espcn_f16*_gpu.py."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_chain_descriptions_are_the_stored_ones(ctx):
    sys.path.insert(0, GOLDEN)
    import make_espcn_chain_descriptions as M

    with open(os.path.join(GOLDEN, "espcn_chain_descriptions.json")) as f:
        want = json.load(f)
    assert len(want) == len(M.FAMILIES) * 3 * 2 * 4 * 2
    got = M.chain_descriptions(ctx)
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        assert got[case] == want[case], case
