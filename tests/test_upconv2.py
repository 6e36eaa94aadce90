"""The host side of conv2d_upconv2.hip (UpSampling2D x2 -> Conv2D 2x2 "same" as nine pre-summed GEMMs on the low-resolution tensor), no GPU needed:
snnhip_upconv2_presum_weights against the index rule of include/snnhip.h restated in NumPy, and its refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADS = [(0, 1, 0, 1), (1, 0, 1, 0), (1, 0, 0, 1), (0, 1, 1, 0)]  # (T, B, L, R): both placements per axis; the last two catch an x / y swap


def axis_entries(p):
    """Per axis with near pad p: e -> (phase, a, taps): output 2 m + phase, tap t reads low-resolution index m + floor((phase - p + t) / 2) = m - p + a."""
    pairs = sorted({(ph, (ph - p + t) // 2 + p) for ph in (0, 1) for t in (0, 1)})
    return [(ph, a, [t for t in (0, 1) if (ph - p + t) // 2 + p == a]) for ph, a in pairs]


def presum(w, pads):
    out = np.zeros((9,) + w.shape[:2], np.float32)
    for ey, (_, _, tys) in enumerate(axis_entries(pads[2])):      # rows are offset by padL ...
        for ex, (_, _, txs) in enumerate(axis_entries(pads[0])):  # ... columns by padT
            for ty in tys:
                for tx in txs:
                    out[3 * ey + ex] += w[:, :, ty, tx]
    return out


def test_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snnhip.h"), encoding="utf-8").read(), flags=re.S)
    assert re.search(r"\bsnnhip_upconv2_presum_weights\s*\(", header)
    assert hasattr(C.CDLL(snn.load_library()), "snnhip_upconv2_presum_weights") and "snnhip_upconv2_presum_weights" in capi.SIGNATURES


@pytest.mark.parametrize("pads", PADS)
def test_presummed_matrices_follow_the_index_rule(built, pads):
    from shadernn_amd import capi

    w = np.random.default_rng(sum(pads[:3])).standard_normal((5, 7, 2, 2)).astype(np.float32)
    got = capi.upconv2_presum_weights(w, pads)
    assert [len(axis_entries(p)) for p in (0, 1)] == [3, 3]
    np.testing.assert_array_equal(got, presum(w, pads))
    # a constant input: the matrices of a phase, summed, are the plain convolution's interior value
    for ey, (py, _, _) in enumerate(axis_entries(pads[2])):
        for ex, (px, _, _) in enumerate(axis_entries(pads[0])):
            phase = [3 * fy + fx for fy, (qy, _, _) in enumerate(axis_entries(pads[2])) for fx, (qx, _, _) in enumerate(axis_entries(pads[0])) if (qy, qx) == (py, px)]
            np.testing.assert_allclose(got[phase].sum(axis=(0, 2)), w.sum(axis=(1, 2, 3)), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape,stride,pads", [((4, 4, 3, 3), 1, (0, 1, 0, 1)), ((4, 4, 2, 2), 2, (0, 1, 0, 1)), ((4, 4, 2, 2), 1, (1, 1, 1, 1)),
                                               ((4, 4, 2, 2), 1, (0, 0, 0, 0)), ((4, 4, 2, 2), 1, (0, 1, 1, 1))])
def test_other_layers_are_refused(built, shape, stride, pads):
    from shadernn_amd import capi

    with pytest.raises(capi.SnnHipError) as e:
        capi.upconv2_presum_weights(np.zeros(shape, np.float32), pads, stride=stride)
    assert e.value.code == -1 and "upconv2_presum_weights" in str(e.value)
