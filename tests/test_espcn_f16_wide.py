"""The host side of the fp16 ESPCN rules at the published widths 1 -> 64 -> 32 -> r*r (espcn_f16_wide.hip), no GPU needed: the lane-ordered fp16
weight images for v_mfma_f32_16x16x32_f16 against a numpy restatement of the operand layout, the refusals of the packing entry point, the header's tile
constants, and models.espcn_weights' new `widths` argument leaving the default net what it was."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1, C2 = 64, 32


def _row_channel(r, row):
    dy, dx = row >> 2, row & 3
    return r * dy + dx if (dy < r and dx < r) else -1


def _gemm_from_image(img, ic, rows):
    """Undo the packing the way the matrix core reads it: in K-step ks, lane l supplies A[row 16 mb + l % 16][k = 32 ks + 8 (l / 16) + j], j = 0..7, for
    row block mb.  A K-step is one tap and 32 channels (ks = tap * ic/32 + channel block), so k = ic * tap + channel: K tap-major, channel-minor.
    Returns (A [rows][9 ic], how often each element was supplied)."""
    kc, mbs = ic // 32, rows // 16
    A = np.full((rows, 9 * ic), np.nan, np.float32)
    hits = np.zeros((rows, 9 * ic), np.int32)
    for ks in range(9 * kc):
        for mb in range(mbs):
            for lane in range(64):
                for j in range(8):
                    row, k = 16 * mb + lane % 16, 32 * ks + 8 * (lane // 16) + j
                    A[row, k] = img[((ks * mbs + mb) * 64 + lane) * 8 + j]
                    hits[row, k] += 1
    return A, hits


@pytest.mark.parametrize("r", [0, 2, 3, 4])
def test_3x3_weight_images_are_the_gemm_operand_in_lane_order(built, r):
    from shadernn_amd import capi

    oc, ic, rows = (C2, C1, C2) if r == 0 else (r * r, C2, 16)
    w = np.random.default_rng(r).standard_normal((oc, ic, 3, 3)).astype(np.float32)
    img = capi.espcn_f16_wide_pack_weights(w, r)
    assert img.dtype == np.float16 and img.shape == (9 * ic * rows,)
    A, hits = _gemm_from_image(img.astype(np.float32), ic, rows)
    assert (hits == 1).all() and not np.isnan(A).any()  # every (row, k) is supplied exactly once
    wh = w.astype(np.float16).astype(np.float32)  # round to nearest even, as the fp16 convolution plans convert
    for row in range(rows):
        ch = row if r == 0 else _row_channel(r, row)
        want = np.zeros(9 * ic, np.float32) if ch < 0 else wh[ch].transpose(1, 2, 0).reshape(-1)  # [tap][ic]
        np.testing.assert_array_equal(A[row], want, err_msg="row %d" % row)


@pytest.mark.parametrize("k", [3, 5])
def test_first_convolution_image_is_64_rows_of_one_k_step(built, k):
    from shadernn_amd import capi

    w = np.random.default_rng(k).standard_normal((C1, 1, k, k)).astype(np.float32)
    img = capi.espcn_f16_wide_pack_weights(w).astype(np.float32)
    assert img.shape == (C1 * 32,)
    A = np.full((C1, 32), np.nan, np.float32)
    hits = np.zeros((C1, 32), np.int32)
    for mb in range(C1 // 16):
        for lane in range(64):
            for j in range(8):
                A[16 * mb + lane % 16, 8 * (lane // 16) + j] = img[(mb * 64 + lane) * 8 + j]
                hits[16 * mb + lane % 16, 8 * (lane // 16) + j] += 1
    assert (hits == 1).all()
    wh = w.astype(np.float16).astype(np.float32).reshape(C1, k * k)
    np.testing.assert_array_equal(A[:, : k * k], wh)
    np.testing.assert_array_equal(A[:, k * k:], 0.0)


@pytest.mark.parametrize("shape,r", [((16, 1, 5, 5), 0), ((64, 1, 7, 7), 0), ((32, 16, 3, 3), 0), ((16, 64, 3, 3), 0), ((32, 32, 3, 3), 0), ((64, 64, 3, 3), 0),
                                     ((1, 32, 3, 3), 1), ((25, 32, 3, 3), 5), ((4, 32, 3, 3), 3), ((4, 16, 3, 3), 2), ((4, 64, 3, 3), 2), ((4, 32, 5, 5), 2),
                                     ((64, 1, 5, 5), 2)])
def test_bad_arguments_are_refused(built, shape, r):
    from shadernn_amd import capi

    with pytest.raises(capi.SnnHipError) as e:
        capi.espcn_f16_wide_pack_weights(np.zeros(shape, np.float32), r)
    assert e.value.code == -1


def test_the_narrow_entry_point_still_refuses_the_wide_shapes(built):
    from shadernn_amd import capi

    for shape in ((32, 64, 3, 3), (4, 32, 3, 3)):
        with pytest.raises(capi.SnnHipError) as e:
            capi.espcn_f16_pack_weights(np.zeros(shape, np.float32), 0 if shape[0] == 32 else 2)
        assert e.value.code == -1


def test_tile_constants_satisfy_what_the_kernels_assert():
    txt = open(os.path.join(ROOT, "shadernn_amd", "csrc", "espcn_f16_wide.h")).read()
    t = {k: int(re.search(r"\b%s = (\d+)" % k, txt).group(1))
         for k in ("kEspcnF16WideC1", "kEspcnF16WideC2", "kEspcnF16WideTW_A", "kEspcnF16WideTH_A", "kEspcnF16WideTW_B", "kEspcnF16WideTH_B")}
    assert (t["kEspcnF16WideC1"], t["kEspcnF16WideC2"]) == (C1, C2)
    assert t["kEspcnF16WideC1"] % 32 == 0 and t["kEspcnF16WideC2"] % 32 == 0  # a K-step is one tap and 32 channels, in both kernels
    assert t["kEspcnF16WideTW_A"] % 16 == 0 and t["kEspcnF16WideTH_A"] % 4 == 0  # whole 16-pixel groups, whole rows per wave
    assert (t["kEspcnF16WideTW_B"], t["kEspcnF16WideTH_B"]) == (32, 8)
    # kernel A's static LDS: the conv1 tile and the largest (5x5) input tile, as halfs, under 64 KB
    tw, th = t["kEspcnF16WideTW_A"], t["kEspcnF16WideTH_A"]
    assert ((th + 2) * (tw + 2) * C1 + (th + 6) * (tw + 6)) * 2 <= 65536


def _swizzled_unit(c_channels, col, slot):
    """The 16-byte bank unit (of the 16 that one LDS cycle serves) of logical slot `slot` of the pixel at tile column `col` (espcn_f16_wide.hip)."""
    if c_channels == 64:
        return (8 * col + (slot ^ (((col >> 1) & 3) << 1))) % 16
    return (4 * col + (slot ^ (((col >> 2) & 1) << 1))) % 16


@pytest.mark.parametrize("c_channels", [64, 32])
def test_the_slot_swizzle_is_conflict_free_for_every_tap(c_channels):
    """ds_read_b128 is served in four lane groups; in K-step (tap, channel block) lane (px = lane % 16, g = lane / 16) reads slot 4*block + g of the pixel
    at column px + fx.  Every group must touch 16 distinct units.  (A row step moves every lane by the same number of bytes.)"""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in grp] for grp in groups]
    for fx in range(3):
        for half in range(2):  # the second 16-pixel group of a tile row
            for block in range(c_channels // 32):
                for grp in groups:
                    units = {_swizzled_unit(c_channels, 16 * half + lane % 16 + fx, 4 * block + lane // 16) for lane in grp}
                    assert len(units) == 16, (fx, half, block, grp)


@pytest.mark.parametrize("r", [2, 3, 4])
def test_default_widths_return_the_net_that_was_always_returned(r):
    from shadernn_amd import models

    a, b = models.espcn_weights(seed=1, scale=r), models.espcn_weights(seed=1, scale=r, widths=(16, 16))
    assert a["name"] == b["name"] and len(a["layers"]) == len(b["layers"]) == 4
    for la, lb in zip(a["layers"], b["layers"]):
        assert sorted(la) == sorted(lb)
        for key in la:
            if isinstance(la[key], np.ndarray):
                np.testing.assert_array_equal(la[key], lb[key])
            else:
                assert la[key] == lb[key], key
    wide = models.espcn_weights(seed=1, scale=r, widths=(64, 32))
    assert [l["w"].shape for l in wide["layers"][:3]] == [(64, 1, 5, 5), (32, 64, 3, 3), (r * r, 32, 3, 3)]
    assert [l["name"] for l in wide["layers"]] == [l["name"] for l in a["layers"]]
