"""The host side of the fp16 ESPCN rules (espcn_f16.hip), no GPU needed: the lane-ordered fp16 weight images for v_mfma_f32_16x16x32_f16 /
_16x16x16_f16 against a numpy restatement of the operand layout, and the depth-to-space row mapping 4*dy + dx <-> r*dy + dx."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row_channel(r, row):
    dy, dx = row >> 2, row & 3
    return r * dy + dx if (dy < r and dx < r) else -1


def _gemm_from_image(img, n_rows=16):
    """Undo the packing the way the matrix core reads it: lane l of K-step s supplies A[row l % 16][k = 32 s + 8 (l / 16) + j], j = 0..7; the last step
    (16x16x16) A[row l % 16][k = 128 + 4 (l / 16) + j], j = 0..3.  Returns A [16][144] with K ordered tap-major, channel-minor (k = 16 tap + ic)."""
    A = np.full((n_rows, 144), np.nan, np.float32)
    for s in range(4):
        for lane in range(64):
            for j in range(8):
                A[lane % 16, 32 * s + 8 * (lane // 16) + j] = img[(s * 64 + lane) * 8 + j]
    for lane in range(64):
        for j in range(4):
            A[lane % 16, 128 + 4 * (lane // 16) + j] = img[2048 + lane * 4 + j]
    return A


@pytest.mark.parametrize("r", [0, 2, 3, 4])
def test_3x3_weight_image_is_the_gemm_operand_in_lane_order(built, r):
    from shadernn_amd import capi

    oc = 16 if r == 0 else r * r
    w = np.random.default_rng(r).standard_normal((oc, 16, 3, 3)).astype(np.float32)
    img = capi.espcn_f16_pack_weights(w, r)
    assert img.dtype == np.float16 and img.shape == (2304,)
    A = _gemm_from_image(img.astype(np.float32))
    assert not np.isnan(A).any()  # every (row, k) is supplied exactly once: 4 * 64 * 8 + 64 * 4 = 16 * 144
    wh = w.astype(np.float16).astype(np.float32)  # round to nearest even, as the fp16 convolution plans convert
    for row in range(16):
        ch = row if r == 0 else _row_channel(r, row)
        want = np.zeros(144, np.float32) if ch < 0 else wh[ch].transpose(1, 2, 0).reshape(9, 16).reshape(-1)  # [tap][ic]
        np.testing.assert_array_equal(A[row], want, err_msg="row %d" % row)


@pytest.mark.parametrize("r", [2, 3, 4])
def test_row_mapping_puts_an_output_row_run_into_one_lane(r):
    """Row 4*dy + dx <-> channel r*dy + dx: a bijection between the channels and the rows with dy, dx < r, and the four accumulator registers of lane
    group g (rows 4g .. 4g+3) are the r horizontally adjacent output pixels (dx = 0 .. r-1) of output row r*y + g."""
    rows = [row for row in range(16) if _row_channel(r, row) >= 0]
    assert sorted(_row_channel(r, row) for row in rows) == list(range(r * r))
    for g in range(4):
        chans = [_row_channel(r, 4 * g + reg) for reg in range(4)]
        if g < r:
            assert chans[:r] == [r * g + dx for dx in range(r)] and all(c < 0 for c in chans[r:])  # depth-to-space: channel r*dy + dx -> (r*y + dy, r*x + dx)
        else:
            assert all(c < 0 for c in chans)


@pytest.mark.parametrize("k", [3, 5])
def test_first_convolution_image_pads_its_taps_to_one_k_step(built, k):
    from shadernn_amd import capi

    w = np.random.default_rng(k).standard_normal((16, 1, k, k)).astype(np.float32)
    img = capi.espcn_f16_pack_weights(w).astype(np.float32)
    assert img.shape == (512,)
    A = np.empty((16, 32), np.float32)
    for lane in range(64):
        A[lane % 16, 8 * (lane // 16): 8 * (lane // 16) + 8] = img[lane * 8: lane * 8 + 8]
    wh = w.astype(np.float16).astype(np.float32).reshape(16, k * k)
    np.testing.assert_array_equal(A[:, : k * k], wh)
    np.testing.assert_array_equal(A[:, k * k:], 0.0)


def test_bad_arguments_are_refused(built):
    from shadernn_amd import capi

    for w, r in ((np.zeros((16, 16, 3, 3), np.float32), 5), (np.zeros((16, 16, 3, 3), np.float32), 1), (np.zeros((16, 1, 7, 7), np.float32), 0),
                 (np.zeros((16, 8, 3, 3), np.float32), 0)):
        with pytest.raises(capi.SnnHipError) as e:
            capi.espcn_f16_pack_weights(w, r)
        assert e.value.code == -1


def test_tile_constants_are_stated_in_the_header():
    txt = open(os.path.join(ROOT, "shadernn_amd", "csrc", "espcn_f16.h")).read()
    t = {k: int(re.search(r"\b%s = (\d+)" % k, txt).group(1)) for k in ("kEspcnF16TW_A", "kEspcnF16TH_A", "kEspcnF16TW_B", "kEspcnF16TH_B")}
    assert t["kEspcnF16TW_A"] % 16 == 0 and t["kEspcnF16TH_A"] % 4 == 0  # whole 16-pixel groups, whole rows per wave
    assert (t["kEspcnF16TW_B"], t["kEspcnF16TH_B"]) == (32, 8)
