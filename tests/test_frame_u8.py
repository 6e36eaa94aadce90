"""CPU-side checks of the 8-bit frame interface: declared in the C-ABI header, exported, bound in Python, built, documented."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("snnhip_u8_in_plan_create", "snnhip_u8_out_plan_create", "snnhip_tensor_download_raw")


def test_frame_u8_symbols_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi

    header = open(os.path.join(ROOT, "include", "snnhip.h")).read()
    lib = ctypes.CDLL(snn.load_library())
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
    assert "clamp(rint(fmaf(x, scale[c], offset[c])), 0, 255)" in header
    assert ctypes.sizeof(capi.U8InDesc) == ctypes.sizeof(capi.U8OutDesc) == 5 * 4 + 8 * 4


def test_frame_u8_kernels_are_built_and_documented():
    import __graft_entry__ as g

    assert "frame_u8.hip" in g.HIP_SOURCES
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("Rule A8", "Rule B8", "conv_kxk_c1o16_wino3x3_c16o16_u8_kernel", "conv3x3_c16o4_d2s_tanh_u8_kernel"):
        assert word in design, word
    assert "tools/bench_frames.py" in open(os.path.join(ROOT, "README.md")).read()
