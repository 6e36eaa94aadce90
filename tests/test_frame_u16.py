"""CPU-side checks of the 16-bit frame interface: declared in the C-ABI header, exported, bound in Python, built, documented."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("snnhip_u16_in_plan_create", "snnhip_u16_out_plan_create")


def test_frame_u16_symbols_are_declared_exported_and_bound(built):
    import shadernn_amd as snn
    from shadernn_amd import capi

    header = open(os.path.join(ROOT, "include", "snnhip.h")).read()
    assert "SNNHIP_U16 = 3" in header
    lib = ctypes.CDLL(snn.load_library())
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
    # the contract is written once, in the header
    assert "y = (float(u >> shift) - means[c]) * norms[c]" in header
    assert "q = unsigned(clamp(rint(fmaf(x, scale[c], offset[c])), 0, maxval)) << shift" in header
    assert capi.U16 == 3 and snn.U16 == 3
    assert ctypes.sizeof(capi.U16InDesc) == (5 + 8 + 1) * 4
    assert ctypes.sizeof(capi.U16OutDesc) == (5 + 8 + 2) * 4
    # the 8-bit descs keep their layout
    assert ctypes.sizeof(capi.U8InDesc) == ctypes.sizeof(capi.U8OutDesc) == (5 + 8) * 4


def test_frame_u16_host_symbols_are_declared_exported_and_bound(built):
    from shadernn_amd import host

    header = open(os.path.join(ROOT, "include", "snn_c.h")).read()
    lib = host.lib()
    for name in ("snn_model_create6", "snn_model_upload_frame_u16", "snn_model_download_frame_u16"):
        assert name + "(" in header, name
        assert hasattr(lib, name), name
    for word in ("SNN_IO_R16", "SNN_IO_RGB16", "SNN_IO_RGBA16", "snn_frame_io2"):
        assert word in header, word
    # a new struct: snn_frame_io keeps its 18 dwords (growing it would break the callers of snn_model_create5)
    assert ctypes.sizeof(host.FrameIO) == 18 * 4 and ctypes.sizeof(host.FrameIO2) == 21 * 4
    assert host.FRAME_FORMATS["R16"] & 0xFF == 1 and host.FRAME_FORMATS["RGB16"] & 0xFF == 3 and host.FRAME_FORMATS["RGBA16"] & 0xFF == 4
    color = open(os.path.join(ROOT, "shadernn_amd", "host", "snn", "color.h")).read()
    assert "R8, RGB8, RGBA8, R16, RGB16, RGBA16 }" in color  # appended: the existing enumerators keep their values


def test_frame_u16_kernels_are_built_and_documented():
    import __graft_entry__ as g

    assert "frame_u16.hip" in g.HIP_SOURCES and "frame_u8.hip" in g.HIP_SOURCES
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("4.12", "u16_in_kernel", "u16_out_kernel", "quantize_u16", "SNNHIP_U16", "conv_kxk_c1o16_wino3x3_c16o16_u16_kernel", "conv3x3_c16o4_d2s_tanh_u16_kernel",
                 "conv3x3_c16oR_d2s_tanh_u16_kernel", "espcn_f16_conv_pair_u16_kernel", "espcn_f16_d2s_u16_kernel", "U16InCfg", "U16OutCfg", "--save-temps"):
        assert word in design, word
    epilogue = open(os.path.join(ROOT, "shadernn_amd", "csrc", "epilogue.h")).read()
    assert "unsigned quantize_u16(float x, float scale, float offset, float maxval)" in epilogue
    assert "SNNHIP_U16" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "frame_u16.hip" in open(os.path.join(ROOT, "README.md")).read()
