"""CPU tests of the camera backbone's backward: its C entries are declared, exported and bound (as tests/test_host.py
checks the others), and the three opt-in switches exist and default to off."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("isf_swin_window_attention_backward", "isf_swin_window_attention_backward_groups",
           "isf_swin_layernorm_backward", "isf_swin_layernorm_backward_parts", "isf_swin_gelu_backward",
           "isf_swin_column_sums", "isf_swin_column_sums_parts", "isf_swin_scale_rows", "isf_swin_operand_rows")


def test_backward_entries_are_declared_exported_and_bound():
    from isfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "isf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(isf_[a-z0-9_]+)\s*\(", code))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        # the parameter count of the declaration is the binding's
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # each entry's comment says which reference lines it differentiates
    block = hdr[hdr.index("Backward of the Swin-T backbone"):hdr.index("int isf_swin_operand_rows")]
    for name in ("isf_swin_window_attention_backward", "isf_swin_layernorm_backward", "isf_swin_gelu_backward",
                 "isf_swin_column_sums", "isf_swin_scale_rows", "isf_swin_operand_rows"):
        entry = block[block.index(" * " + name):]
        entry = entry[:re.search(r"\n \* isf_|\Z", entry[3:]).start() + 3]
        assert re.search(r"(swin|transformer)\.py:\d+|mmcv FFN", entry), name
    # workspace sizes are host arithmetic: no device needed
    assert lib.isf_swin_layernorm_backward_parts(0) == 0 and lib.isf_swin_layernorm_backward_parts(105) % 4 == 0
    assert lib.isf_swin_column_sums_parts(1) == 1
    assert lib.isf_swin_window_attention_backward_groups(2, 9, 10, 3) == 8          # 2 images x 2 x 2 windows
    assert 0 < lib.isf_swin_window_attention_backward_groups(12, 96, 264, 3) <= 1024 // 3


def test_backward_switches_default_to_off():
    from isfusion_amd.detector import ISFusionDetector
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    from isfusion_amd.swin import SwinTransformer
    sig = inspect.signature(SwinTransformer.forward_train)
    assert sig.parameters["backward"].default is False
    assert list(sig.parameters)[:3] == ["self", "x", "drop_keep"] and sig.parameters["drop_keep"].default is None
    sig = inspect.signature(GeneralizedLSSFPN.forward_train)
    assert sig.parameters["input_grads"].default is False
    assert ISFusionDetector.camera_backward is False
    assert "camera_backward" not in inspect.signature(ISFusionDetector.__init__).parameters


def test_no_float_atomics_in_the_backward():
    """DESIGN.md section 4.0g counts the float-atomic sites of csrc/: the backbone's backward adds none"""
    src = open(os.path.join(ROOT, "is-fusion_amd", "csrc", "isf_swin_train.hip")).read()
    src = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"atomic", src, flags=re.I)
