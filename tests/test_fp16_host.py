"""The fp16 data path's host side (no GPU): the C ABI names its element type and entry points, the ctypes table types them,
and the precision switch rejects what it does not know."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Entry points that versions 2-8 of the ABI spelled once per element type (suffixes _x, _xs, _bf16, _f16, _f32x, _f32x3, _taps);
# version 9 has one per operation and takes the type as an E2FGVI_* argument.
REMOVED = ("e2fgvi_conv2d_bf16x", "e2fgvi_conv2d_f16x", "e2fgvi_conv2d_f32x", "e2fgvi_conv2d_f32x3",
           "e2fgvi_packed_conv_weight_bf16x_size", "e2fgvi_pack_conv_weight_bf16x", "e2fgvi_packed_conv_weight_bf16x_taps_size",
           "e2fgvi_pack_conv_weight_bf16x_taps", "e2fgvi_packed_conv_weight_f16x_size", "e2fgvi_pack_conv_weight_f16x",
           "e2fgvi_packed_conv_weight_f16x_taps_size", "e2fgvi_pack_conv_weight_f16x_taps", "e2fgvi_packed_conv_weight_f32x_size",
           "e2fgvi_pack_conv_weight_f32x", "e2fgvi_packed_conv_weight_f32x_taps_size", "e2fgvi_pack_conv_weight_f32x_taps",
           "e2fgvi_packed_conv_weight_f32x3_size", "e2fgvi_pack_conv_weight_f32x3", "e2fgvi_packed_conv_weight_f32x3_taps_size",
           "e2fgvi_pack_conv_weight_f32x3_taps", "e2fgvi_pack_dcn_weight_bf16", "e2fgvi_pack_dcn_weight_f16", "e2fgvi_pack_dcn_weight_x3",
           "e2fgvi_focal_attention_bf16", "e2fgvi_focal_attention_f16", "e2fgvi_focal_attention_bf16_variant",
           "e2fgvi_nchw_to_nhwc_x", "e2fgvi_resize_bilinear_bf16", "e2fgvi_resize_bilinear_f16", "e2fgvi_prop_cond_x",
           "e2fgvi_prop_cond_xs", "e2fgvi_spynet_level_input_x", "e2fgvi_spynet_level_input_x_f16", "e2fgvi_layernorm_x",
           "e2fgvi_window_pool_x", "e2fgvi_ffn_fold_x", "e2fgvi_ffn_unfold_gelu_x", "e2fgvi_ffn_fold_gelu_x", "e2fgvi_ffn_unfold_x",
           "e2fgvi_ffn_unfold_gelu", "e2fgvi_softcomp_fold_bf16", "e2fgvi_softcomp_fold_f16")
# consolidated entry point -> (the arguments of the form it replaces, int32 arguments added to them).  Letters: p pointer,
# i int32, l int64, f float, a int32 array, d descriptor.  The replaced form is the bf16 one (for e2fgvi_resize_bilinear the
# fp32 one, whose NCHW / affine arguments stay); those that took their `_x` / `_xs` signature over unchanged add nothing, the
# weight packers of the LDS-DMA convolution add `mode` and `tap_packed`.
CONSOLIDATED = {
    "e2fgvi_nchw_to_nhwc": ("ppiiiiiiffp", 0),
    "e2fgvi_spynet_level_input": ("ppppppiiip", 1),
    "e2fgvi_prop_cond": ("pipiipplpippiiiip", 0),
    "e2fgvi_layernorm": ("ppppilip", 0),
    "e2fgvi_window_pool": ("pipppiiiip", 0),
    "e2fgvi_ffn_fold": ("ppiiiiiiip", 1),
    "e2fgvi_ffn_unfold": ("ppiiiiiiip", 1),
    "e2fgvi_softcomp_fold": ("ppppiiiiiip", 1),
    "e2fgvi_resize_bilinear": ("piipiiiiiiiippp", 1),
    "e2fgvi_focal_attention_16": ("pppippiiiip", 1),
    "e2fgvi_packed_dcn_weight_size": ("iiii", 1),
    "e2fgvi_pack_dcn_weight": ("ppiiiiip", 1),
    "e2fgvi_conv2d_x": ("dp", 1),
    "e2fgvi_packed_conv_weight_x_size": ("iiiiia", 2),
    "e2fgvi_pack_conv_weight_x": ("ppiiiiiap", 2),
}


def _header():
    with open(os.path.join(ROOT, "include", "e2fgvi_hip.h")) as f:
        return f.read()


def test_header_defines_the_fp16_element_type():
    m = re.search(r"^#define E2FGVI_F16 (\d+)", _header(), re.M)
    assert m and int(m.group(1)) == 3
    from e2fgvi_amd import lib
    assert lib.DT_F16 == 3 and lib.DT_BF16 == 1 and lib.DT_F32 == 0


def _letters(argtypes):
    import ctypes as C
    from e2fgvi_amd import lib
    code = {C.c_void_p: "p", C.c_int32: "i", C.c_int64: "l", C.c_float: "f", C.POINTER(C.c_int32): "a", C.POINTER(lib.ConvXDesc): "d"}
    return "".join(code[a] for a in argtypes)


def test_f16_entry_points_are_declared_and_typed_like_their_bf16_siblings():
    """fp16 is served by the entry points that serve bf16: one declaration per operation, the element type an argument"""
    from e2fgvi_amd import lib
    h = _header()
    for name in REMOVED:
        assert not re.search(r"\b%s\b" % name, h), name + " is still named in the header"
        assert name not in lib.SYMBOLS, name + " is still in the ctypes table"
    for name, (old, added) in CONSOLIDATED.items():
        assert len(re.findall(r"^(?:int|int64_t) %s\(" % name, h, re.M)) == 1, name + " must be declared exactly once"
        new = _letters(lib.SYMBOLS[name][1])
        assert new.count("i") == old.count("i") + added, (name, new, old)
        assert all(new.count(c) == old.count(c) for c in "plfad"), (name, new, old)
    assert "e2fgvi_focal_attention_16_variant" in lib.SYMBOLS


def test_one_size_function_serves_every_element_type():
    """the packed-weight sizes through the consolidated size functions: fp16 takes the bf16 packing, the split-operand packing is
    three planes of the fp32 geometry, an unknown element code is refused (size functions only: nothing is launched)"""
    import ctypes
    from e2fgvi_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    L = lib.load()
    F32, BF16, X3, F16 = lib.DT_F32, lib.DT_BF16, lib.DT_BF16X3, lib.DT_F16
    assert (F32, BF16, X3, F16) == tuple(int(re.search(r"^#define E2FGVI_%s (\d+)" % n, _header(), re.M).group(1))
                                         for n in ("F32", "BF16", "BF16X3", "F16"))
    # (tap_packed, Cout, groups, KH, KW, cpg): the tap-packed layers of test_host_logic and one plain layer of two sources
    for taps, cout, groups, kh, kw, cpg in ((1, 512, 1, 7, 7, [40]), (1, 32, 1, 7, 7, [8]), (1, 64, 1, 3, 3, [24]),
                                            (0, 128, 1, 3, 3, [128, 128])):
        arr = (ctypes.c_int32 * len(cpg))(*cpg)

        def size(mode):
            return L.e2fgvi_packed_conv_weight_x_size(mode, taps, cout, groups, kh, kw, len(cpg), arr)
        assert size(BF16) > 0 and size(F32) > 0
        assert size(F16) == size(BF16)
        assert size(X3) == 3 * size(F32)
        assert size(7) < 0
        assert b"E2FGVI_F16" in L.e2fgvi_last_error()            # the message names the accepted codes
    n32 = L.e2fgvi_packed_dcn_weight_size(F32, 128, 256, 3, 3)
    assert n32 > 0
    assert L.e2fgvi_packed_dcn_weight_size(X3, 128, 256, 3, 3) == 3 * n32
    assert L.e2fgvi_packed_dcn_weight_size(BF16, 128, 256, 3, 3) == n32
    assert L.e2fgvi_packed_dcn_weight_size(F16, 128, 256, 3, 3) == n32


@pytest.mark.parametrize("bad", ["half", "float16", "FP16", "bfloat16", "", None])
def test_a_bad_precision_string_raises_value_error(bad):
    from e2fgvi_amd.engine import Engine
    with pytest.raises(ValueError):
        Engine({}, "e2fgvi", "cpu", precision=bad)
