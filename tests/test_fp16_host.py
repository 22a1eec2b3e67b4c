"""The fp16 data path's host side (no GPU): the C ABI names its element type and entry points, the ctypes table types them,
and the precision switch rejects what it does not know."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_SYMBOLS = ("e2fgvi_conv2d_f16x", "e2fgvi_packed_conv_weight_f16x_size", "e2fgvi_pack_conv_weight_f16x",
               "e2fgvi_packed_conv_weight_f16x_taps_size", "e2fgvi_pack_conv_weight_f16x_taps", "e2fgvi_focal_attention_f16",
               "e2fgvi_softcomp_fold_f16", "e2fgvi_resize_bilinear_f16", "e2fgvi_pack_dcn_weight_f16",
               "e2fgvi_spynet_level_input_x_f16")
BF16_SIBLINGS = {"e2fgvi_conv2d_f16x": "e2fgvi_conv2d_bf16x", "e2fgvi_packed_conv_weight_f16x_size": "e2fgvi_packed_conv_weight_bf16x_size",
                 "e2fgvi_pack_conv_weight_f16x": "e2fgvi_pack_conv_weight_bf16x",
                 "e2fgvi_packed_conv_weight_f16x_taps_size": "e2fgvi_packed_conv_weight_bf16x_taps_size",
                 "e2fgvi_pack_conv_weight_f16x_taps": "e2fgvi_pack_conv_weight_bf16x_taps",
                 "e2fgvi_focal_attention_f16": "e2fgvi_focal_attention_bf16", "e2fgvi_softcomp_fold_f16": "e2fgvi_softcomp_fold_bf16",
                 "e2fgvi_resize_bilinear_f16": "e2fgvi_resize_bilinear_bf16", "e2fgvi_pack_dcn_weight_f16": "e2fgvi_pack_dcn_weight_bf16",
                 "e2fgvi_spynet_level_input_x_f16": "e2fgvi_spynet_level_input_x"}


def _header():
    with open(os.path.join(ROOT, "include", "e2fgvi_hip.h")) as f:
        return f.read()


def test_header_defines_the_fp16_element_type():
    m = re.search(r"^#define E2FGVI_F16 (\d+)", _header(), re.M)
    assert m and int(m.group(1)) == 3
    from e2fgvi_amd import lib
    assert lib.DT_F16 == 3 and lib.DT_BF16 == 1 and lib.DT_F32 == 0


def test_f16_entry_points_are_declared_and_typed_like_their_bf16_siblings():
    from e2fgvi_amd import lib
    h = _header()
    for name in F16_SYMBOLS:
        assert re.search(r"\b%s\(" % name, h), name + " is not declared in the header"
        assert name in lib.SYMBOLS, name + " is not in the ctypes table"
        assert lib.SYMBOLS[name][0] == lib.SYMBOLS[BF16_SIBLINGS[name]][0], name
        assert [str(a) for a in lib.SYMBOLS[name][1]] == [str(a) for a in lib.SYMBOLS[BF16_SIBLINGS[name]][1]], name


@pytest.mark.parametrize("bad", ["half", "float16", "FP16", "bfloat16", "", None])
def test_a_bad_precision_string_raises_value_error(bad):
    from e2fgvi_amd.engine import Engine
    with pytest.raises(ValueError):
        Engine({}, "e2fgvi", "cpu", precision=bad)
