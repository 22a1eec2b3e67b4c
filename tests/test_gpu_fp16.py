"""The fp16 data path (Engine(precision="fp16"), net.precision = "fp16"): the bf16 data path with IEEE half as the 16-bit type.

Kernel level, in the style of test_gpu_bf16x.py: operands are rounded to fp16 first and the reference takes the SAME rounded
values (fp64 torch), so what is compared is the kernel's own arithmetic -- fp32 accumulation (fp32 tolerances) and, for 16-bit
results, one fp16 rounding (2^-11 relative), 8x finer than bf16's.  End to end: against the real reference's fixtures, next to
the bf16 path on the same clip."""
import importlib
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_bound, assert_close, err, fp32_tol, gen as _gen, name_seed, nchw, nhwc

pytestmark = pytest.mark.gpu
F16 = torch.float16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def conv64(x, w, b=None, **kw):
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), **kw)


def assert_close_f16(got, ref, what="", ulps=1.0, abs_rms=5e-4):
    """for results stored as fp16: |got - ref| <= ulps * 2^-10 * |ref| + abs_rms * rms(ref) elementwise (one fp16 rounding is
    2^-11 relative; the default allows it twice)"""
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), what + ": non-finite output"
    rms = ref.pow(2).mean().sqrt().item()
    excess = ((got - ref).abs() - ((ulps * 2.0 ** -10) * ref.abs() + abs_rms * rms)).max().item()
    assert excess <= 0, "%s: error exceeds %.1f x 2^-10 relative + %.1e x rms by %.3e" % (what, ulps, abs_rms, excess)


def _is_half(got, ref32):
    assert_is_half_of(got, ref32, "fp16 result")
    return True


def _bits(t):
    return t.detach().cpu().view(torch.int16)


def assert_is_half_of(got, ref32, what=""):
    """the fp16 tensor `got` holds the bits of .half() of the fp32 tensor `ref32` -- rounded on the CPU (round to nearest even,
    subnormals kept), the rounding the kernels are specified to reproduce"""
    g, r = _bits(got), ref32.detach().cpu().half().view(torch.int16)
    bad = (g != r).nonzero()
    if len(bad):
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements are not .half() of the fp32 result (first at %s: %r vs fp32 %r)"
                             % (what, len(bad), g.numel(), i, got.detach().cpu()[i].item(), ref32.detach().cpu()[i].item()))


# ------------------------------------------------------------------------------------------------------------- conversions
def test_cast_fp32_to_fp16_is_bit_equal_to_half(dev):
    """ties (to even), subnormals (and the rounding into and out of them), +-65504 and its neighbours, overflow to +-inf,
    +-inf and NaN: the bits of torch's .half()"""
    from e2fgvi_amd import ops
    g = _gen(1603)
    eps = 2.0 ** -10
    special = [0.0, -0.0, 1.0, -1.0, 1.0 + eps / 2, 1.0 + 3 * eps / 2, -(1.0 + eps / 2), 2049.0, 2051.0, 4097.0,   # ties
               65504.0, -65504.0, 65503.0, 65505.0, 65519.0, 65519.996, 65520.0, -65520.0, 65536.0, 1e6, -1e30,        # range
               2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -26, 1.5 * 2.0 ** -24, -2.0 ** -24,
               2.0 ** -14 - 2.0 ** -25, 6.1e-5, 5.96e-8, 1e-10, -1e-10, 1e-45,                                       # subnormals
               float("inf"), float("-inf"), float("nan"), float("-nan")]
    x = torch.tensor(special, dtype=torch.float32)
    # ...and a million random values over the whole fp16 range (and beyond), with their exact midpoints
    r = torch.randn(1 << 20, generator=g) * torch.pow(2.0, torch.randint(-30, 18, (1 << 20,), generator=g).float())
    mid = (torch.randn(1 << 14, generator=g) * 100).half().float()
    mid = mid + mid.abs() * (2.0 ** -11)                  # halfway to the next fp16 (for normal values)
    x = torch.cat([x, r, mid])
    x = torch.cat([x, x.new_zeros((-x.numel()) % 4)])
    h = ops.cast(x.to(dev), F16)
    assert h.dtype == F16
    assert _is_half(h, x), "fp32 -> fp16 differs from .half() at %d elements" % int((_bits(h) != _bits(x.half())).sum())
    back = ops.cast(h, torch.float32)
    ref = x.half().float()
    same = (back.cpu() == ref) | (torch.isnan(back.cpu()) & torch.isnan(ref))
    assert bool(same.all()), "fp16 -> fp32 is not exact"


# ------------------------------------------------------------------------------------------------------------- conv / linear
def _bf16_table_tiles():
    from e2fgvi_amd import tile_table
    return sorted({v for k, v in tile_table.TILES.items() if k[0] == "x"})


# name, N, H, W, cpg (per source), groups, Cout, k, stride, pad, tiles ("table": every tile code of the bf16 rows of the
# checked-in decision table, plus every row-shift code)
CASES = [
    ("3x3 128->128", 2, 20, 28, [128], 1, 128, 3, 1, 1, "table"),
    ("3x3 concat 128+128+128+8 -> 128 (conv_offset.0)", 1, 12, 20, [128, 128, 128, 8], 1, 128, 3, 1, 1, (0, 1, 4, 11, 14, 16, 17)),
    ("1x1 256 -> 1536 (qkv)", 3, 7, 11, [256], 1, 1536, 1, 1, 0, (0, 1, 6, 7, 8)),
    ("3x3 groups 8, 32+48 -> 256 (encoder.14)", 2, 10, 12, [32, 48], 8, 256, 3, 1, 1, (0, 3, 5, 12, 13, 18)),
    ("3x3 stride 2, 8 -> 64 (encoder.0)", 2, 24, 40, [8], 1, 64, 3, 2, 1, (0, 2)),
    ("3x3 64 -> 3 (decoder.6 shape)", 2, 24, 36, [64], 1, 3, 3, 1, 1, (0, 3, 13, 18)),
    ("7x7 8 -> 32 (spynet .0): tap-packed", 2, 20, 28, [8], 1, 32, 7, 1, 3, (0, 1, 3, 5)),
    ("7x7 stride 3 pad 3, 40 -> 512 (FFN fc2 as a conv): tap-packed", 2, 30, 54, [40], 1, 512, 7, 3, 3, (0, 1, 7)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_f16x(dev, case):
    from e2fgvi_amd import ops
    name, N, H, W, cpg, groups, Cout, k, stride, pad, tiles = case
    if tiles == "table":
        tiles = sorted(set(_bf16_table_tiles()) | {0, 11, 12, 13, 14, 16, 17, 18})
    g = _gen(name_seed(name, 16))
    w = (torch.randn(Cout, sum(cpg), k, k, generator=g) / math.sqrt(sum(cpg) * k * k)).half().float()
    bias = torch.randn(Cout, generator=g) * 0.1
    srcs, parts = [], []
    for si, c in enumerate(cpg):
        ld = c * groups + 16
        t = torch.randn(N, H, W, ld, generator=g)
        if si == 0:
            t[..., 8:12] *= 2.0 ** -16              # fp16 subnormals (and values that round into them) as operands
        t = t.half()
        srcs.append(t)
        parts.append(t[..., 8:8 + c * groups].float())
    x = torch.cat([torch.cat([p_[..., gi * c:(gi + 1) * c] for p_, c in zip(parts, cpg)], -1) for gi in range(groups)], -1)
    ref0 = conv64(nchw(x), w, bias, stride=stride, padding=pad, groups=groups)
    tol = fp32_tol(sum(cpg) * k * k, floor=3e-5)
    layer = ops.PackedConvX(w.to(dev), bias.to(dev), cpg, groups=groups, stride=stride, pad=pad, dtype=F16)
    assert layer.taps == (len(cpg) == 1 and cpg[0] <= 56 and k > 1 and groups == 1)
    src_d = [(s.to(dev), 8) for s in srcs]
    res16 = torch.randn(N, ref0.shape[2], ref0.shape[3], Cout, generator=g).half().to(dev)
    for tile in tiles:
        if tile >= 10 and (k != 3 or stride != 1 or layer.taps):
            continue
        out2 = torch.empty(N, ref0.shape[2], ref0.shape[3], Cout, dtype=F16, device=dev)
        out = layer(src_d, out_dtype=torch.float32, act=ops.ACT_LRELU, slope=0.1, tile=tile, out2=out2)
        assert_close(nchw(out.cpu()), F.leaky_relu(ref0, 0.1), tol, "%s tile %d fp32 out" % (name, tile))
        assert _is_half(out2, out), "%s tile %d: dst2 is not .half() of the fp32 result" % (name, tile)
        o16 = layer(src_d, act=ops.ACT_LRELU, slope=0.1, tile=tile)
        assert o16.dtype == F16 and _is_half(o16, out), "%s tile %d: fp16 dst" % (name, tile)
        # fp16 residual == the same values as an fp32 residual, rounded once
        r16 = layer(src_d, residual=res16, act=ops.ACT_RELU, tile=tile)
        r32 = layer(src_d, out_dtype=torch.float32, residual=res16.float(), act=ops.ACT_RELU, tile=tile)
        assert _is_half(r16, r32), "%s tile %d: fp16 residual" % (name, tile)
    if groups == 1:
        outn = layer(src_d, act=ops.ACT_TANH, out_nchw=True)
        assert_close(outn.cpu(), torch.tanh(ref0), tol, name + " NCHW fp32 out")
    with pytest.raises(TypeError):
        layer([(s.to(dev).bfloat16(), 8) for s in srcs])                 # bf16 sources on an fp16 layer


def test_linear_f16x_and_bad_arguments(dev):
    from e2fgvi_amd import ops
    from e2fgvi_amd.lib import HipError
    g = _gen(1616)
    rows, cin, cout = 3000, 512, 1536
    w = (torch.randn(cout, cin, generator=g) / math.sqrt(cin)).half().float()
    b = torch.randn(cout, generator=g) * 0.1
    x = torch.randn(rows, cin, generator=g).half()
    layer = ops.PackedLinearX(w.to(dev), b.to(dev), dtype=F16)
    ref = F.linear(x.double(), w.double(), b.double())
    out = layer(x.to(dev), out_dtype=torch.float32)
    assert_close(out.cpu(), ref, fp32_tol(cin, floor=3e-5), "linear f16")
    assert _is_half(layer(x.to(dev)), out)
    # the fp32 layer keeps refusing fp16 input; fp16 layers refuse bf16 input; split planes are not an fp16 form
    with pytest.raises(TypeError):
        ops.PackedConv(torch.randn(32, 16, 3, 3, device=dev), None, [16], pad=1)([torch.zeros(1, 4, 4, 16, device=dev, dtype=F16)])
    with pytest.raises(TypeError):
        layer(x.to(dev).bfloat16())
    d = layer._desc([(x.to(dev).view(rows, 1, 1, cin), 0)], torch.empty(rows, 1, 1, cout, device=dev), 0, None, 0, 0, 0.0, None, False)
    d.dst2, d.dst2_split_from, d.dst2_plane_stride, d.dst2_ld = out.data_ptr(), 512, rows * 1024, 1024
    d.wpacked = layer.wpacked.data_ptr()
    with pytest.raises(HipError):
        from e2fgvi_amd import lib as _L
        _L.check(layer._fn(__import__("ctypes").byref(d), None), "conv2d_x (fp16) split planes")


# ------------------------------------------------------------------------------------------------------------- attention
def _attention_ref(qkv, kvp, tab, nk, B, T, fh, fw):
    """the focal window attention evaluated in fp32 on the device from the key table's definition (include/e2fgvi_hip.h):
    per window and frame, nkeys[win] references (v >= 0: token v of that frame; v < 0: pooled window -(v+1) of that frame)
    and 210 - nkeys[win] zero-padded slots that score exactly -100"""
    ntok, nwin = fh * fw, (fh // 5) * (fw // 9)
    q_all, kv_tok, kv_pool = qkv.float().view(B, T, ntok, 1536), qkv.float().view(B, T, ntok, 1536), kvp.float().view(B, T, nwin, 1536)
    out = torch.empty(B, T, ntok, 512, device=qkv.device)
    ys, xs = torch.meshgrid(torch.arange(fh), torch.arange(fw), indexing="ij")
    win_of = ((ys // 5) * (fw // 9) + xs // 9).reshape(-1).to(qkv.device)
    for b in range(B):
        for w in range(nwin):
            qi = (win_of == w).nonzero().view(-1)
            refs = tab[w, :nk[w]].long()
            tok = refs >= 0
            keys = []
            for t in range(T):
                kv = torch.empty(len(refs), 1536, device=qkv.device)
                kv[tok] = kv_tok[b, t, refs[tok]]
                kv[~tok] = kv_pool[b, t, (-(refs[~tok] + 1))]
                keys.append(kv)
            kv = torch.cat(keys, 0)
            npad = T * (210 - int(nk[w]))
            q = q_all[b][:, qi].reshape(-1, 1536)
            for h in range(4):
                qh, kh, vh = q[:, h * 128:(h + 1) * 128], kv[:, 512 + h * 128:512 + (h + 1) * 128], kv[:, 1024 + h * 128:1024 + (h + 1) * 128]
                s = (qh @ kh.t()) * (128 ** -0.5)
                s = torch.cat([s, torch.full((s.shape[0], 1), -100.0, device=s.device)], 1)
                m = s.max(1, keepdim=True).values
                e = torch.exp(s - m)
                e[:, -1] *= npad
                o = (e[:, :-1] @ vh) / e.sum(1, keepdim=True)
                out[b][:, qi, h * 128:(h + 1) * 128] = o.view(T, len(qi), 128)
    return out.view(-1, 512)


@pytest.mark.parametrize("B,T,fh,fw,variants", [(1, 3, 10, 18, (1, 12, 14, 18, 22, 24, 28)), (2, 2, 20, 36, (0, 1, 14, 24)),
                                                 (1, 10, 10, 18, (0, 1, 18, 28)),
                                                 (1, 152, 5, 9, (0,))])        # T > 150: only the register-staged kernel fits
def test_focal_attention_f16(dev, B, T, fh, fw, variants):
    """every kernel variant e2fgvi_focal_attention_16_variant can select, on fp16 rows (P rounded to fp16 for the PV product,
    the output rounded once): elementwise within 2^-10 relative + 2e-3 x rms -- a sixth of the bf16 kernel's allowance"""
    from e2fgvi_amd import ops
    from e2fgvi_amd.engine import build_key_table
    from e2fgvi_amd.synth import rolled_valid_index
    g = _gen(160 + T)
    ntok, nwin = fh * fw, (fh // 5) * (fw // 9)
    qkv = (torch.randn(B * T * ntok, 1536, generator=g) * 1.5).half().to(dev)
    kvp = (torch.randn(B * T * nwin, 1536, generator=g) * 1.5).half().to(dev)
    tab, nk = build_key_table(fh, fw, rolled_valid_index().tolist())
    tab_d, nk_d = torch.from_numpy(tab).to(dev), torch.from_numpy(nk).to(dev)
    ref = _attention_ref(qkv, kvp, tab_d, nk, B, T, fh, fw)
    both = torch.cat([qkv, kvp], 0)
    rows = qkv.shape[0]
    for variant in variants:
        o = ops.focal_attention_bf16(both[:rows], both[rows:], tab_d, nk_d, B, T, fh, fw, variant=variant or None)
        assert o.dtype == F16
        assert_close_f16(o, ref, "fp16 attention %dx%d T=%d variant %d" % (fh, fw, T, variant), ulps=1.0, abs_rms=2e-3)


# ------------------------------------------------------------------------------------------------------------- deformable conv
@pytest.mark.parametrize("tile", [0, 1, 2, 5, 7, 101])
def test_mdcn_f16_planar(dev, tile):
    """the deformable conv with fp16 planar sources (what the fp16 engine passes), fp16 weights and fp16 MFMA against the fp32
    oracle of mmcv's op on the SAME fp16 features: the sampled slab and the weights carry one 2^-11 rounding each"""
    from e2fgvi_amd import ops
    from oracle.dcn import modulated_deform_conv2d
    g = _gen(4416)
    N, C, H, W, Co, dg = 1, 256, 14, 22, 128, 16
    x = torch.randn(N, C, H, W, generator=g)
    x[:, 5:9] *= 2.0 ** -17                                 # subnormal fp16 features
    x16 = x.half()
    off = torch.randn(N, dg * 18, H, W, generator=g) * 3.0
    msk = torch.rand(N, dg * 9, H, W, generator=g)
    w = (torch.randn(Co, C, 3, 3, generator=g) / 48).half().float()
    b = torch.randn(Co, generator=g)
    ref = modulated_deform_conv2d(x16.float(), off, msk, w, b, 1, 1, 1, 1, dg)
    layer = ops.PackedDcn(w.to(dev), b.to(dev), dg, pad=1, mfma="fp16")
    xs = [ops.to_planar16(nhwc(x16[:, :128]).contiguous().to(dev)), ops.to_planar16(nhwc(x16[:, 128:]).contiguous().to(dev))]
    out = layer(xs, nhwc(off).to(dev), mask=nhwc(msk).to(dev), tile=tile, planar=True)
    assert_close(nchw(out.cpu()), ref, 3e-3, "mdcn fp16 planar tile %d" % tile)            # bf16: 1.5e-2
    o16 = layer(xs, nhwc(off).to(dev), mask=nhwc(msk).to(dev), tile=tile, planar=True, out_dtype=F16)
    assert _is_half(o16, out)
    with pytest.raises(Exception):
        layer([nhwc(x[:, :128]).contiguous().to(dev), nhwc(x[:, 128:]).contiguous().to(dev)], nhwc(off).to(dev),
              mask=nhwc(msk).to(dev))                       # fp16 products take fp16 sources


# ------------------------------------------------------------------------------------------------------------- tail, SoftComp
def test_tail_f16(dev):
    from e2fgvi_amd import ops
    g = _gen(1661)
    N, H, W = 2, 37, 70
    x = torch.randn(N, H, W, 72, generator=g)
    x[..., :4] *= 2.0 ** -17
    x = x.half()
    w = (torch.randn(3, 64, 3, 3, generator=g) / 24).half().float()
    b = torch.randn(3, generator=g) * 0.1
    tail = ops.PackedTailConv(w.to(dev), b.to(dev), dtype=F16)
    out = tail([x.to(dev)[..., :72]], act=ops.ACT_TANH)
    ref = torch.tanh(conv64(nchw(x[..., :64].float()), w, b, padding=1))
    assert_close(out.cpu(), ref, fp32_tol(64 * 9, floor=3e-5), "tail fp16")


def test_softcomp_gather_f16(dev):
    """SoftComp in gather form on fp16 tokens: the fp32 result equals the fp32 gather of the same fp16 values within fp32 rounding,
    the fp16 result is its .half()"""
    from e2fgvi_amd import ops
    g = _gen(1670)
    F_, fh, fw, Cc = 2, 10, 18, 128
    H, W = 3 * fh, 3 * fw
    w = (torch.randn(49 * Cc, 512, generator=g) / 24).half().float()
    bias = torch.randn(49 * Cc, generator=g) * 0.1
    tok = torch.randn(F_, fh, fw, 512, generator=g).half()
    s16 = ops.SoftCompGather(w.to(dev), bias.to(dev), Cc, dtype=F16)
    s32 = ops.SoftCompGather(w.to(dev), bias.to(dev), Cc, dtype=torch.float32)
    t16 = tok.to(dev)
    ref = s32(t16.float(), out_dtype=torch.float32)
    got32 = s16(t16, out_dtype=torch.float32)
    assert_close(got32.cpu(), ref.cpu(), fp32_tol(512 * 9, floor=3e-5), "softcomp gather fp16 -> fp32")
    got16 = s16(t16)
    assert got16.dtype == F16 and _is_half(got16, got32)


# ------------------------------------------------------------------------------------------------------------- typed helpers
def test_typed_helper_kernels_f16(dev):
    """fp16 variants of the HBM-bound helpers == their fp32 versions on the same fp16 values, rounded once (.half())"""
    from e2fgvi_amd import ops
    g = _gen(1621)
    BT, fh, fw, H, W = 2, 10, 18, 30, 54
    x = torch.randn(BT * fh * fw, 512, generator=g)
    x[:7] *= 2.0 ** -18                                      # rows whose LayerNorm input is tiny (outputs stay normal)
    gm, bt = torch.randn(512, generator=g), torch.randn(512, generator=g) * 1e-5     # subnormal shifts
    y32 = ops.layernorm(x.to(dev), gm.to(dev), bt.to(dev))
    y16 = ops.layernorm(x.to(dev), gm.to(dev), bt.to(dev), out_dtype=F16)
    # the fp16 store of the last multiply-add is ONE rounding (v_fma_mix*_f16: the fp16 of the exact gamma * xhat + beta), the
    # fp32 kernel's .half() two: they can differ by one fp16 step where the fp32 value sits on an fp16 midpoint (2^-13 of them)
    d = (_bits(y16).int() - y32.cpu().half().view(torch.int16).int()).abs()
    assert int(d.max()) <= 1 and int((d > 0).sum()) <= y16.numel() * 2.0 ** -11, (int(d.max()), int((d > 0).sum()))
    w45, b1 = (torch.full((45,), 1 / 45.) + 0.02 * torch.randn(45, generator=g)).to(dev), torch.zeros(1, device=dev)
    xs = (y16.float() * 2.0 ** -14).half()                   # mostly subnormal window-pool operands and results
    for xb in (y16, xs):
        assert _is_half(ops.window_pool(xb, w45, b1, BT, fh, fw), ops.window_pool(xb.float(), w45, b1, BT, fh, fw))
    hid = torch.randn(BT * fh * fw, 49 * 40, generator=g).half().to(dev)
    f16, f32 = ops.ffn_fold(hid, BT, fh, fw, H, W, 40), ops.ffn_fold(hid.float(), BT, fh, fw, H, W, 40)
    assert f16.dtype == F16 and _is_half(f16, f32)
    assert _is_half(ops.ffn_unfold_gelu(f16, fh, fw), ops.ffn_unfold_gelu(f16.float(), fh, fw))
    g16, g32 = ops.ffn_fold_gelu(hid, BT, fh, fw, H, W, 40), ops.ffn_fold_gelu(hid.float(), BT, fh, fw, H, W, 40)
    assert _is_half(g16, g32)
    assert _is_half(ops.ffn_unfold(g16, fh, fw), ops.ffn_unfold(g16.float(), fh, fw))
    emb = torch.randn(BT * fh * fw, 49 * 128, generator=g).half().to(dev)
    res = torch.randn(BT, H, W, 128, generator=g).half().to(dev)
    bias = torch.randn(H, W, 128, generator=g).to(dev)
    s16 = ops.softcomp_fold(emb, BT, fh, fw, H, W, 128, bias_hwc=bias, residual=res)
    s32 = ops.softcomp_fold(emb.float(), BT, fh, fw, H, W, 128, bias_hwc=bias, residual=res.float())
    assert s16.dtype == F16 and _is_half(s16, s32)
    r16, r32 = ops.resize_bilinear(res, (2 * H, 2 * W), True), ops.resize_bilinear(res.float(), (2 * H, 2 * W), True)
    assert r16.dtype == F16
    assert_close_f16(r16, r32, "x2 upsample fp16", ulps=1.0, abs_rms=1e-6)
    fr = torch.rand(2, 3, 24, 40, generator=g).to(dev)
    n16 = ops.nchw_to_nhwc(fr, ld=8, out_dtype=F16)
    assert torch.equal(_bits(n16[..., :3].contiguous()), _bits(fr.permute(0, 2, 3, 1).half().contiguous())) and float(n16[..., 3:].abs().max()) == 0
    n16w = ops.nchw_to_nhwc(torch.rand(1, 40, 9, 11, generator=g).to(dev), ld=48, out_dtype=F16)      # tiled transpose
    assert n16w.dtype == F16 and float(n16w[..., 40:].abs().max()) == 0
    # nhwc_to_planar16 is layout only
    p = ops.to_planar16(res)
    assert p.dtype == F16 and torch.equal(_bits(p), _bits(res.view(BT, H, W, 8, 16).permute(3, 0, 1, 2, 4).contiguous()))
    # prop_cond: fp16 warp sources and cond, the flows as an 8-channel fp16 conv source
    fp, f2 = torch.randn(1, 12, 20, 128, generator=g).half().to(dev), torch.randn(1, 12, 20, 128, generator=g).half().to(dev)
    fa, fb = (torch.randn(1, 12, 20, 2, generator=g) * 2).to(dev), (torch.randn(1, 12, 20, 2, generator=g) * 2).to(dev)
    c16, fl, fl8 = ops.prop_cond(fp, f2, fa, fb, 12 * 20 * 2, cond_dtype=F16, flows8=True)
    c32, fl32 = ops.prop_cond(fp.float(), f2.float(), fa, fb, 12 * 20 * 2)
    assert c16.dtype == F16 and fl8.dtype == F16
    assert _is_half(c16, c32) and torch.equal(fl, fl32)
    assert _is_half(fl8[..., :4].contiguous(), fl32) and float(fl8[..., 4:].abs().max()) == 0
    cf, _, fl8f = ops.prop_cond(fp.float(), f2.float(), fa, fb, 12 * 20 * 2, cond_dtype=F16, flows8=True)   # fp32 sources
    assert _is_half(cf, c32) and torch.equal(_bits(fl8f), _bits(fl8))
    with pytest.raises(Exception):
        ops.prop_cond(fp, f2, fa, fb, 12 * 20 * 2, cond_dtype=torch.bfloat16)      # fp16 sources need an fp16 cond
    # SPyNet level input: the fp16 copy of the 8 channels
    pyr = torch.rand(3, 16, 24, 4, generator=g).to(dev)
    ri, si = torch.tensor([0, 1], dtype=torch.int32, device=dev), torch.tensor([1, 2], dtype=torch.int32, device=dev)
    fprev = torch.randn(2, 8, 12, 2, generator=g).to(dev)
    o32, o16 = ops.spynet_level_input(pyr, ri, si, fprev, copy_dtype=F16)
    assert o16.dtype == F16 and _is_half(o16, o32)
    # cast back and forth on a real activation
    assert torch.equal(_bits(ops.cast(x.to(dev), F16)), _bits(x.half())) and torch.equal(ops.cast(y16, torch.float32), y16.float())


# ------------------------------------------------------------------------------------------------------------- end to end
def _net(model, kind, dev, precision):
    from e2fgvi_amd.synth import synth_state_dict
    net = importlib.import_module("model." + model).InpaintGenerator()
    net.load_state_dict(synth_state_dict(model, kind, 0))
    net = net.to(dev).eval()
    net.precision = precision
    return net


GOLDEN_FIXTURES = ["g7_e2fgvi_stress_t10_lt10.npz", "g11_e2fgvi_peaked_t10_lt10.npz",
                   "g9_hq_stress_720x1296_t10_lt10.npz", "g10_hq_stress_1080x1944_t8_lt8.npz",
                   "g14_hq_default_720x1296_t10_lt10_benchclip.npz", "g12_hq_peaked_240x432_t6_lt4.npz",
                   "g13_hq_peaked_720x1296_t4_lt3.npz",
                   "g3_hq_stress_120x216_t4_lt3.npz", "g5_hq_stress_720x1296_t3_lt2.npz", "g6_hq_stress_1080x1944_t2_lt2.npz"]


@pytest.mark.parametrize("fixture", GOLDEN_FIXTURES)
def test_fp16_path_against_reference_golden_next_to_bf16(dev, fixture):
    """fp16 and bf16 forwards of the same fixture against the REAL reference's sub-sampled outputs (tests/golden/make_golden.py).
    fp16 rounds every stored activation and MFMA operand 8x finer (2^-11 against 2^-8): its max error and its rms error must each
    be at most a third of bf16's, and on the default and stress weights its max error at most 2e-3.  Output finite throughout."""
    from tests.util import golden_case
    z, model, kind, x, lt, so, sf = golden_case(os.path.join(GOLDEN, fixture))
    rms_ref = float(z["out_stats"][2])
    res = {}
    for precision in ("fp16", "bf16"):
        net = _net(model, kind, dev, precision)
        out, (ff, fb) = net(x.to(dev), lt)
        out = out.cpu()
        assert np.isfinite(out.numpy()).all(), "%s %s: non-finite output" % (fixture, precision)
        diff = out[:, :, ::so, ::so].numpy().astype(np.float64) - z["out_sub"]
        fl = max(np.abs(ff.cpu()[..., ::sf, ::sf].numpy() - z["flow_fwd_sub"]).max(), np.abs(fb.cpu()[..., ::sf, ::sf].numpy() - z["flow_bwd_sub"]).max())
        res[precision] = (np.abs(diff).max(), np.sqrt((diff ** 2).mean()) / rms_ref, fl)
        del net, out
        torch.cuda.empty_cache()
    (m16, r16, fl16), (mb, rb, flb) = res["fp16"], res["bf16"]
    print("FP16TABLE %s | fp16 max %.3e rms %.3e flow %.3e | bf16 max %.3e rms %.3e flow %.3e | ratio max %.2f rms %.2f"
          % (fixture, m16, r16, fl16, mb, rb, flb, mb / max(m16, 1e-30), rb / max(r16, 1e-30)))
    assert_bound(m16, mb / 3, "fp16 golden %s max abs <= bf16 / 3" % fixture)
    assert_bound(r16, rb / 3, "fp16 golden %s rms <= bf16 / 3" % fixture)
    if kind in ("default", "stress"):
        assert_bound(m16, 2e-3, "fp16 golden %s max abs" % fixture)


# ------------------------------------------------------------------------------------------------------------- behaviour
def test_fp16_forwards_are_bit_identical_and_graph_replay_matches_eager(dev):
    from e2fgvi_amd import runner
    from e2fgvi_amd.synth import synth_clip
    net = _net("e2fgvi_hq", "stress", dev, "fp16")
    x = synth_clip(1, 10, 240, 432, seed=5, moving=True)[0].to(dev)
    a = net(x, 10)[0].clone()
    b = net(x, 10)[0].clone()
    assert torch.equal(a, b), "two fp16 forwards of one clip differ"
    step = runner.ShardedStep(net, x, 10)
    for _ in range(3):
        step.run()
    out = step.finish().clone()
    torch.cuda.synchronize()
    assert step.graphed
    assert torch.equal(out, a), "fp16 graph replay differs from the eager forward"


def test_fp16_video_windows_in_flight_return_the_bytes_of_one_at_a_time(dev):
    from e2fgvi_amd import video
    from tests.test_video_driver import _toy_video
    frames, masks = _toy_video(23, 120, 200, seed=9)
    net = _net("e2fgvi_hq", "stress", dev, "fp16")
    ref = video.inpaint_video(net, np.stack(frames), np.stack(masks), 5, 10, -1)
    out = video.inpaint_video(net, np.stack(frames), np.stack(masks), 5, 10, -1, in_flight=2)
    assert np.array_equal(out, ref), "in_flight=2: %d bytes differ" % int((out != ref).sum())


def test_fp16_spynet_side_stream_is_deterministic(dev):
    """SPyNet on a side stream beside 16-bit MFMA tiles gives exactly the single-stream result (fp16 MFMA)"""
    from e2fgvi_amd.engine import Engine
    from e2fgvi_amd.synth import synth_clip, synth_state_dict
    eng = Engine(synth_state_dict("e2fgvi", "stress", 0), "e2fgvi", dev, precision="fp16")
    assert eng.x16 and eng.dtype == F16 and eng.overlap_flows
    x = synth_clip(1, 4, 240, 432, seed=3, moving=True)[0].to(dev)
    eng.overlap_flows = False
    base, (bf, bb) = eng.forward(x, 3)
    torch.cuda.synchronize()
    eng.overlap_flows = True
    for _ in range(40):
        got, (ff, fb) = eng.forward(x, 3)
        torch.cuda.synchronize()
        assert torch.equal(ff, bf) and torch.equal(fb, bb) and torch.equal(got, base)
