"""Saturated pre-activations through every place that computes the deformable alignment's offset / mask post-processing
(ACT_DCNPOST: max_residue * tanh + flow on the offsets, sigmoid on the masks, on the hardware exp2 + rcp of csrc/common.h), and
LayerNorm rows off unit scale.

The other tests of these epilogues feed pre-activations within about +-3.  Here the geometries and the small random weights of
those tests are kept and the bias (for the deformable conv's own fused form: the raw conv_offset channel) of channel c is
V[c % 17], V = (0, +-1e-3, +-3, +-9, +-20, +-45, +-90, +-200, +-1e4): 17 is coprime with the 144 channels of each third, so both
offset halves and the masks see every value -- exp2 arguments from denormal-small to far past +-128, where exp2 returns 0 / +inf
and the rcp behind it must give exactly 1 / 0.

Bounds: the tolerance of the test the geometry comes from, applied per chunk (each offset half and the mask third against its
own rms); where |pre-activation| >= 200 the masks are exactly 0.0 / 1.0 and the offsets equal fp32(+-10 + flow) to 1 ulp;
everything finite."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_bound, assert_close, gen as _gen, nchw, nhwc

pytestmark = pytest.mark.gpu

V = (0.0, 1e-3, -1e-3, 3.0, -3.0, 9.0, -9.0, 20.0, -20.0, 45.0, -45.0, 90.0, -90.0, 200.0, -200.0, 1e4, -1e4)


def sat_values(C, shift=0):
    return torch.tensor([V[(c + shift) % 17] for c in range(C)], dtype=torch.float32)


def conv64(x, w, b=None, **kw):
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), **kw)


def dcnpost_ref(raw, fl, max_residue=10.0):
    """feat_prop.py:38-53 in float64.  raw: [N, C, H, W] pre-activations, fl: [N, H, W, 4] = (u1, v1, u2, v2) per pixel.
    Returns (finished [N, C, H, W], the flow term of the offset channels [N, 2C/3, H, W])"""
    raw, fl = raw.double(), nchw(fl).double()
    o1, o2, m = torch.chunk(raw, 3, 1)
    rep = o1.shape[1] // 2
    flow = torch.cat([fl[:, 0:2].flip(1).repeat(1, rep, 1, 1), fl[:, 2:4].flip(1).repeat(1, rep, 1, 1)], 1)
    return torch.cat([max_residue * torch.tanh(torch.cat([o1, o2], 1)) + flow, torch.sigmoid(m)], 1), flow


def check_dcnpost(out, raw, fl, tol, what, need_saturated=True):
    """out: the kernel's [N, C, H, W] fp32 result for the float64 pre-activations `raw`"""
    out = out.detach().float().cpu()
    ref, flow = dcnpost_ref(raw, fl)
    C3 = raw.shape[1] // 3
    for name, lo in (("offsets 1", 0), ("offsets 2", C3), ("masks", 2 * C3)):
        assert_close(out[:, lo:lo + C3], ref[:, lo:lo + C3], tol, "%s, %s" % (what, name))
    sat = raw.abs() >= 200
    m_sat = sat[:, 2 * C3:]
    if need_saturated:
        assert bool(m_sat.any()) and bool(sat[:, :C3].any()) and bool(sat[:, C3:2 * C3].any())
    want_m = (raw[:, 2 * C3:] > 0).float()
    bad = int((out[:, 2 * C3:][m_sat] != want_m[m_sat]).sum())
    assert bad == 0, "%s: %d saturated masks are not exactly 0.0 / 1.0" % (what, bad)
    want_o = (10.0 * torch.sign(raw[:, :2 * C3]) + flow).float()                # fp32(+-10 + flow)
    ulp = torch.nextafter(want_o.abs(), torch.full_like(want_o, float("inf"))) - want_o.abs()
    o_sat = sat[:, :2 * C3]
    over = ((out[:, :2 * C3] - want_o).abs() / ulp)[o_sat]
    if over.numel():
        assert_bound(over.max().item(), 1.0, what + ": saturated offsets vs fp32(+-10 + flow), in ulps")


def _fp32_case(seed, N, H, W, wscale, Cout=432, cin=128):
    g = _gen(seed)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(Cout, cin, 3, 3, generator=g) * wscale
    fl = torch.randn(N, H, W, 4, generator=g) * 2
    return x, w, fl


# ------------------------------------------------------------------------------------------------ conv epilogues, fp32
@pytest.mark.parametrize("tile", [0, 10003, 10024])
def test_saturated_dcnpost_igemm_and_halo(dev, tile):
    """the geometry of test_conv_dcn_postprocess_epilogue on the implicit-GEMM kernel and two halo-staged tiles (one tap and a
    kernel row of weights per stage)"""
    from e2fgvi_amd import ops
    x, w, fl = _fp32_case(3000, 2, 14, 22, 1 / 40)
    b = sat_values(432)
    raw = conv64(x, w, b, padding=1)
    layer = ops.PackedConv(w.to(dev), b.to(dev), [128], pad=1)
    out = layer([nhwc(x).to(dev)], residual=fl.to(dev), act=ops.ACT_DCNPOST, slope=10.0, tile=tile)
    check_dcnpost(nchw(out.cpu()), raw, fl, 3e-5, "saturated DCNPOST, conv tile %d" % tile)


def test_saturated_dcnpost_halo16(dev):
    """the 16-output-channel halo tile has its own epilogue: 12 channels = 4 + 4 offsets and 4 masks per launch, so the values go
    through in five launches"""
    from e2fgvi_amd import ops
    x, w, fl = _fp32_case(3001, 2, 17, 40, 1 / 20, Cout=12, cin=32)
    for r in range(5):
        b = torch.tensor([V[(c % 4 + 4 * r) % 17] for c in range(12)])
        raw = conv64(x, w, b, padding=1)
        layer = ops.PackedConv(w.to(dev), b.to(dev), [32], pad=1)
        out = layer([nhwc(x).to(dev)], residual=fl.to(dev), act=ops.ACT_DCNPOST, slope=10.0, tile=10042)
        check_dcnpost(nchw(out.cpu()), raw, fl, 3e-5, "saturated DCNPOST, halo16 tile, values %d.." % (4 * r), need_saturated=False)


@pytest.mark.parametrize("tile", [0, 32, 64, 132, 164, 2464])
def test_saturated_dcnpost_winograd(dev, tile):
    """the geometries of test_conv3x3_winograd_dcnpost (F(2x2,3x3) block shapes) and test_conv3x3_winograd4_dcnpost (2464)"""
    from e2fgvi_amd import ops
    wide = tile == 2464
    H, W = (32, 56) if wide else (30, 54)
    x, w, fl = _fp32_case(3002, 2, H, W, 1 / math.sqrt(128 * 9))
    b = sat_values(432)
    raw = conv64(x, w, b, padding=1)
    layer = ops.PackedConv(w.to(dev), b.to(dev), [128], pad=1, algo="winograd")
    out = layer([nhwc(x).to(dev)], residual=fl.to(dev), act=ops.ACT_DCNPOST, slope=10.0, tile=tile)
    tol = 5e-5
    if wide:
        from tests.test_gpu_wino4 import wtol
        tol = max(5e-5, 2 * wtol(tile, 128))
    check_dcnpost(nchw(out.cpu()), raw, fl, tol, "saturated DCNPOST, Winograd tile %d" % tile)


# ------------------------------------------------------------------------------------------------ split operands, 16-bit
def test_saturated_dcnpost_x3(dev):
    """the geometry of test_x3_dcn_postprocess_and_nchw on the split-operand GEMM"""
    from e2fgvi_amd import ops
    x, w, fl = _fp32_case(3003, 2, 14, 22, 1 / 40)
    b = sat_values(432)
    raw = conv64(x, w, b, padding=1)
    layer = ops.PackedConvX(w.to(dev), b.to(dev), [128], pad=1, dtype=torch.float32, x3=True)
    out = layer([nhwc(x).to(dev)], residual=fl.to(dev), act=ops.ACT_DCNPOST, slope=10.0)
    check_dcnpost(nchw(out.cpu()), raw, fl, 3e-5, "saturated DCNPOST, split-operand conv")


@pytest.mark.parametrize("shape", [132, 164, 32, 5132, 6064])
def test_saturated_dcnpost_winograd_x3(dev, shape):
    """the geometry of test_conv3x3_winograd_x3_epilogues on the split-operand Winograd kernel"""
    from e2fgvi_amd import ops
    x, w, fl = _fp32_case(3004, 2, 30, 54, 1 / math.sqrt(128 * 9))
    b = sat_values(432)
    raw = conv64(x, w, b, padding=1)
    layer = ops.PackedConv(w.to(dev), b.to(dev), [128], pad=1, algo="winograd")
    out = layer([nhwc(x).to(dev)], residual=fl.to(dev), act=ops.ACT_DCNPOST, slope=10.0, tile=ops.W3_BASE + shape)
    check_dcnpost(nchw(out.cpu()), raw, fl, 5e-5, "saturated DCNPOST, split-operand Winograd shape %d" % shape)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_saturated_dcnpost_16bit(dev, dtype):
    """the geometry of test_conv_bf16x_dcn_postprocess: 16-bit operands (the reference takes the same rounded values), fp32
    accumulation, bias and epilogue, fp32 result"""
    from e2fgvi_amd import ops
    g = _gen(3005)
    N, H, W, dg = 1, 12, 20, 16
    x = torch.randn(N, H, W, 128, generator=g).to(dtype)
    w = torch.randn(27 * dg, 128, 3, 3, generator=g) * (0.3 / math.sqrt(128 * 9))
    fl = torch.randn(N, H, W, 4, generator=g) * 3
    b = sat_values(27 * dg)
    raw = conv64(nchw(x.float()), w.to(dtype).float(), b, padding=1)
    layer = ops.PackedConvX(w.to(dev), b.to(dev), [128], pad=1, dtype=dtype)
    for tile in (0, 1, 5):
        out = layer([x.to(dev)], out_dtype=torch.float32, residual=fl.to(dev), act=ops.ACT_DCNPOST, slope=10.0, tile=tile)
        check_dcnpost(nchw(out.cpu()), raw, fl, 5e-5, "saturated DCNPOST, %s conv tile %d" % (dtype, tile))


# ------------------------------------------------------------------------------------------------ the deformable conv's own form
def _mdcn_case(seed, N, H, W, scale, rounding=None):
    """two 128-channel sources, the raw conv_offset output with saturated channels, flows; the oracle on offsets and masks
    computed in float64"""
    from oracle.dcn import modulated_deform_conv2d
    g = _gen(seed)
    dg = 16
    a = torch.randn(N, 128, H, W, generator=g)
    c = torch.randn(N, 128, H, W, generator=g)
    if rounding is not None:
        a, c = a.to(rounding), c.to(rounding)
    raw = torch.randn(N, 432, H, W, generator=g) * scale + sat_values(432).view(1, 432, 1, 1)
    fl = torch.randn(N, H, W, 4, generator=g) * 2
    w = torch.randn(128, 256, 3, 3, generator=g) / 48
    if rounding == torch.float16:
        w = w.half().float()
    b = torch.randn(128, generator=g)
    fin, _ = dcnpost_ref(raw, fl)
    assert torch.isfinite(fin).all()
    ref = modulated_deform_conv2d(torch.cat([a, c], 1).float(), fin[:, :288].float(), fin[:, 288:].float(), w, b, 1, 1, 1, 1, dg)
    return a, c, raw, fl, w, b, ref, dg


@pytest.mark.parametrize("mfma,tiles", [("fp32", (0, 1, 2, 4, 5, 6)), ("x3", (0, 1, 2, 3, 4, 5, 6, 7))])
def test_saturated_mdcn_fused(dev, mfma, tiles):
    """the geometry of test_mdcn_e2fgvi_fused / test_mdcn_x3: flows=..., max_residue=10.0, every tile those tests run"""
    from e2fgvi_amd import ops
    a, c, raw, fl, w, b, ref, dg = _mdcn_case(3006, 1, 30, 54, 0.5)
    layer = ops.PackedDcn(w.to(dev), b.to(dev), dg, pad=1, mfma=mfma)
    srcs = [nhwc(a).to(dev), nhwc(c).to(dev)]
    for tile in tiles:
        out = layer(srcs, nhwc(raw).to(dev), flows=fl.to(dev), max_residue=10.0, tile=tile)
        assert_close(nchw(out.cpu()), ref, 5e-5, "saturated mdcn %s fused tile %d" % (mfma, tile))


@pytest.mark.parametrize("tile", [0, 1, 2, 4, 5, 6, 7, 101, 106])
def test_saturated_mdcn_bf16(dev, tile):
    """the geometry and bound of test_mdcn_bf16_mfma, bf16 sources, the post-processing fused as the bf16 path calls it"""
    from e2fgvi_amd import ops
    a, c, raw, fl, w, b, ref, dg = _mdcn_case(3007, 1, 14, 22, 0.7, torch.bfloat16)
    layer = ops.PackedDcn(w.to(dev), b.to(dev), dg, pad=1, mfma="bf16")
    out = layer([nhwc(a).contiguous().to(dev), nhwc(c).contiguous().to(dev)], nhwc(raw).to(dev), flows=fl.to(dev), max_residue=10.0, tile=tile)
    assert_close(nchw(out.cpu()), ref, 1.5e-2, "saturated mdcn bf16 fused tile %d" % tile)


@pytest.mark.parametrize("tile", [0, 1, 2, 5, 7, 101])
def test_saturated_mdcn_f16_planar(dev, tile):
    """the geometry and bound of test_mdcn_f16_planar: fp16 planar sources, fp16 weights and products"""
    from e2fgvi_amd import ops
    a, c, raw, fl, w, b, ref, dg = _mdcn_case(3008, 1, 14, 22, 0.7, torch.float16)
    layer = ops.PackedDcn(w.to(dev), b.to(dev), dg, pad=1, mfma="fp16")
    xs = [ops.to_planar16(nhwc(a).contiguous().to(dev)), ops.to_planar16(nhwc(c).contiguous().to(dev))]
    out = layer(xs, nhwc(raw).to(dev), flows=fl.to(dev), max_residue=10.0, tile=tile, planar=True)
    assert_close(nchw(out.cpu()), ref, 3e-3, "saturated mdcn fp16 planar fused tile %d" % tile)


# ------------------------------------------------------------------------------------------------ LayerNorm off unit scale
def test_layernorm_off_unit_scale(dev):
    """C = 512, fp32 output, against F.layer_norm in float64 on the same fp32 inputs.  The kernel sums a row in at most 14
    roundings on the way to the mean (4 + 4 adds per lane, 6 shuffle steps), each <= 2^-24 of |mean| x the partial's share, so the
    mean is off by <= ~16 x 2^-24 |mean| and every output by that over std: allowed 5e-6 (the unit-scale bound of
    test_layernorm_and_pool) + 16 x 2^-24 x |mean| / std, relative to rms(ref).  Rows constant at 3.0: every partial sum is exact,
    the centred row is exactly 0 and the output is beta, bit for bit."""
    from e2fgvi_amd import ops
    g = _gen(3010)
    Cc, rows = 512, 37
    gm, bt = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    const = ops.layernorm(torch.full((rows, Cc), 3.0).to(dev), gm.to(dev), bt.to(dev))
    assert torch.equal(const.cpu(), bt.expand(rows, Cc)), "constant rows: the output is not beta"
    cases = [("N(64, 1)", torch.randn(rows, Cc, generator=g) + 64), ("N(4096, 1)", torch.randn(rows, Cc, generator=g) + 4096),
             ("N(0, 1) x 2^-40", torch.randn(rows, Cc, generator=g) * 2.0 ** -40),
             ("N(0, 1) x 2^40", torch.randn(rows, Cc, generator=g) * 2.0 ** 40)]
    for name, x in cases:
        xd = x.double()
        ratio = (xd.mean(1).abs() / xd.std(1, unbiased=False)).max().item()
        ref = F.layer_norm(xd, (Cc,), gm.double(), bt.double(), 1e-5)
        out = ops.layernorm(x.to(dev), gm.to(dev), bt.to(dev))
        assert_close(out.cpu(), ref, 5e-6 + 16 * 2.0 ** -24 * ratio, "layernorm rows %s" % name)
