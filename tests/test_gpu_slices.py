"""No kernel reads or writes outside its operands' slices (include/e2fgvi_hip.h, "Operands are slices"; DESIGN.md, same title).

Every float entry point, at the case lists and forced tiles of its own tests, is run three times: (A) the tight call those tests
make, (B) the same call with every source, residual, flow, offset, mask and table inside a NaN-poisoned arena -- channel offsets,
pixel strides wider than the slice, guards of an image row in front and behind -- and every destination inside an arena prefilled
with a NaN of a distinctive payload, (C) the float64 reference of the family's test.  Asserted (tests/embedding.py):
  1. B's slice is finite and within the family's own tolerance of C (the functions and numbers are imported, none is new);
  2. B's slice is bit-identical to A: strides and neighbours change no bit;
  3. no element of a destination arena outside the slice lost the sentinel's bits;
  4. every input arena is bit-equal to its snapshot.
0 * NaN = NaN: a kernel that loads a neighbour's channel against a zero-packed weight, or re-reads valid data against zero
weights across a slice boundary, is right on finite data and fails 1 here.  A launcher that refuses an embedded layout raises: a
failure, never a skip."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests import embedding as E
from tests import helper_cases as K
from tests import mdcn_cases as M
from tests import test_gpu_bf16x as TB
from tests import test_gpu_fp16 as TH
from tests import test_gpu_mdcn_geometry as TM
from tests import test_gpu_ops as TO
from tests import test_gpu_tail as TT
from tests import test_gpu_wino4 as TW
from tests import test_gpu_x3_halo as TXH
from tests.util import (assert_close, assert_close_bf16, assert_one_conv_launch, fp32_tol, gen, launch_trace, name_seed, nchw,
                        nhwc)

pytestmark = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# Cases whose embedded call takes, by the launcher's design, another code path than the tight one (an alignment-dependent vector
# path, say) and are therefore exempt from assertion 2 -- 1, 3 and 4 hold for them all the same.  {case id: "file:line of the
# launcher's decision"}.  It must not grow silently: the length is asserted below.
BIT_EXEMPT = {}
N_BIT_EXEMPT = 0

CASES = []          # (id, function(dev)) -- filled below, one pytest case each
_RAN = []


def case(cid):
    def reg(fn):
        CASES.append((cid, fn))
        return fn
    return reg


def _up(v, g):
    return -(-v // g) * g


def _tight(cid, A):
    return None if cid in BIT_EXEMPT else A


# ===================================================================================================== convolutions
def _virtual_concat(srcs, cpg, groups):
    """NHWC sources -> the NCHW input of the equivalent grouped conv: group gi takes channels [gi*c, (gi+1)*c) of every source"""
    return nchw(torch.cat([torch.cat([s[..., gi * c:(gi + 1) * c].float() for s, c in zip(srcs, cpg)], -1) for gi in range(groups)], -1))


def _conv_data(seed, N, H, W, cpg, groups, Cout, k, dtype=F32):
    """sources (NHWC, `dtype`), weight and bias (fp32; the weight rounded to `dtype`) of a case, drawn once"""
    g = gen(seed)
    srcs = [torch.randn(N, H, W, groups * c, generator=g).to(dtype) for c in cpg]
    cin_g = sum(cpg)
    w = (torch.randn(Cout, cin_g, k, k, generator=g) / math.sqrt(cin_g * k * k)).to(dtype).float()
    b = torch.randn(Cout, generator=g) * 0.5
    return g, srcs, w, b


def _embed_sources(dev, srcs, cpg, groups, G):
    """source s at channel G * (s + 1) of pixels of coff + groups * cpg[s] + G channels"""
    pairs, arenas = [], []
    for s, (t, c) in enumerate(zip(srcs, cpg)):
        coff = G * (s + 1)
        v, a = E.embed(t, ld=coff + groups * c + G, coff=coff, device=dev)
        pairs.append((v, coff))
        arenas.append(a)
    return pairs, arenas


def _embed_residual(dev, res, layout, G):
    """(view, coff, arena): "aligned" -- channel G of pixels of a multiple of G channels; "odd" -- channel 3 of Cout + 3;
    "guard" -- its own fixed layout ([pixel][4] flows), guards only"""
    Cr = res.shape[-1]
    if layout == "guard":
        v, a = E.embed(res, device=dev)
        return v, 0, a
    coff, ld = (3, Cr + 3) if layout == "odd" else (G, _up(2 * G + Cr, G))
    v, a = E.embed(res, ld=ld, coff=coff, device=dev)
    return v, coff, a


def conv_abc(dev, cid, what, layer, srcs, cpg, groups, G, kw, check, res=None, res_layout="aligned", out_dtype=F32, out_nchw=False,
             out2_dtype=None, symbol=None):
    """A (tight) and B (embedded) of one conv call through `layer` (PackedConv / PackedConvX), the slice checks, then
    check(B's slice on the host, what) for the family's tolerance against its reference"""
    from e2fgvi_amd import ops
    N, H, W, _ = srcs[0].shape
    Ho, Wo = layer.out_hw(H, W)
    Cout = layer.Cout
    kw = dict(kw, out_nchw=out_nchw)
    if isinstance(layer, ops.PackedConvX):
        kw["out_dtype"] = out_dtype
    a2 = torch.empty(N, Ho, Wo, Cout, dtype=out2_dtype, device=dev) if out2_dtype else None
    akw = dict(kw, out2=a2) if out2_dtype else kw
    A = layer([t.to(dev) for t in srcs], residual=None if res is None else res.to(dev), **akw)
    torch.cuda.synchronize()
    pairs, arenas = _embed_sources(dev, srcs, cpg, groups, G)
    rv, rc = None, 0
    if res is not None:
        rv, rc, ra = _embed_residual(dev, res, res_layout, G)
        arenas.append(ra)
    snaps = [(a, E.snapshot(a)) for a in arenas]
    if out_nchw:
        ov, oa = E.embed_like((N, Cout, Ho, Wo), F32, dev)
        oc, width = 0, Wo
    else:
        ov, oa = E.embed_like((N, Ho, Wo, Cout), out_dtype, dev, ld=_up(2 * G + Cout, G), coff=G)
        oc, width = G, Cout
    bkw = kw
    if out2_dtype:
        o2v, o2a = E.embed_like((N, Ho, Wo, Cout), out2_dtype, dev)
        bkw = dict(kw, out2=o2v)
    with launch_trace() as trace:
        layer(pairs, out=ov, out_coff=oc, residual=rv, res_coff=rc, **bkw)
    torch.cuda.synchronize()
    if symbol is not None:         # one launch through the asked-for entry point: a refused tile replaced by another kernel fails here
        assert_one_conv_launch(trace, symbol, tile=kw.get("tile"), what=what)
    got = E.check_slices(ov, oa, oc, width, tight=_tight(cid, A), sources=snaps, what=what)
    if out2_dtype:
        E.check_slices(o2v, o2a, 0, Cout, tight=_tight(cid, a2), what=what + " (out2)")
    check(got.cpu(), what)
    return got


def _closer(ref, tol):
    return lambda got, what: assert_close(got, ref, tol, what)


# ------------------------------------------------------------------------------------------- implicit GEMM, halo, row-staged tiles
def _igemm(dev, cid, row, nopk=False, out_nchw=False):
    from e2fgvi_amd import ops
    N, H, W, cpg, groups, Cout, k, stride, pad, act, use_res, tile, bk = row
    g, srcs, w, b = _conv_data(name_seed(cid), N, H, W, cpg, groups, Cout, k)
    ref = TO.conv64(_virtual_concat(srcs, cpg, groups), w, b, stride=stride, padding=pad, groups=groups)
    res = torch.randn(N, ref.shape[2], ref.shape[3], Cout, generator=g) if use_res else None
    if res is not None:
        ref = ref + nchw(res)
    ref = TO._act_ref(ref, act, 0.2)
    layer = ops.PackedConv(w.to(dev), b.to(dev), cpg, groups=groups, stride=stride, pad=pad, bk=bk)
    layer.nopk = nopk
    conv_abc(dev, cid, cid, layer, srcs, cpg, groups, 4, dict(act=act, slope=0.2, tile=tile),
             _closer(ref if out_nchw else nhwc(ref), fp32_tol(sum(cpg) * k * k)), res=res, out_nchw=out_nchw,
             symbol="e2fgvi_conv2d_nhwc_nopk" if nopk else "e2fgvi_conv2d_nhwc")


for _i, _row in enumerate(TO.CONV_CASES):
    case("igemm %02d %s" % (_i, "x".join(str(v) for v in _row)))(lambda dev, cid, row=_row: _igemm(dev, cid, row))
case("igemm nopk %s" % "x".join(str(v) for v in TO.CONV_CASES[6]))(lambda dev, cid: _igemm(dev, cid, TO.CONV_CASES[6], nopk=True))
case("igemm nchw out %s" % "x".join(str(v) for v in TO.CONV_CASES[20]))(lambda dev, cid: _igemm(dev, cid, TO.CONV_CASES[20], out_nchw=True))


def _linear(dev, cid, rows, cin, cout):
    """PackedLinear on 2-D operands, a 256-row GEMM tile of poison in front of and behind x, the residual and the result"""
    from e2fgvi_amd import ops
    g = gen(name_seed(cid))
    x = torch.randn(rows, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) / math.sqrt(cin)
    b = torch.randn(cout, generator=g)
    r = torch.randn(rows, cout, generator=g)
    lin = ops.PackedLinear(w.to(dev), b.to(dev))
    A = lin(x.to(dev), residual=r.to(dev))
    xv, xa = E.embed(x, device=dev)
    rv, ra = E.embed(r, device=dev)
    snaps = [(a, E.snapshot(a)) for a in (xa, ra)]
    ov, oa = E.embed_like((rows, cout), F32, dev)
    lin(xv, out=ov, residual=rv)
    torch.cuda.synchronize()
    got = E.check_slices(ov, oa, 0, cout, tight=_tight(cid, A), sources=snaps, what=cid)
    assert_close(got.cpu(), F.linear(x.double(), w.double(), b.double()) + r, fp32_tol(cin), cid)


for _shape in ((77, 512, 512), (130, 512, 1960)):
    case("linear %dx%d->%d" % _shape)(lambda dev, cid, s=_shape: _linear(dev, cid, *s))


# ------------------------------------------------------------------------------------------- Winograd F(2x2), F(2x4), split operands
def _wino_layer(dev, cid, N, H, W, cpg, groups, Cout, act):
    from e2fgvi_amd import ops
    g, srcs, w, b = _conv_data(name_seed(cid), N, H, W, cpg, groups, Cout, 3)
    ref = nhwc(TO._act_ref(TO.conv64(_virtual_concat(srcs, cpg, groups), w, b, stride=1, padding=1, groups=groups), act, 0.2))
    return srcs, ref, ops.PackedConv(w.to(dev), b.to(dev), cpg, groups=groups, stride=1, pad=1, algo="winograd")


def _wino(dev, cid, row, tiles, symbol, tol_of):
    N, H, W, cpg, groups, Cout, act = row
    srcs, ref, layer = _wino_layer(dev, cid, N, H, W, cpg, groups, Cout, act)
    for tile in tiles:
        conv_abc(dev, cid, "%s tile %d" % (cid, tile), layer, srcs, cpg, groups, 4, dict(act=act, slope=0.2, tile=tile),
                 _closer(ref, tol_of(sum(cpg))), symbol=symbol)


def _w3(shapes):
    from e2fgvi_amd import ops
    return tuple(ops.W3_BASE + s for s in shapes)


W3_SHAPES = (132, 164, 32, 5132, 6064)
for _i, _row in enumerate(TO.WINO_CASES):
    _name = "x".join(str(v) for v in _row[:7])
    case("wino %02d %s" % (_i, _name))(lambda dev, cid, row=_row[:7]: _wino(
        dev, cid, row, (32, 64, 132, 164), "e2fgvi_conv3x3_winograd", lambda cin: fp32_tol(cin * 9, floor=3e-5)))
    case("wino x3 %02d %s" % (_i, _name))(lambda dev, cid, row=_row[:7]: _wino(
        dev, cid, row, _w3(W3_SHAPES), "e2fgvi_conv3x3_winograd_x3", lambda cin: fp32_tol(cin * 9, floor=3e-5)))
for _i, _row in enumerate(TW.W4_CASES):
    case("wino4 %02d %s" % (_i, "x".join(str(v) for v in _row[:7])))(lambda dev, cid, row=_row[:7]: _wino(
        dev, cid, row, (2464,), "e2fgvi_conv3x3_winograd4", lambda cin: TW.wtol(2464, cin)))


def _wino_residual(dev, cid, H, W, tiles, symbol, tol):
    """the residual tests' shape (2 x 128 x H x W -> 128, LeakyReLU 0.1): residual at channel 4 of pixels of 136, and at channel 3
    of pixels of 131 (no 16-byte alignment)"""
    from e2fgvi_amd import ops
    g, srcs, w, b = _conv_data(name_seed(cid), 2, H, W, [128], 1, 128, 3)
    raw = TO.conv64(_virtual_concat(srcs, [128], 1), w, b, padding=1)
    layer = ops.PackedConv(w.to(dev), b.to(dev), [128], pad=1, algo="winograd")
    for layout in ("aligned", "odd"):
        res = torch.randn(2, H, W, 128, generator=g)
        ref = nhwc(F.leaky_relu(raw + nchw(res), 0.1))
        for tile in tiles:
            conv_abc(dev, cid, "%s %s residual tile %d" % (cid, layout, tile), layer, srcs, [128], 1, 4, dict(act=2, slope=0.1, tile=tile),
                     _closer(ref, tol), res=res, res_layout=layout, symbol=symbol)


def _wino_dcnpost(dev, cid, H, W, tiles, symbol, tol, make=None, dtype=F32):
    """ACT_DCNPOST (2 x 128 x H x W -> 432): the flows' [pixel][4] layout is fixed, so they get guards only.  make(w, b): another
    layer class on the same call (the implicit GEMM, the LDS-DMA GEMMs); the Winograd layer otherwise"""
    from e2fgvi_amd import ops
    g, srcs, w, b = _conv_data(name_seed(cid), 2, H, W, [128], 1, 432, 3, dtype=dtype)
    fl = torch.randn(2, H, W, 4, generator=g) * 3
    o1, o2, m = torch.chunk(TO.conv64(_virtual_concat(srcs, [128], 1), w, b, padding=1), 3, 1)
    off1, off2 = torch.chunk(10 * torch.tanh(torch.cat([o1, o2], 1)), 2, 1)
    f1, f2 = fl[..., 0:2].permute(0, 3, 1, 2), fl[..., 2:4].permute(0, 3, 1, 2)
    ref = nhwc(torch.cat([off1 + f1.flip(1).repeat(1, 72, 1, 1), off2 + f2.flip(1).repeat(1, 72, 1, 1), torch.sigmoid(m)], 1))
    layer = make(w.to(dev), b.to(dev)) if make else ops.PackedConv(w.to(dev), b.to(dev), [128], pad=1, algo="winograd")
    for tile in tiles:
        conv_abc(dev, cid, "%s tile %d" % (cid, tile), layer, srcs, [128], 1, 4 if dtype == F32 else 8,
                 dict(act=ops.ACT_DCNPOST, slope=10.0, tile=tile), _closer(ref, tol), res=fl, res_layout="guard", symbol=symbol)


case("wino residual")(lambda dev, cid: _wino_residual(dev, cid, 30, 54, (0, 64, 132), "e2fgvi_conv3x3_winograd", 3e-5))
case("wino dcnpost")(lambda dev, cid: _wino_dcnpost(dev, cid, 30, 54, (0, 32, 164), "e2fgvi_conv3x3_winograd", 5e-5))
case("wino4 residual")(lambda dev, cid: _wino_residual(dev, cid, 32, 56, (2464,), "e2fgvi_conv3x3_winograd4", TW.wtol(2464, 128)))
case("wino4 dcnpost")(lambda dev, cid: _wino_dcnpost(dev, cid, 32, 56, (2464,), "e2fgvi_conv3x3_winograd4", max(5e-5, 2 * TW.wtol(2464, 128))))
case("wino x3 residual")(lambda dev, cid: _wino_residual(dev, cid, 30, 54, _w3(W3_SHAPES), "e2fgvi_conv3x3_winograd_x3", 3e-5))
def _other_dcnpost(kind):
    """test_conv_dcn_postprocess_epilogue, test_conv_bf16x_dcn_postprocess and test_x3_dcn_postprocess_and_nchw: their sizes, tiles
    and bounds"""
    from e2fgvi_amd import ops
    if kind == "igemm":
        return dict(H=14, W=22, tiles=(0,), symbol="e2fgvi_conv2d_nhwc", tol=3e-5, make=lambda w, b: ops.PackedConv(w, b, [128], pad=1))
    if kind == "bf16x":
        return dict(H=12, W=20, tiles=(0, 1, 5), symbol="e2fgvi_conv2d_x", tol=5e-5, dtype=BF16, make=lambda w, b: ops.PackedConvX(w, b, [128], pad=1))
    return dict(H=14, W=22, tiles=(0,), symbol="e2fgvi_conv2d_x", tol=3e-5, make=lambda w, b: ops.PackedConvX(w, b, [128], pad=1, dtype=F32, x3=True))


for _kind in ("igemm", "bf16x", "x3"):
    case("%s dcnpost" % _kind)(lambda dev, cid, kind=_kind: _wino_dcnpost(dev, cid, **_other_dcnpost(kind)))
case("wino x3 dcnpost")(lambda dev, cid: _wino_dcnpost(dev, cid, 30, 54, _w3(W3_SHAPES), "e2fgvi_conv3x3_winograd_x3", 5e-5))


# ------------------------------------------------------------------------------------------- tail conv
_TAIL_TOL = {F32: 2e-5, BF16: 2e-5, F16: fp32_tol(64 * 9, floor=3e-5)}      # test_conv3x3_tail's and test_tail_f16's


def _tail(dev, cid, row, dtype):
    """source pixels of ld + granule channels of which the first 64 are read; the NCHW destination guarded"""
    from e2fgvi_amd import ops
    N, H, W, ld, act, use_bias = row
    g = gen(name_seed(cid))
    x = torch.randn(N, H, W, 64, generator=g).to(dtype)
    w = (torch.randn(3, 64, 3, 3, generator=g) / 24.0).to(dtype).float()
    b = torch.randn(3, generator=g) * 0.1 if use_bias else None
    ref = F.conv2d(nchw(x.float()).double(), w.double(), None if b is None else b.double(), padding=1)
    ref = torch.tanh(ref) if act == 3 else F.leaky_relu(ref, 0.2) if act == 2 else ref
    conv = ops.PackedTailConv(w.to(dev), None if b is None else b.to(dev), dtype=dtype)
    A = conv([x.to(dev)], act=act, slope=0.2)
    xv, xa = E.embed(x, ld=ld + (4 if dtype == F32 else 8), coff=0, device=dev)
    snap = E.snapshot(xa)
    ov, oa = E.embed_like((N, 3, H, W), F32, dev)
    conv([xv], out=ov, act=act, slope=0.2)
    torch.cuda.synchronize()
    got = E.check_slices(ov, oa, 0, W, tight=_tight(cid, A), sources=[(xa, snap)], what=cid)
    assert_close(got.cpu(), ref, _TAIL_TOL[dtype], cid)


for _row in TT.CASES:
    for _dt, _nm in ((F32, "fp32"), (BF16, "bf16"), (F16, "fp16")):
        case("tail %s %s" % ("x".join(str(v) for v in _row), _nm))(lambda dev, cid, row=_row, dt=_dt: _tail(dev, cid, row, dt))


# ------------------------------------------------------------------------------------------- LDS-DMA GEMMs: bf16 / fp16 / f32x / x3
def _x_layer(dev, cid, N, H, W, cpg, groups, Cout, k, stride, pad, dtype, **kw):
    from e2fgvi_amd import ops
    g, srcs, w, b = _conv_data(name_seed(cid), N, H, W, cpg, groups, Cout, k, dtype=dtype)
    ref0 = TB.conv64(_virtual_concat(srcs, cpg, groups), w, b, stride=stride, padding=pad, groups=groups)
    layer = ops.PackedConvX(w.to(dev), b.to(dev), cpg, groups=groups, stride=stride, pad=pad, dtype=dtype, **kw)
    return g, srcs, nhwc(ref0), layer


def _conv16(dev, cid, row, dtype):
    """test_conv_bf16x / test_conv_f16x: every tile with an fp32 result (LeakyReLU) and a 16-bit second copy; then 16-bit result with
    a 16-bit residual (ReLU), fp32 result with an fp32 residual, and the fp32 NCHW store"""
    from e2fgvi_amd import ops
    name, N, H, W, cpg, groups, Cout, k, stride, pad, tiles = row
    if tiles == "table":
        tiles = sorted(set(TH._bf16_table_tiles()) | {0, 11, 12, 13, 14, 16, 17, 18})
    g, srcs, ref0, layer = _x_layer(dev, cid, N, H, W, cpg, groups, Cout, k, stride, pad, dtype)
    tol = fp32_tol(sum(cpg) * k * k, floor=3e-5)
    res32 = torch.randn(ref0.shape, generator=g)
    res16 = res32.to(dtype)

    def close16(tile):
        """16-bit result: bf16 as test_conv_bf16x holds it; fp16 as test_conv_f16x does -- .half() of the fp32 result of the same call"""
        if dtype == BF16:
            return lambda got, what: assert_close_bf16(got.float(), F.relu(ref0 + res16.float()), what, abs_rms=1e-4)
        r32 = layer([t.to(dev) for t in srcs], out_dtype=F32, residual=res16.float().to(dev), act=ops.ACT_RELU, tile=tile).cpu()
        return lambda got, what: TH.assert_is_half_of(got, r32, what)
    for tile in tiles:
        if tile >= 10 and (k != 3 or stride != 1 or layer.taps):
            continue
        out32 = conv_abc(dev, cid, "%s tile %d fp32 out + out2" % (cid, tile), layer, srcs, cpg, groups, 8,
                         dict(act=ops.ACT_LRELU, slope=0.1, tile=tile), _closer(F.leaky_relu(ref0, 0.1), tol), out2_dtype=dtype,
                         symbol="e2fgvi_conv2d_x")
        o16 = conv_abc(dev, cid, "%s tile %d 16-bit out, 16-bit residual" % (cid, tile), layer, srcs, cpg, groups, 8,
                       dict(act=ops.ACT_RELU, tile=tile), close16(tile), res=res16, out_dtype=dtype,
                       symbol="e2fgvi_conv2d_x")
        del out32, o16
    conv_abc(dev, cid, cid + " fp32 residual", layer, srcs, cpg, groups, 8, dict(act=ops.ACT_NONE), _closer(ref0 + res32, tol), res=res32)
    if groups == 1:
        conv_abc(dev, cid, cid + " NCHW out", layer, srcs, cpg, groups, 8, dict(act=ops.ACT_TANH), _closer(nchw(torch.tanh(ref0)), tol),
                 out_nchw=True)


def _conv32x(dev, cid, row, x3):
    """test_conv_f32x / test_conv_x3: fp32 operands, fp32 residual, LeakyReLU, every tile of the case below 10 (x3: and 1, 5, 7, 8,
    107, 108); the fp32 NCHW store where groups == 1"""
    from e2fgvi_amd import ops
    name, N, H, W, cpg, groups, Cout, k, stride, pad, tiles = row
    g, srcs, ref0, layer = _x_layer(dev, cid, N, H, W, cpg, groups, Cout, k, stride, pad, F32, x3=x3)
    res = torch.randn(ref0.shape, generator=g)
    tol = fp32_tol(sum(cpg) * k * k)
    tiles = sorted(set(t for t in tiles if t < 10) | ({1, 5, 7, 8, 107, 108} if x3 else set()))
    for tile in tiles:
        conv_abc(dev, cid, "%s tile %d" % (cid, tile), layer, srcs, cpg, groups, 4, dict(act=ops.ACT_LRELU, slope=0.1, tile=tile),
                 _closer(F.leaky_relu(ref0 + res, 0.1), tol), res=res, symbol="e2fgvi_conv2d_x")
    if groups == 1:
        conv_abc(dev, cid, cid + " NCHW out", layer, srcs, cpg, groups, 4, dict(act=ops.ACT_NONE), _closer(nchw(ref0), tol), out_nchw=True)


def _conv32x_taps(dev, cid, row, x3):
    from e2fgvi_amd import ops
    name, N, H, W, cin, Cout, k, stride, pad, tiles = row
    g, srcs, ref0, layer = _x_layer(dev, cid, N, H, W, [cin], 1, Cout, k, stride, pad, F32, taps=True, x3=x3)
    assert layer.taps
    res = torch.randn(ref0.shape, generator=g)
    for tile in tiles:
        conv_abc(dev, cid, "%s tile %d" % (cid, tile), layer, srcs, [cin], 1, 4, dict(tile=tile), _closer(ref0 + res, fp32_tol(cin * k * k)),
                 res=res, symbol="e2fgvi_conv2d_x")


for _row in TB.CASES:
    case("bf16x " + _row[0])(lambda dev, cid, row=_row: _conv16(dev, cid, row, BF16))
    case("f32x " + _row[0])(lambda dev, cid, row=_row: _conv32x(dev, cid, row, False))
    case("x3 " + _row[0])(lambda dev, cid, row=_row: _conv32x(dev, cid, row, True))
for _row in TH.CASES:
    case("f16x " + _row[0])(lambda dev, cid, row=_row: _conv16(dev, cid, row, F16))
for _row in TB.F32_TAP_CASES:
    case("f32x taps " + _row[0])(lambda dev, cid, row=_row: _conv32x_taps(dev, cid, row, False))
    case("x3 taps " + _row[0])(lambda dev, cid, row=_row: _conv32x_taps(dev, cid, row, True))


def _halo_x3(dev, cid, row):
    """test_gpu_x3_halo.CASES on tiles 51 / 52; compared at unit scale as there"""
    from e2fgvi_amd import ops
    name, N, H, W, cin, cout, has_bias, act, has_res, scale = row
    g = gen(name_seed(cid))
    w = torch.randn(cout, cin, 7, 7, generator=g) / math.sqrt(cin * 49)
    b = torch.randn(cout, generator=g) * 0.1 if has_bias else None
    x = torch.randn(N, H, W, cin, generator=g) * scale
    ref = TB.conv64(nchw(x), w, b, padding=3)
    res = torch.randn(N, H, W, cout, generator=g) if has_res else None
    if has_res:
        ref = ref + nchw(res).double()
    ref = nhwc(F.relu(ref) if act else ref) / scale
    layer = ops.PackedConvX(w.to(dev), None if b is None else b.to(dev), [cin], pad=3, dtype=F32, x3=True)
    for tile in TXH.HALO_TILES:
        conv_abc(dev, cid, "%s tile %d" % (cid, tile), layer, [x], [cin], 1, 4, dict(act=ops.ACT_RELU if act else ops.ACT_NONE, tile=tile),
                 lambda got, what: assert_close(got.double() / scale, ref, fp32_tol(cin * 49), what), res=res, symbol="e2fgvi_conv2d_x")


for _row in TXH.CASES:
    case("x3 halo " + _row[0])(lambda dev, cid, row=_row: _halo_x3(dev, cid, row))


def _qkv_planes(dev, cid, rows):
    """test_qkv_epilogue_writes_the_attention_planes: the split-operand GEMM writes the Q columns to the fp32 rows and the K / V
    columns to three bf16 planes.  Embedded: x, the fp32 rows and the planes each with a GEMM tile of guard rows; the K / V
    columns of the fp32 rows are outside what the call may store, so they must keep the sentinel as well."""
    from e2fgvi_amd import lib as L, ops
    g = gen(name_seed(cid))
    w = (torch.randn(1536, 512, generator=g) * 0.05)
    b = torch.randn(1536, generator=g)
    x = torch.randn(rows, 512, generator=g)
    ref = F.linear(x.double(), w.double(), b.double())
    layer = ops.PackedConvX(w.to(dev), b.to(dev), [512], dtype=F32, x3=True)
    x4 = x.to(dev).view(rows, 1, 1, 512)
    xv, xa = E.embed(x, device=dev)
    snap = E.snapshot(xa)
    ran = 0
    for tile in (1, 2, 4, 5, 6, 7, 8, 107, 108):
        full = torch.empty(rows, 1, 1, 1536, device=dev)
        try:
            layer([x4], out=full, tile=tile)
        except L.HipError:                       # a tile this row count does not admit, as in the tight test
            continue
        planes = torch.zeros(3, rows, 1024, dtype=BF16, device=dev)
        tight = torch.empty(rows, 1, 1, 1536, device=dev)
        layer([x4], out=tight, tile=tile, planes=planes, split_from=512)
        ov, oa = E.embed_like((rows, 1536), F32, dev)
        pv, pa = E.embed_like((3, rows, 1024), BF16, dev, guard=E.GEMM_TILE_ROWS * 1024)
        layer([xv.view(rows, 1, 1, 512)], out=ov.view(rows, 1, 1, 1536), tile=tile, planes=pv, split_from=512)
        torch.cuda.synchronize()
        what = "%s tile %d" % (cid, tile)
        got = E.check_slices(ov, oa, 0, 512, tight=_tight(cid, tight.view(rows, 1536)[:, :512]), sources=[(xa, snap)], what=what)
        E.check_slices(pv, pa, 0, 1024, tight=_tight(cid, planes), what=what + " planes")
        assert torch.equal(pv, ops.split3_kv(full.view(rows, 1536))), what + ": planes differ from split3_kv of the fp32 rows"
        assert_close(got.cpu(), ref[:, :512], fp32_tol(512), what)
        ran += 1
    assert ran >= 4, ran


for _rows in (256, 1000):
    case("x3 qkv planes rows %d" % _rows)(lambda dev, cid, rows=_rows: _qkv_planes(dev, cid, rows))


# ===================================================================================================== deformable conv
def _dcn_embedded(layer, srcs, offset, mask, flows, out, out_coff, tile, max_residue=10.0, planar=False):
    """e2fgvi_mdcn_nhwc with the descriptor filled as ops.PackedDcn.__call__ fills it, plus what that wrapper cannot say:
    srcs = [(tensor, channels read)] with rows wider than the channels read (src_ld > src_c), a destination channel offset"""
    from e2fgvi_amd import lib as L, ops
    d = L.MdcnDesc()
    t0 = srcs[0][0]
    N, H, W = t0.shape[1:4] if planar else t0.shape[:3]
    d.src_planar = int(planar)
    for i, (t, c) in enumerate(srcs):
        d.src[i], d.src_ld[i], d.src_c[i] = t.data_ptr(), (c if planar else t.shape[3]), c
    d.src_dtype, d.nsrc = ops._dt(t0), len(srcs)
    d.Ho = (H + 2 * layer.pad - (layer.dil * (layer.KH - 1) + 1)) // layer.stride + 1
    d.Wo = (W + 2 * layer.pad - (layer.dil * (layer.KW - 1) + 1)) // layer.stride + 1
    d.N, d.H, d.W = N, H, W
    d.KH, d.KW, d.stride, d.pad, d.dil = layer.KH, layer.KW, layer.stride, layer.pad, layer.dil
    d.deform_groups, d.Cout = layer.dg, layer.Cout
    d.offset, d.off_ld = offset.data_ptr(), offset.shape[3]
    if mask is None:
        d.mask, d.mask_ld = offset.data_ptr() + 4 * layer.dg * 2 * layer.KH * layer.KW, offset.shape[3]
    else:
        d.mask, d.mask_ld = mask.data_ptr(), mask.shape[3]
    if flows is not None:
        d.flows = flows.data_ptr()
    d.max_residue = max_residue
    d.wpacked = layer.wpacked.data_ptr()
    d.bias = layer.bias.data_ptr() if layer.bias is not None else None
    d.dst, d.dst_ld, d.dst_coff, d.tile, d.dst_dtype = out.data_ptr(), out.shape[3], out_coff, tile, ops._dt(out)
    d.mfma_dtype = layer._mfma_dtype
    L.check(L.load().e2fgvi_mdcn_nhwc(C.byref(d), ops._stream()), "mdcn_nhwc")


def _dcn(dev, cid, name, variant, form, tiles, planar=False):
    """form "generic": offsets and masks in their own guarded tensors; "one": one tensor 6 (7) columns wider than dg*3*K, the extra
    columns poisoned; "fused": the raw conv_offset output and the flows.  Both sources in rows G channels wider than what is read
    (planar sources: their layout is fixed, guards only), the destination at channel G of wider pixels; fp32 results at every
    tile, and the 16-bit result of the 16-bit variants at the first."""
    from e2fgvi_amd import ops
    mfma, rounding, tol, _ = TM.VARIANTS[variant]
    c = M.fused_case(name, rounding) if form == "fused" else M.case(name, rounding)
    geo = c["geo"]
    layer, xs = TM._layer(dev, name, mfma), TM._sources(dev, c)
    G = 4 if rounding is None else 8
    kw = {}
    if form == "fused":
        tight_args = (nhwc(c["raw"]),)
        kw = dict(flows=nhwc(c["flows"]), max_residue=M.MAX_RESIDUE)
    elif form == "one":       # (A is the generic form at the same tile: test_one_tensor_form holds the two bit-equal, and an odd
        cols = geo.dg * 3 * geo.K                        # dg*3*K is no row stride the library takes)
        tight_args = (nhwc(c["off"]),)
        kw = dict(mask=nhwc(c["msk"]))
        wide = cols + 6 + (cols + 6) % 2
    else:
        tight_args = (nhwc(c["off"]),)
        kw = dict(mask=nhwc(c["msk"]))
    if planar:
        xs = [ops.to_planar16(x) for x in xs]
    # B's operands
    arenas = []

    def emb(t, **k):
        v, a = E.embed(t, device=dev, **k)
        arenas.append(a)
        return v
    if planar:
        bsrc = [(emb(x), x.shape[0] * 16) for x in xs]
    else:
        bsrc = [(emb(x, ld=x.shape[3] + G, coff=0), x.shape[3]) for x in xs]
    if form == "one":
        boff, bmask = emb(torch.cat((tight_args[0], kw["mask"]), 3), ld=wide, coff=0), None
    else:
        boff, bmask = emb(tight_args[0]), emb(kw["mask"]) if "mask" in kw else None
    bflows = emb(kw["flows"]) if "flows" in kw else None
    snaps = [(a, E.snapshot(a)) for a in arenas]
    targs = [t.to(dev) for t in tight_args]
    tkw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    runs = [(tile, F32) for tile in tiles] + ([(tiles[0], rounding)] if rounding is not None else [])
    for tile, dt in runs:
        what = "%s tile %d -> %s" % (cid, tile, dt)
        A = layer(xs, *targs, tile=tile, out_dtype=dt, planar=planar, **tkw)
        ov, oa = E.embed_like((geo.N, geo.Ho, geo.Wo, geo.Cout), dt, dev, ld=_up(2 * G + geo.Cout, G), coff=G)
        _dcn_embedded(layer, bsrc, boff, bmask, bflows, ov, G, tile, max_residue=kw.get("max_residue", 10.0), planar=planar)
        torch.cuda.synchronize()
        got = E.check_slices(ov, oa, G, geo.Cout, tight=_tight(cid, A), sources=snaps, what=what)
        assert_close(nchw(got.float().cpu()), c["ref"], tol, what)


# test_one_tensor_form's and test_fused_form's tiles; fp16 (which those two leave out) at the bf16 ones
_ONE_TILES = {"fp32": (1, 5, 103), "x3": (7,), "bf16": (6, 106), "fp16": (6, 106)}
for _v in TM.VARIANTS:
    for _n in ("one_pixel", "two_sources"):
        case("mdcn generic %s %s" % (_n, _v))(lambda dev, cid, n=_n, v=_v: _dcn(dev, cid, n, v, "generic", TM.VARIANTS[v][3]))
for _v in ("bf16", "fp16"):
    case("mdcn generic planar two_sources %s" % _v)(lambda dev, cid, v=_v: _dcn(
        dev, cid, "two_sources", v, "generic", [t for t in TM.VARIANTS[v][3] if t], planar=True))
for _v, _t in _ONE_TILES.items():
    case("mdcn one tensor wide_group %s" % _v)(lambda dev, cid, v=_v, t=_t: _dcn(dev, cid, "wide_group", v, "one", t))
for _v, _t in dict(TM.FUSED_TILES, fp16=TM.FUSED_TILES["bf16"]).items():
    case("mdcn fused two_sources %s" % _v)(lambda dev, cid, v=_v, t=_t: _dcn(dev, cid, "two_sources", v, "fused", t))


# ===================================================================================================== attention
ATT_SHAPES = ((1, 3, 10, 18), (2, 2, 20, 36))
_ATT = {}


def _att_data(B, T, fh, fw):
    """(xn, xp, qkv, kvp, tab, nk, sd) of a shape, test_focal_attention's construction, drawn once"""
    from e2fgvi_amd.engine import build_key_table
    from e2fgvi_amd.synth import rolled_valid_index
    from oracle import e2fgvi_oracle as O
    if (B, T, fh, fw) not in _ATT:
        g = gen(600 + fh)
        xn = torch.randn(B, T, fh, fw, 512, generator=g)
        sd = {"a.qkv.weight": torch.randn(1536, 512, generator=g) / math.sqrt(512) * 2.0, "a.qkv.bias": torch.randn(1536, generator=g) * 0.1,
              "pool_layers.0.weight": torch.full((1, 45), 1 / 45.) + 0.02 * torch.randn(1, 45, generator=g), "pool_layers.0.bias": torch.zeros(1)}
        xp = O.pool_windows(sd, "", xn)
        qkv = F.linear(xn.reshape(-1, 512), sd["a.qkv.weight"], sd["a.qkv.bias"])
        kvp = F.linear(xp.permute(0, 3, 1, 2, 4).reshape(-1, 512), sd["a.qkv.weight"], sd["a.qkv.bias"])
        tab, nk = build_key_table(fh, fw, rolled_valid_index().tolist())
        _ATT[B, T, fh, fw] = (xn, xp, qkv, kvp, torch.from_numpy(tab), torch.from_numpy(nk), sd)
    return _ATT[B, T, fh, fw]


def _att_ref(B, T, fh, fw, rows16=None):
    """the oracle's roll / partition / cat / softmax chain: in fp32 on the fp32 rows, or on the given 16-bit-rounded rows"""
    from oracle import e2fgvi_oracle as O
    key = (B, T, fh, fw, "ref", None if rows16 is None else rows16[0].dtype)
    if key not in _ATT:
        xn, xp, qkv, kvp, tab, nk, sd = _att_data(B, T, fh, fw)
        if rows16 is None:
            pre = O.window_attention(sd, "a.", xn, xp, preproj=True)
        else:
            pre = O.window_attention({}, "a.", xn, xp, preproj=True, qkv_rows=rows16[0].float().view(B, T, fh, fw, 1536),
                                     qkv_pool_rows=rows16[1].float().view(B, T, fh // 5, fw // 9, 1536))
        _ATT[key] = O.window_reverse(pre, B, T, fh, fw).reshape(-1, 512)
    return _ATT[key]


def _att_tables(dev, tab, nk, ntok):
    """the engine's key table with every entry past nkeys[win] replaced by a valid but wrong reference, in a guarded arena.  (The
    engine's own table holds 0 there, so 0 would change nothing: the last token stands in the rows, 0 in the guards.)"""
    wrong = tab.clone()
    for w_ in range(tab.shape[0]):
        wrong[w_, int(nk[w_]):] = ntok - 1
    tv, ta = E.embed(wrong, poison=0, device=dev)
    nv, na = E.embed(nk, poison=0, device=dev)
    return tv, nv, [ta, na]


def _attention(dev, cid, B, T, fh, fw, kind, variants):
    from e2fgvi_amd import ops
    xn, xp, qkv, kvp, tab, nk, sd = _att_data(B, T, fh, fw)
    rows, ntok = qkv.shape[0], fh * fw
    dt = {"bf16": BF16, "fp16": F16}.get(kind, F32)
    if kind == "fp16":                  # test_focal_attention_f16's rows and its reference (the key table's definition, in fp32)
        g = gen(name_seed(cid))
        qkv, kvp = (torch.randn(qkv.shape, generator=g) * 1.5).half(), (torch.randn(kvp.shape, generator=g) * 1.5).half()
        ref = TH._attention_ref(qkv.to(dev), kvp.to(dev), tab.to(dev), nk, B, T, fh, fw).cpu()
    elif kind == "bf16":
        qkv, kvp = qkv.bfloat16(), kvp.bfloat16()
        ref = _att_ref(B, T, fh, fw, (qkv, kvp))
    else:
        ref = _att_ref(B, T, fh, fw)
    both = torch.cat([qkv, kvp], 0)
    both_d = both.to(dev)
    tab_d, nk_d = tab.to(dev), nk.to(dev)
    tv, nv, tab_arenas = _att_tables(dev, tab, nk, ntok)

    def close(got, what):
        if kind == "bf16":
            assert_close_bf16(got, ref, what, ulps=1.0, abs_rms=1.2e-2)
        elif kind == "fp16":
            TH.assert_close_f16(got, ref, what, ulps=1.0, abs_rms=2e-3)
        else:
            assert_close(got, ref, TO.ATT_TOL, what)

    def run(q, p, t_, n_, out, variant):
        if kind == "fp32":
            return ops.focal_attention(q, p, t_, n_, B, T, fh, fw, out=out, waves=variant)
        if kind == "x3":
            return ops.focal_attention_x3(q, p, t_, n_, B, T, fh, fw, out=out, waves=variant)
        return ops.focal_attention_bf16(q, p, t_, n_, B, T, fh, fw, out=out, variant=variant or None)
    # layout 1: qkv and kv_pool the two halves of one guarded allocation, as the engine lays them out; layout 2: each its own arena
    bv, ba = E.embed(both, device=dev)
    qv, qa = E.embed(qkv, device=dev)
    kv_, ka = E.embed(kvp, device=dev)
    if kind == "x3":                    # the K / V operand is the three planes of all rows: guards around them
        planes = ops.split3_kv(both_d)
        pv, pa = E.embed(planes.cpu(), guard=E.GEMM_TILE_ROWS * 1024, device=dev)
        tight_p = planes
        layouts = [("one allocation", bv[:rows], pv, [ba, pa]), ("own arenas", qv, pv, [qa, pa])]
    else:
        tight_p = both_d[rows:]
        layouts = [("one allocation", bv[:rows], bv[rows:], [ba]), ("own arenas", qv, kv_, [qa, ka])]
    for variant in variants:
        A = run(both_d[:rows], tight_p, tab_d, nk_d, None, variant)
        for lname, q, p, arenas in layouts:
            what = "%s variant %s, %s" % (cid, variant, lname)
            snaps = [(a, E.snapshot(a)) for a in arenas + tab_arenas]
            ov, oa = E.embed_like((rows, 512), dt, dev)
            run(q, p, tv, nv, ov, variant)
            torch.cuda.synchronize()
            got = E.check_slices(ov, oa, 0, 512, tight=_tight(cid, A), sources=snaps, what=what)
            close(got.cpu(), what)


_ATT_VARIANTS = {"fp32": {s: (0, 2, 4, 12, 14, 22, 24, 32, 34) for s in ATT_SHAPES}, "x3": {s: (0, 2, 4, 8, 14) for s in ATT_SHAPES},
                 "bf16": {s: (0, 1, 12, 14, 18, 22, 24, 28) for s in ATT_SHAPES},
                 "fp16": {ATT_SHAPES[0]: (1, 12, 14, 18, 22, 24, 28), ATT_SHAPES[1]: (0, 1, 14, 24)}}
for _k, _per in _ATT_VARIANTS.items():
    for _s, _vs in _per.items():
        case("attention %s %dx%dx%dx%d" % ((_k,) + _s))(lambda dev, cid, k=_k, s=_s, vs=_vs: _attention(dev, cid, *s, k, vs))


# ===================================================================================================== helpers
class _GuardedAllocations:
    """stands in for the `torch` module inside e2fgvi_amd.ops: every tensor a wrapper allocates for its result comes out of an arena
    prefilled with the sentinel, so results the caller cannot pass in are guarded like the ones it can"""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _new(self, shape, dtype, device, zero):
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
        v, a = E.embed_like(shape, dtype or F32, device)
        if zero:
            v.zero_()
        self.made.append((v, a))
        return v

    def empty(self, *shape, dtype=None, device=None):
        return self._new(shape, dtype, device, False)

    def zeros(self, *shape, dtype=None, device=None):
        return self._new(shape, dtype, device, True)


def helper_ab(dev, cid, what, fn, tight_args, emb_args, arenas, outs=()):
    """A = fn(*tight_args); B = fn(*emb_args) with the wrapper's own allocations guarded.  `outs`: (view, arena) of destinations
    passed in by the caller among emb_args.  Every result of B: untouched around it, finite, bit-equal to A's; returns B's results"""
    from e2fgvi_amd import ops
    A = fn(*tight_args)
    A = A if isinstance(A, tuple) else (A,)
    torch.cuda.synchronize()
    snaps = [(a, E.snapshot(a)) for a in arenas]
    proxy = _GuardedAllocations()
    ops.torch = proxy
    try:
        Bt = fn(*emb_args)
    finally:
        ops.torch = torch
    Bt = Bt if isinstance(Bt, tuple) else (Bt,)
    torch.cuda.synchronize()
    arena_of = {v.data_ptr(): a for v, a in list(proxy.made) + list(outs)}
    assert len(A) == len(Bt)
    res = []
    for i, (a_, b_) in enumerate(zip(A, Bt)):
        assert b_.data_ptr() in arena_of, "%s: result %d is not in a guarded arena" % (what, i)
        res.append(E.check_slices(b_, arena_of[b_.data_ptr()], 0, b_.shape[-1], tight=_tight(cid, a_), sources=snaps if i == 0 else (),
                                  what="%s result %d" % (what, i)))
    return res


def _g(dev, t, arenas, **kw):
    v, a = E.embed(t, device=dev, **kw)
    arenas.append(a)
    return v


@case("helper nchw_to_nhwc")
def _h_nchw_to_nhwc(dev, cid):
    """C = 3 into pixels of 4 and of 8, C = 5 into pixels of 12, all three output types: the pad channels are written as zeros
    (they are inside the destination), the guards keep the sentinel; x * 0.5 + 0.5 is one fp32 rounding, the store one more"""
    from e2fgvi_amd import ops
    for Cc, ld in ((3, 4), (3, 8), (5, 12)):
        x = torch.randn(2, Cc, 11, 13, generator=gen(name_seed(cid) + ld))
        ref = F.pad(nhwc(x * 0.5 + 0.5), (0, ld - Cc))
        for dt in (F32, BF16, F16):
            arenas = []
            xv = _g(dev, x, arenas)
            got, = helper_ab(dev, cid, "%s C=%d ld=%d %s" % (cid, Cc, ld, dt), lambda t: ops.nchw_to_nhwc(t, ld=ld, scale=0.5, shift=0.5, out_dtype=dt),
                             (x.to(dev),), (xv,), arenas)
            assert torch.equal(E.bits(got.cpu()), E.bits(ref.to(dt))), (Cc, ld, dt)
            assert int(E.bits(got[..., Cc:]).abs().max()) == 0, "pad channels must be +0"


@case("helper nhwc_to_nchw ld > C")
def _h_nhwc_to_nchw(dev, cid):
    from e2fgvi_amd import ops
    x = torch.randn(3, 21, 45, 37, generator=gen(name_seed(cid)))
    arenas = []
    xv = _g(dev, x, arenas, ld=40, coff=0)
    tight = F.pad(x, (0, 3)).to(dev)
    got, = helper_ab(dev, cid, cid, lambda t: ops.nhwc_to_nchw(t, channels=37), (tight,), (xv,), arenas)
    assert torch.equal(got.cpu(), nchw(x))


@case("helper resize_bilinear")
def _h_resize(dev, cid):
    """channels = 3 of a source of pixels of 4 (the fourth poisoned) into pixels of 4 (the fourth zero), both align_corners; and the
    vec4 kernel at test_resize_vec4_path's shape"""
    from e2fgvi_amd import ops
    for name in ("resize general align 13x7->7x13 C3", "resize general half 13x7->7x13 C3"):
        c = K.case(name)
        x, (Ho, Wo), sc, sh = c["x"], c["out_hw"], c["scale"].to(dev), c["shift"].to(dev)
        arenas = []
        xv = _g(dev, x, arenas, ld=4, coff=0)
        got, = helper_ab(dev, cid, name, lambda t: ops.resize_bilinear(t, (Ho, Wo), c["align"], channels=3, out_ld=4, scale=sc, shift=sh),
                         (F.pad(x, (0, 1)).to(dev),), (xv,), arenas)
        assert int(E.bits(got[..., 3]).abs().max()) == 0, name + ": pad channel"
        K.check(got[..., :3], K.reference(c)[0], K.allowed(c)[0], name)
    x = torch.randn(2, 64, 30, 54, generator=gen(21))
    arenas = []
    xv = _g(dev, nhwc(x), arenas)
    got, = helper_ab(dev, cid, "resize vec4", lambda t: ops.resize_bilinear(t, (60, 108), True), (nhwc(x).to(dev),), (xv,), arenas)
    assert_close(got.cpu(), nhwc(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)), 2e-6, "resize vec4")


@case("helper prop_cond")
def _h_prop_cond(dev, cid):
    """fp32 and 16-bit sources and cond, with and without flow_b, the flows again as an 8-channel source: feat_n2 in pixels 8
    channels wider than C, the flows of all images and steps in one guarded tensor, cond and flows passed in guarded"""
    from e2fgvi_amd import ops
    c0 = K.case("prop general 5x7 C16")
    for with_b in (True, False):
        for dt in (F32, BF16, F16):
            c = dict(c0, ib=c0["ib"] if with_b else None)
            if dt != F32:
                c = dict(c, fp=c["fp"].to(dt).float(), f2=c["f2"].to(dt).float())
            ref, allowed = K.reference(c), K.allowed(c)
            N, T, H, W, _ = c["flows"].shape
            Cc = c["fp"].shape[3]
            fp, f2 = c["fp"].to(dt), c["f2"].to(dt)
            what = "%s flow_b=%s %s" % (cid, with_b, dt)
            arenas = []
            fpv, f2v, flv = _g(dev, fp, arenas), _g(dev, f2, arenas, ld=Cc + 8, coff=0), _g(dev, c["flows"], arenas)
            condv, conda = E.embed_like((N, H, W, 2 * Cc), dt, dev)
            flowv, flowa = E.embed_like((N, H, W, 4), F32, dev)
            fl = c["flows"].to(dev)

            def run(fp_, f2_, fl_, cond, flows):
                return ops.prop_cond(fp_, f2_ if with_b else None, fl_[0, c["ia"]], fl_[0, c["ib"]] if with_b else None, T * H * W * 2,
                                     cond=cond, flows=flows, cond_dtype=dt, flows8=True)
            cond, flows, fl8 = helper_ab(dev, cid, what, run, (fp.to(dev), f2.to(dev), fl, None, None), (fpv, f2v, flv, condv, flowv), arenas,
                                         outs=[(condv, conda), (flowv, flowa)])
            K.check(cond, ref[0], allowed[0], what + " cond", dt)
            K.check(flows, ref[1], allowed[1], what + " flows")
            K.check(fl8[..., :4], ref[1], allowed[1], what + " flows8", fl8.dtype)
            assert int(E.bits(fl8[..., 4:]).abs().max()) == 0, what + ": flows8 channels 4..7"


@case("helper spynet_level_input, avgpool2")
def _h_spynet(dev, cid):
    from e2fgvi_amd import ops
    c = K.case("spynet general 4x6")
    arenas = []
    pyr, fprev = _g(dev, c["pyr"], arenas), _g(dev, c["flow_prev"], arenas)
    ids = [torch.tensor(c[k], dtype=torch.int32) for k in ("ref_idx", "supp_idx")]
    idv = [_g(dev, t, arenas, poison=0) for t in ids]
    out, out16 = helper_ab(dev, cid, cid, lambda p, r, s, f: ops.spynet_level_input(p, r, s, f, copy_dtype=BF16),
                           (c["pyr"].to(dev), ids[0].to(dev), ids[1].to(dev), c["flow_prev"].to(dev)), (pyr, idv[0], idv[1], fprev), arenas)
    K.check(out, K.reference(c)[0], K.allowed(c)[0], cid)
    K.check(out16, K.reference(c)[0], K.allowed(c)[0], cid + " copy", BF16)
    c = K.case("avgpool 6x10 C3")
    arenas = []
    xv = _g(dev, c["x"], arenas)
    got, = helper_ab(dev, cid, "avgpool2", ops.avgpool2, (c["x"].to(dev),), (xv,), arenas)
    K.check_exact(got, K.reference(c)[0], "avgpool2")


@case("helper layernorm + window_pool into one buffer")
def _h_norm_pool(dev, cid):
    """the engine's layout (Engine.block): the LayerNorm result and the pooled windows are the two halves of one buffer -- neither
    call may touch the other half; fp32 and bf16"""
    from e2fgvi_amd import ops
    g = gen(name_seed(cid))
    BT, fh, fw, Cc = 3, 5, 9, 512
    rows, prow = BT * fh * fw, BT
    x = torch.randn(rows, Cc, generator=g) * 3 + 1
    gm, bt = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    w45, b1 = 1 / 45. + 0.02 * torch.randn(45, generator=g), torch.randn(1, generator=g)
    for dt in (F32, BF16):
        what = "%s %s" % (cid, dt)
        arenas = []
        xv, gv, bv, wv, b1v = [_g(dev, t, arenas) for t in (x, gm, bt, w45, b1)]
        snaps = [(a, E.snapshot(a)) for a in arenas]
        n1_t = ops.layernorm(x.to(dev), gm.to(dev), bt.to(dev), out_dtype=dt)
        pool_t = ops.window_pool(n1_t, w45.to(dev), b1.to(dev), BT, fh, fw)
        nbuf, narena = E.embed_like((rows + prow, Cc), dt, dev)
        ops.layernorm(xv, gv, bv, out=nbuf[:rows])
        torch.cuda.synchronize()
        n1 = E.check_slices(nbuf[:rows], narena, 0, Cc, tight=_tight(cid, n1_t), sources=snaps, what=what + " layernorm")
        before = E.snapshot(narena)
        ops.window_pool(nbuf[:rows], wv, b1v, BT, fh, fw, out=nbuf[rows:])
        torch.cuda.synchronize()
        after = E.snapshot(narena)
        g0 = (nbuf.data_ptr() - narena.data_ptr()) // narena.element_size() + rows * Cc
        before[g0:g0 + prow * Cc], after[g0:g0 + prow * Cc] = 0, 0
        assert torch.equal(before, after), what + ": window_pool changed elements outside its half of the buffer"
        for a, s in snaps:
            E.assert_sources_intact(a, s, what)
        pool = nbuf[rows:]
        assert torch.isfinite(pool.float()).all() and torch.equal(E.bits(pool), E.bits(pool_t)), what + " window_pool"
        cl = dict(kind="layernorm", exact=False, x=x, gamma=gm, beta=bt)
        K.check(n1, K.reference(cl)[0], K.allowed(cl)[0], what + " layernorm", dt)
        cp = dict(kind="window_pool", exact=False, x=n1.float().cpu().view(BT, fh, fw, Cc), w45=w45, b1=b1)
        K.check(pool, K.reference(cp)[0], K.allowed(cp)[0], what + " window_pool", dt)


@case("helper ffn_fold, ffn_unfold, softcomp_fold")
def _h_fold(dev, cid):
    """FFN fold / unfold with the GELU in either place and the SoftComp fold with bias and residual, fp32 and bf16, at helper_cases'
    4 x 7 image (H % 3 = 1, W % 3 = 1) with 8 channels"""
    from e2fgvi_amd import ops
    c0 = K.case("fold general 4x7 C8")
    Fr, fh, fw, H, W, Cc = c0["dims"]
    for dt in (F32, BF16):
        c = c0 if dt == F32 else dict(c0, hid=c0["hid"].to(dt).float(), res=c0["res"].to(dt).float())
        ref, allowed = K.reference(c), K.allowed(c)
        hid, res, bias = c["hid"].to(dt), c["res"].to(dt), c["bias"]
        what = "%s %s" % (cid, dt)
        arenas = []
        hv, rv, bv = _g(dev, hid, arenas), _g(dev, res, arenas), _g(dev, bias, arenas)
        folded, = helper_ab(dev, cid, what + " ffn_fold", lambda h: ops.ffn_fold(h, *c["dims"]), (hid.to(dev),), (hv,), arenas[:1])
        K.check(folded, ref[0], allowed[0], what + " ffn_fold", dt)
        gel, = helper_ab(dev, cid, what + " ffn_fold_gelu", lambda h: ops.ffn_fold_gelu(h, *c["dims"]), (hid.to(dev),), (hv,), arenas[:1])
        if dt == F32:
            assert_close(gel.cpu(), F.gelu(ref[0]), 1e-5, what + " ffn_fold_gelu")
        for gelu, fn in ((0, ops.ffn_unfold), (1, ops.ffn_unfold_gelu)):
            farenas = []
            fv = _g(dev, folded.cpu(), farenas)
            uv, ua = E.embed_like((Fr * fh * fw, 49 * Cc), dt, dev)
            unf, = helper_ab(dev, cid, "%s ffn_unfold gelu=%d" % (what, gelu), lambda f_, o: fn(f_, fh, fw, out=o),
                             (folded.contiguous(), None), (fv, uv), farenas, outs=[(uv, ua)])
            if not gelu:          # a gather: the float64 gather of its own input, rounded back, bit for bit
                K.check_exact(unf, K.ffn_unfold_ref(folded.cpu(), fh, fw, False), what + " ffn_unfold")
            elif dt == F32:
                assert_close(unf.cpu(), K.ffn_unfold_ref(folded.cpu(), fh, fw, True), 1e-5, what + " ffn_unfold_gelu")
        sc, = helper_ab(dev, cid, what + " softcomp_fold", lambda h, b_, r: ops.softcomp_fold(h, *c["dims"], bias_hwc=b_, residual=r),
                        (hid.to(dev), bias.to(dev), res.to(dev)), (hv, bv, rv), arenas)
        K.check(sc, ref[2], allowed[2], what + " softcomp_fold", dt)


@case("helper SoftCompGather")
def _h_softcomp_gather(dev, cid):
    """test_softcomp_gather's smallest shape: tokens and result guarded; nine scattering launches into one destination"""
    from e2fgvi_amd import ops
    g = gen(name_seed(cid))
    F_, fh, fw, C_, hid = 2, 5, 9, 128, 512
    w = torch.randn(49 * C_, hid, generator=g) / math.sqrt(hid * 9)
    b = torch.randn(49 * C_, generator=g) * 0.1
    tok = torch.randn(F_, fh, fw, hid, generator=g)
    for dt in (F32, BF16):
        tok_r, w_r = (tok.to(dt).double(), w.to(dt).double())
        emb = F.linear(tok_r.view(F_, fh * fw, hid), w_r, b.double())
        ref = nhwc(F.fold(emb.permute(0, 2, 1), output_size=(3 * fh, 3 * fw), kernel_size=(7, 7), stride=(3, 3), padding=(3, 3)))
        layer = ops.SoftCompGather(w.to(dev), b.to(dev), C_, dtype=dt)
        what = "%s %s" % (cid, dt)
        A = layer(tok.to(dt).to(dev))
        arenas = []
        tv = _g(dev, tok.to(dt), arenas)
        snaps = [(a, E.snapshot(a)) for a in arenas]
        ov, oa = E.embed_like((F_, 3 * fh, 3 * fw, C_), dt, dev)
        layer(tv, out=ov)
        torch.cuda.synchronize()
        got = E.check_slices(ov, oa, 0, C_, tight=_tight(cid, A), sources=snaps, what=what)
        if dt == BF16:
            assert_close_bf16(got.float().cpu(), ref, what, abs_rms=1e-4)
        else:
            assert_close(got.cpu(), ref, fp32_tol(9 * hid), what)


@case("helper cast, split3_kv, to_planar16")
def _h_cast(dev, cid):
    from e2fgvi_amd import ops
    g = gen(name_seed(cid))
    x = torch.randn(260, generator=g) * torch.pow(2.0, torch.randint(-12, 12, (260,), generator=g).float())
    for src, dst in ((F32, BF16), (F32, F16), (BF16, F32), (F16, F32)):
        xs = x.to(src)
        arenas = []
        xv = _g(dev, xs, arenas)
        got, = helper_ab(dev, cid, "cast %s -> %s" % (src, dst), lambda t: ops.cast(t, dst), (xs.to(dev),), (xv,), arenas)
        assert torch.equal(E.bits(got.cpu()), E.bits(xs.to(dst)))
    rows = torch.randn(77, 1536, generator=g)
    arenas = []
    rv = _g(dev, rows, arenas)
    pv, pa = E.embed_like((3, 77, 1024), BF16, dev, guard=E.GEMM_TILE_ROWS * 1024)
    planes, = helper_ab(dev, cid, "split3_kv", lambda t, o: ops.split3_kv(t, out=o), (rows.to(dev), None), (rv, pv), arenas, outs=[(pv, pa)])
    assert torch.equal(planes.double().sum(0).cpu(), rows[:, 512:].double())
    x16 = torch.randn(2, 7, 9, 48, generator=g).bfloat16()
    arenas = []
    xv = _g(dev, x16, arenas)
    ov, oa = E.embed_like((3, 2, 7, 9, 16), BF16, dev)
    got, = helper_ab(dev, cid, "to_planar16", lambda t, o: ops.to_planar16(t, out=o), (x16.to(dev), None), (xv, ov), arenas, outs=[(ov, oa)])
    assert torch.equal(got.cpu(), x16.view(2, 7, 9, 3, 16).permute(3, 0, 1, 2, 4).contiguous())


# ===================================================================================================== the test
@pytest.mark.parametrize("cid,fn", CASES, ids=[c[0] for c in CASES])
def test_embedded(dev, cid, fn):
    fn(dev, cid)
    _RAN.append(cid)


def test_every_listed_case_ran(dev, request):
    """the cases of this module that were selected all ran to their end (none skipped, none excepted away), the ids are unique,
    and the list of cases exempt from bit-equality has the stated length"""
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)
    assert len(BIT_EXEMPT) == N_BIT_EXEMPT, "cases exempt from assertion 2: %s" % sorted(BIT_EXEMPT)
    selected = [it for it in request.session.items if it.fspath == request.node.fspath and getattr(it, "originalname", "") == "test_embedded"]
    if not request.config.getoption("keyword"):
        assert len(selected) == len(CASES), "%d cases listed, %d collected" % (len(CASES), len(selected))
    assert len(_RAN) == len(selected), "%d cases selected, %d ran" % (len(selected), len(_RAN))
    print("%d cases, %d embedded calls checked" % (len(_RAN), E.CHECKED[0]))
