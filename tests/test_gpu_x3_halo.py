"""The halo-staged split-operand 7x7 kernel (csrc/conv_bf16x.hip conv_halo_x3_kernel; tiles 51: 16x16-pixel tiles, 52: 8x16) --
SPyNet's 32 -> 64 and 64 -> 32 layers with the input patch staged and split once per 16-channel block instead of once per tap.
It is an fp32 kernel like the other split-operand tiles: against a float64 conv2d it meets tests/util.fp32_tol(Cin * 49), its error
stays within 1.5x of the implicit-GEMM tile's (3 / 5) on the same inputs plus 1e-6 of the output rms (tests/test_gpu_x3.py holds the
split GEMM to the same), reruns and runs on a side stream return the same bits, and what it does not cover answers EUNSUP."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_bf16x import conv64
from tests.util import assert_close, assert_one_conv_launch, err, fp32_tol, gen as _gen, launch_trace, name_seed, nchw, nhwc

pytestmark = pytest.mark.gpu

HALO_TILES = (51, 52)

# name, N, H, W, Cin, Cout, bias, act (0 none, 1 ReLU), residual, input scale
CASES = [
    ("2x4: smaller than a tile, all halo (SPyNet level 0)", 3, 2, 4, 32, 64, True, 0, False, 1.0),
    ("13x21: ragged in both axes, partial last tile", 2, 13, 21, 64, 32, True, 1, False, 1.0),
    ("16x32: exact tiles", 2, 16, 32, 32, 64, False, 1, False, 1.0),
    ("24x48: several tiles per image, residual", 2, 24, 48, 64, 32, True, 0, True, 1.0),
    ("13x21 32 -> 16: padded columns", 2, 13, 21, 32, 16, True, 1, False, 1.0),
    ("13x21 64 -> 64", 2, 13, 21, 64, 64, False, 0, False, 1.0),
    ("inputs x 1e-20", 2, 13, 21, 64, 64, False, 0, False, 1e-20),
    ("inputs x 1e+20", 2, 13, 21, 32, 32, False, 0, False, 1e+20),
]

_DATA = {}


def _data(case):
    """operands and the float64 reference of a case, computed once"""
    if case[0] in _DATA:
        return _DATA[case[0]]
    name, N, H, W, cin, cout, has_bias, act, has_res, scale = case
    g = _gen(name_seed(name, 31))
    w = torch.randn(cout, cin, 7, 7, generator=g) / math.sqrt(cin * 49)
    b = torch.randn(cout, generator=g) * 0.1 if has_bias else None
    wide = torch.randn(N, H, W, cin + 8, generator=g) * scale          # the source sits at channel 4 of a wider tensor
    ref = conv64(nchw(wide[..., 4:4 + cin]), w, b, padding=3)
    res = None
    if has_res:
        res = torch.randn(N, H, W, cout + 8, generator=g)              # ... and so does the residual (res_coff = 4)
        ref = ref + nchw(res[..., 4:4 + cout]).double()
    if act:
        ref = F.relu(ref)
    # (compared at unit scale, in float64: tests/util.err floors the reference's rms at 1e-12, far above the 1e-20 case's outputs)
    _DATA[case[0]] = (w, b, wide, res, nhwc(ref) / scale)
    return _DATA[case[0]]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_halo_tiles_against_float64(dev, case):
    from e2fgvi_amd import ops
    name, N, H, W, cin, cout, has_bias, act, has_res, scale = case
    w, b, wide, res, ref = _data(case)
    layer = ops.PackedConvX(w.to(dev), None if b is None else b.to(dev), [cin], pad=3, dtype=torch.float32, x3=True)
    srcs = [(wide.to(dev), 4)]
    kw = dict(residual=None if res is None else res.to(dev), res_coff=4 if has_res else 0, act=ops.ACT_RELU if act else ops.ACT_NONE)
    gemm_tile = 3 if cout <= 32 else 5
    e_gemm = err(layer(srcs, tile=gemm_tile, **kw).cpu().double() / scale, ref)[1]
    for tile in HALO_TILES:
        out = torch.full((N, H, W, cout + 12), 7.0, device=dev)        # the result in a channel slice of a pre-filled tensor
        with launch_trace() as trace:
            layer(srcs, out=out, out_coff=8, tile=tile, **kw)
        what = "%s, tile %d" % (name, tile)
        assert_one_conv_launch(trace, "e2fgvi_conv2d_x", tile=tile, kernel="conv_f32x3", what=what)
        assert bool((torch.cat([out[..., :8], out[..., 8 + cout:]], -1) == 7.0).all()), what + ": wrote outside its channel slice"
        got = out[..., 8:8 + cout].cpu().double() / scale
        _, e = assert_close(got, ref, fp32_tol(cin * 49), what)
        print("%s: %.2e of the output rms (tile %d: %.2e)" % (what, e, gemm_tile, e_gemm))
        assert e <= 1.5 * e_gemm + 1e-6, "%s: error %.3e against tile %d's %.3e" % (what, e, gemm_tile, e_gemm)


@pytest.mark.parametrize("why,cpg,cout,stride", [("stride 2", [32], 64, 2), ("two sources", [16, 16], 64, 1), ("Cin = 8", [8], 32, 1),
                                                 ("Cout = 96", [32], 96, 1)])
def test_rejected_calls_answer_eunsup_and_the_layer_falls_back(dev, why, cpg, cout, stride):
    from e2fgvi_amd import lib as L, ops
    g = _gen(name_seed(why, 37))
    cin = sum(cpg)
    w = (torch.randn(cout, cin, 7, 7, generator=g) / math.sqrt(cin * 49)).to(dev)
    srcs = [torch.randn(2, 13, 21, c, generator=g).to(dev) for c in cpg]
    layer = ops.PackedConvX(w, None, cpg, stride=stride, pad=3, dtype=torch.float32, x3=True)
    want = layer(srcs).clone()
    for tile in HALO_TILES:
        layer.tune = False
        with pytest.raises(L.HipError, match=r"code -2\)"):            # E2FGVI_EUNSUP
            layer(srcs, tile=tile)
        layer.tune = True                                              # a tabled tile the call rejects: the library's default runs
        assert torch.equal(layer(srcs, tile=tile), want), "%s, tile %d: not the fallback's result" % (why, tile)


def test_epilogue_variants_the_halo_tiles_do_not_cover_answer_eunsup(dev):
    from e2fgvi_amd import lib as L, ops
    g = _gen(41)
    w = (torch.randn(32, 32, 7, 7, generator=g) / 40).to(dev)
    x = torch.randn(2, 13, 21, 32, generator=g).to(dev)
    layer = ops.PackedConvX(w, None, [32], pad=3, dtype=torch.float32, x3=True)
    tapped = ops.PackedConvX(w, None, [32], pad=3, dtype=torch.float32, x3=True, taps=True)
    for tile in HALO_TILES:
        with pytest.raises(L.HipError, match=r"code -2\)"):
            layer([x], out=torch.empty(2, 32, 13, 21, device=dev), out_nchw=True, tile=tile)
        with pytest.raises(L.HipError, match=r"code -2\)"):
            layer([x], out_dtype=torch.bfloat16, tile=tile)
        with pytest.raises(L.HipError, match=r"code -2\)"):
            tapped([x], tile=tile)


def test_reruns_and_side_stream_runs_return_the_same_bits(dev):
    """50 reruns bit-identical; then the kernel on a side stream beside an encoder-sized split-operand Winograd launch on the main
    stream (what SPyNet's layers run beside in every forward: the class of hazard of DESIGN.md C1 / C4), 20 times: the bits of the
    serial run"""
    from e2fgvi_amd import ops
    g = _gen(43)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    x = rnd(18, 32, 64, 64)                                            # spynet.4.2's call
    layer = ops.PackedConvX(rnd(32, 64, 7, 7) / 56, rnd(32) * 0.1, [64], pad=3, dtype=torch.float32, x3=True)
    enc = ops.PackedConv(rnd(384, 256, 3, 3) * 0.02, rnd(384), [256], pad=1, algo="winograd")
    ex = rnd(10, 60, 108, 256)
    eout = torch.empty(10, 60, 108, 384, device=dev)
    wide = ops.W3_BASE + ops.W3_WIDE
    enc([ex], out=eout, act=ops.ACT_LRELU, slope=0.2, tile=wide)
    eref = eout.clone()
    side, main = torch.cuda.Stream(device=dev), torch.cuda.current_stream()
    for tile in HALO_TILES:
        first = layer([x], act=ops.ACT_RELU, tile=tile).clone()
        bad = sum(int(not torch.equal(layer([x], act=ops.ACT_RELU, tile=tile), first)) for _ in range(50))
        assert bad == 0, "tile %d: %d of 50 reruns differ" % (tile, bad)
        out = torch.empty_like(first)
        bad = 0
        for _ in range(20):
            out.fill_(float("nan"))
            eout.fill_(float("nan"))
            side.wait_stream(main)
            with torch.cuda.stream(side):
                for _ in range(3):
                    layer([x], out=out, act=ops.ACT_RELU, tile=tile)
            for _ in range(2):
                enc([ex], out=eout, act=ops.ACT_LRELU, slope=0.2, tile=wide)
            main.wait_stream(side)
            torch.cuda.synchronize()
            bad += int(not (torch.equal(out, first) and torch.equal(eout, eref)))
        assert bad == 0, "tile %d: %d of 20 runs beside the Winograd launch differ from the serial run" % (tile, bad)
