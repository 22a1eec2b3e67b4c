"""e2fgvi_mdcn_nhwc off the propagation's geometry and at the image borders: the cases of tests/mdcn_cases.py (stride, pad,
dilation, KH != KW, more than one 16-channel block per group, an odd unit count, fewer K chunks than K groups, a second and
partial column tile, two sources of unequal width, offsets that land ON the borders and the guard's edges) through every entry
form of ops.PackedDcn, against the float64 reference ref64.  The bounds are the ones the other DCN tests hold the same
arithmetic to: 5e-5 x rms for fp32 and the split-operand (x3) products, 1.5e-2 for bf16 products, 3e-3 for fp16; with 16-bit
sources the reference takes the same rounded sources.  tests/test_mdcn_cases.py shows that a kernel with a wrong border rule,
swapped axes, a wrong stride / pad / dilation, a wrong channel block or a wrong flow half is >= 0.1 x rms away."""
import pytest
import torch

from tests import mdcn_cases as M
from tests.util import assert_close, nchw, nhwc

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
# variant -> (PackedDcn mfma=, storage type of the sources (None: fp32), bound, tiles of the generic form)
VARIANTS = {
    "fp32": ("fp32", None, 5e-5, (0, 1, 2, 3, 4, 5, 6, 101, 103, 105, 106)),
    "x3": ("x3", None, 5e-5, (0, 1, 3, 5, 7, 106)),
    "bf16_fp32src": ("bf16", None, 1.5e-2, (0, 1, 5, 6, 7, 106)),
    "bf16": ("bf16", BF16, 1.5e-2, (0, 1, 5, 6, 7, 106)),
    "fp16": ("fp16", F16, 3e-3, (0, 1, 5, 6, 7, 106)),
}
# (variant, tile) pairs the library refuses with E2FGVI_EUNSUP (a tile whose LDS image does not fit): asserted to raise, never
# skipped.  By mdcn_fits_lds() every tile listed above fits in every variant, so the set is empty and each of them must run.
REFUSED = set()
EUNSUP = r"code -2\)"

_LAYERS = {}


def _layer(dev, name, mfma):
    """one PackedDcn (packed weights on the device) per case and arithmetic, shared by the tests"""
    from e2fgvi_amd import ops
    if (name, mfma) not in _LAYERS:
        c = M.case(name)
        geo = c["geo"]
        _LAYERS[name, mfma] = ops.PackedDcn(c["w"].to(dev), c["b"].to(dev), geo.dg, geo.stride, geo.pad, geo.dil, mfma=mfma)
    return _LAYERS[name, mfma]


def _sources(dev, c):
    """the case's NCHW features as the NHWC source list of its geometry (one or two sources), in their storage type"""
    parts = torch.split(c["x"], c["geo"].chans, 1)
    return [nhwc(p).to(dev) for p in parts]


def _run(layer, variant, tile, *args, **kw):
    """a launch at an explicit tile; a refused (variant, tile) pair must raise E2FGVI_EUNSUP and yields None"""
    from e2fgvi_amd.lib import HipError
    if (variant, tile) in REFUSED:
        with pytest.raises(HipError, match=EUNSUP):
            layer(*args, tile=tile, **kw)
        return None
    return layer(*args, tile=tile, **kw)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", M.NAMES)
def test_generic_form(dev, name, variant):
    """separate offset and mask tensors, every tile of the variant; two_sources also from planar 16-bit sources, bit-equal to
    the NHWC call at the same explicit tile"""
    from e2fgvi_amd import ops
    mfma, rounding, tol, tiles = VARIANTS[variant]
    c = M.case(name, rounding)
    layer, xs = _layer(dev, name, mfma), _sources(dev, c)
    off, msk = nhwc(c["off"]).to(dev), nhwc(c["msk"]).to(dev)
    planar = [ops.to_planar16(x) for x in xs] if rounding is not None and name == "two_sources" else None
    for tile in tiles:
        out = _run(layer, variant, tile, xs, off, mask=msk)
        if out is None:
            continue
        assert_close(nchw(out.cpu()), c["ref"], tol, "mdcn geometry %s %s tile %d" % (name, variant, tile))
        if planar is not None and tile:
            assert torch.equal(layer(planar, off, mask=msk, tile=tile, planar=True), out), (variant, tile)


@pytest.mark.parametrize("name", M.NAMES)
def test_one_tensor_form(dev, name):
    """mask=None: finished offsets and masks in ONE tensor, 6 columns wider than dg*3*K (the columns behind the masks hold NaN:
    nothing may read them), the mask words aliased behind the offsets.  Bit-equal to the generic form at the same tile.  Where
    dg*3*K + 6 is odd the library refuses the row stride (dy, dx are one 8-byte word) and the tensor gets a seventh column."""
    from e2fgvi_amd.lib import HipError
    c16 = {None: M.case(name), BF16: M.case(name, BF16)}
    geo = c16[None]["geo"]
    off, msk = nhwc(c16[None]["off"]), nhwc(c16[None]["msk"])
    cols = geo.dg * 3 * geo.K

    def one(extra):
        return torch.cat((off, msk, torch.full((geo.N, geo.Ho, geo.Wo, extra), float("nan"))), 3).to(dev)
    both = one(6)
    if (cols + 6) % 2:
        with pytest.raises(HipError, match=r"code -1\)"):
            _layer(dev, name, "fp32")(_sources(dev, c16[None]), both)
        both = one(7)
    off, msk = off.to(dev), msk.to(dev)
    for variant, tile in (("fp32", 1), ("fp32", 5), ("fp32", 103), ("x3", 7), ("bf16", 6), ("bf16", 106)):
        mfma, rounding, tol, _ = VARIANTS[variant]
        layer, xs = _layer(dev, name, mfma), _sources(dev, c16[rounding])
        want = layer(xs, off, mask=msk, tile=tile)
        got = layer(xs, both, tile=tile)
        assert torch.isfinite(got).all() and torch.equal(got, want), (name, variant, tile)
    assert_close(nchw(got.cpu()), c16[BF16]["ref"], 1.5e-2, "mdcn geometry %s one tensor bf16 tile 106" % name)


FUSED = [(n, v) for n in M.EVEN_DG for v in ("fp32", "x3")] + [("two_sources", "bf16")]
FUSED_TILES = {"fp32": (0, 2, 4, 5, 6, 101), "x3": (0, 1, 5, 7, 106), "bf16": (0, 5, 6, 7, 106)}


@pytest.mark.parametrize("name,variant", FUSED)
def test_fused_form(dev, name, variant):
    """the raw conv_offset output plus flows, max_residue = 1.5 (the residual no larger than the border bands the flows aim at);
    the reference applies max_residue * tanh, the flip and the sigmoid in float64"""
    mfma, rounding, tol, _ = VARIANTS[variant]
    c = M.fused_case(name, rounding)
    layer, xs = _layer(dev, name, mfma), _sources(dev, c)
    raw, flows = nhwc(c["raw"]).to(dev), nhwc(c["flows"]).to(dev)
    for tile in FUSED_TILES[variant]:
        out = _run(layer, variant, tile, xs, raw, flows=flows, max_residue=M.MAX_RESIDUE)
        if out is not None:
            assert_close(nchw(out.cpu()), c["ref"], tol, "mdcn geometry fused %s %s tile %d" % (name, variant, tile))


@pytest.mark.parametrize("variant,tile", [("fp32", 3), ("bf16", 6), ("fp16", 7)])
@pytest.mark.parametrize("name", ["row_kernel", "five_by_five"])
def test_wide_out(dev, name, variant, tile):
    """out= with Cout + 24 channels, prefilled: the first Cout channels are the result (for a 16-bit out: the fp32 result
    rounded once, bit for bit), the other 24 keep their bits.  row_kernel: four column tiles at BN = 64, two at 128, the last
    partial; five_by_five: an odd Cout and an odd row stride under a 16-bit store."""
    mfma, rounding, tol, _ = VARIANTS[variant]
    c = M.case(name, rounding)
    geo = c["geo"]
    layer, xs = _layer(dev, name, mfma), _sources(dev, c)
    off, msk = nhwc(c["off"]).to(dev), nhwc(c["msk"]).to(dev)
    out32 = layer(xs, off, mask=msk, tile=tile)
    assert_close(nchw(out32.cpu()), c["ref"], tol, "mdcn geometry %s %s tile %d (wide out)" % (name, variant, tile))
    for dt in (torch.float32, rounding or BF16):               # (fp32 products store bf16 as well)
        wide = torch.full((geo.N, geo.Ho, geo.Wo, geo.Cout + 24), -12345.0, dtype=dt, device=dev)
        assert layer(xs, off, mask=msk, tile=tile, out=wide) is wide
        assert torch.equal(wide[..., :geo.Cout], out32.to(dt)), (name, variant, dt)
        assert torch.equal(wide[..., geo.Cout:], torch.full_like(wide[..., geo.Cout:], -12345.0)), (name, variant, dt)


@pytest.mark.parametrize("name", ["stride2_two_ntiles", "dilated"])
def test_mmcv_module(dev, name):
    """mmcv_ops.ModulatedDeformConv2d, NCHW in and out, with a stride and with a dilation"""
    from e2fgvi_amd import mmcv_ops
    c = M.case(name)
    geo = c["geo"]
    mod = mmcv_ops.ModulatedDeformConv2d(geo.C, geo.Cout, (geo.KH, geo.KW), geo.stride, geo.pad, geo.dil, 1, geo.dg, bias=True)
    with torch.no_grad():
        mod.weight.copy_(c["w"])
        mod.bias.copy_(c["b"])
    mod = mod.to(dev)
    out = mod(c["x"].to(dev), c["off"].to(dev), c["msk"].to(dev))
    assert tuple(out.shape) == (geo.N, geo.Cout, geo.Ho, geo.Wo)
    assert_close(out.cpu(), c["ref"], 5e-5, "mdcn geometry %s mmcv module" % name)


@pytest.mark.parametrize("variant,tile", [("fp32", 2), ("x3", 7), ("bf16_fp32src", 6)])
def test_nonfinite_and_huge_offsets(dev, variant, tile):
    """offsets of +-inf, nan, +-3e9 (beyond int32) and 1e30 fail the guard: the sample is dropped (every corner address is the
    out-of-range sentinel before any load, every weight 0 by select) and the output is what it is with those offsets at +-1e6,
    bit for bit.  The library before this test formed the weights as NaN * (mask = 0) for an inf / nan offset: all three
    variants failed the assertion below with "non-finite output" (no fault)."""
    mfma, rounding, tol, _ = VARIANTS[variant]
    c = M.case("wide_group", rounding)
    off, far, ref = M.nonfinite_case("wide_group")
    layer, xs = _layer(dev, "wide_group", mfma), _sources(dev, c)
    msk = nhwc(c["msk"]).to(dev)
    out = layer(xs, nhwc(off).to(dev), mask=msk, tile=tile)
    assert_close(nchw(out.cpu()), ref, tol, "mdcn geometry non-finite offsets %s tile %d" % (variant, tile))
    assert torch.equal(out, layer(xs, nhwc(far).to(dev), mask=msk, tile=tile))
