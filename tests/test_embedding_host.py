"""tests/embedding.py on the CPU: the embedding gives the tensor back bit for bit, and the check the GPU tests run
(embedding.check_slices) bites -- a 3x3 conv that reads a neighbour's channels against zero weights, and one that stores a channel or
a pixel past its slice, each fail it with a diagnosis that names the region; the correct conv passes."""
import pytest
import torch
import torch.nn.functional as F

from tests import embedding as E
from tests.util import gen

N, H, W, CIN, COUT = 2, 5, 7, 8, 4
LD, COFF = 20, 8                     # source pixels of 20 channels, the conv's 8 from channel 8 on
DLD, DCOFF = 12, 4                   # destination pixels of 12 channels, the result's 4 from channel 4 on


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("ld,coff", [(None, 0), (8, 0), (24, 0), (24, 8)])
def test_round_trip(dtype, ld, coff):
    t = torch.randn(N, H, W, 8, generator=gen(1)).to(dtype)
    t[0, 0, 0, 0], t[0, 0, 0, 1] = -0.0, 2.0 ** -20
    view, arena = E.embed(t, ld=ld, coff=coff)
    assert view.is_contiguous() and view.dtype == dtype and tuple(view.shape) == (N, H, W, ld or 8)
    assert torch.equal(E.bits(view[..., coff:coff + 8]), E.bits(t))
    g = (view.data_ptr() - arena.data_ptr()) // arena.element_size()
    assert g >= (W + 2) * (ld or 8) and (g * arena.element_size()) % 16 == 0 and arena.numel() == 2 * g + view.numel()
    rest = torch.ones(arena.numel(), dtype=torch.bool)
    rest[g:g + view.numel()].view(-1, ld or 8)[:, coff:coff + 8] = False
    assert torch.isnan(arena[rest].float()).all(), "everything around the slice is NaN"
    dview, darena = E.embed_like((N, H, W, 8), dtype, "cpu", ld=ld, coff=coff)
    assert (E.bits(darena) == E.SENTINEL_BITS[dtype]).all() and torch.isnan(darena.float()).all()
    E.assert_untouched(darena, dview, coff, 8)
    dview[..., coff:coff + 8] = t
    E.check_slices(dview, darena, coff, 8, tight=t.clone(), sources=[(arena, E.snapshot(arena))])


def test_two_dimensional_operands_get_a_gemm_tile_of_rows():
    t = torch.randn(77, 16, generator=gen(2))
    view, arena = E.embed(t)
    g = (view.data_ptr() - arena.data_ptr()) // 4
    assert g >= 256 * 16 and torch.equal(view, t) and torch.isnan(arena[:g]).all() and torch.isnan(arena[g + t.numel():]).all()
    tab, tarena = E.embed(torch.arange(12, dtype=torch.int32).view(3, 4), poison=0)
    assert torch.equal(tab, torch.arange(12, dtype=torch.int32).view(3, 4)) and int(tarena.sum()) == 66


# ------------------------------------------------------------------------------------------------ the checker bites
def _operands():
    g = gen(3)
    x = torch.randn(N, H, W, CIN, generator=g)
    w = torch.randn(COUT, CIN, 3, 3, generator=g) / 8
    return x, w, F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).contiguous()


def _run(standin):
    """the embedded call of a stand-in `standin(src_view, w, dst_arena, dst_view)` through the GPU tests' check"""
    x, w, tight = _operands()
    src, sarena = E.embed(x, ld=LD, coff=COFF)
    dst, darena = E.embed_like(tight.shape, torch.float32, "cpu", ld=DLD, coff=DCOFF)
    snap = E.snapshot(sarena)
    standin(src, w, darena, dst)
    return E.check_slices(dst, darena, DCOFF, COUT, tight=tight, sources=[(sarena, snap)], what="stand-in")


def _conv_slice(src, w):
    return F.conv2d(src[..., COFF:COFF + CIN].permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)


def test_correct_conv_passes():
    def conv(src, w, darena, dst):
        dst[..., DCOFF:DCOFF + COUT] = _conv_slice(src, w)
    assert torch.equal(_run(conv), _operands()[2])


def test_zero_weight_leak_is_caught():
    """F.conv2d over the whole wide buffer with the weights zero-padded to LD channels: right on finite neighbours, NaN on these"""
    def conv(src, w, darena, dst):
        wide = torch.zeros(COUT, LD, 3, 3)
        wide[:, COFF:COFF + CIN] = w
        dst[..., DCOFF:DCOFF + COUT] = F.conv2d(src.permute(0, 3, 1, 2), wide, padding=1).permute(0, 2, 3, 1)
    with pytest.raises(AssertionError, match=r"non-finite values inside the result slice .*outside a source's slice reached the result"):
        _run(conv)
    # ... and the same stand-in is right when the neighbours are finite: what the suite's older slice tests would have seen
    x, w, tight = _operands()
    src = torch.full((N, H, W, LD), 7.0)
    src[..., COFF:COFF + CIN] = x
    wide = torch.zeros(COUT, LD, 3, 3)
    wide[:, COFF:COFF + CIN] = w
    assert torch.allclose(F.conv2d(src.permute(0, 3, 1, 2), wide, padding=1).permute(0, 2, 3, 1), tight, atol=1e-5)


def test_store_one_channel_past_the_slice_is_caught():
    def conv(src, w, darena, dst):
        dst[..., DCOFF + 1:DCOFF + COUT + 1] = _conv_slice(src, w)
    with pytest.raises(AssertionError, match=r"first at flat index \d+ = pixel 0, channel %d \(the slice is channels \[%d, %d\) of %d\), "
                                             r"last at \d+ = pixel %d, channel %d" % (DCOFF + COUT, DCOFF, DCOFF + COUT, DLD,
                                                                                     N * H * W - 1, DCOFF + COUT)):
        _run(conv)


def test_store_one_pixel_past_the_last_row_is_caught():
    def conv(src, w, darena, dst):
        g = (dst.data_ptr() - darena.data_ptr()) // 4
        shifted = darena[g + DLD:g + DLD + dst.numel()].view(dst.shape)             # every pixel one further on
        shifted[..., DCOFF:DCOFF + COUT] = _conv_slice(src, w)
    with pytest.raises(AssertionError, match=r"%d elements outside .* = guard-after\[%d\] \(%d elements behind the view\)"
                                             % (COUT, DCOFF + COUT - 1, DCOFF + COUT)):
        _run(conv)


def test_a_store_of_zero_or_nan_outside_the_slice_is_caught_and_a_changed_source_too():
    x, w, tight = _operands()
    for value in (0.0, float("nan")):
        dst, darena = E.embed_like(tight.shape, torch.float32, "cpu", ld=DLD, coff=DCOFF)
        dst[..., DCOFF:DCOFF + COUT] = tight
        darena[3] = value
        with pytest.raises(AssertionError, match=r"guard-before\[3\]"):
            E.check_slices(dst, darena, DCOFF, COUT, tight=tight)
    src, sarena = E.embed(x, ld=LD, coff=COFF)
    snap = E.snapshot(sarena)
    src[0, 0, 0, 0] = 1.0
    with pytest.raises(AssertionError, match="source arena changed"):
        E.assert_sources_intact(sarena, snap, "src")
    dst, darena = E.embed_like(tight.shape, torch.float32, "cpu", ld=DLD, coff=DCOFF)
    dst[..., DCOFF:DCOFF + COUT] = tight
    off = tight.clone()
    off[1, 2, 3, 1] = -off[1, 2, 3, 1]
    with pytest.raises(AssertionError, match="differ in their bits"):
        E.check_slices(dst, darena, DCOFF, COUT, tight=off)
