"""tests/helper_cases.py without a device: the restatements against torch's own operators in float64, the condition that makes the
exact cases exact, and every wrong reading caught by some case."""
import pytest
import torch
import torch.nn.functional as F

from tests import helper_cases as K
from tests.util import gen

F64 = torch.float64
_REF, _ALLOWED = {}, {}


def _ref(name):
    if name not in _REF:
        _REF[name] = K.reference(K.case(name))
    return _REF[name]


def _allowed(name):
    if name not in _ALLOWED:
        _ALLOWED[name] = K.allowed(K.case(name))
    return _ALLOWED[name]


# ------------------------------------------------------------------------------------------------ restatement == torch in float64
@pytest.mark.parametrize("pad", ["zeros", "border"])
def test_warp_is_grid_sample(pad):
    g = gen(4101)
    N, H, W, C = 2, 6, 10, 5
    src = torch.randn(N, H, W, C, generator=g, dtype=F64)
    flow = torch.randn(N, H, W, 2, generator=g, dtype=F64) * 3
    K._plant(flow[0], K.edge_targets(H, W, 0.3))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    grid = torch.stack([2 * (xs + flow[..., 0]) / (W - 1) - 1, 2 * (ys + flow[..., 1]) / (H - 1) - 1], -1)
    ref = F.grid_sample(src.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode=pad, align_corners=True).permute(0, 2, 3, 1)
    assert (K.warp(src, flow, pad) - ref).abs().max().item() <= 1e-9


# sizes whose fp32 ratio is the exact ratio: F.interpolate in float64 then computes with the same scale as the restatement
@pytest.mark.parametrize("align,size_in,size_out", [(True, (13, 7), (7, 13)), (True, (12, 6), (5, 17)), (True, (5, 9), (1, 1)),
                                                    (True, (1, 3), (4, 9)), (False, (12, 5), (16, 8)), (False, (24, 7), (64, 4)),
                                                    (False, (1, 8), (4, 16)), (False, (6, 6), (6, 6))])
def test_resize_is_interpolate(align, size_in, size_out):
    x = torch.randn(2, *size_in, 3, generator=gen(4102), dtype=F64)
    ref = F.interpolate(x.permute(0, 3, 1, 2), size=size_out, mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
    assert (K.resize_ref(x, *size_out, align) - ref).abs().max().item() <= 1e-9
    sc, sh = torch.tensor([2.0, -0.3, 1.7], dtype=F64), torch.tensor([0.1, 5.0, -1.0], dtype=F64)
    assert (K.resize_ref(x, *size_out, align, sc, sh) - (ref * sc + sh)).abs().max().item() <= 1e-9


def test_up2x_is_interpolate_x2():
    x = torch.randn(3, 1, 1, 2, generator=gen(4103), dtype=F64)                 # the 1 x 1 level: both scales 0
    assert torch.equal(K.up2x_align(x), x.expand(3, 2, 2, 2))
    x = torch.randn(2, 3, 5, 2, generator=gen(4104), dtype=F64)
    ref = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert (K.up2x_align(x) - ref).abs().max().item() <= 1e-6                   # (2/5 and 4/9 as fp32: 3e-8 relative)


@pytest.mark.parametrize("H,W", K.FOLD_SIZES)
def test_fold_wrapper_is_the_gather_of_the_header(H, W):
    """F.fold / F.unfold behind the [tap][c] wrappers == the fold written out pixel by pixel, the unfold of a fold of ones counts"""
    fh, fw = K.token_grid(H, W)
    C = 4
    p = K._ints(gen(4105), (2 * fh * fw, 49 * C)).double()
    s, cnt = K.fold_sum(p, 2, fh, fw, H, W, C)
    s2, cnt2 = K.fold_gather(p, 2, fh, fw, H, W, C)
    assert torch.equal(s, s2) and torch.equal(cnt[..., 0], cnt2)
    rows = K.ffn_unfold_ref(s, fh, fw, False)
    pad = K.unfold_padding(2, fh, fw, H, W, C)
    assert rows.shape == p.shape and float(rows[pad].abs().max() if pad.any() else 0) == 0
    t = rows.view(2, fh, fw, 7, 7, C)                        # token (ly, lx), tap (ki, kj) is pixel (3ly-3+ki, 3lx-3+kj)
    for ly, lx, ki, kj in ((0, 0, 3, 3), (fh - 1, fw - 1, 3, 3), (fh - 1, 0, 3 + (H - 1) % 3, 4 if W > 1 else 3)):
        assert torch.equal(t[:, ly, lx, ki, kj], s[:, 3 * ly - 3 + ki, 3 * lx - 3 + kj])


def test_window_pool_is_a_strided_conv():
    c = K.case("window_pool general 10x27 C4")
    x = c["x"].double().permute(0, 3, 1, 2).reshape(-1, 1, 10, 27)
    ref = F.conv2d(x, c["w45"].double().view(1, 1, 5, 9), c["b1"].double(), stride=(5, 9)).view(3, 4, 2, 3).permute(0, 2, 3, 1).reshape(-1, 4)
    assert (K.window_pool_ref(c["x"], c["w45"], c["b1"]) - ref).abs().max().item() <= 1e-12


def test_half_ulp():
    v = torch.tensor([1.0, 1.5, 1.999, 2.0, 3e-6, 65504.0, 1e-30], dtype=F64)
    for dt, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
        hu = K.half_ulp(v, dt)
        assert torch.equal(hu[:4], torch.tensor([2.0 ** -bits] * 3 + [2.0 ** (1 - bits)], dtype=F64))
        ok = v[:6] if dt == torch.float16 else v
        assert ((ok.to(dt).double() - ok).abs() <= K.half_ulp(ok, dt)).all()


# ------------------------------------------------------------------------------------------------ what makes an exact case exact
@pytest.mark.parametrize("name", K.names(exact=True))
def test_exact_cases_need_no_rounding(name):
    """the restatement evaluated with one fp32 rounding per operation gives the float64 values: no operation of the case rounds, so
    no evaluation order and no fused multiply-add can change a bit.  (The normalised fold ends in a division by the overlap count:
    there the fp32 quotient must be the float64 quotient rounded once, and the sum in front of it exact.)"""
    c = K.case(name)
    r32, r64 = K.reference(c, torch.float32), _ref(name)
    for i, (a, b) in enumerate(zip(r32, r64)):
        assert a.dtype == torch.float32 and b.dtype == F64 and torch.isfinite(b).all()
        if i in K.quotients(c):
            assert torch.equal(a, b.float()), (name, i)
        else:
            assert torch.equal(a.double(), b), (name, i, (a.double() - b).abs().max().item())
    if c["kind"] == "fold":
        s32, s64 = K.fold_sum(c["hid"], *c["dims"], torch.float32)[0], K.fold_sum(c["hid"], *c["dims"])[0]
        assert torch.equal(s32.double(), s64)


def test_far_flows_give_zero_or_the_clamped_pixel():
    c = K.case("prop exact 6x10")
    cond, flows = _ref(c["name"])
    far = (c["flows"][:, 1].abs() > 1e9).any(-1)
    assert int(far.sum()) == 10 and float(cond[far].abs().max()) == 0 and torch.equal(flows[far][:, 2:], flows[far][:, :2])
    s = K.case("spynet exact 2x2")
    out = _ref(s["name"])[0]
    fp = s["flow_prev"][:, 0, 0]
    for n in [i for i in range(fp.shape[0]) if float(fp[i].abs().max()) > 1e9]:
        img = s["pyr"][s["supp_idx"][n]][..., :3].double()
        cx = 1 if fp[n, 0] > 1 else 0 if fp[n, 0] < -1 else None
        cy = 1 if fp[n, 1] > 1 else 0 if fp[n, 1] < -1 else None
        if cx is not None and cy is not None:
            assert torch.equal(out[n, :, :, 3:6], img[cy, cx].expand(2, 2, 3)), n


def test_cases_cover_the_border_classes():
    """the sample positions of the propagation cases hit every border class on both axes: q at 0, n - 1, -1 and n, inside (-1, 0) and (n - 1, n),
    and a flow of 0"""
    for name in ("prop exact 6x10", "prop exact 5x7 no flow_b", "prop general 6x10"):
        c = K.case(name)
        H, W = c["fp"].shape[1:3]
        ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
        fa = c["flows"][0, 1].double()
        for q, n in ((xs + fa[..., 0], W), (ys + fa[..., 1], H)):
            for what, hit in (("0", q == 0), ("n-1", q == n - 1), ("(-1,0)", (q > -1) & (q < 0)), ("-1", q == -1),
                              ("(n-1,n)", (q > n - 1) & (q < n)), ("n", q == n)):
                assert hit.any(), (name, what)
        assert (fa == 0).all(-1).any()


# ------------------------------------------------------------------------------------------------ the wrong readings
@pytest.mark.parametrize("variant", K.VARIANTS)
def test_every_wrong_reading_moves_some_case(variant):
    """by more than the case's allowed error; on an exact case any difference counts"""
    kinds = {"zeros_as_border": ("prop_cond",), "border_as_zeros": ("spynet",), "corner_at_W": ("prop_cond",), "swap_xy": ("prop_cond", "spynet"),
             "flow_b_at_p": ("prop_cond",), "flow_up_not_doubled": ("spynet",), "align_flipped": ("resize",), "no_clamp0": ("resize",),
             "i1_unclamped": ("resize",), "tap_kj_ki": ("fold",), "count9": ("fold",), "no_l_hi_clamp": ("fold",),
             "unbiased_var": ("layernorm",), "eps_outside": ("layernorm",), "stride1": ("avgpool",)}[variant]
    caught = []
    for kind in kinds:
        for name in K.names(kind):
            got = K.reference(K.case(name), variant=variant)
            if any(bool(((g - r).abs() > a).any()) for g, r, a in zip(got, _ref(name), _allowed(name))):
                caught.append(name)
        assert caught, (variant, kind)
    assert any(not K.case(n)["exact"] for n in caught) or kinds == ("avgpool",), "%s: caught by no general case" % variant
    assert any(K.case(n)["exact"] for n in caught) or kinds == ("layernorm",), "%s: caught by no exact case" % variant


def test_cast_inputs_hold_the_edges():
    for dt in (torch.float16, torch.bfloat16):
        x = K.cast_inputs(dt, 260)
        y = x.to(dt)
        assert x.numel() == 260 and K.cast_inputs(dt, 4).numel() == 4
        assert torch.isinf(y[torch.isfinite(x)]).any() and (y[x != 0] == 0).any() and torch.isinf(x).sum() == 2
        sub = (y != 0) & (y.float().abs() < (2.0 ** -14 if dt == torch.float16 else 2.0 ** -126))
        assert sub.any() and (torch.signbit(x) & (x == 0)).any()
        assert (y.float() != x).any()
