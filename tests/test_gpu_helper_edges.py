"""The helper kernels of csrc/misc.hip against the float64 restatements of tests/helper_cases.py, at their edges.

Exact cases (every intermediate fits 24 bits, checked without a device in tests/test_helper_cases.py) must equal the float64
result bit for bit: rounded once to the output type, no tolerance.  General cases are held to K.allowed(case), which is derived
from the case's own tensors and the kernel's operation count (tests/helper_cases.py says how), plus half a unit in the last place
of a 16-bit output.  The 16-bit variants get 16-bit-representable inputs and the same float64 reference, not the fp32 kernel.

Kernel instantiations of misc.hip and the test that launches each (test_every_helper_entry_point_is_launched holds the symbols
against a launch trace):
  e2fgvi_nchw_to_nhwc        nchw_to_nhwc_kernel<float | bf16 | f16>, nchw_small_to_nhwc8_kernel<...>, nchw_small_to_nhwc4_kernel<...>
                             -- test_layout_edges
  e2fgvi_nhwc_to_nchw        nhwc_to_nchw_kernel -- test_layout_edges
  e2fgvi_nhwc_to_planar16    nhwc_to_planar16_kernel -- test_layout_edges
  e2fgvi_resize_bilinear     resize_bilinear_kernel (NCHW source; NHWC with C % 4 != 0), resize_bilinear_vec4_kernel<float | bf16 | f16>
                             -- test_resize_edges
  e2fgvi_avgpool2_nhwc       avgpool2_kernel -- test_avgpool_edges
  e2fgvi_spynet_level_input  spynet_level_input_kernel<bf16 | f16> (no copy: the bf16 one) -- test_spynet_edges
  e2fgvi_prop_cond           prop_cond_kernel<float, float, bf16>, <bf16, float>, <f16, float>, <bf16, bf16>, <f16, f16> -- test_prop_cond_edges
  e2fgvi_layernorm           layernorm_kernel<1 | 2 | 3 | 4, float | bf16 | f16> -- test_layernorm_edges
  e2fgvi_window_pool         window_pool_kernel<float | bf16 | f16> -- test_window_pool_edges
  e2fgvi_ffn_fold            fold_kernel<true, T, T, T, false | true>, T = float | bf16 | f16 -- test_fold_edges
  e2fgvi_ffn_unfold          unfold_gelu_kernel<T, true | false> -- test_fold_edges
  e2fgvi_softcomp_fold       fold_kernel<false, T, T, T> -- test_fold_edges
  e2fgvi_cast                cast_kernel<float, bf16 | f16>, cast_kernel<bf16 | f16, float> -- test_cast_edges
Not reached: the 64-bit branch of FlatIdx (more than 2^32 threads: tens of GB), NaN / infinite coordinates (undefined by the header)."""
import os
import re

import pytest
import torch

from tests import helper_cases as K
from tests.util import assert_close, launch_trace

pytestmark = pytest.mark.gpu
F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "e2fgvi_hip.h")
GUARD = 64


def _guarded(shape, dtype, dev):
    """a destination of `shape` inside a larger buffer filled with a sentinel -> (tensor, check): check() fails if a byte outside
    the destination changed"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), -77.0, dtype=dtype, device=dev)
    def check(what):
        g = torch.cat([flat[:GUARD], flat[GUARD + n:]]).float().cpu()
        assert bool((g == -77.0).all()), what + ": wrote outside its destination"
    return flat[GUARD:GUARD + n].view(shape), check


def _expect(got, ref, bound, exact, what):
    if exact:
        K.check_exact(got, ref, what)
    else:
        K.check(got, ref, bound, what, got.dtype)


def _rounded(c, dtype, keys):
    """the case with its feature tensors rounded to dtype: 16-bit-representable inputs for the 16-bit kernels"""
    c2 = dict(c)
    for k in keys:
        c2[k] = c[k].to(dtype).float()
    return c2


# ------------------------------------------------------------------------------------------------------------------ propagation
def _run_prop(c, src, cond_dt, dev):
    from e2fgvi_amd import ops
    fl = c["flows"].to(dev)
    N, T, H, W, _ = fl.shape
    C = c["fp"].shape[3]
    cond, chk_c = _guarded((N, H, W, 2 * C), cond_dt, dev)
    flows, chk_f = _guarded((N, H, W, 4), F32, dev)
    fb = None if c["ib"] is None else fl[0, c["ib"]]
    f2 = None if fb is None else c["f2"].to(src).to(dev)
    out = ops.prop_cond(c["fp"].to(src).to(dev), f2, fl[0, c["ia"]], fb, T * H * W * 2, cond=cond, flows=flows, flows8=True)
    chk_c(c["name"] + " cond"); chk_f(c["name"] + " flows")
    return out


@pytest.mark.parametrize("name", K.names("prop_cond"))
def test_prop_cond_edges(dev, name):
    """zeros-padded warps of the propagation: every border class, flows of 0, +-3e9 and +-1e30 (exact cases), two images with
    their own flow base at a stride > H W 2, feat_n2 wider than C, flow_b present and absent, the flows again as a 16-bit conv
    source beside every cond type.  Bound: K.warp_bound -- cond 1: one rounding of q = p + f (2^-24 |q|) x the neighbour
    differences around q, + 8 roundings x max|v|; flow_n2: the same for the warped flow_b, + one addition; cond 2: flow_n2's error
    on top of q's rounding.  flow_n1 is a copy: exact in every case."""
    c0 = K.case(name)
    C = c0["fp"].shape[3]
    modes = [(F32, F32)] + ([(F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)] if C % 16 == 0 else [])
    for src, cond_dt in modes:
        c = _rounded(c0, src, ("fp", "f2")) if src != F32 else c0
        ref, allowed, what = K.reference(c), K.allowed(c), "%s [%s -> %s]" % (name, src, cond_dt)
        cond, flows, fl8 = _run_prop(c, src, cond_dt, dev)
        assert cond.dtype == cond_dt and fl8.dtype == (F16 if cond_dt == F16 else BF16)
        _expect(cond, ref[0], allowed[0], c["exact"], what + " cond")
        _expect(flows, ref[1], allowed[1], c["exact"], what + " flows")
        if c["exact"]:                                       # (far flows overflow fp16: the copy holds the infinity .half() gives)
            K.check_exact(fl8[..., :4], ref[1], what + " flows8")
        else:
            K.check(fl8[..., :4], ref[1], allowed[1], what + " flows8", fl8.dtype)
        assert float(fl8[..., 4:].abs().max()) == 0, what + ": flows8 channels 4..7"


# ------------------------------------------------------------------------------------------------------------------ SPyNet
@pytest.mark.parametrize("name", K.names("spynet"))
def test_spynet_edges(dev, name):
    """border-padded warp by the doubled, x2-upsampled previous flow.  2 x 2 level: the previous level is 1 x 1, both scales 0,
    flow_up = 2 flow_prev exactly -- one pair per border class and per far flow, the result is the clamped pixel bit for bit.
    Bound of the general cases: flow_up is a resize (K.resize_bound: s = scale32 d is one rounding, <= 2^-24 s) doubled; the
    warp's q carries that error plus its own rounding (K.warp_bound, border continuation).  The three reference channels are
    copies: exact."""
    from e2fgvi_amd import ops
    c = K.case(name)
    ref, allowed = K.reference(c)[0], K.allowed(c)[0]
    ids = [torch.tensor(c[k], dtype=torch.int32, device=dev) for k in ("ref_idx", "supp_idx")]
    fprev = None if c["flow_prev"] is None else c["flow_prev"].to(dev)
    out = ops.spynet_level_input(c["pyr"].to(dev), ids[0], ids[1], fprev)
    _expect(out, ref, allowed, c["exact"], name)
    for dt in (BF16, F16):
        o32, o16 = ops.spynet_level_input(c["pyr"].to(dev), ids[0], ids[1], fprev, copy_dtype=dt)
        assert o16.dtype == dt and torch.equal(o32, out)
        if c["exact"]:
            K.check_exact(o16, ref, "%s copy %s" % (name, dt))
        else:
            K.check(o16, ref, allowed, "%s copy %s" % (name, dt), dt)


# ------------------------------------------------------------------------------------------------------------------ resize
def _resize_runs(c):
    """(label, input tensor, channels-last?, kwargs of ops.resize_bilinear, scale, shift, dtype) of every path a case's C reaches"""
    x, C, sc, sh = c["x"], c["x"].shape[3], c["scale"], c["shift"]
    runs = []
    if C == 3:
        runs.append(("nchw scalar out_ld 4", x, True, dict(out_ld=4), sc, sh, F32))
    if C % 4:
        runs.append(("nhwc scalar", x, False, {}, sc, sh, F32))
        runs.append(("nhwc scalar, no affine", x, False, {}, None, None, F32))
    else:
        runs.append(("vec4", x, False, {}, sc, sh, F32))
        runs.append(("vec4, no affine", x, False, {}, None, None, F32))
        runs.extend(("16-bit", x, False, {}, None, None, dt) for dt in (BF16, F16))
    return runs


@pytest.mark.parametrize("exact", [True, False])
def test_resize_edges(dev, exact):
    """every path (NCHW scalar with a zero pad channel, NHWC scalar at C = 3 and 6, vec4 with and without the affine, 16-bit at
    C = 8 and 16 in both types), N = 2, at: outputs and inputs of one row / column, identity, the half-pixel rows that clamp to
    0, up- and downscales.  Bound (general): K.resize_bound -- the source position is one (align_corners) or two (half-pixel)
    fp32 roundings of an expression in the launcher's own fp32 scale, times the neighbour differences around it, + 8 roundings x
    max|v|, + two for the affine."""
    from e2fgvi_amd import ops
    for name in K.names("resize", exact):
        c = K.case(name)
        Ho, Wo = c["out_hw"]
        for label, x, as_nchw, kw, sc, sh, dt in _resize_runs(c):
            xin = x.to(dt).float() if dt != F32 else x
            ref = K.resize_ref(xin, Ho, Wo, c["align"], sc, sh)
            bound = 0.0 if exact else K.resize_bound(xin, Ho, Wo, c["align"], sc, sh)
            src = xin.permute(0, 3, 1, 2).contiguous() if as_nchw else xin.to(dt)
            out = ops.resize_bilinear(src.to(dev), (Ho, Wo), c["align"], src_nchw=as_nchw, **(kw if dt == F32 else {}),
                                      **({} if dt != F32 else dict(scale=None if sc is None else sc.to(dev), shift=None if sh is None else sh.to(dev))))
            what = "%s [%s %s]" % (name, label, dt)
            assert out.dtype == dt
            if "out_ld" in kw:
                assert float(out[..., 3].abs().max()) == 0, what + ": pad channel"
                out = out[..., :3]
            _expect(out, ref, bound, exact, what)


# ------------------------------------------------------------------------------------------------------------------ fold / unfold
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("H,W", K.FOLD_SIZES)
def test_fold_edges(dev, H, W, exact):
    """FFN fold / unfold and SoftComp fold at H % 3 = 0, 1, 2 (other overlap counts, another upper token clamp) and at a single
    pixel; C = 4, 12 (fp32), 8 (fp32, bf16, fp16); two frames; both GELU placements; bias and residual present and absent.
    Exact: integer operands, the sums are exact and the fp32 division by the count is correctly rounded, so the normalised fold
    is the float64 quotient rounded once.  General, a pixel under n tokens: n - 1 additions and (n > 1) the division, so
    gamma(n - 1 + [n > 1]) x fold(|hid|) / n, gamma(k) = k 2^-24 / (1 - k 2^-24); SoftComp n + 1 roundings with bias and
    residual, n - 1 without; a pixel under one token (the whole 1 x 1 image) is a copy: exact.  The unfold is a gather: equal to
    the gather of its own input, padding taps exactly 0.  GELU paths: 1e-5 x rms, test_fold_unfold's figure for erff; 16-bit: + half a unit of the result, and where the GELU reads the
    rounded fold + max|GELU'| = 1.13 x half a unit of the fold."""
    from e2fgvi_amd import ops
    fh, fw = K.token_grid(H, W)
    single = (H, W) == (1, 1)                                # one token, count 1: the fold copies, whatever the data
    for C, dts in ((4, (F32,)), (12, (F32,)), (8, (F32, BF16, F16))):
        c0 = K.case("fold %s %dx%d C%d" % ("exact" if exact else "general", H, W, C))
        pad = K.unfold_padding(2, fh, fw, H, W, C)
        for dt in dts:
            c = _rounded(c0, dt, ("hid", "res")) if dt != F32 else c0
            what = "%s %s" % (c0["name"], dt)
            ref, allowed = K.reference(c), K.allowed(c)
            hid, res, bias = c["hid"].to(dt).to(dev), c["res"].to(dt).to(dev), c["bias"].to(dev)
            folded = ops.ffn_fold(hid, *c["dims"])
            _expect(folded, ref[0], allowed[0], exact or single, what + " ffn_fold")
            unf, chk = _guarded((2 * fh * fw, 49 * C), dt, dev)
            ops.ffn_unfold(folded, fh, fw, out=unf)
            chk(what + " ffn_unfold")
            assert torch.equal(unf.cpu(), K.ffn_unfold_ref(folded.cpu(), fh, fw, False).to(dt)), what + ": the unfold is not the gather of its input"
            if exact:
                K.check_exact(unf, ref[1], what + " ffn_unfold")
            # GELU behind the unfold (the reference's order) and in front of it (the engine's)
            g_ref = K.ffn_unfold_ref(ref[0], fh, fw, True)
            a, b = ops.ffn_unfold_gelu(folded, fh, fw), ops.ffn_unfold(ops.ffn_fold_gelu(hid, *c["dims"]), fh, fw)
            assert float(a.cpu()[pad].abs().max() if pad.any() else 0) == 0 and float(b.cpu()[pad].abs().max() if pad.any() else 0) == 0, what
            if dt == F32:
                assert torch.equal(a, b), what + ": GELU(fold) + unfold != fold + GELU(unfold)"
                assert_close(a.cpu(), g_ref, 1e-5, what + " ffn_unfold_gelu")
            else:
                tol = 1e-5 * g_ref.pow(2).mean().sqrt().item() + (0 if exact else 1.13 * K.ffn_unfold_ref(allowed[0], fh, fw, False))
                K.check(b, g_ref, tol, what + " fold_gelu + unfold", dt)
                K.check(a, g_ref, tol + 1.13 * K.half_ulp(K.ffn_unfold_ref(ref[0], fh, fw, False), dt), what + " fold + unfold_gelu", dt)
            sc = ops.softcomp_fold(hid, *c["dims"], bias_hwc=bias, residual=res)
            _expect(sc, ref[2], allowed[2], exact, what + " softcomp_fold")
            sc0 = ops.softcomp_fold(hid, *c["dims"])
            s_abs, n_tok = K.fold_sum(c["hid"].abs(), *c["dims"])
            _expect(sc0, K.softcomp_fold_ref(c["hid"], *c["dims"]), K.gamma(n_tok - 1) * s_abs, exact or single, what + " softcomp_fold, no bias, no residual")


# ------------------------------------------------------------------------------------------------------------------ LayerNorm, pools
@pytest.mark.parametrize("C", [256, 512, 768, 1024])
def test_layernorm_edges(dev, C):
    """the four widths (VPL = C / 256 = 1..4), one row and five (a block holds four), the three output types, unit-scale data,
    against F.layer_norm in float64.  Bound: K.ln_bound -- test_layernorm_off_unit_scale's, with 4 VPL + 8 roundings on the way
    to the mean; 16-bit outputs: + half a unit of the result (the fp16 store fuses the last multiply-add into one rounding, which
    this covers: nothing here is an exact case, the reciprocal square root rounds)."""
    from e2fgvi_amd import ops
    for rows in (1, 5):
        c = K.case("layernorm %d rows C%d" % (rows, C))
        ref = K.reference(c)[0]
        args = [c[k].to(dev) for k in ("x", "gamma", "beta")]
        for dt in (F32, BF16, F16):
            out, chk = _guarded((rows, C), dt, dev)
            ops.layernorm(*args, out=out)
            chk(c["name"])
            if dt == F32:
                assert_close(out.cpu(), ref, K.ln_bound(c["x"]), c["name"])
            else:
                K.check(out, ref, K.allowed(c)[0], "%s %s" % (c["name"], dt), dt)


def test_avgpool_edges(dev):
    """C = 1, 3, 4, 6 on 2 x 2 and 6 x 10 inputs, integer data: four integers and a quarter, exact"""
    from e2fgvi_amd import ops
    for name in K.names("avgpool"):
        c = K.case(name)
        K.check_exact(ops.avgpool2(c["x"].to(dev)), K.reference(c)[0], name)


@pytest.mark.parametrize("exact", [True, False])
def test_window_pool_edges(dev, exact):
    """Linear(45 -> 1) over 5 x 9 windows: one window and 2 x 3 of them per image, three images, C = 4, 12 (fp32), 8 (all types).
    Exact: integer tokens, weights in 64ths.  General: 45 multiply-adds behind the bias, <= gamma(46) x (|b| + sum |w| |x|)."""
    from e2fgvi_amd import ops
    for name in K.names("window_pool", exact):
        c0 = K.case(name)
        BT, fh, fw, C = c0["x"].shape
        for dt in (F32, BF16, F16) if C == 8 else (F32,):
            c = _rounded(c0, dt, ("x",)) if dt != F32 else c0
            out, chk = _guarded((BT * (fh // 5) * (fw // 9), C), dt, dev)
            ops.window_pool(c["x"].to(dt).to(dev), c["w45"].to(dev), c["b1"].to(dev), BT, fh, fw, out=out)
            chk(name)
            _expect(out, K.reference(c)[0], K.allowed(c)[0], exact, "%s %s" % (name, dt))


# ------------------------------------------------------------------------------------------------------------------ casts, layouts
@pytest.mark.parametrize("n", K.CAST_N)
@pytest.mark.parametrize("dt", [BF16, F16])
def test_cast_edges(dev, dt, n):
    """fp32 -> 16 bit == torch's conversion on the host (round to nearest even, overflow to infinity, subnormals kept, signed
    zeros), bit for bit; 16 bit -> fp32 is exact; n = 4 (one thread) and 260 (a second block)"""
    from e2fgvi_amd import ops
    x = K.cast_inputs(dt, n)
    y = ops.cast(x.to(dev), dt)
    assert y.dtype == dt and torch.equal(y.cpu().view(torch.int16), x.to(dt).view(torch.int16))
    back = ops.cast(y, F32)
    assert torch.equal(back.cpu().view(torch.int32), x.to(dt).float().view(torch.int32))


def test_layout_edges(dev):
    """the three NCHW -> NHWC kernels in the three output types and the way back: integer data, y = x * 0.5 + 0.25 exact, 5 x 7
    pixels (no multiple of the 32-pixel tile), two images, pad channels zero; NHWC -> planar-16 is a permutation"""
    from e2fgvi_amd import ops
    g = K.gen(4201)
    for C, ld in ((3, 4), (1, 4), (3, 8), (5, 8), (37, 40), (3, 5)):      # small4, small4, small8, small8, tiled, tiled
        x = K._ints(g, (2, C, 5, 7))
        ref = torch.nn.functional.pad(x.double().permute(0, 2, 3, 1) * 0.5 + 0.25, (0, ld - C))
        ref[..., C:] = 0
        for dt in (F32, BF16, F16):
            K.check_exact(ops.nchw_to_nhwc(x.to(dev), ld=ld, scale=0.5, shift=0.25, out_dtype=dt), ref, "nchw_to_nhwc C%d ld%d %s" % (C, ld, dt))
        y = ops.nchw_to_nhwc(x.to(dev), ld=ld)
        assert torch.equal(ops.nhwc_to_nchw(y, channels=C).cpu(), x)
    for dt in (BF16, F16):
        t = K._ints(g, (2, 5, 7, 32)).to(dt)
        assert torch.equal(ops.to_planar16(t.to(dev)).cpu(), t.view(2, 5, 7, 2, 16).permute(3, 0, 1, 2, 4).contiguous())


def test_every_helper_entry_point_is_launched(dev):
    """the helper entry points the header declares == the ones this module's docstring lists; a trace of one small call of each
    records them all"""
    from e2fgvi_amd import ops
    text = open(HEADER).read()
    section = text[text.index("Small HBM-bound kernels"):]
    section = section[:section.index("LDS-DMA implicit-GEMM")]
    declared = set(re.findall(r"^int (e2fgvi_\w+)\(", section, re.M))
    assert len(declared) == 12, sorted(declared)
    listed = set(re.findall(r"^  (e2fgvi_\w+) ", __doc__, re.M))
    assert declared <= listed and listed - declared == {"e2fgvi_nhwc_to_planar16"}, (sorted(declared - listed), sorted(listed - declared))
    with launch_trace() as trace:
        x = torch.ones(1, 4, 2, 2, device=dev)
        y = ops.nchw_to_nhwc(x)
        ops.nhwc_to_nchw(y)
        ops.resize_bilinear(y, (3, 3), True)
        ops.avgpool2(y)
        ids = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.spynet_level_input(y, ids, ids, None)
        ops.prop_cond(y, None, torch.zeros(1, 2, 2, 2, device=dev), None, 8)
        ops.layernorm(torch.ones(1, 256, device=dev), torch.ones(256, device=dev), torch.ones(256, device=dev))
        ops.window_pool(torch.ones(1, 5, 9, 4, device=dev), torch.ones(45, device=dev), torch.ones(1, device=dev), 1, 5, 9)
        f = ops.ffn_fold(torch.ones(1, 49 * 4, device=dev), 1, 1, 1, 1, 1, 4)
        ops.ffn_unfold(f, 1, 1)
        ops.softcomp_fold(torch.ones(1, 49 * 4, device=dev), 1, 1, 1, 1, 1, 4)
        ops.to_planar16(ops.cast(torch.ones(1, 1, 1, 16, device=dev), BF16))
    torch.cuda.synchronize()
    seen = {r["symbol"] for r in trace}
    assert listed <= seen, sorted(listed - seen)
