"""The helper kernels of csrc/misc.hip (flow warps, bilinear resizes, fold / unfold, window pooling, LayerNorm, 2x2 mean): plain
torch restatements written from the contracts in include/e2fgvi_hip.h, the named cases that tests/test_helper_cases.py (no device)
and tests/test_gpu_helper_edges.py (the kernels) both run, and deliberately wrong readings of the text.

Every restatement takes `dt`: torch.float64 is the reference; torch.float32 evaluates the same formula with one fp32 rounding per
operation.  The warps work in pixel coordinates (q = p + flow), not through grid_sample's normalised ones.

Two classes of case:
  exact    every intermediate of the operation fits 24 significand bits (flows in quarters, integer features, dyadic resize ratios
           and weights), so any evaluation order, with or without fused multiply-adds, gives the float64 result bit for bit.  The
           CPU test checks that condition (restatement in fp32 == restatement in fp64); the GPU test then asks torch.equal.
  general  randn data, non-dyadic flows and ratios; `allowed(case)` derives the error an fp32 evaluation may have from the case's
           own tensors: (coordinate error) x (largest neighbour difference around the sample, per axis) + K x 2^-24 x max|v| for
           the samplers (a bilinear sample is continuous in its position, also across an integer and across the image edge),
           (number of roundings) x 2^-24 x sum|terms| for the sums.

VARIANTS are wrong readings; the CPU test requires each of them to move some case by more than that case's allowed error."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.util import gen, name_seed

F64, F32 = torch.float64, torch.float32
EPS = 2.0 ** -24
T2T = dict(kernel_size=(7, 7), stride=(3, 3), padding=(3, 3))

VARIANTS = ("zeros_as_border", "border_as_zeros", "corner_at_W", "swap_xy", "flow_b_at_p", "flow_up_not_doubled", "align_flipped",
            "no_clamp0", "i1_unclamped", "tap_kj_ki", "count9", "no_l_hi_clamp", "unbiased_var", "eps_outside", "stride1")


# ------------------------------------------------------------------------------------------------------------------ warps
def warp(src, flow, pad, dt=F64, variant=None):
    """src [N,H,W,C], flow [N,H,W,2] (x, y) -> src sampled at q = p + flow with four-corner bilinear weights.  pad "zeros": a
    corner outside the image contributes 0; "border": q is clamped to [0, W-1] x [0, H-1] first."""
    if variant == "zeros_as_border" and pad == "zeros":
        pad = "border"
    elif variant == "border_as_zeros" and pad == "border":
        pad = "zeros"
    src, flow = src.to(dt), flow.to(dt)
    if variant == "swap_xy":
        flow = flow.flip(-1)
    N, H, W, C = src.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    qx, qy = xs + flow[..., 0], ys + flow[..., 1]
    if pad == "border":
        qx, qy = qx.clamp(0, W - 1), qy.clamp(0, H - 1)
    fx, fy = qx.floor(), qy.floor()
    lx, ly = qx - fx, qy - fy
    n = torch.arange(N)[:, None, None]
    xmax = W if variant == "corner_at_W" else W - 1
    out = torch.zeros(N, H, W, C, dtype=dt)
    for dy, wy in ((0, 1 - ly), (1, ly)):
        for dx, wx in ((0, 1 - lx), (1, lx)):
            cx, cy = fx + dx, fy + dy                       # kept in floating point: a far flow has no integer form
            valid = (cx >= 0) & (cx <= xmax) & (cy >= 0) & (cy <= H - 1)
            w = torch.where(valid, wy * wx, torch.zeros((), dtype=dt))
            out = out + w[..., None] * src[n, cy.clamp(0, H - 1).long(), cx.clamp(0, W - 1).long()]
    return out


def warp_zeros(src, flow, dt=F64, variant=None):
    return warp(src, flow, "zeros", dt, variant)


def warp_border(src, flow, dt=F64, variant=None):
    return warp(src, flow, "border", dt, variant)


# ------------------------------------------------------------------------------------------------------------------ resize
def scale32(size_in, size_out, align):
    """the fp32 value the launcher forms (resize_scales in misc.hip), as a Python float"""
    if align:
        return float(np.float32(size_in - 1) / np.float32(size_out - 1)) if size_out > 1 else 0.0
    return float(np.float32(size_in) / np.float32(size_out))


def src_index(size_out, size_in, align, dt=F64, variant=None):
    """torch's upsample_bilinear2d index rule -> (i0, i1, l1, s) per output index"""
    if variant == "align_flipped":
        align = not align
    sc = torch.tensor(scale32(size_in, size_out, align), dtype=dt)
    d = torch.arange(size_out, dtype=dt)
    if align:
        s = sc * d
    else:
        s = sc * (d + 0.5) - 0.5
        if variant != "no_clamp0":
            s = s.clamp(min=0)
    i0 = s.trunc().clamp(max=size_in - 1)
    i1 = i0 + 1 if variant == "i1_unclamped" else (i0 + 1).clamp(max=size_in - 1)
    return i0.long(), i1.long(), s - i0, s


def resize_ref(x, Ho, Wo, align, scale=None, shift=None, dt=F64, variant=None):
    """x [N,H,W,C] -> [N,Ho,Wo,C], then v * scale[c] + shift[c]"""
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 1, W + 1, C, dtype=dt)           # (the row / column of zeros is what an unclamped i1 would read)
    xp[:, :H, :W] = x.to(dt)
    y0, y1, ly, _ = src_index(Ho, H, align, dt, variant)
    x0, x1, lx, _ = src_index(Wo, W, align, dt, variant)
    ly, lx = ly[:, None, None], lx[None, :, None]
    hy, hx = 1 - ly, 1 - lx
    r0, r1 = xp[:, y0], xp[:, y1]
    v = hy * (hx * r0[:, :, x0] + lx * r0[:, :, x1]) + ly * (hx * r1[:, :, x0] + lx * r1[:, :, x1])
    if scale is not None:
        v = v * scale.to(dt)
    if shift is not None:
        v = v + shift.to(dt)
    return v


def up2x_align(flow_prev, dt=F64, variant=None):
    """[N,h,w,2] -> [N,2h,2w,2], bilinear, align_corners = True"""
    return resize_ref(flow_prev, 2 * flow_prev.shape[1], 2 * flow_prev.shape[2], True, dt=dt, variant=variant)


# ------------------------------------------------------------------------------------------------------------------ SPyNet, propagation
def spynet_level_input_ref(pyr, ref_idx, supp_idx, flow_prev, dt=F64, variant=None):
    """pyr [F,h,w,>=3] -> [Np,h,w,8] = ref(3) | warp_border(supp, flow_up)(3) | flow_up(2), flow_up = 2 * up2x(flow_prev) or 0"""
    p = pyr[..., :3].to(dt)
    Np, (h, w) = len(ref_idx), pyr.shape[1:3]
    if flow_prev is None:
        fu = torch.zeros(Np, h, w, 2, dtype=dt)
    else:
        fu = up2x_align(flow_prev, dt, variant) * (1.0 if variant == "flow_up_not_doubled" else 2.0)
    return torch.cat([p[list(ref_idx)], warp_border(p[list(supp_idx)], fu, dt, variant), fu], -1)


def prop_cond_ref(fp, f2, fa, fb, dt=F64, variant=None):
    """fp [N,H,W,C], f2 [N,H,W,>=C], fa / fb [N,H,W,2] -> (cond [N,H,W,2C], flows [N,H,W,4])"""
    C = fp.shape[3]
    f1 = fa.to(dt)
    c1 = warp_zeros(fp, f1, dt, variant)
    if fb is None:
        return torch.cat([c1, torch.zeros_like(c1)], -1), torch.cat([f1, torch.zeros_like(f1)], -1)
    fn2 = f1 + (fb.to(dt) if variant == "flow_b_at_p" else warp_zeros(fb, f1, dt, variant))
    return torch.cat([c1, warp_zeros(f2[..., :C], fn2, dt, variant)], -1), torch.cat([f1, fn2], -1)


# ------------------------------------------------------------------------------------------------------------------ fold / unfold
def _to_cols(p, Fr, L, C, variant=None):
    """the kernels' rows [Fr*L, (tap = ki*7+kj)*C + c] -> F.fold's columns [Fr, c*49 + tap, L]"""
    t = p.reshape(Fr, L, 7, 7, C)
    if variant == "tap_kj_ki":
        t = t.transpose(2, 3)
    return t.permute(0, 4, 2, 3, 1).reshape(Fr, C * 49, L)


def _from_cols(cols, Fr, L, C, variant=None):
    t = cols.reshape(Fr, C, 7, 7, L).permute(0, 4, 2, 3, 1)
    if variant == "tap_kj_ki":
        t = t.transpose(2, 3)
    return t.reshape(Fr * L, 49 * C)


def fold_gather(p, Fr, fh, fw, H, W, C, clamp=True):
    """the fold as the header words it, output pixel by output pixel: (Y, X) sums tap (Y+3-3ly, X+3-3lx) of every token (ly, lx)
    with 0 <= Y+3-3ly <= 6 (same for X) -> (sum [Fr,H,W,C], count [H,W]).  clamp=False is the wrong reading that does not stop
    at the last token row / column: the flat row index then runs into the next row, the next frame, or (read as 0) off the end."""
    e = p.reshape(Fr * fh * fw, 49, C)

    def rng(Y, L):
        hi = (Y + 3) // 3
        return [l for l in range(max(0, -((3 - Y) // 3)), (min(hi, L - 1) if clamp else hi) + 1)]
    out, cnt = torch.zeros(Fr, H, W, C, dtype=p.dtype), torch.zeros(H, W, dtype=p.dtype)
    for Y in range(H):
        lys = rng(Y, fh)
        for X in range(W):
            lxs = rng(X, fw)
            cnt[Y, X] = len(lys) * len(lxs)
            for f in range(Fr):
                for ly in lys:
                    for lx in lxs:
                        t = (f * fh + ly) * fw + lx
                        if t < e.shape[0]:
                            out[f, Y, X] += e[t, (Y + 3 - 3 * ly) * 7 + (X + 3 - 3 * lx)]
    return out, cnt


def fold_sum(p, Fr, fh, fw, H, W, C, dt=F64, variant=None):
    """overlap-add fold of rows [Fr*fh*fw, 49*C] -> (sum [Fr,H,W,C], overlap count [H,W,1])"""
    p = p.to(dt)
    if variant == "no_l_hi_clamp":
        s, cnt = fold_gather(p, Fr, fh, fw, H, W, C, clamp=False)
        return s, cnt[..., None]
    s = F.fold(_to_cols(p, Fr, fh * fw, C, variant), output_size=(H, W), **T2T).permute(0, 2, 3, 1)
    cnt = F.fold(torch.ones(1, 49, fh * fw, dtype=dt), output_size=(H, W), **T2T)[0, 0][..., None]
    return s, (torch.full_like(cnt, 9.0) if variant == "count9" else cnt)


def ffn_fold_ref(hid, Fr, fh, fw, H, W, C, gelu, dt=F64, variant=None):
    s, cnt = fold_sum(hid, Fr, fh, fw, H, W, C, dt, variant)
    v = s / cnt
    return F.gelu(v) if gelu else v


def ffn_unfold_ref(folded, fh, fw, gelu, dt=F64, variant=None):
    """[Fr,H,W,C] -> [Fr*fh*fw, 49*C], zero padding, then the GELU (GELU(0) = 0)"""
    Fr, H, W, C = folded.shape
    rows = _from_cols(F.unfold(folded.to(dt).permute(0, 3, 1, 2), **T2T), Fr, fh * fw, C, variant)
    return F.gelu(rows) if gelu else rows


def unfold_padding(Fr, fh, fw, H, W, C):
    """bool [Fr*fh*fw, 49*C]: the taps that lie in the zero padding"""
    inside = F.unfold(torch.ones(Fr, C, H, W, dtype=F64), **T2T)
    return _from_cols(inside, Fr, fh * fw, C) == 0


def softcomp_fold_ref(emb, Fr, fh, fw, H, W, C, bias_hwc=None, residual=None, dt=F64, variant=None):
    s, _ = fold_sum(emb, Fr, fh, fw, H, W, C, dt, variant)
    if bias_hwc is not None:
        s = s + bias_hwc.to(dt)
    if residual is not None:
        s = s + residual.to(dt)
    return s


def token_grid(H, W):
    return (H - 1) // 3 + 1, (W - 1) // 3 + 1


# ------------------------------------------------------------------------------------------------------------------ the rest
def window_pool_ref(x, w45, b1, dt=F64):
    """x [BT,fh,fw,C] -> [BT * fh/5 * fw/9, C]: Linear(45 -> 1) over each 5 x 9 window, weight index py*9 + px"""
    BT, fh, fw, C = x.shape
    t = x.to(dt).reshape(BT, fh // 5, 5, fw // 9, 9, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 45, C)
    return (t * w45.to(dt)[None, :, None]).sum(1) + b1.to(dt)


def layernorm_ref(x, gamma, beta, dt=F64, variant=None):
    x, gamma, beta = x.to(dt), gamma.to(dt), beta.to(dt)
    if variant is None or variant not in ("unbiased_var", "eps_outside"):
        return F.layer_norm(x, (x.shape[-1],), gamma, beta, 1e-5)
    xc = x - x.mean(-1, keepdim=True)
    var = xc.pow(2).sum(-1, keepdim=True) / (x.shape[-1] - (1 if variant == "unbiased_var" else 0))
    rstd = 1 / (var.sqrt() + 1e-5) if variant == "eps_outside" else 1 / (var + 1e-5).sqrt()
    return xc * rstd * gamma + beta


def avgpool2_ref(x, dt=F64, variant=None):
    """[N,H,W,C] -> [N,H/2,W/2,C], the mean of each 2 x 2 block"""
    N, H, W, C = x.shape
    s = x.to(dt).permute(0, 3, 1, 2)
    if variant == "stride1":
        return F.avg_pool2d(F.pad(s, (0, W // 2, 0, H // 2)), 2, 1)[:, :, :H // 2, :W // 2].permute(0, 2, 3, 1)
    return F.avg_pool2d(s, 2, 2).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------------------ error bounds
def gamma(k):
    """k roundings in a row: (1 + 2^-24)^k - 1 <= k 2^-24 / (1 - k 2^-24), the bound of a sum's relative error to all orders"""
    return k * EPS / (1 - k * EPS)


def half_ulp(ref, dtype):
    """half a unit in the last place of `dtype` at |ref|: what one rounding of the exact value to bf16 / fp16 may add"""
    if dtype == F32:
        return torch.zeros_like(ref)
    bits, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    e = torch.frexp(ref.abs().clamp(min=2.0 ** -140))[1].double() - 1            # |ref| in [2^e, 2^(e+1))
    return torch.pow(torch.tensor(2.0, dtype=F64), e.clamp(min=emin) - bits)


def _around(src, pad, qx, qy):
    """largest |difference of x-neighbours| and |difference of y-neighbours| of src (all channels) over the 5 x 5 pixels around
    floor(q); src continued by zeros or by its border pixels.  A sample that moves by d << 1 px changes by at most d x that."""
    N, H, W, C = src.shape
    P = F.pad(src.to(F64).permute(0, 3, 1, 2), (3, 3, 3, 3), mode="replicate" if pad == "border" else "constant")
    dx = F.pad((P[..., 1:] - P[..., :-1]).abs().amax(1), (0, 1))
    dy = F.pad((P[..., 1:, :] - P[..., :-1, :]).abs().amax(1), (0, 0, 0, 1))
    n = torch.arange(N)[:, None, None]
    iy, ix = (qy.floor().clamp(-3, H + 2) + 3).long(), (qx.floor().clamp(-3, W + 2) + 3).long()
    return (F.max_pool2d(dx[:, None], 5, 1, 2)[:, 0][n, iy, ix], F.max_pool2d(dy[:, None], 5, 1, 2)[:, 0][n, iy, ix])


def warp_bound(src, flow, pad, dqx=0.0, dqy=0.0):
    """[N,H,W,1] bound on |fp32 warp - exact warp|.  The position q = p + f carries the error dq the flow came with plus one fp32
    rounding of the sum, <= 2^-24 |q| (a q beyond the image by more than a pixel samples a constant: its error does not count);
    the weights 1 - l, the four products w.w, w.v and the three additions are <= 8 roundings of values <= max|v|."""
    N, H, W, C = src.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    qx, qy = xs + flow[..., 0].to(F64), ys + flow[..., 1].to(F64)
    Dx, Dy = _around(src, pad, qx, qy)
    ex, ey = dqx + EPS * qx.abs().clamp(max=W + 1), dqy + EPS * qy.abs().clamp(max=H + 1)
    return (ex * Dx + ey * Dy + 8 * EPS * float(src.abs().max()))[..., None]


def resize_bound(x, Ho, Wo, align, scale=None, shift=None):
    """[N,Ho,Wo,C] bound.  The source position s = scale32 * d is one rounding (<= 2^-24 s), scale32 * (d + 0.5) - 0.5 two
    (<= 2^-24 (2 s + 0.5)); then as warp_bound; the affine adds two roundings of its result."""
    N, H, W, C = x.shape
    sy, sx = src_index(Ho, H, align)[3], src_index(Wo, W, align)[3]
    ey, ex = (EPS * sy, EPS * sx) if align else (EPS * (2 * sy + 0.5), EPS * (2 * sx + 0.5))
    qy, qx = torch.broadcast_tensors(sy.clamp(max=H - 1)[None, :, None], sx.clamp(max=W - 1)[None, None, :])
    Dx, Dy = _around(x, "border", qx.expand(N, Ho, Wo), qy.expand(N, Ho, Wo))
    b = (ex[None, None, :] * Dx + ey[None, :, None] * Dy + 8 * EPS * float(x.abs().max()))[..., None].expand(N, Ho, Wo, C)
    if scale is not None:
        b = b * scale.abs().to(F64)
    if scale is not None or shift is not None:
        b = b + 2 * EPS * resize_ref(x.abs(), Ho, Wo, align, None if scale is None else scale.abs(), None if shift is None else shift.abs())
    return b


# ------------------------------------------------------------------------------------------------------------------ case data
def _ints(g, shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _quarters(g, shape, span):
    """multiples of 1/4 in [-span, span]"""
    return torch.randint(-4 * span, 4 * span + 1, shape, generator=g).float() / 4


def _plant(flow, targets, start=0):
    """flow [H,W,2]: pixel k (row-major from `start`) gets the flow that puts its sample at targets[k] = (qx, qy)"""
    H, W = flow.shape[:2]
    for k, (qx, qy) in enumerate(targets):
        y, x = divmod(start + k, W)
        flow[y, x, 0], flow[y, x, 1] = qx - x, qy - y
    return flow


def edge_targets(H, W, frac):
    """sample positions on every border class; frac = the fractional offset used inside the half-open bands"""
    a, b = float(W - 1), float(H - 1)
    return [(0.0, 0.0), (a, b), (0.0, b), (a, 0.0), (-frac, 2.0), (2.0, -frac), (-1.0, 1.0), (1.0, -1.0), (a + frac, 2.0),
            (2.0, b + frac), (float(W), 1.0), (1.0, float(H)), (-frac, -frac), (a + frac, b + frac), (-1.0, -1.0), (float(W), float(H)),
            (a + frac, -frac), (3.0, 2.0), (a, 2.0 + frac), (2.0 + frac, b)]


FAR = (3e9, -3e9, 1e30, -1e30)


def _plant_far(flow, start):
    """flows beyond int32 and beyond any pixel grid, alone and paired, on pixels from `start` on"""
    H, W = flow.shape[:2]
    vals = [(f, 0.0) for f in FAR] + [(0.0, f) for f in FAR] + [(3e9, -1e30), (-1e30, 3e9)]
    for k, (u, v) in enumerate(vals):
        y, x = divmod(start + k, W)
        flow[y, x, 0], flow[y, x, 1] = u, v
    return flow


def _prop(name, H, W, C, exact, with_fb, C2=None):
    g = gen(name_seed(name))
    N, T = 2, 3                                              # the engine's flows: [N, T, H, W, 2], image n at n * T*H*W*2
    feat = (lambda s: _ints(g, s)) if exact else (lambda s: torch.randn(s, generator=g))
    fp, f2 = feat((N, H, W, C)), feat((N, H, W, C2 or C))
    fl = _quarters(g, (N, T, H, W, 2), 3) if exact else torch.randn(N, T, H, W, 2, generator=g) * 2
    frac = 0.25 if exact else 0.3
    _plant(fl[0, 1], edge_targets(H, W, frac))               # flow_a of image 0: every border class ...
    fl[0, 1, H - 1, W - 1] = 0.0                             # ... and a flow of 0
    if exact:
        _plant_far(fl[1, 1], 3)
        fl[1, 1, 0, 0], fl[1, 1, 0, 1] = torch.tensor([64.0, -64.0]), torch.tensor([-63.75, 0.25])
        fl[:, 0] = _quarters(g, (N, H, W, 2), 5)
        fl[0, 0, 0, :4, 0] = torch.tensor([64.0, -64.0, 63.75, -0.25])
    return dict(kind="prop_cond", exact=exact, fp=fp, f2=f2, flows=fl, ia=1, ib=0 if with_fb else None)


def _spynet(name, h, w, exact, mode):
    g = gen(name_seed(name))
    Fr = 4
    pyr = F.pad(_ints(g, (Fr, h, w, 3)) if exact else torch.randn(Fr, h, w, 3, generator=g), (0, 1))
    if mode == "pairs2x2":                                   # previous level 1 x 1: flow_up = 2 * flow_prev everywhere, exact
        halves = sorted({v / 2 for t in edge_targets(2, 2, 0.25) for v in t} | {-1.5, 2.5, 0.125})
        vals = [(u, v) for u in halves for v in (0.0, u, -u)] + [(f, 0.0) for f in FAR] + [(0.5, f) for f in FAR] + [(3e9, -1e30)]
        fprev = torch.tensor(vals).view(-1, 1, 1, 2)
        Np = fprev.shape[0]
        ref_idx, supp_idx = [i % Fr for i in range(Np)], [(3 * i + 1) % Fr for i in range(Np)]
    else:
        ref_idx, supp_idx = [0, 1, 2, 3, 3, 1, 2], [1, 2, 3, 2, 1, 1, 0]      # forward, reversed, repeated, a frame with itself
        Np = len(ref_idx)
        if mode == "noflow":
            fprev = None
        else:
            fprev = torch.randn(Np, h // 2, w // 2, 2, generator=g) * 1.5
            fprev[0] = 0.0
            fprev[1, 0, 0], fprev[1, -1, -1] = torch.tensor([-2.3, -1.7]), torch.tensor([3.1, 2.2])   # beyond both borders
    return dict(kind="spynet", exact=exact, pyr=pyr, ref_idx=ref_idx, supp_idx=supp_idx, flow_prev=fprev)


def _resize(name, size_in, size_out, align, C, exact, affine, N=2):
    g = gen(name_seed(name))
    x = _ints(g, (N, *size_in, C)) if exact else torch.randn(N, *size_in, C, generator=g)
    sc = sh = None
    if affine:
        sc = (torch.tensor([2.0, 0.5, 1.5, -1.0, 0.25, 4.0, -0.5, 1.0])[:C] if exact else torch.randn(C, generator=g) + 1.5)
        sh = (torch.tensor([0.25, -0.5, 1.0, 0.0, -2.0, 0.75, 3.0, -0.125])[:C] if exact else torch.randn(C, generator=g))
    return dict(kind="resize", exact=exact, x=x, out_hw=tuple(size_out), align=align, scale=sc, shift=sh)


def _fold(name, H, W, C, exact):
    g = gen(name_seed(name))
    Fr, (fh, fw) = 2, token_grid(H, W)
    feat = (lambda s: _ints(g, s)) if exact else (lambda s: torch.randn(s, generator=g))
    return dict(kind="fold", exact=exact, dims=(Fr, fh, fw, H, W, C), hid=feat((Fr * fh * fw, 49 * C)), bias=feat((H, W, C)),
                res=feat((Fr, H, W, C)))


def _pool(name, fh, fw, C, exact):
    g = gen(name_seed(name))
    BT = 3
    if exact:
        x, w45, b1 = _ints(g, (BT, fh, fw, C)), torch.randint(-64, 65, (45,), generator=g).float() / 64, torch.tensor([0.375])
    else:
        x, w45, b1 = torch.randn(BT, fh, fw, C, generator=g), 1 / 45. + 0.02 * torch.randn(45, generator=g), torch.randn(1, generator=g)
    return dict(kind="window_pool", exact=exact, x=x, w45=w45, b1=b1)


def _ln(name, rows, C):
    g = gen(name_seed(name))
    return dict(kind="layernorm", exact=False, x=torch.randn(rows, C, generator=g), gamma=torch.randn(C, generator=g),
                beta=torch.randn(C, generator=g))


def _avg(name, H, W, C):
    return dict(kind="avgpool", exact=True, x=_ints(gen(name_seed(name)), (2, H, W, C)))


FOLD_SIZES = ((1, 1), (4, 7), (8, 9), (9, 13), (10, 11))
_B = {}
_B.update({"prop exact 6x10": lambda n: _prop(n, 6, 10, 8, True, True, C2=12), "prop exact 5x7 no flow_b": lambda n: _prop(n, 5, 7, 8, True, False),
           "prop exact 5x7 C16": lambda n: _prop(n, 5, 7, 16, True, True, C2=24), "prop general 6x10": lambda n: _prop(n, 6, 10, 8, False, True, C2=12),
           "prop general 5x7 no flow_b": lambda n: _prop(n, 5, 7, 8, False, False), "prop general 5x7 C16": lambda n: _prop(n, 5, 7, 16, False, True)})
_B.update({"spynet exact 2x2": lambda n: _spynet(n, 2, 2, True, "pairs2x2"), "spynet exact 4x6 no flow": lambda n: _spynet(n, 4, 6, True, "noflow"),
           "spynet general 4x6": lambda n: _spynet(n, 4, 6, False, "flow"), "spynet general 6x10": lambda n: _spynet(n, 6, 10, False, "flow")})
for _a, _i, _o in ((True, (5, 9), (9, 17)), (True, (9, 17), (17, 5)), (True, (17, 3), (5, 9)), (True, (5, 9), (1, 1)), (True, (1, 9), (9, 1)),
                   (True, (9, 1), (17, 17)), (True, (5, 9), (5, 9)), (False, (8, 16), (16, 8)), (False, (16, 8), (8, 32)), (False, (8, 8), (32, 16)),
                   (False, (1, 8), (4, 16)), (False, (8, 1), (16, 4)), (False, (8, 16), (8, 16))):
    for _c in (3, 6, 8, 16):
        _B["resize exact %s %dx%d->%dx%d C%d" % ("align" if _a else "half", *_i, *_o, _c)] = \
            (lambda n, a=_a, i=_i, o=_o, c=_c: _resize(n, i, o, a, c, True, c in (3, 8)))
for _a, _i, _o in ((True, (13, 7), (7, 13)), (False, (13, 7), (7, 13)), (True, (12, 24), (5, 43)), (False, (12, 24), (5, 43)),
                   (False, (24, 43), (6, 11)), (True, (24, 43), (6, 11)), (False, (7, 5), (13, 12))):
    for _c in (3, 6, 8, 16):
        _B["resize general %s %dx%d->%dx%d C%d" % ("align" if _a else "half", *_i, *_o, _c)] = \
            (lambda n, a=_a, i=_i, o=_o, c=_c: _resize(n, i, o, a, c, False, c in (3, 8)))
for _h, _w in FOLD_SIZES:
    for _c in (4, 8, 12):
        _B["fold exact %dx%d C%d" % (_h, _w, _c)] = (lambda n, h=_h, w=_w, c=_c: _fold(n, h, w, c, True))
        _B["fold general %dx%d C%d" % (_h, _w, _c)] = (lambda n, h=_h, w=_w, c=_c: _fold(n, h, w, c, False))
for _h, _w in ((5, 9), (10, 27)):
    for _c in (4, 8, 12):
        _B["window_pool exact %dx%d C%d" % (_h, _w, _c)] = (lambda n, h=_h, w=_w, c=_c: _pool(n, h, w, c, True))
        _B["window_pool general %dx%d C%d" % (_h, _w, _c)] = (lambda n, h=_h, w=_w, c=_c: _pool(n, h, w, c, False))
for _c in (256, 512, 768, 1024):
    for _r in (1, 5):
        _B["layernorm %d rows C%d" % (_r, _c)] = (lambda n, r=_r, c=_c: _ln(n, r, c))
for _h, _w in ((2, 2), (6, 10)):
    for _c in (1, 3, 4, 6):
        _B["avgpool %dx%d C%d" % (_h, _w, _c)] = (lambda n, h=_h, w=_w, c=_c: _avg(n, h, w, c))
NAMES = tuple(_B)
_CACHE = {}


def case(name):
    """the named case (built once; its tensors are shared and must not be written to)"""
    if name not in _CACHE:
        _CACHE[name] = dict(_B[name](name), name=name)
    return _CACHE[name]


def names(kind=None, exact=None):
    """names of the cases of a kind ("prop_cond", "spynet", "resize", "fold", "window_pool", "layernorm", "avgpool")"""
    return [n for n in NAMES if (kind is None or case(n)["kind"] == kind) and (exact is None or case(n)["exact"] == exact)]


def prop_flows(c):
    """(flow_a, flow_b or None) as [N,H,W,2] views of the case's [N,T,H,W,2] flows"""
    return c["flows"][:, c["ia"]], (None if c["ib"] is None else c["flows"][:, c["ib"]])


def reference(c, dt=F64, variant=None):
    """the outputs of the case's operation(s), a tuple of tensors of dt"""
    k = c["kind"]
    if k == "prop_cond":
        fa, fb = prop_flows(c)
        return prop_cond_ref(c["fp"], c["f2"], fa, fb, dt, variant)
    if k == "spynet":
        return (spynet_level_input_ref(c["pyr"], c["ref_idx"], c["supp_idx"], c["flow_prev"], dt, variant),)
    if k == "resize":
        return (resize_ref(c["x"], *c["out_hw"], c["align"], c["scale"], c["shift"], dt, variant),)
    if k == "fold":                                          # (normalised fold, its unfold, SoftComp fold with bias and residual)
        Fr, fh, fw, H, W, C = c["dims"]
        folded = ffn_fold_ref(c["hid"], *c["dims"], False, dt, variant)
        return (folded, ffn_unfold_ref(folded, fh, fw, False, dt, variant),
                softcomp_fold_ref(c["hid"], *c["dims"], c["bias"], c["res"], dt, variant))
    if k == "window_pool":
        return (window_pool_ref(c["x"], c["w45"], c["b1"], dt),)
    if k == "layernorm":
        return (layernorm_ref(c["x"], c["gamma"], c["beta"], dt, variant),)
    if k == "avgpool":
        return (avgpool2_ref(c["x"], dt, variant),)
    raise KeyError(k)


def quotients(c):
    """outputs of an exact case that hold a correctly rounded quotient (sum / overlap count) instead of an exact value"""
    return (0, 1) if c["kind"] == "fold" else ()


def ln_bound(x):
    """allowed max|y - ref| / rms(ref) of the LayerNorm kernel at C = 256 VPL: test_layernorm_off_unit_scale's bound with its
    rounding count restated -- 4 VPL additions per lane and 6 shuffle steps on the way to the mean (+ the division, + the
    subtraction), each <= 2^-24 |mean|, over std; 5e-6 for everything behind the centred row."""
    xd = x.double()
    ratio = (xd.mean(1).abs() / xd.std(1, unbiased=False)).max().item()
    return 5e-6 + (4 * (x.shape[1] // 256) + 8) * EPS * ratio


def allowed(c):
    """per output of reference(c): the largest |fp32 evaluation - reference| the arithmetic allows, a tensor or a float (absolute);
    0 for exact cases"""
    ref = reference(c)
    if c["exact"]:
        return tuple(0.0 for _ in ref)
    k = c["kind"]
    if k == "prop_cond":
        fa, fb = prop_flows(c)
        C = c["fp"].shape[3]
        b1 = warp_bound(c["fp"], fa, "zeros")
        zero2 = torch.zeros_like(fa, dtype=F64)
        if fb is None:
            return torch.cat([b1.expand(-1, -1, -1, C), torch.zeros_like(ref[0][..., C:])], -1), torch.cat([zero2, zero2], -1)
        fn2 = ref[1][..., 2:]
        e2 = warp_bound(fb, fa, "zeros") + EPS * fn2.abs()                   # flow_n2: the warped flow_b, one more addition
        b2 = warp_bound(c["f2"][..., :C], fn2, "zeros", e2[..., 0], e2[..., 1])
        return torch.cat([b1.expand(-1, -1, -1, C), b2.expand(-1, -1, -1, C)], -1), torch.cat([zero2, e2], -1)
    if k == "spynet":
        fp = c["flow_prev"]
        h, w = c["pyr"].shape[1:3]
        efu = 2 * resize_bound(fp, h, w, True)                               # (the doubling is exact)
        fu = ref[0][..., 6:]
        bw = warp_bound(c["pyr"][c["supp_idx"]][..., :3], fu, "border", efu[..., 0], efu[..., 1])
        return (torch.cat([torch.zeros_like(ref[0][..., :3]), bw.expand(-1, -1, -1, 3), efu], -1),)
    if k == "resize":
        return (resize_bound(c["x"], *c["out_hw"], c["align"], c["scale"], c["shift"]),)
    if k == "fold":          # a pixel under n tokens: n - 1 additions, and the division where n > 1; SoftComp: + bias + residual
        Fr, fh, fw, H, W, C = c["dims"]
        s, n = fold_sum(c["hid"].abs(), *c["dims"])
        b = gamma(n - 1 + (n > 1)) * s / n
        return (b, ffn_unfold_ref(b, fh, fw, False), gamma(n + 1) * (s + c["bias"].abs() + c["res"].abs()))
    if k == "window_pool":                                   # 45 multiply-adds behind the bias
        return (gamma(46) * window_pool_ref(c["x"].abs(), c["w45"].abs(), c["b1"].abs()),)
    if k == "layernorm":
        return (ln_bound(c["x"]) * ref[0].pow(2).mean().sqrt().item(),)
    raise KeyError(k)


def check(got, ref, bound, what, dtype=F32):
    """|got - ref| <= bound + half a unit of `dtype` at ref, element by element (bound: a float or a tensor that broadcasts); where
    that is 0 the values must be equal.  The largest measured / allowed ratio goes to the margin log."""
    from tests.util import assert_bound
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got.float()).all(), what + ": non-finite output"
    e = (got.double() - ref).abs()
    b = (torch.as_tensor(bound, dtype=F64) + half_ulp(ref, dtype)).expand_as(e)
    z = b == 0
    assert not z.any() or float(e[z].max()) == 0, "%s: %d values that must be exact differ" % (what, int((e[z] > 0).sum()))
    if not z.all():
        assert_bound((e[~z] / b[~z]).max().item(), 1.0, what)


def check_exact(got, ref, what):
    """got == the float64 result rounded once to got's type (an exact case's result is an fp32 number, so the way a conversion
    from float64 to 16 bits goes through fp32 adds no second rounding)"""
    exp = ref.to(got.dtype)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(exp.shape), (what, tuple(got.shape), tuple(exp.shape))
    bad = ~((got == exp) | (torch.isnan(got) & torch.isnan(exp)))
    assert not bad.any(), "%s: %d of %d values differ, first at %s: got %r, expected %r" % (
        what, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(got[bad][0]), float(exp[bad][0]))


CAST_N = (4, 260)


def cast_inputs(dtype, n):
    """fp32 values at the edges of a conversion to bf16 / fp16: ties to even, the largest finite value and the first that overflows,
    subnormals, signed zeros, infinities; padded to n with a ramp"""
    if dtype == torch.float16:
        v = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 65504.0, 65519.996, 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25,
             2.0 ** -25 * (1 + 2.0 ** -23), 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, 0.0, -0.0, math.inf, -math.inf]
    else:
        big = float(torch.tensor(3.3895313892515355e38))    # the largest finite bf16
        v = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, big, big * (1 + 2.0 ** -9), 3.4e38, -3.4e38, 2.0 ** -133, 2.0 ** -134,
             2.0 ** -134 * 1.5, 2.0 ** -126 - 2.0 ** -134, 2.0 ** -149, 0.0, -0.0, math.inf, -math.inf]
    v = v[:n] if n < len(v) else v + [(-1) ** i * (1 + i / 97.0) * 2.0 ** (i % 7 - 3) for i in range(n - len(v))]
    return torch.tensor(v, dtype=F32)
