"""Deformable-conv cases off the model's geometry, offsets built from where each sample lands, and a float64 reference.

Every other GPU test of e2fgvi_mdcn_nhwc runs the propagation's geometry (3x3, stride 1, pad 1, dilation 1, 16 channels per
deform group, one column tile) on i.i.d. Gaussian offsets, which never put a sample ON an integer position or on the guard's
edges -1 and H.  The cases below are the smallest shapes that reach each remaining path of csrc/mdcn.hip
(tests/test_mdcn_cases.py checks, on the CPU, that the inputs do what this text says; tests/test_gpu_mdcn_geometry.py runs the
kernel on them).  Columns: N, source channels, H x W, Cout, deform groups, KH x KW, stride, pad, dilation.

    one_pixel           4, [16],     1x1,   32,  1, 3x3, 1,1,1   9 units (odd: half-filled last K chunk); M = 4 < BM
    wide_group          2, [32],     7x9,   40,  1, 3x3, 1,1,1   two 16-channel blocks per group (cgq = 2)
    stride2_two_ntiles  2, [64],     9x11,  136, 2, 3x3, 2,1,1   Ho x Wo 5x6; cgq = 2; a second, partial column tile (Npad 160)
    dilated             1, [64],     9x11,  24,  4, 3x3, 1,2,2   dilation
    pointwise_short_k   3, [48],     5x6,   8,   1, 1x1, 1,0,1   cgq = 3; 3 units = 2 K chunks < the K groups of tiles 5 and 7
    row_kernel          1, [32],     8x10,  200, 2, 1x3, 1,0,1   KH != KW; Ho x Wo 8x8; Cout 200
    five_by_five        2, [32],     10x12, 33,  2, 5x5, 2,2,1   50 units; odd Cout
    no_pad              1, [96],     6x7,   48,  2, 3x3, 1,0,1   48 channels per group; Ho x Wo 4x5
    two_sources         2, [32, 96], 6x8,   64,  8, 3x3, 1,1,1   source boundary after group 1, flow half after group 3

Offsets.  For every (image, group, tap, output pixel) and each axis a landing coordinate `t` is chosen and the offset is
t - (o * stride - pad + k * dil).  Per axis of length L the landing classes are the twelve positions CLASS_NAMES (around
both guard edges and both border pixels, integers included), two far ones (-1e4, +1e6) and six shares of interior multiples
of 1/4 in [0, L - 1]; the classes are dealt out by cycling through a seeded permutation of the samples, so each class's count
is known, not drawn.  All values are small dyadic numbers: the fp32 position the kernel forms equals the float64 one exactly
and no border decision can flip on rounding.  Masks are uniform in [0, 1); sources ~ randn, weights ~ randn / sqrt(C K), bias ~
randn.  No GPU import here."""
import math

import torch

from tests.util import gen, name_seed

#            N  channels  H   W  Cout dg KH KW stride pad dil
CASES = {
    "one_pixel": (4, [16], 1, 1, 32, 1, 3, 3, 1, 1, 1),
    "wide_group": (2, [32], 7, 9, 40, 1, 3, 3, 1, 1, 1),
    "stride2_two_ntiles": (2, [64], 9, 11, 136, 2, 3, 3, 2, 1, 1),
    "dilated": (1, [64], 9, 11, 24, 4, 3, 3, 1, 2, 2),
    "pointwise_short_k": (3, [48], 5, 6, 8, 1, 1, 1, 1, 0, 1),
    "row_kernel": (1, [32], 8, 10, 200, 2, 1, 3, 1, 0, 1),
    "five_by_five": (2, [32], 10, 12, 33, 2, 5, 5, 2, 2, 1),
    "no_pad": (1, [96], 6, 7, 48, 2, 3, 3, 1, 0, 1),
    "two_sources": (2, [32, 96], 6, 8, 64, 8, 3, 3, 1, 1, 1),
}
NAMES = tuple(CASES)
EVEN_DG = tuple(n for n in NAMES if CASES[n][5] % 2 == 0)          # the fused form (flows) needs an even group count

# landing classes of one axis of length L: (name, position as a function of L); then the far ones and the interior shares
CLASS_NAMES = ("-1.25", "-1", "-0.75", "-0.25", "0", "0.5", "L-1.5", "L-1", "L-0.75", "L-0.25", "L", "L+0.25")
FAR = (-1.0e4, 1.0e6)
INTERIOR_SHARES = 6
NCLASS = len(CLASS_NAMES) + len(FAR) + INTERIOR_SHARES            # 20: the cycle length
MUTATIONS = ("clamp", "allfour", "swap", "stride", "dil", "pad", "cq", "flow_half")


class Geometry:
    def __init__(self, name):
        (self.N, self.chans, self.H, self.W, self.Cout, self.dg, self.KH, self.KW, self.stride, self.pad, self.dil) = CASES[name]
        self.name = name
        self.C = sum(self.chans)
        self.K = self.KH * self.KW
        self.cg = self.C // self.dg
        self.Ho = (self.H + 2 * self.pad - (self.dil * (self.KH - 1) + 1)) // self.stride + 1
        self.Wo = (self.W + 2 * self.pad - (self.dil * (self.KW - 1) + 1)) // self.stride + 1
        self.samples = self.N * self.dg * self.K * self.Ho * self.Wo
        self.conv = (self.stride, self.pad, self.dil, self.dg)         # the trailing arguments of ref64()


def class_positions(L):
    """the twelve fixed landing positions and the two far ones of an axis of length L, in class order"""
    return [-1.25, -1.0, -0.75, -0.25, 0.0, 0.5, L - 1.5, L - 1.0, L - 0.75, L - 0.25, float(L), L + 0.25] + list(FAR)


def _landings(g, shape, L):
    """landing coordinates (float64) and class indices of `shape` samples on an axis of length L: sample perm[i] gets class
    i mod NCLASS; classes >= 14 are interior multiples of 1/4 in [0, L - 1]"""
    n = int(torch.tensor(shape).prod())
    perm = torch.randperm(n, generator=g)
    cls = torch.empty(n, dtype=torch.long)
    cls[perm] = torch.arange(n) % NCLASS
    fixed = torch.tensor(class_positions(L), dtype=torch.float64)
    interior = torch.randint(0, 4 * (L - 1) + 1, (n,), generator=g).double() / 4
    t = torch.where(cls < len(fixed), fixed[cls.clamp(max=len(fixed) - 1)], interior)
    return t.view(shape), cls.view(shape)


def base_positions(geo):
    """o * stride - pad + k * dil of every (tap, output pixel), per axis: float64 [K, Ho, Wo] each"""
    k = torch.arange(geo.K)
    by = (torch.arange(geo.Ho).view(1, -1, 1) * geo.stride - geo.pad + (k // geo.KW).view(-1, 1, 1) * geo.dil).double()
    bx = (torch.arange(geo.Wo).view(1, 1, -1) * geo.stride - geo.pad + (k % geo.KW).view(-1, 1, 1) * geo.dil).double()
    return by.expand(geo.K, geo.Ho, geo.Wo), bx.expand(geo.K, geo.Ho, geo.Wo)


def build_inputs(name):
    """the fp32 tensors of case `name` in mmcv's layouts (NCHW; offset [N, dg*2*K, Ho, Wo] as (g, tap, dy / dx)), plus the
    float64 landing coordinates ty, tx and their class indices cy, cx, each [N, dg, K, Ho, Wo]"""
    geo = Geometry(name)
    g = gen(name_seed("mdcn case " + name))
    x = torch.randn(geo.N, geo.C, geo.H, geo.W, generator=g)
    w = torch.randn(geo.Cout, geo.C, geo.KH, geo.KW, generator=g) / math.sqrt(geo.C * geo.K)
    b = torch.randn(geo.Cout, generator=g)
    msk = torch.rand(geo.N, geo.dg * geo.K, geo.Ho, geo.Wo, generator=g)
    shape = (geo.N, geo.dg, geo.K, geo.Ho, geo.Wo)
    ty, cy = _landings(g, shape, geo.H)
    tx, cx = _landings(g, shape, geo.W)
    by, bx = base_positions(geo)
    off = torch.stack((ty - by, tx - bx), 3).reshape(geo.N, geo.dg * 2 * geo.K, geo.Ho, geo.Wo).float()
    return dict(geo=geo, x=x, w=w, b=b, off=off, msk=msk, ty=ty, tx=tx, cy=cy, cx=cx)


def fused_offsets(raw, flows, max_residue, dg, K, mut=None):
    """SecondOrderDeformableAlignment's post-processing of the raw conv_offset output [N, dg*3*K, Ho, Wo] in float64:
    offset = max_residue * tanh(raw[:2/3]) + flow.flip(1) -- flows[:, 0:2] for the first half of the groups, flows[:, 2:4]
    for the second -- and mask = sigmoid(raw[2/3:]).  Returns (offset, mask) in mmcv's layouts."""
    raw, flows = raw.double(), flows.double()
    o1, o2, m = torch.chunk(raw, 3, 1)
    q1, q2 = torch.chunk(max_residue * torch.tanh(torch.cat((o1, o2), 1)), 2, 1)
    f1, f2 = flows[:, 0:2], flows[:, 2:4]
    if mut == "flow_half":
        f2 = f1
    q1 = q1 + f1.flip(1).repeat(1, dg * K // 2, 1, 1)
    q2 = q2 + f2.flip(1).repeat(1, dg * K // 2, 1, 1)
    return torch.cat((q1, q2), 1), torch.sigmoid(m)


def ref64(x, offset, mask, w, b, stride, pad, dil, dg, mut=None, flows=None, max_residue=None):
    """modulated_deform_conv2d in float64: this file's own restatement of the algorithm in oracle/dcn.py's docstring, with
    mmcv's guard applied as a SELECT -- torch.where(inside, ...) on the position before floor() and on the weights -- so that a
    sample with a non-finite or huge position contributes exactly 0, as in mmcv (which skips it).  NCHW in and out.
    flows: `offset` is the raw conv_offset output and `mask` is ignored (fused_offsets above).
    mut: a deliberately wrong variant (MUTATIONS), for the bite checks:
        clamp      border replication instead of zero corners        allfour   a sample with any corner outside is dropped
        swap       dy <-> dx                                         stride    treated as 1
        dil        treated as 1                                      pad       off by one
        cq         16-channel block cq of a group reads block 0      flow_half every group takes the first flow"""
    assert mut is None or mut in MUTATIONS, mut
    N, C, H, W = x.shape
    Co, _, KH, KW = w.shape
    K = KH * KW
    Ho = (H + 2 * pad - (dil * (KH - 1) + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * (KW - 1) + 1)) // stride + 1
    cg = C // dg
    if flows is not None:
        offset, mask = fused_offsets(offset, flows, max_residue, dg, K, mut)
    assert tuple(offset.shape) == (N, dg * 2 * K, Ho, Wo) and tuple(mask.shape) == (N, dg * K, Ho, Wo)
    x, w = x.double(), w.double()
    off = offset.double().view(N, dg, K, 2, Ho, Wo)
    dy, dx = (off[:, :, :, 1], off[:, :, :, 0]) if mut == "swap" else (off[:, :, :, 0], off[:, :, :, 1])
    m = mask.double().view(N, dg, K, Ho, Wo)
    s_, p_, d_ = (1 if mut == "stride" else stride), (pad + 1 if mut == "pad" else pad), (1 if mut == "dil" else dil)
    k = torch.arange(K)
    py = (torch.arange(Ho).view(1, -1, 1) * s_ - p_ + (k // KW).view(-1, 1, 1) * d_).double() + dy
    px = (torch.arange(Wo).view(1, 1, -1) * s_ - p_ + (k % KW).view(-1, 1, 1) * d_).double() + dx
    inside = (py > -1) & (px > -1) & (py < H) & (px < W)            # False for NaN
    py, px = torch.where(inside, py, 0.0), torch.where(inside, px, 0.0)
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    hy, hx = 1 - ly, 1 - lx
    y0, x0 = y0.long(), x0.long()
    y1, x1 = y0 + 1, x0 + 1
    if mut == "allfour":
        inside = inside & (y0 >= 0) & (y1 <= H - 1) & (x0 >= 0) & (x1 <= W - 1)
    xf = x.reshape(N, dg, cg, H * W)
    if mut == "cq":
        xf = xf.view(N, dg, cg // 16, 16, H * W)[:, :, :1].expand(N, dg, cg // 16, 16, H * W).reshape(N, dg, cg, H * W)
    P = K * Ho * Wo

    def corner(yy, xx, wgt):
        ok = inside if mut == "clamp" else inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(N, dg, 1, P)
        v = torch.gather(xf, 3, idx.expand(N, dg, cg, P))
        return v * torch.where(ok, wgt * m, 0.0).reshape(N, dg, 1, P)

    cols = corner(y0, x0, hy * hx) + corner(y0, x1, hy * lx) + corner(y1, x0, ly * hx) + corner(y1, x1, ly * lx)
    out = torch.einsum("ok,nkp->nop", w.reshape(Co, C * K), cols.reshape(N, C * K, Ho * Wo)).reshape(N, Co, Ho, Wo)
    return out if b is None else out + b.double().view(1, -1, 1, 1)


def rms(t):
    return t.double().pow(2).mean().sqrt().item()


_CACHE = {}


def case(name, rounding=None):
    """case `name`, its sources rounded to `rounding` (None: fp32 as built; torch.bfloat16 / torch.float16), built once per
    process and shared by every test: the dict of build_inputs() with x in its storage type and ref = ref64 on those values.
    Nothing in it may be written to."""
    key = ("generic", name, rounding)
    if key not in _CACHE:
        c = dict(build_inputs(name))
        if rounding is not None:
            c["x"] = c["x"].to(rounding)
        c["ref"] = ref64(c["x"].float(), c["off"], c["msk"], c["w"], c["b"], *c["geo"].conv)
        _CACHE[key] = c
    return _CACHE[key]


MAX_RESIDUE = 1.5


def fused_case(name, rounding=None):
    """the fused form of an even-dg case: raw conv_offset output ~ 0.5 randn [N, dg*3*K, Ho, Wo] and flows [N, 4, Ho, Wo] whose
    two fields put the CENTRE tap of each half of the groups on a landing class (dealt out as above, per image, half and pixel),
    max_residue = 1.5; ref = ref64 of the float64 post-processing.  x, w, b are the generic case's."""
    key = ("fused", name, rounding)
    if key not in _CACHE:
        base = case(name, rounding)
        geo = base["geo"]
        g = gen(name_seed("mdcn fused case " + name))
        raw = 0.5 * torch.randn(geo.N, geo.dg * 3 * geo.K, geo.Ho, geo.Wo, generator=g)
        ty, _ = _landings(g, (geo.N, 2, geo.Ho, geo.Wo), geo.H)
        tx, _ = _landings(g, (geo.N, 2, geo.Ho, geo.Wo), geo.W)
        by, bx = base_positions(geo)
        kc = (geo.KH // 2) * geo.KW + geo.KW // 2
        fy, fx = ty - by[kc], tx - bx[kc]                             # v (added to dy) and u (added to dx)
        flows = torch.stack((fx[:, 0], fy[:, 0], fx[:, 1], fy[:, 1]), 1).float()
        c = dict(geo=geo, x=base["x"], w=base["w"], b=base["b"], raw=raw, flows=flows)
        c["ref"] = ref64(c["x"].float(), raw, None, c["w"], c["b"], *geo.conv, flows=flows, max_residue=MAX_RESIDUE)
        _CACHE[key] = c
    return _CACHE[key]


NONFINITE_VALUES = (float("inf"), float("-inf"), float("nan"), 3e9, -3e9, 1e30)


def nonfinite_case(name="wide_group"):
    """case `name` with a handful of offsets replaced by +-inf, nan, +-3e9 (beyond int32) and 1e30, three of each, on samples
    that land inside the image otherwise: (off, off_far, ref) -- the offsets, the same with those values replaced by +-1e6
    (nan: +1e6), and ref64 of the latter.  mmcv's guard drops such a sample; so must every implementation."""
    key = ("nonfinite", name)
    if key not in _CACHE:
        c = case(name)
        geo = c["geo"]
        g = gen(name_seed("mdcn nonfinite " + name))
        good = ((c["ty"] > -1) & (c["ty"] < geo.H) & (c["tx"] > -1) & (c["tx"] < geo.W)).reshape(-1).nonzero().view(-1)
        pick = good[torch.randperm(len(good), generator=g)[:3 * len(NONFINITE_VALUES)]]
        axis = torch.arange(len(pick)) % 2
        off = c["off"].clone().view(geo.N, geo.dg, geo.K, 2, geo.Ho, geo.Wo).permute(0, 1, 2, 4, 5, 3).reshape(-1, 2)
        far = off.clone()
        for i, (s, a) in enumerate(zip(pick.tolist(), axis.tolist())):
            v = NONFINITE_VALUES[i % len(NONFINITE_VALUES)]
            off[s, a] = v
            far[s, a] = -1e6 if v < 0 else 1e6
        back = lambda t: t.view(geo.N, geo.dg, geo.K, geo.Ho, geo.Wo, 2).permute(0, 1, 2, 5, 3, 4).reshape(c["off"].shape).contiguous()
        off, far = back(off), back(far)
        _CACHE[key] = (off, far, ref64(c["x"], far, c["msk"], c["w"], c["b"], *geo.conv))
    return _CACHE[key]
