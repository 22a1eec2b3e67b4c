"""Every decision of the kernel table (e2fgvi_amd/tile_table.py), through the dispatch that acts on it.

The table says which conv / linear kernel each layer of the engine runs.  The kernel-level tests force tile codes on geometries of
their own; the table's own (layer geometry, tile code) pairs ran only inside whole forwards, under end-to-end bounds that a wrong
partial block or channel tail of one layer can hide below.  Here the parametrisation IS the table: every distinct (geometry, code)
pair, size class dropped, is one case, so a regenerated table is covered without an edit.  Each case

  * builds the layer as its key describes it (class, channels per source, groups, kernel, stride, padding, K granule, Winograd or
    not, tuned or not, split-operand alternative or not; 16-bit rows in bf16 AND fp16, which share the bf16 entries: ops._dt_key),
  * keeps the channel geometry and the epilogue and shrinks the pixels to about 2100-2600 per call, awkwardly: two images, sizes off
    the 16-pixel block and the 8-row tile (34x38; 34x36 where the wide-tile Winograd rule needs W % 4 == 0), odd inputs under the
    strided layers (67x75 -> 34x38, 91x100 -> 31x34), 2 x 1051 rows for the Linears -- a multiple of neither 32, 64 nor 128,
  * copies the row into the table under the size class of that call and calls the layer with tile=0, so that ops._decision returns
    the row and PackedConv.__call__ / PackedConvX.__call__ -- the code under test -- pick the launch,
  * asserts from the launch trace that exactly ONE conv kernel was launched, through the entry point the code stands for and with
    the tile the code names: the dispatch replaces a tabled kernel that the launcher rejects by the static default without an
    error, and that second launch fails the case,
  * compares with F.conv2d / F.linear in fp64 on the CPU (same epilogue) under the project's derived bounds (tests/util.fp32_tol),
    sources at a channel offset inside wider tensors, the result in a channel slice of a pre-filled tensor whose other bytes must
    stay untouched.

No case is skipped.  A tabled kernel that rejected its small shape would get the smallest shape it accepts, with the reason in a
comment in _shape(); today none does.  The four tests at the top need no GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from e2fgvi_amd import ops, tile_table
from tests.test_gpu_fp16 import assert_is_half_of
from tests.util import (assert_close, assert_one_conv_launch, fp32_tol, gen as _gen, launch_trace, name_seed, nchw, nhwc, tabled)

BF16, F16 = torch.bfloat16, torch.float16
SF = ops._SIZE_FIELD


def table_pairs(tiles):
    """the distinct (geometry, tile code) pairs of a decision table: keys without their size-class field"""
    pairs = {(k[:SF] + k[SF + 1:], int(v)) for k, v in tiles.items()}
    return sorted(pairs, key=lambda p: (isinstance(p[0][0], str), repr(p[0]), p[1]))


def pair_id(pair):
    """'x 512<-128+192 k3s1p1g2 out16 tile17' / 'f32 128<-128+128 k3s1p1g1 bk32 res act2 wino x3 code46064'"""
    geom, code = pair
    if isinstance(geom[0], str):
        fam, cout, cpg, kh, kw, s, p, g, odt, nchw_, taps = geom
        words = [fam, "%d<-%s" % (cout, "+".join(map(str, cpg))), "k%ds%dp%dg%d" % (kh, s, p, g), "out32" if odt == 0 else "out16"]
        words += ["nchw"] * bool(nchw_) + ["taps"] * bool(taps) + ["tile%d" % code]
    else:
        cout, cpg, kh, kw, s, p, g, bk, res, act, wino, tune, static = geom[:13]
        words = ["f32", "%d<-%s" % (cout, "+".join(map(str, cpg))), "k%ds%dp%dg%d" % (kh, s, p, g), "bk%d" % bk]
        words += ["res"] * bool(res) + ["act%d" % act] + ["wino"] * bool(wino) + ["tune"] * bool(tune)
        words += ["static%d" % static] * bool(static) + list(geom[13:]) + ["code%d" % code]
    return " ".join(words)


PAIRS = table_pairs(tile_table.TILES)
IDS = [pair_id(p) for p in PAIRS]


# --------------------------------------------------------------------------------------------------------- without a GPU
def code_family(code):
    """the family of a table value: what the dispatch of ops.PackedConv / PackedConvX does with it"""
    if code >= ops.W3_BASE:
        return "w3" if code - ops.W3_BASE in ops.W3_CANDIDATES else None            # split-operand Winograd, its block shape
    if code >= ops.X3_BASE:
        return "x3" if 1 <= code - ops.X3_BASE < 200 else None                       # split-operand GEMM, its tile
    if code in ops.W4_CODES:
        return "w4"                                                                  # wide-tile fp32 Winograd
    if 2000 <= code < 2100:
        return "dma" if code > 2000 else None                                        # LDS-DMA fp32 GEMM, its tile
    if 0 <= code < 256 or 10000 <= code < ops.X3_BASE:
        return "own"                                             # the layer's own kernel, its tile (0: static; 200 ... 255: implicit GEMM)
    return None


def test_every_pair_of_the_table_is_a_case():
    """the parametrisation holds each distinct (geometry, code) pair of the table once, under a readable id of its own"""
    distinct = {(k[:SF] + k[SF + 1:], v) for k, v in tile_table.TILES.items()}
    assert len(PAIRS) == len(distinct) and set(PAIRS) == distinct
    assert len(set(IDS)) == len(IDS), "two pairs share an id"
    assert len({g for g, _ in PAIRS}) == len({k[:SF] + k[SF + 1:] for k in tile_table.TILES})
    assert tile_table.TABLE_FORMAT == ops.TABLE_FORMAT and PAIRS, "the checked-in table would be ignored"
    for k in tile_table.TILES:
        assert len(k) in (12, 14, 15) and (len(k) == 12) == isinstance(k[0], str), "neither key layout: %r" % (k,)
        assert len(k) < 15 or k[14] == "x3", k


def test_every_code_of_the_table_decodes_to_a_known_family():
    """a typo or a new family cannot slip past the enumeration: every value is a code the dispatch acts on, and one that the layer
    its key describes would not ignore (the split kernels only where the key asks for them, tiles of the own / LDS-DMA kernels
    only on tuned layers, the split Winograd kernel only on Winograd calls, the 16-bit rows on their own kernel)"""
    for key, code in tile_table.TILES.items():
        fam = code_family(code)
        assert isinstance(code, int) and fam is not None, "%r: %r is no known tile code" % (key, code)
        if isinstance(key[0], str):
            allowed = {"x": {"own"}, "x32": {"own"}, "x3": {"own"}, "x32+3": {"own", "x3"}}[key[0]]
            assert code < 200 or fam == "x3", "%r: %d is no tile of the LDS-DMA kernel" % (key, code)
        else:
            use_wino, tune, x3 = key[11], key[12], key[14:] == ("x3",)
            allowed = {"own"} if tune or code == 0 else set()
            allowed |= {"dma"} if tune and not use_wino else set()
            allowed |= ({"x3"} | ({"w3"} if use_wino else set())) if x3 else set()
        assert fam in allowed, "%r: code %d (%s) is ignored by the layer this key describes" % (key, code, fam)


def test_decode_names_the_family_of_every_code():
    """ops._decode, the dispatch's one decoder, against code_family above (an independent restatement) on every value of the
    table and on every candidate the timed selection can record, its base added; the argument recombines to the code"""
    base = {"own": 0, "w4": 0, "dma": 2000, "x3": ops.X3_BASE, "w3": ops.W3_BASE}
    assert ops.DMA_BASE == 2000 and (ops.X3_BASE, ops.W3_BASE) == (30000, 40000) and ops.W4_CODES == {2464: (2, 64)}
    codes = set(tile_table.TILES.values()) | set(ops.W4_CODES) | set(ops.TUNE_CANDIDATES) | set(ops.WINO_CANDIDATES)
    codes |= set(ops.XTUNE_CANDIDATES) | set(ops.XTUNE_ROWSHIFT)                                   # tiles of a PackedConvX's own kernel
    codes |= {2000 + t for t in ops.XTUNE_CANDIDATES if t < 100}                                   # ... as a tuned fp32 layer's alternative
    codes |= {ops.X3_BASE + t for t in ops.XTUNE_CANDIDATES}                                       # ... on split operands
    codes |= {ops.W3_BASE + s for s in ops.W3_CANDIDATES + (ops.W3_WIDE, ops.W3_WIDE_FALLBACK)}
    assert len(codes) > 40
    for code in sorted(codes):
        fam, arg = ops._decode(code)
        assert fam is not None and fam == code_family(code), "code %d: _decode says %s, code_family %s" % (code, fam, code_family(code))
        assert base[fam] + arg == code, "code %d: (%s, %r) does not recombine" % (code, fam, arg)
        assert fam != "w4" or arg in ops.W4_CODES
    # 107 / 108, the ping-pong tiles, exist on split operands only: the fp32 LDS-DMA kernel answers EUNSUP, PackedConvX._time_tiles
    # skips what it cannot launch, and so no timed selection records 2107 / 2108.  They are no code of the LDS-DMA family (2000 ... 2099):
    # neither restatement calls them one, and a tuned layer ignores them (its own tiles end below 2000)
    for code in (2000 + t for t in ops.XTUNE_CANDIDATES if t >= 100):
        assert ops._decode(code)[0] != "dma" and code_family(code) is None, code


def test_image_chunks_by_plain_arithmetic():
    """the 4 GiB rule of the 32-bit buffer resources: batches below it are one chunk, others go in runs of whole images"""
    chunks = lambda N, per_img: list(ops._image_chunks(N, per_img))
    assert chunks(5, 2 ** 30) == [(0, 3), (3, 5)]
    assert chunks(5, 2 ** 31) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert chunks(1, 2 ** 40) == [(0, 1)], "a single image is never split"
    assert chunks(7, 100) == [(0, 7)] and chunks(3, (2 ** 32 - 2) // 3) == [(0, 3)], "N * per_img < 2^32 - 1: one chunk"
    assert chunks(3, (2 ** 32 - 2) // 3 + 1) == [(0, 2), (2, 3)], "the first size past the limit"


# --------------------------------------------------------------------------------------------------------- shapes and references
def _shape(KH, stride, pad, linear, w4):
    """(N, H, W) of the test call.  No tabled kernel rejects these shapes today; one that does gets the smallest shape it accepts
    here, with the reason."""
    if linear:
        return (2 * 1051, 1, 1)                      # rows: 2102 = 16 x 128 + 54
    if KH == 1:
        return (2, 31, 37)
    if (KH, stride, pad) == (3, 1, 1):
        return (2, 34, 36 if w4 else 38)             # even (Winograd); W % 4 == 0 where the static kernel is F(2x4)
    Ho, Wo = (31, 34) if stride == 3 else (33, 35) if stride == 1 else (34, 38)
    return (2, (Ho - 1) * stride + KH - 2 * pad, (Wo - 1) * stride + KH - 2 * pad)


def _act_ref(x, act, slope):
    return {ops.ACT_NONE: lambda: x, ops.ACT_RELU: lambda: F.relu(x), ops.ACT_LRELU: lambda: F.leaky_relu(x, slope),
            ops.ACT_TANH: lambda: torch.tanh(x)}[act]()


class _Data:
    pass


_DATA = {}


def _data(dt16, Cout, cpg, KH, KW, stride, pad, groups, has_res, act, shape):
    """operands and the fp64 reference of one layer call, computed once per (geometry, element type) and shared by its tiles.
    dt16: the 16-bit type operands and weights are rounded to first (the reference takes the same rounded values), or None."""
    sig = (str(dt16), Cout, tuple(cpg), KH, KW, stride, pad, groups, bool(has_res), act, shape)
    if sig in _DATA:
        return _DATA[sig]
    N, H, W = shape
    linear = (H, W, KH, len(cpg)) == (1, 1, 1, 1)
    g = _gen(name_seed(repr(sig), 97))
    rnd = (lambda t: t) if dt16 is None else (lambda t: t.to(dt16).float())
    d = _Data()
    d.K = sum(cpg) * KH * KW
    d.w = rnd(torch.randn(Cout, sum(cpg), KH, KW, generator=g) / math.sqrt(d.K))
    d.b = torch.randn(Cout, generator=g) * 0.1
    d.lead = 0 if linear else (4 if dt16 is None else 8)        # the sources sit at this channel offset inside wider tensors
    d.srcs, parts = [], []
    for si, c in enumerate(cpg):
        t = torch.randn(N, H, W, c * groups + 2 * d.lead, generator=g)
        if si == 0 and dt16 is not None:                        # subnormals of the 16-bit type (and values that round into them)
            t[..., d.lead:d.lead + 4] *= 2.0 ** -16 if dt16 is F16 else 2.0 ** -130
        t = rnd(t)
        d.srcs.append(t)
        parts.append(t[..., d.lead:d.lead + c * groups])
    # virtual concat: group gi takes channels [gi*c, (gi+1)*c) of every source, in source order
    x = torch.cat([torch.cat([p_[..., gi * c:(gi + 1) * c] for p_, c in zip(parts, cpg)], -1) for gi in range(groups)], -1)
    ref = F.conv2d(nchw(x).double(), d.w.double(), d.b.double(), stride=stride, padding=pad, groups=groups)
    Ho, Wo = ref.shape[2:]
    d.res, d.res_coff, d.slope = None, 0, 0.1
    if act == ops.ACT_DCNPOST:
        # conv_offset's last layer (feat_prop.py:38-53): the residual is the [pixel][4] flows, the slope the offset range
        d.res, d.slope = torch.randn(N, Ho, Wo, 4, generator=g) * 2, 10.0
        f1, f2 = nchw(d.res[..., 0:2]).double(), nchw(d.res[..., 2:4]).double()
        o1, o2, m = torch.chunk(ref, 3, 1)
        q1, q2 = torch.chunk(10 * torch.tanh(torch.cat([o1, o2], 1)), 2, 1)
        rep = q1.shape[1] // 2
        ref = torch.cat([q1 + f1.flip(1).repeat(1, rep, 1, 1), q2 + f2.flip(1).repeat(1, rep, 1, 1), torch.sigmoid(m)], 1)
    else:
        if has_res:
            d.res_coff = 0 if linear else 4
            d.res = torch.randn(N, Ho, Wo, Cout + 2 * d.res_coff, generator=g)
            ref = ref + nchw(d.res[..., d.res_coff:d.res_coff + Cout]).double()
        ref = _act_ref(ref, act, d.slope)
    d.ref = nhwc(ref)
    d.Ho, d.Wo = Ho, Wo
    _DATA[sig] = d
    return d


def _untouched(wide, coff, Cout, what):
    rest = torch.cat([wide[..., :coff], wide[..., coff + Cout:]], -1)
    assert bool((rest == 7.0).all()), what + ": wrote outside its channel slice"


# --------------------------------------------------------------------------------------------------------- fp32 keys (PackedConv)
def _check_fp32_key(dev, geom, code):
    Cout, cpg, KH, KW, stride, pad, groups, bk, has_res, act, use_wino, tune, static = geom[:13]
    x3 = geom[13:] == ("x3",)
    what = pair_id((geom, code))
    linear = (KH, KW, len(cpg), groups) == (1, 1, 1, 1)
    w4 = static in ops.W4_CODES
    shape = _shape(KH, stride, pad, linear, w4)
    d = _data(None, Cout, cpg, KH, KW, stride, pad, groups, has_res, act, shape)
    N, Ho, Wo = shape[0], d.Ho, d.Wo
    # the layer as Engine.__init__ builds it: PackedLinear for the token Linears, PackedConv(algo="auto") otherwise
    if linear:
        layer = ops.PackedLinear(d.w.view(Cout, -1).to(dev), d.b.to(dev), bk=bk)
    else:
        layer = ops.PackedConv(d.w.to(dev), d.b.to(dev), cpg, groups=groups, stride=stride, pad=pad, bk=bk, algo="auto")
    layer.tune, layer.try_x3 = bool(tune), x3
    assert layer.bk == bk and (layer.algo == "auto") == bool(use_wino), what
    srcs = [(s.to(dev), d.lead) for s in d.srcs]
    res = None if d.res is None else d.res.to(dev)
    qkv = Cout == 1536 and code_family(code) == "x3"            # the engine's qkv call: the epilogue writes the K / V planes
    coff = 4

    def call():
        if linear:
            out = torch.full((N, Cout), float("nan"), device=dev)
            planes = torch.zeros(3, N, Cout - 512, dtype=BF16, device=dev) if qkv else None
            layer(srcs[0][0].view(N, -1), out=out, residual=None if res is None else res.view(N, -1), act=act, slope=d.slope,
                  kv_planes=planes)
            return out, planes
        out = torch.full((N, Ho, Wo, Cout + 12), 7.0, device=dev)
        layer(srcs, out=out, out_coff=coff, residual=res, res_coff=d.res_coff, act=act, slope=d.slope)
        return out, None

    key = geom[:SF] + (int(4.0 * math.log2(N * Ho * Wo)),) + geom[SF:]
    with tabled({key: code}, w4_minpix=0 if w4 else None) as asked:
        first, _ = call()                                        # eager: builds the weight packings of what runs
        with launch_trace() as trace:
            out, planes = call()
        torch.cuda.synchronize()
    assert asked == [(key, code)] * 2, "%s: the layer looked up %r" % (what, asked)
    fam = code_family(code)
    own = "e2fgvi_conv3x3_winograd4" if (use_wino and w4) else "e2fgvi_conv3x3_winograd" if use_wino else "e2fgvi_conv2d_nhwc"
    symbol, tile, kernel = {"w3": ("e2fgvi_conv3x3_winograd_x3", code, None),
                            "x3": ("e2fgvi_conv2d_x", code - ops.X3_BASE, "conv_f32x3"),
                            "dma": ("e2fgvi_conv2d_x", code - 2000, "conv_f32x"),
                            "own": (own, code or static, None)}[fam]
    assert_one_conv_launch(trace, symbol, tile=tile, kernel=kernel, what=what)
    assert torch.equal(first, out) or qkv, what + ": the second launch differs from the first"
    wino = fam == "w3" or (fam == "own" and use_wino)
    tol = 3e-5 if act == ops.ACT_DCNPOST else fp32_tol(d.K, floor=3e-5) if wino else fp32_tol(d.K)
    if not linear:
        _untouched(out, coff, Cout, what)
        assert_close(out[..., coff:coff + Cout].cpu(), d.ref, tol, what)
        return
    ref = d.ref.view(N, Cout)
    if not qkv:
        assert_close(out.cpu(), ref, tol, what)
        return
    # the plane-writing epilogue: Q in the fp32 rows, K / V as three bf16 planes that sum to the fp32 value -- bit for bit what
    # e2fgvi_split3_kv makes of the fp32 rows of the same kernel and tile -- and nothing in the fp32 K / V columns
    assert not [r for r in trace if r["symbol"] == "e2fgvi_split3_kv"], what + ": the planes came from split3_kv, not the epilogue"
    assert bool(torch.isnan(out[:, 512:]).all()), what + ": the fp32 K / V columns must not be stored"
    assert_close(out[:, :512].cpu(), ref[:, :512], tol, what + " Q columns")
    assert_close(planes.double().sum(0).cpu(), ref[:, 512:], tol, what + " K / V planes")
    full = torch.empty(N, 1, 1, Cout, device=dev)
    layer.alt3([(srcs[0][0].view(N, 1, 1, -1), 0)], out=full, tile=code - ops.X3_BASE)
    assert torch.equal(planes, ops.split3_kv(full.view(N, Cout))), what + ": planes differ from split3_kv of the fp32 rows"
    assert torch.equal(planes.double().sum(0), full.view(N, Cout)[:, 512:].double()) and torch.equal(out[:, :512], full.view(N, Cout)[:, :512])


# --------------------------------------------------------------------------------------------------------- X keys (PackedConvX)
def _check_x_key(dev, geom, code):
    fam, Cout, cpg, KH, KW, stride, pad, groups, odt, out_nchw, taps = geom
    linear = (KH, KW, len(cpg), groups) == (1, 1, 1, 1)
    shape = _shape(KH, stride, pad, linear, False)
    # the epilogue (an X key names none): conv_offset.6 keeps its offset / mask post-processing; the other fp32 results take an
    # fp32 residual as the token Linears and SPyNet's last layer do, the 16-bit ones a leaky ReLU as the conv stacks do
    act = ops.ACT_DCNPOST if (Cout == 432 and odt == 0) else ops.ACT_NONE if odt == 0 else ops.ACT_LRELU
    has_res = odt == 0
    for dt in ((BF16, F16) if fam == "x" else (None,)):
        what = pair_id((geom, code)) + ("" if dt is None else " fp16" if dt is F16 else " bf16")
        d = _data(dt, Cout, cpg, KH, KW, stride, pad, groups, has_res, act, shape)
        N, Ho, Wo = shape[0], d.Ho, d.Wo
        kw = dict(dtype=dt or torch.float32)
        if dt is None:
            kw.update(taps=True if taps else None, x3=fam == "x3")
        if linear:
            layer = ops.PackedLinearX(d.w.view(Cout, -1).to(dev), d.b.to(dev), dtype=kw["dtype"])
        else:
            layer = ops.PackedConvX(d.w.to(dev), d.b.to(dev), cpg, groups=groups, stride=stride, pad=pad, **kw)
        layer.tune, layer.try_x3 = True, fam == "x32+3"
        assert layer.taps == bool(taps), what
        cast = (lambda t: t.to(dev)) if dt is None else (lambda t: t.to(dev).to(dt))
        srcs = [(cast(s), d.lead) for s in d.srcs]
        res = None if d.res is None else d.res.to(dev)
        coff = 8

        def call(odtype, second):
            """one call with an `odtype` result (and a 16-bit second copy, out2, beside an fp32 one): (result, its slice, out2)"""
            o2 = None
            if linear:
                out = torch.full((N, Cout), 7.0, dtype=odtype, device=dev)
                if second:
                    o2 = torch.zeros(N, Cout, dtype=dt, device=dev)
                layer(srcs[0][0].view(N, -1), out=out, residual=None if res is None else res.view(N, -1), act=act, slope=d.slope, out2=o2)
                return out, out, o2
            if out_nchw:
                out = torch.full((N, Cout, Ho, Wo), 7.0, device=dev)
                layer(srcs, out=out, residual=res, res_coff=d.res_coff, act=act, slope=d.slope, out_nchw=True)
                return out, out.permute(0, 2, 3, 1), None
            out = torch.full((N, Ho, Wo, Cout + 24), 7.0, dtype=odtype, device=dev)
            if second:
                o2 = torch.zeros(N, Ho, Wo, Cout, dtype=dt, device=dev)
            layer(srcs, out=out, out_coff=coff, residual=res, res_coff=d.res_coff, act=act, slope=d.slope, out2=o2)
            return out, out[..., coff:coff + Cout], o2

        sc = int(4.0 * math.log2(N * Ho * Wo))
        key = geom[:SF] + (sc,) + geom[SF:]
        # a 16-bit row is also run with an fp32 result, on the same tile (the key of that call names the fp32 result type): the
        # 16-bit result must be the rounding of those fp32 values
        key32 = key[:SF + 1] + (0,) + key[SF + 2:]
        runs = [(torch.float32 if odt == 0 else dt, key)] + ([(torch.float32, key32)] if odt != 0 else [])
        got = []
        with tabled({key: code, key32: code}) as asked:
            for odtype, k in runs:
                second = dt is not None and odtype == torch.float32 and not out_nchw and act != ops.ACT_DCNPOST      # (as the engine calls it)
                first = call(odtype, second)[0]                  # eager: builds the weight packing of what runs
                with launch_trace() as trace:
                    out, sl, o2 = call(odtype, second)
                torch.cuda.synchronize()
                if code >= ops.X3_BASE:
                    tile, kernel = code - ops.X3_BASE, "conv_f32x3"
                else:
                    tile, kernel = code, {None: "conv_f32x3" if fam == "x3" else "conv_f32x", BF16: "conv_bf16x", F16: "conv_f16x"}[dt]
                assert_one_conv_launch(trace, "e2fgvi_conv2d_x", tile=tile, kernel=kernel, what=what)
                assert torch.equal(first, out), what + ": the second launch differs from the first"
                if not linear and not out_nchw:
                    _untouched(out, coff, Cout, what)
                got.append((sl, o2))
        assert asked == [(k, code) for _, k in runs for _ in (0, 1)], "%s: the layer looked up %r" % (what, asked)
        out32, o2 = got[-1]
        ref = d.ref.view(out32.shape)
        tol = fp32_tol(d.K) if dt is None else fp32_tol(d.K, floor=3e-5)
        if act == ops.ACT_DCNPOST:
            tol = 3e-5
        assert_close(out32.cpu(), ref, tol, what + " fp32 result")
        for r16, name in ([] if dt is None else [(o2, "out2")] + ([(got[0][0], "16-bit result")] if odt != 0 else [])):
            if r16 is None:
                continue
            if dt is F16:
                assert_is_half_of(r16.contiguous(), out32.contiguous(), "%s: %s" % (what, name))
            else:
                assert torch.equal(r16.cpu(), out32.cpu().bfloat16()), "%s: %s is not the bf16 rounding of the fp32 result" % (what, name)


def check_pair(dev, geom, code):
    (_check_x_key if isinstance(geom[0], str) else _check_fp32_key)(dev, geom, code)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_tabled_kernel_runs_and_is_right(dev, pair):
    check_pair(dev, *pair)
