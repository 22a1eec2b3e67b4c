"""qkv rows that drive the fused attention kernels off unit scale, and their float64 reference.

Every other attention test draws its rows from unit-scale Gaussians: the logits stay within about +-20, the mass of the
zero-padded pooled slots (score exactly -100, V = 0) is ~1e-50 of the denominator, the running maximum settles in the first
tiles and both key groups hold similar mass.  The regimes below are built so that the terms those tests cannot see carry the
result (tests/test_attention_regimes.py checks, on the CPU, that they do; tests/test_gpu_attention_regimes.py runs every kernel
family on them).

Rows are laid out as the kernels read them: token rows [B*T*fh*fw, 1536] in (b, t, y, x) order, pooled rows
[B*T*nWh*nWw, 1536] in (b, t, wy, wx) order, each [q | k | v] with head h in columns h*128 .. h*128+127 of its third.
With u = ones(128), 128^-0.5 * u.u = sqrt(128), so k = (c / sqrt(128)) u shifts the logits of q = u by exactly c.
N is a fresh standard normal, drawn in the order q, k, v, token rows before pooled rows; v is always N.

    control    q = 2 N           k = 2 N                          logits N(0, 4^2): the other tests' regime
    pad_mass   q = u             k = -(100 / sqrt(128)) u + N     logits -100 + N(0, 1): level with the pads
    shifted    q = u             k = -(250 / sqrt(128)) u + 4 N   logits -250 + N(0, 4^2): the pads take all the mass, except in
                                                                  the interior window, which has none
    peaked     q = sqrt(40) N    k = sqrt(40) N                   logits N(0, 40^2): a one-hot softmax
    late_max   q = u + 0.05 N    k = (c / sqrt(128)) u + 0.5 N    c = 30 f - 40 for the token rows of frame f, 30 f + 20 for its
                                                                  pooled rows: the maximum rises to the last keys of the list
    uniform    q = N             k = 0                            all logits 0: the mean of V over the key list, duplicates incl.

The grid is B = 1, T = 2, 25 x 81 tokens = 5 x 9 windows: the smallest with an interior window (row 2, column 4: all 210 key
slots valid, no pads); every other window has 180 ... 209 keys per frame and the rest as pads."""
import math

import torch

from tests.util import gen, name_seed

REGIMES = ("control", "pad_mass", "shifted", "peaked", "late_max", "uniform")
B, T, FH, FW = 1, 2, 25, 81
NWH, NWW = FH // 5, FW // 9
INTERIOR = 2 * NWW + 4                  # the window with 210 valid key slots


def build_rows(name):
    """(token rows, pooled rows) of regime `name`, fp32"""
    g = gen(name_seed("attention regime " + name))
    u, r = torch.ones(128), math.sqrt(128.0)
    out = []
    for per_frame, pooled in ((FH * FW, False), (NWH * NWW, True)):
        n = B * T * per_frame
        frame = ((torch.arange(n) // per_frame) % T).float().view(n, 1, 1)

        def N():
            return torch.randn(n, 4, 128, generator=g)
        if name == "control":
            q, k = 2 * N(), 2 * N()
        elif name == "pad_mass":
            q, k = u.expand(n, 4, 128), -(100 / r) * u + N()
        elif name == "shifted":
            q, k = u.expand(n, 4, 128), -(250 / r) * u + 4 * N()
        elif name == "peaked":
            q, k = math.sqrt(40.0) * N(), math.sqrt(40.0) * N()
        elif name == "late_max":
            q = u + 0.05 * N()
            k = ((30 * frame + (20 if pooled else -40)) / r) * u + 0.5 * N()
        elif name == "uniform":
            q, k = N(), torch.zeros(n, 4, 128)
        else:
            raise KeyError(name)
        v = N()
        out.append(torch.cat([t.reshape(n, 512) for t in (q, k, v)], 1).float().contiguous())
    return tuple(out)


def key_table():
    """(tab, nkeys) of the grid, as the engine builds them"""
    from e2fgvi_amd.engine import build_key_table
    from oracle.e2fgvi_oracle import rolled_valid_index
    return build_key_table(FH, FW, rolled_valid_index().tolist())


def window_rows(win, frame=None):
    """indices of the token rows (= output rows) of window `win`, all frames or one"""
    wy, wx = divmod(win, NWW)
    ys, xs = torch.meshgrid(torch.arange(wy * 5, wy * 5 + 5), torch.arange(wx * 9, wx * 9 + 9), indexing="ij")
    idx = (ys * FW + xs).reshape(-1)
    frames = range(T) if frame is None else (frame,)
    return torch.cat([f * FH * FW + idx for f in frames])


def reference(tok, pool, dtype=torch.float64, oracle=None):
    """the oracle's roll / partition / cat / softmax chain on the given rows, evaluated in `dtype`: [B*T*fh*fw, 512] in token
    order.  `oracle`: another module object with the oracle's functions (the CPU tests pass an edited copy)."""
    if oracle is None:
        from oracle import e2fgvi_oracle as oracle
    x = torch.zeros(B, T, FH, FW, 512, dtype=dtype)                # shapes and dtype only
    xp = torch.zeros(B, NWH, NWW, T, 512, dtype=dtype)
    pre = oracle.window_attention({}, "a.", x, xp, preproj=True, qkv_rows=tok.to(dtype).view(B, T, FH, FW, 1536),
                                  qkv_pool_rows=pool.to(dtype).view(B, T, NWH, NWW, 1536))
    return oracle.window_reverse(pre, B, T, FH, FW).reshape(-1, 512)


def interior_logits(tok, pool):
    """float64 logits 128^-0.5 q.k of the interior window's queries against that window's whole key list, from the rows and
    the key table alone: ([T*45 queries, 4 heads, T*210 keys], is_pooled_of_last_frame [T*210])"""
    tab, nk = key_table()
    assert nk[INTERIOR] == 210
    refs = torch.from_numpy(tab[INTERIOR, :210]).long()
    keys, last_pool = [], []
    for f in range(T):
        trow = f * FH * FW + refs.clamp(min=0)
        prow = f * NWH * NWW + (-(refs + 1)).clamp(min=0)
        k = torch.where((refs >= 0).view(-1, 1), tok[trow, 512:1024].double(), pool[prow, 512:1024].double())
        keys.append(k)
        last_pool.append((refs < 0) & (f == T - 1))
    k = torch.cat(keys).view(-1, 4, 128)
    q = tok[window_rows(INTERIOR), :512].double().view(-1, 4, 128)
    return torch.einsum("qhd,khd->qhk", q, k) * 128 ** -0.5, torch.cat(last_pool)


_CACHE = {}


def case(name, rounding=None):
    """regime `name` with its rows rounded to `rounding` (None: fp32 as built; torch.bfloat16 / torch.float16), computed once
    per process and shared by the kernel families: dict(tok, pool: the rows in their storage type; ref: the float64 oracle on
    those rows; e32: max |oracle in float32 - ref| / rms(ref), the noise of a plain fp32 evaluation of the same operator).
    Nothing in it may be written to."""
    key = (name, rounding)
    if key not in _CACHE:
        tok, pool = build_rows(name)
        if rounding is not None:
            tok, pool = tok.to(rounding), pool.to(rounding)
        ref = reference(tok.float(), pool.float())
        r32 = reference(tok.float(), pool.float(), torch.float32)
        e32 = (r32.double() - ref).abs().max().item() / max(ref.pow(2).mean().sqrt().item(), 1e-300)
        _CACHE[key] = dict(tok=tok, pool=pool, ref=ref, ref32=r32, e32=e32)
    return _CACHE[key]
