"""Operands as slices of larger, poisoned allocations: the contract of include/e2fgvi_hip.h ("a kernel's result depends on no byte
outside the declared slices of its operands and it changes no byte outside the declared slice of its destinations") made testable.

    view, arena = embed(t, ld=..., coff=...)        # t in channels [coff, coff + C) of pixels of ld channels, guards around
    ... run the kernel on `view` ...
    check_slices(view, arena, coff, C, tight=..., sources=[(arena_s, snapshot(arena_s)), ...])

Sources, residuals and tables are surrounded by quiet NaN (0 * NaN = NaN: a load of a neighbour's channel against a zero weight
shows); destinations are prefilled with a NaN of a distinctive payload, written and compared as integer bits, so a store of a NaN, a
zero or a stale value outside the slice shows as well.  No float comparison decides anything here.  Plain helper module: tests/
test_embedding_host.py runs it on the CPU, tests/test_gpu_slices.py on the kernels."""
import math

import torch

NAN = "nan"                 # poison of sources: quiet NaN
SENTINEL = "sentinel"       # poison of destinations: the bits below
SENTINEL_BITS = {torch.float32: 0x7fc0dead, torch.bfloat16: 0x7fc1, torch.float16: 0x7e01}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.int32: torch.int32}
_ALIGN = 128                # elements: guards are multiples of 256 bytes, so the view is aligned like a fresh allocation
GEMM_TILE_ROWS = 256
CHECKED = [0]               # calls of check_slices that passed (tests/test_gpu_slices.py reports the count)


def bits(t):
    """the tensor's elements as integers of the same width"""
    return t.contiguous().view(_INT[t.dtype])


def _fill(arena, poison):
    if poison == NAN:
        arena.fill_(float("nan"))
    elif poison == SENTINEL:
        bits(arena).fill_(SENTINEL_BITS[arena.dtype])
    else:                   # an integer table's replacement value
        arena.fill_(poison)


def default_guard(shape):
    """one image row plus two pixels of a 4-D layout ([N,H,W,ld]: (W + 2) * ld; [N,C,H,W]: (H + 2) * W), one 256-row tile of a 2-D
    operand, 4096 elements otherwise"""
    if len(shape) == 4:
        return (shape[2] + 2) * shape[3]
    if len(shape) == 2:
        return GEMM_TILE_ROWS * shape[1]
    return 4096


def embed(t, ld=None, coff=0, guard=None, poison=NAN, device=None):
    """(view, arena): `arena` is one flat allocation of t's dtype filled with the poison; `view` a contiguous tensor of shape
    [..., ld] (t.shape when ld is None) inside it, `guard` elements (rounded up to 256 bytes) of poison in front and behind, with
    t in channels [coff, coff + C)."""
    device = t.device if device is None else device
    C = t.shape[-1]
    shape = tuple(t.shape) if ld is None else tuple(t.shape[:-1]) + (ld,)
    if coff < 0 or coff + C > shape[-1]:
        raise ValueError("channels [%d, %d) do not fit pixels of %d" % (coff, coff + C, shape[-1]))
    n = math.prod(shape)
    g = default_guard(shape) if guard is None else guard
    g = -(-max(g, 1) // _ALIGN) * _ALIGN
    arena = torch.empty(g + n + g, dtype=t.dtype, device=device)
    _fill(arena, poison)
    view = arena[g:g + n].view(shape)
    view[..., coff:coff + C] = t.to(device)
    return view, arena


def embed_like(shape, dtype, device, ld=None, coff=0, guard=None):
    """a destination: (view, arena) for a result of `shape` ([..., C]) with every element, the slice included, at the sentinel"""
    full = tuple(shape) if ld is None else tuple(shape[:-1]) + (ld,)
    n = math.prod(full)
    g = default_guard(full) if guard is None else guard
    g = -(-max(g, 1) // _ALIGN) * _ALIGN
    arena = torch.empty(g + n + g, dtype=dtype, device=device)
    _fill(arena, SENTINEL)
    return arena[g:g + n].view(full), arena


def snapshot(arena):
    return bits(arena).clone()


def _where(i, g, n, ld, coff, C):
    if i < g:
        return "guard-before[%d] (%d elements in front of the view)" % (i, g - i)
    if i >= g + n:
        return "guard-after[%d] (%d elements behind the view)" % (i - g - n, i - g - n + 1)
    p, c = divmod(i - g, ld)
    return "pixel %d, channel %d (the slice is channels [%d, %d) of %d)" % (p, c, coff, coff + C, ld)


def _offset(arena, view):
    return (view.data_ptr() - arena.data_ptr()) // arena.element_size()


def assert_untouched(arena, view, coff, C, what=""):
    """every element of the arena outside channels [coff, coff + C) of the view still holds the sentinel's bits"""
    g, n, ld = _offset(arena, view), view.numel(), view.shape[-1]
    bad = bits(arena).cpu() != SENTINEL_BITS[arena.dtype]
    bad[g:g + n].view(-1, ld)[:, coff:coff + C] = False
    if bad.any():
        idx = bad.nonzero().view(-1)
        first, last = int(idx[0]), int(idx[-1])
        raise AssertionError("%s: %d elements outside the destination's slice were written; first at flat index %d = %s, last at %d = %s"
                             % (what, idx.numel(), first, _where(first, g, n, ld, coff, C), last, _where(last, g, n, ld, coff, C)))


def assert_sources_intact(arena, snap, what=""):
    """a source arena is bit-equal to its snapshot"""
    now = bits(arena)
    if not torch.equal(now, snap):
        idx = (now != snap).nonzero().view(-1)
        raise AssertionError("%s: %d elements of a source arena changed (first at flat index %d, last at %d)"
                             % (what, idx.numel(), int(idx[0]), int(idx[-1])))


def check_slices(view, arena, coff, C, tight=None, sources=(), what=""):
    """what every embedded call must satisfy, in this order: nothing outside the destination's slice written (assert_untouched),
    every source arena intact, the slice finite (a NaN there is poison that reached the result: a read outside a source's slice),
    and -- given the tight call's result -- the slice bit-identical to it.  Returns the slice."""
    assert_untouched(arena, view, coff, C, what)
    for a, snap in sources:
        assert_sources_intact(a, snap, what)
    got = view[..., coff:coff + C]
    finite = torch.isfinite(got.float())
    if not finite.all():
        idx = (~finite).reshape(-1, C).nonzero()
        raise AssertionError("%s: %d non-finite values inside the result slice (first at pixel %d, channel %d of the slice): poison from "
                             "outside a source's slice reached the result" % (what, idx.shape[0], int(idx[0, 0]), int(idx[0, 1])))
    if tight is not None:
        assert tuple(tight.shape) == tuple(got.shape), (what, tuple(tight.shape), tuple(got.shape))
        same = bits(got) == bits(tight)
        if not same.all():
            idx = (~same).reshape(-1, C).nonzero()
            raise AssertionError("%s: %d elements of the embedded call's slice differ in their bits from the tight call's result (first at "
                                 "pixel %d, channel %d)" % (what, idx.shape[0], int(idx[0, 0]), int(idx[0, 1])))
    CHECKED[0] += 1
    return got
