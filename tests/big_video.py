"""Videos of more than 2^32 bytes for tests/test_gpu_video_scale.py (test infrastructure, no tests in here): a small base clip of
k frames repeated along L on the device, every tile a scene of its own, and the comparison of a device result with the numpy
restatement's result for ONE tile, byte for byte over the whole buffer, in chunks on the device.  Nothing large goes to the host.

A kernel that forms a byte offset in 32 bits reads (or writes) `offset mod 2^32`.  With a tile whose size does not divide 2^32 that
address lies at another phase of the tile grid, so the wrong bytes differ from the right ones: wrap_is_visible() asserts it of the
buffer itself, and wrapped_tile() gives the host the bytes such a kernel would fetch, for a restatement run that must then differ
from the expected one."""
import contextlib
import time

import numpy as np
import torch

WRAP = 1 << 32                    # the byte offset the buffers must pass
CHUNK = 1 << 30                   # bytes compared at a time
PEAK_MAX = 64 << 30               # no test may hold more


def tiles_past(tile_bytes, total=None):
    """the tiles of `tile_bytes` a buffer needs to pass `total` bytes (WRAP) with two whole tiles behind it, one frame dropped or not"""
    return (WRAP if total is None else total) // int(tile_bytes) + 4


def nbytes(base):
    return int(np.asarray(base).nbytes)


def tiled(base, n, dev, drop=0):
    """base [k, ...] on the host -> [n k - drop, ...] on the device: Tensor.repeat along the first axis, the last `drop` entries
    left off (flows: L - 1 of them)"""
    t = torch.from_numpy(np.array(base)).to(dev)                  # a writable copy: the cases are read-only
    out = t.repeat((n,) + (1,) * (t.dim() - 1))
    return out[:out.shape[0] - drop] if drop else out


def tiled_planes(base, n, dev):
    """base [2, k, ...] on the host -> [2, n k, ...] on the device: the two planes of a tracker, each repeated along its frames"""
    t = torch.from_numpy(np.array(base)).to(dev)
    return t.repeat((1, n) + (1,) * (t.dim() - 2))


def scene_of(L, k, dev):
    """int32 [L]: every tile of k frames a scene of its own"""
    return (torch.arange(L, device=dev) // k).to(torch.int32)


def padded_flows(flows, seed):
    """flows [k-1, H, W, 2] of a tile -> [k, H, W, 2]: the flow of the pair between two tiles behind them (finite, unlike any of the
    tile's own), so that the tiled flows are periodic with the frames"""
    flows = np.asarray(flows)
    rng = np.random.RandomState(seed)
    pad = (3.0 * (2 * rng.random_sample(flows.shape[1:]) - 1)).astype(flows.dtype)
    return np.ascontiguousarray(np.concatenate([flows, pad[None]]))


def tile_mismatch(got, want_tile, chunk=None):
    """None when got [m, ...] on the device is want_tile [k, ...] (host) repeated (the last tile may be cut short), else a string
    that names the first tile that differs.  Compared on the device, at most `chunk` bytes at a time."""
    want = torch.from_numpy(np.array(want_tile)).to(got.device)
    if got.dtype != want.dtype or tuple(got.shape[1:]) != tuple(want.shape[1:]):
        return "dtype / shape %s %s against %s %s" % (got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    if not got.is_contiguous():
        return "not contiguous"
    k, m = want.shape[0], got.shape[0]
    per = max(1, (CHUNK if chunk is None else chunk) // max(1, want.numel() * want.element_size()))
    whole = m // k
    for a in range(0, whole, per):
        b = min(a + per, whole)
        g = got[a * k:b * k].view((b - a,) + tuple(want.shape))
        w = want.unsqueeze(0).expand_as(g)
        if not torch.equal(g, w):
            bad = int((g != w).flatten(1).any(1).nonzero()[0])
            return "tile %d of %d differs in %d entries" % (a + bad, whole, int((g[bad] != want).sum()))
    rest = m - whole * k
    if rest and not torch.equal(got[whole * k:], want[:rest]):
        return "the %d entries behind the last whole tile differ" % rest
    return None


def assert_tiled(got, want_tile, what):
    bad = tile_mismatch(got, want_tile)
    assert bad is None, "%s: %s" % (what, bad)


def as_bytes(t):
    """a contiguous device tensor as its bytes"""
    assert t.is_contiguous()
    return t.view(-1).view(torch.uint8)


def wrap_is_visible(t, tile_bytes, what):
    """t passes 2^32 bytes, its tile does not divide 2^32, and the bytes of the first tile's worth from offset 2^32 on differ from
    those a 32-bit offset would fetch in their place -- the same for offset 2^31, where a signed offset turns negative"""
    flat = as_bytes(t)
    n = int(tile_bytes)
    assert flat.numel() >= WRAP + 2 * n, (what, flat.numel())
    assert WRAP % n != 0, (what, n)
    assert not torch.equal(flat[WRAP:WRAP + n], flat[:n]), what
    half = WRAP // 2
    assert not torch.equal(flat[half:half + n], flat[:n]), what


def wrapped_tile(base, tile_index=None, wrap=None):
    """the bytes of tile `tile_index` (default: the first that lies wholly past 2^32) of the tiled `base`, as a kernel that forms its
    byte offsets in 32 bits would fetch them: byte g of the buffer comes from g mod 2^32.  The buffer is periodic, so byte g holds
    base's byte g mod its size.  Host arrays only."""
    base = np.ascontiguousarray(base)
    wrap = WRAP if wrap is None else wrap
    flat = base.reshape(-1).view(np.uint8)
    n = flat.size
    i = wrap // n + 1 if tile_index is None else tile_index
    g = i * n + np.arange(n, dtype=np.int64)
    return flat[(g % wrap) % n].view(base.dtype).reshape(base.shape)


def tile_windows(n_tiles, tile_bytes, others=()):
    """the tiles to look at when an output depends on the frame number: the first, those that hold byte offsets 2^31 and 2^32 of
    a buffer with `tile_bytes` a tile (and of those of `others`), and the last; sorted, each once"""
    at = {0, n_tiles - 1}
    for nb in (tile_bytes,) + tuple(others):
        for off in (WRAP // 2, WRAP):
            if off // nb < n_tiles:
                at.add(int(off // nb))
    return sorted(at)


@contextlib.contextmanager
def measured(name, dev):
    """prints the wall time and the peak of device memory of the block, and holds the peak under 64 GiB; frees the cache behind it"""
    cuda = torch.device(dev).type == "cuda"
    if cuda:
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    try:
        yield
        if cuda:
            torch.cuda.synchronize(dev)
    finally:
        dt = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated(dev) if cuda else 0
        print("%s: %.2f s, peak %.2f GiB" % (name, dt, peak / float(1 << 30)))
        if cuda:
            torch.cuda.empty_cache()
    assert peak < PEAK_MAX, (name, peak)
