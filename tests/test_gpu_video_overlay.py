"""Static overlays on the device: the gradient sums and the dilated edge map (csrc/video.hip overlay_stats_kernel /
overlay_edges_kernel) against the numpy restatement of tests/overlay_cases.py, every integer equal, video.overlay_mask against the
restatement's mask on the tennis fixture, and inpaint_video(masks_u8="overlay") against the call with that mask, byte for byte."""
import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import overlay_cases as O
from tests.test_gpu_video_restore import _stand_in_model

pytestmark = pytest.mark.gpu

CH = ops.OVERLAY_CHUNK
# single pixels, rows and columns (narrower than the four-pixel load: the byte-wise instantiation), rows of four, five and six pixels
# (both edge items load the same or overlapping pixels); tiles with
# one column / one row more than a tile and one less than two; three chunks of 8, 8 and 9 frames; one frame below and above the
# shortest chunk, and the same around two of them, where one chunk (stores) becomes two (atomics); 1025 tiles, so no more than two
# chunks, of 8 and 9 frames
SHAPES = [(1, 1, 1), (2, 1, 7), (3, 5, 1), (3, 3, 4), (2, 2, 5), (2, 3, 6), (4, 35, 3), (5, 33, 65), (7, 31, 129), (25, 60, 108), (CH - 1, 33, 65),
          (CH + 1, 33, 65), (2 * CH - 1, 33, 65), (2 * CH, 33, 65), (2 * CH + 1, 32 * 1024 + 1, 1)]


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    buf = torch.zeros(a.size + shift, dtype=torch.uint8, device=dev)
    return buf[shift:].view(a.shape).copy_(torch.from_numpy(np.ascontiguousarray(a)))


@pytest.mark.parametrize("L,H,W", SHAPES, ids=str)
def test_overlay_stats_is_the_restatement(dev, L, H, W):
    """every content kind of overlay_cases.content; the base of the frames is moved off its alignment by hand (a frame of 5 x 1 or
    33 x 65 pixels is an odd number of bytes besides, so every other frame starts misaligned anyway)"""
    for i, kind in enumerate(O.CONTENTS):
        f = O.content(kind, L, H, W)
        want = torch.from_numpy(O.stats_np(f))
        for shift in (0, 1 + i % 3) if H * W <= 33 * 65 else (i % 4,):
            got = ops.overlay_stats(_up(f, dev, shift))
            assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (3, H, W)
            assert torch.equal(got.cpu(), want), (kind, shift, int((got.cpu() != want).sum()))


def test_overlay_stats_largest_sums(dev):
    """what the int32 planes must hold at the most: M = 510 per frame on the inverting checkerboard, |S| = 255 per frame on the step"""
    L, H, W = 2 * CH + 2, 40, 70
    got = ops.overlay_stats(_up(O.content("checker", L, H, W), dev))
    assert int(got[2].max()) == 510 * L and not got[:2].any()
    got = ops.overlay_stats(_up(O.content("step255", L, H, W), dev))
    assert int(got[1].abs().max()) == 255 * L == int(got[0].abs().max())


EDGE_MAPS = [(1, 1), (5, 7), (33, 65), (70, 130)]


@pytest.mark.parametrize("H,W", EDGE_MAPS, ids=str)
def test_overlay_edges_is_the_restatement(dev, H, W):
    """radius 0, 1, 3 and 16 on maps smaller than the radius and on maps that are no multiple of the tile; on the moving kinds the
    thresholds leave scattered edges (19 and 174 of 9100 pixels at 70 x 130, which radius 16 does not yet join into a full map
    for the first) or edges all over the map, frame borders included"""
    L = 6
    for kind, g_min, coh in (("random", 150, 200), ("random", 90, 100), ("toy", 120, 190), ("vstep", 32, 256), ("vstep", 120, 256),
                             ("vstep", 121, 256), ("step255", 255, 256), ("checker", 32, 1), ("zeros", 1, 1)):
        s = O.stats_np(O.content(kind, L, H, W))
        sd = torch.from_numpy(s).to(dev)
        for radius in (0, 1, 3, 16):
            want, n = O.dilated_np(s, L, g_min, coh, radius)
            D, count = ops.overlay_edges(sd, L, g_min, coh, radius)
            assert D.is_cuda and D.dtype == torch.uint8 and tuple(D.shape) == (H, W)
            assert count.is_cuda and count.dtype == torch.int32 and tuple(count.shape) == (1,)
            assert torch.equal(D.cpu(), torch.from_numpy(want)), (kind, radius)
            assert int(count.item()) == n == int(D.sum().item()), (kind, radius)
        if kind == "vstep" and W > 1:                   # coherence = 256 at equality, M = g_min L at equality; one more fails
            assert (n > 0) == (g_min <= 120)
        if kind == "random" and g_min == 150 and (H, W) == (70, 130):
            assert 0 < n < H * W


def test_overlay_edges_compares_in_64_bits(dev):
    """sums of 2^22 frames: 256 (|Sx| + |Sy|) and g_min L pass 2^31"""
    L = ops.OVERLAY_FRAMES_MAX
    m = 510 * L
    assert m < 2 ** 31 < 256 * 255 * L
    s = np.zeros((3, 2, 3), np.int32)
    s[2] = m
    s[0, 0] = (255 * L, -255 * L, 255 * L)              # with Sy below: coherent
    s[1, 0] = (255 * L, 255 * L, -255 * L)
    s[0, 1] = (255 * L, -255 * L + 1, 0)                # one short of M; exactly M / 2
    s[1, 1] = (255 * L - 1, 255 * L, -255 * L)
    sd = torch.from_numpy(s).to(dev)
    for g_min, coh in ((510, 256), (510, 255), (510, 128), (510, 129), (511, 1), (1, 256)):
        want, n = O.dilated_np(s, L, g_min, coh, 0)
        D, count = ops.overlay_edges(sd, L, g_min, coh, 0)
        assert torch.equal(D.cpu(), torch.from_numpy(want)) and int(count.item()) == n, (g_min, coh)
    assert O.dilated_np(s, L, 510, 256, 0)[1] == 3 and O.dilated_np(s, L, 510, 128, 0)[1] == 6 and O.dilated_np(s, L, 511, 1, 0)[1] == 0


def test_overlay_ops_check_their_arguments(dev):
    f = torch.zeros((3, 7, 5, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError):
        ops.overlay_stats(f.int())
    with pytest.raises(TypeError):
        ops.overlay_stats(f.cpu())
    for bad in (f[..., :2].contiguous(), f.permute(0, 2, 1, 3), f[:0], f[:, :0], f[0]):
        with pytest.raises(ValueError):
            ops.overlay_stats(bad)
    s = ops.overlay_stats(f)
    assert not s.any()
    with pytest.raises(TypeError):
        ops.overlay_edges(s.float(), 3, 32, 224, 3)
    with pytest.raises(TypeError):
        ops.overlay_edges(s.cpu(), 3, 32, 224, 3)
    for bad in (s[:2].contiguous(), s[0], s.permute(0, 2, 1)):
        with pytest.raises(ValueError):
            ops.overlay_edges(bad, 3, 32, 224, 3)
    for args in ((0, 32, 224, 3), (ops.OVERLAY_FRAMES_MAX + 1, 32, 224, 3), (3, 0, 224, 3), (3, 32, 0, 3), (3, 32, 257, 3),
                 (3, 32, 224, -1), (3, 32, 224, 17), (3, True, 224, 3), (3, 32, 224.0, 3), (3, 32, 224, False)):
        with pytest.raises(ValueError):
            ops.overlay_edges(s, *args)
    D, count = ops.overlay_edges(s, 3, 1, 1, 16)
    assert not D.any() and int(count.item()) == 0


def test_overlay_entries_refuse_bad_arguments(dev):
    """the C entries: E2FGVI_EINVAL from the arguments alone, in front of any launch (the addresses are never read)"""
    so = lib.load()
    base = 1 << 20
    good = dict(frames=base, L=3, H=7, W=5, stats=base + (1 << 16), g_min=32, coherence=224, radius=3, out=base + (1 << 17),
                count=base + (1 << 18))
    o_stats = ("frames", "L", "H", "W", "stats")
    o_edges = ("stats", "L", "H", "W", "g_min", "coherence", "radius", "out", "count")

    def st(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_overlay_stats(*[a[k] for k in o_stats], None)

    def ed(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_overlay_edges(*[a[k] for k in o_edges], None)

    for k in ("frames", "stats"):
        assert st(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
    for k in ("stats", "out", "count"):
        assert ed(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
    for rc in (st, ed):
        for L in (0, -2, (1 << 22) + 1):
            assert rc(L=L) == -1 and b"2^22" in so.e2fgvi_last_error()
        for v in (0, -1):
            assert rc(H=v) == -1 and rc(W=v) == -1
        assert rc(H=46341, W=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
        assert rc(H=0x7fffffff, W=0x7fffffff) == -1 and rc(H=65536, W=32768) == -1
        assert rc(stats=good["stats"] + 2) == -1 and b"aligned" in so.e2fgvi_last_error()
    assert ed(count=good["count"] + 1) == -1 and b"aligned" in so.e2fgvi_last_error()
    assert ed(g_min=0) == -1 and b"g_min" in so.e2fgvi_last_error()
    assert ed(coherence=0) == -1 and ed(coherence=257) == -1 and b"coherence" in so.e2fgvi_last_error()
    assert ed(radius=-1) == -1 and ed(radius=17) == -1 and b"radius" in so.e2fgvi_last_error()
    assert so.e2fgvi_abi_version() == 9 == lib.ABI_VERSION


# ------------------------------------------------------------------------------------------------ the mask
@pytest.mark.parametrize("name", ["plain", "alpha1.0", "alpha0.5"])
def test_overlay_mask_is_the_restatement(dev, name):
    f = O.clip(name)
    want = O.clip_mask(name)
    got = video.overlay_mask(f, device=dev)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (240, 432)
    assert np.array_equal(got, want), int((got != want).sum())
    assert want.any() == (name != "plain")
    fd = torch.from_numpy(f.copy()).to(dev)
    assert np.array_equal(video.overlay_mask(fd), want) and np.array_equal(fd.cpu().numpy(), f)
    if name == "alpha0.5":                              # other thresholds: every stage moves
        kw = dict(g_min=20, coherence=200, radius=5, min_area=40, max_fraction=0.5)
        assert np.array_equal(video.overlay_mask(fd, **kw), O.mask_np(f, **kw))


def test_overlay_mask_refuses_a_still_clip(dev):
    f = O.clip("still")
    with pytest.raises(ValueError, match="static"):
        video.overlay_mask(f, device=dev)
    got = video.overlay_mask(f[:, :120, :216], max_fraction=1.0, device=dev)
    assert np.array_equal(got, O.mask_np(f[:, :120, :216], max_fraction=1.0)) and got.any()


def test_overlay_runs_are_the_same_bits(dev):
    """the sums of a clip that takes the atomics, the edge map and the mask: twice, and on a side stream"""
    f = _up(O.clip("alpha0.5"), dev, 3)
    a = ops.overlay_stats(f)
    Da, na = ops.overlay_edges(a, 25, 32, 224, 3)
    ma = video.overlay_mask(f)
    b = ops.overlay_stats(f)
    assert torch.equal(a, b) and torch.equal(torch.from_numpy(O.stats_np(O.clip("alpha0.5"))), a.cpu())
    Db, nb = ops.overlay_edges(b, 25, 32, 224, 3)
    assert torch.equal(Da, Db) and torch.equal(na, nb)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = ops.overlay_stats(f)
        Dc, nc = ops.overlay_edges(c, 25, 32, 224, 3)
        mc = video.overlay_mask(f)
    side.synchronize()
    assert torch.equal(a, c) and torch.equal(Da, Dc) and torch.equal(na, nc) and np.array_equal(ma, mc)
    assert np.array_equal(ma, O.clip_mask("alpha0.5"))


# ------------------------------------------------------------------------------------------------ the driver
def test_inpaint_video_overlay_is_the_call_with_the_mask(dev):
    """a 12-frame toy clip with a static patch drawn into it, the stand-in model of the other driver tests: masks_u8="overlay" gives
    the bytes of the call with the mask broadcast over the frames -- found in the caller's frames, not in the resized ones"""
    f = O.patch_video()
    L, H, W = f.shape[:3]
    net = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    mask = video.overlay_mask(f, device=dev)
    assert np.array_equal(mask, O.mask_np(f)) and mask[44:68, 154:194].all() and 1000 < (mask > 0).sum() < 4000
    masks = np.ascontiguousarray(np.broadcast_to(mask, (L, H, W)))
    want = video.inpaint_video(net, f, masks, device=dev, size=(108, 60), restore=True)
    got = video.inpaint_video(net, f, "overlay", device=dev, size=(108, 60), restore=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == f.shape
    assert np.array_equal(got, want), int((got != want).sum())
    far = ~O.dilate_np(mask > 0, 16)                    # the paste follows the mask the model saw: dilated by 4 of its pixels, 2.3 : 1
    assert (got[:, mask > 0] != f[:, mask > 0]).any() and np.array_equal(got[:, far], f[:, far])
    fd = torch.from_numpy(f).to(dev)
    kw = dict(size=(108, 60), restore=True, region="holes", feather=2)
    assert np.array_equal(video.inpaint_video(net, fd, "overlay", **kw), video.inpaint_video(net, f, masks, device=dev, **kw))
    assert np.array_equal(fd.cpu().numpy(), f)
    # without size the mask is used as it is
    assert np.array_equal(video.inpaint_video(net, f, "overlay", device=dev), video.inpaint_video(net, f, masks, device=dev))


def test_inpaint_video_overlay_without_an_overlay(dev):
    """no static edge: the path of masks without a hole pixel; a still clip raises instead of inpainting the scenery"""
    f = O.content("toy", 12, 60, 108)
    calls = []

    def net(x, n):
        calls.append(tuple(x.shape))
        return _stand_in_model(x.cpu(), n)[0].to(dev), None

    assert not video.overlay_mask(f, device=dev).any()
    zeros = np.zeros(f.shape[:3], np.uint8)
    got = video.inpaint_video(net, f, "overlay", device=dev)
    n = len(calls)
    assert np.array_equal(got, video.inpaint_video(net, f, zeros, device=dev)) and len(calls) == 2 * n
    assert np.array_equal(video.inpaint_video(net, f, "overlay", device=dev, size=(108, 60), region="holes", restore=True), f)
    assert len(calls) == 2 * n
    with pytest.raises(ValueError, match="static"):
        video.inpaint_video(net, np.repeat(O.clip("plain")[:1, :120, :216], 6, 0), "overlay", device=dev)
    with pytest.raises(ValueError, match="overlay"):
        video.inpaint_video(net, f, "bogus", device=dev)
    assert len(calls) == 2 * n
