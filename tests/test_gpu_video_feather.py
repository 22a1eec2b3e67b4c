"""video.restore_frames(feather=r) / ops.restore_blend(feather=r) (csrc/video.hip, the FEATHER form of restore_u8_kernel) and
inpaint_video(restore=True, feather=r) on the device, against the numpy restatement that tests/test_video_feather.py pins to scipy
and Pillow.  Every comparison is bit-exact."""
import importlib

import numpy as np
import pytest
import torch

from e2fgvi_amd import ops, video
from tests.test_gpu_video_region import RESTORE_BOXES
from tests.test_gpu_video_restore import GOLD, _stand_in_model, _toy_video
from tests.test_video_feather import BOXES, far_from, feather_np, feather_parts
from tests.test_video_restore import PAIRS, frames, masks

# the kernel's tile (csrc/video.hip: RT_W, RT_H)
RT_W, RT_H = 128, 8


def _t(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(dev, wh, WH, r, seed, box=None):
    (w, h), (W, H) = wh, WH
    m = masks(h, w, seed)
    L = 3
    for k in range(0, len(m), L):                                   # L = 3: two launches cover the six mask kinds
        lo = frames(L, w, h, seed + k)
        src = frames(L, W, H, seed + k + 50)
        got = video.restore_frames(lo, m[k:k + L], src, dev, box=box, feather=r)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (L, H, W, 3)
        ref = feather_np(lo, m[k:k + L], src, r, box)
        got = got.cpu().numpy()
        for i in range(L):
            assert np.array_equal(got[i], ref[i]), (wh, WH, r, box, k + i, int((got[i] != ref[i]).sum()))
        if k == 0:
            assert np.array_equal(got[0], src[0])                   # the empty mask: every tile copied


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 3, 16])
@pytest.mark.parametrize("wh,WH", PAIRS + [((108, 60), (250, 131)), ((60, 34), (300, 170))])
def test_restore_frames_feather_is_the_restatement(dev, wh, WH, r):
    """the size pairs of the hard paste's test; per pair the six mask kinds.  The corner pixels and the diagonal put the ring into
    tiles without a hole pixel of their own -- below and beside the tile of the pixel, at r = 16 four tile rows away (the next
    test pins one such case) -- and (9, 4) and (300, 3) are frames smaller than the window: n comes from the clipped extents"""
    (w, h), (W, H) = wh, WH
    _check(dev, wh, WH, r, seed=w + 3 * h + 5 * W + 7 * H + r)


@pytest.mark.gpu
def test_the_ring_reaches_tiles_without_a_hole_pixel(dev):
    """said once on its own: one hole pixel of lo whose 5 x 5 block of M lies in tile column 1 and tile row 5 of 60 x 34 -> 300 x 170.
    At r = 16 the ring reaches tile column 0 and tile row 1, four tile rows up; none of those tiles holds a pixel of M"""
    (w, h), (W, H), r = (60, 34), (300, 170), 16
    m = np.zeros((1, h, w), np.uint8)
    m[0, 8, 26] = 1
    _, M, _, c, n = feather_parts(np.zeros((1, h, w, 3), np.uint8), m, (W, H), r)
    ys, xs = np.nonzero(M[0])
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (130, 134, 40, 44) and ys.min() // RT_H == 5
    ring = (c[0] > 0) & ~M[0]
    assert ring[:, :RT_W].any() and ring[RT_H:2 * RT_H].any() and not ring[:RT_H].any()
    lo, src = frames(1, w, h, 3), frames(1, W, H, 4)
    got = video.restore_frames(lo, m, src, dev, feather=r).cpu().numpy()
    ref = feather_np(lo, m, src, r)
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert (ref[0, RT_H:2 * RT_H][ring[RT_H:2 * RT_H]] != src[0, RT_H:2 * RT_H][ring[RT_H:2 * RT_H]]).any()


@pytest.mark.gpu
def test_restore_frames_feather_direct_path(dev):
    """strong shrinking: the lo patch of a tile exceeds the LDS budget (the horizontal values come from global memory per vertical
    tap), and so does the low-resolution rectangle of the halo (the mask is gathered through the tables without staging)"""
    _check(dev, (400, 300), (90, 47), 3, seed=447)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 3, 16])
def test_restore_feather_same_size_is_a_pure_blend(dev, r):
    f, src, m = frames(6, 140, 33, 1), frames(6, 140, 33, 2), masks(33, 140, 3)
    got = video.restore_frames(_t(dev)(f), _t(dev)(m), src, feather=r).cpu().numpy()
    assert np.array_equal(got, feather_np(f, m, src, r))
    assert np.array_equal(got[m != 0], f[m != 0])


@pytest.mark.gpu
@pytest.mark.parametrize("r", [3, 16])
@pytest.mark.parametrize("box", RESTORE_BOXES, ids=str)
def test_restore_frames_feather_in_a_box(dev, box, r):
    """the 400 x 30 frame (four tiles across, four down) and the boxes of the hard paste's test: edges one short of, on and one past
    a tile's, inside one tile, flush with the frame.  The full mask and the corner pixels are holes the box cuts: the ramp stops at
    the box and every byte outside it is the source's (feather_np leaves them)"""
    _check(dev, (36, 20), (400, 30), r, seed=sum(box) + r, box=box)


@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES, ids=str)
def test_restore_frames_feather_in_a_box_of_a_taller_frame(dev, box):
    """the boxes of the CPU test on 160 x 90 (twelve tile rows): the ring crosses tile rows inside a box"""
    _check(dev, (36, 20), (160, 90), 16, seed=sum(box), box=box)
    _check(dev, (36, 20), (160, 90), 1, seed=sum(box) + 1, box=box)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_blend(dev, wh, WH, box, r, seed, touch=None):
    """tests/test_gpu_video_track.py's blend check with the feathered paste: L = 4 source frames, a window of two, lo[0] -> frame 3
    (its first paste), lo[1] -> frame 1 (blended); acc starts with quarter fractions, so every write shows in the bits"""
    (w, h), (W, H) = wh, WH
    left, upper, right, lower = box
    L, ids, first = 4, (3, 1), (1, 0)
    t = _t(dev)
    m = masks(h, w, seed)
    src = frames(L, W, H, seed + 50)
    acc0 = ((np.arange(L * H * W * 3, dtype=np.int64) * 7 + seed) % 251).astype(np.float32).reshape(L, H, W, 3) + np.float32(0.25)
    tabs = video._restore_tables((h, w), (lower - upper, right - left), dev)
    tl, tu, tr, tb = touch or box
    outside = np.ones((H, W), bool)
    outside[tu:tb, tl:tr] = False
    for k in range(0, len(m), 2):                                   # three launches cover the six mask kinds
        lo = frames(2, w, h, seed + k)
        img = feather_np(lo, m[k:k + 2], src[list(ids)], r, box).astype(np.float32)
        want = acc0.copy()
        want[3, tu:tb, tl:tr] = img[0, tu:tb, tl:tr]
        want[1, tu:tb, tl:tr] = acc0[1, tu:tb, tl:tr] * np.float32(0.5) + img[1, tu:tb, tl:tr] * np.float32(0.5)
        acc = t(acc0)
        out = ops.restore_blend(t(lo), t(m[k:k + 2]), t(src), torch.tensor(ids, dtype=torch.int32, device=dev),
                                torch.tensor(first, dtype=torch.uint8, device=dev), acc, *tabs, box=box, touch=touch, feather=r)
        assert out is acc
        got = acc.cpu().numpy()
        for fr in range(L):
            assert np.array_equal(_bits(got[fr]), _bits(want[fr])), (wh, WH, box, touch, r, k, fr, int((got[fr] != want[fr]).sum()))
        assert np.array_equal(_bits(got[[0, 2]]), _bits(acc0[[0, 2]]))
        assert np.array_equal(_bits(got[:, outside]), _bits(acc0[:, outside]))


@pytest.mark.gpu
@pytest.mark.parametrize("box,touch,r", [((129, 9, 260, 29), None, 3), ((127, 7, 390, 25), None, 16),
                                         ((129, 9, 260, 29), (100, 3, 300, 30), 16), ((130, 9, 200, 15), (0, 0, 400, 30), 3)], ids=str)
def test_restore_blend_feather_is_the_restatement_plus_the_blend(dev, box, touch, r):
    """first = 1 (frame 3) and first = 0 (frame 1) in one window; a touched rectangle larger than the box, up to the whole frame:
    between the box and its rim img is src, beyond the rim -- and in frames 0 and 2 -- acc is untouched to the bit"""
    _check_blend(dev, (36, 20), (400, 30), box, r, seed=sum(box) + r, touch=touch)


@pytest.mark.gpu
def test_restore_blend_feather_skips_an_id_outside_the_video_and_checks_the_radius(dev):
    (w, h), (W, H), box = (36, 20), (160, 47), (30, 5, 113, 40)
    t = _t(dev)
    lo, m, src = t(frames(2, w, h, 1)), t(masks(h, w, 2)[4:6]), t(frames(4, W, H, 3))
    first = torch.tensor([1, 0], dtype=torch.uint8, device=dev)
    tabs = video._restore_tables((h, w), (35, 83), dev)
    acc = ops.u8_to_float(src) + 0.25
    keep = acc.clone()
    ops.restore_blend(lo, m, src, torch.tensor([4, -1], dtype=torch.int32, device=dev), first, acc, *tabs, box=box, feather=5)
    assert torch.equal(acc, keep)
    ids = torch.tensor([3, 1], dtype=torch.int32, device=dev)
    for bad in (-1, 17, 2.0, None):
        with pytest.raises(ValueError, match="feather"):
            ops.restore_blend(lo, m, src, ids, first, acc, *tabs, box=box, feather=bad)
        with pytest.raises(ValueError, match="feather"):
            ops.restore_u8(lo, m, src[:2], *tabs, box=box, feather=bad)
    assert torch.equal(acc, keep)
    # one frame in range, one not: only frame 3 changes
    ops.restore_blend(lo, m, src, torch.tensor([3, 9], dtype=torch.int32, device=dev), first, acc, *tabs, box=box, feather=5)
    assert torch.equal(acc[:3], keep[:3]) and not torch.equal(acc[3], keep[3])
    want = feather_np(lo[:1].cpu().numpy(), m[:1].cpu().numpy(), src[3:].cpu().numpy(), 5, box)[0].astype(np.float32)
    left, upper, right, lower = box
    assert np.array_equal(acc[3, upper:lower, left:right].cpu().numpy(), want[upper:lower, left:right])


def _net(dev, calls=None):
    def net(x, n):
        y = _stand_in_model(x.cpu(), n)[0]
        if calls is not None:
            calls.append((y, n, x.shape[0]))
        return y.to(dev), None
    return net


@pytest.mark.gpu
def test_feather_zero_is_the_call_without_the_argument(dev):
    (w, h), (W, H) = (36, 20), (160, 90)
    lo, m, src = frames(6, w, h, 1), masks(h, w, 2), frames(6, W, H, 3)
    assert torch.equal(video.restore_frames(lo, m, src, dev, feather=0), video.restore_frames(lo, m, src, dev))
    box = (10, 7, 150, 85)
    assert torch.equal(video.restore_frames(lo, m, src, dev, box=box, feather=0), video.restore_frames(lo, m, src, dev, box=box))
    f, mk = _toy_video(7, 131, 250, seed=4)
    for kw in ({}, {"region": "hole"}, {"region": "track"}):
        a = video.inpaint_video(_net(dev), f, mk, device=dev, size=(108, 60), restore=True, feather=0, **kw)
        b = video.inpaint_video(_net(dev), f, mk, device=dev, size=(108, 60), restore=True, **kw)
        assert np.array_equal(a, b) and (a != f).any(), kw


def _pred_u8(y, n, h, w):
    """test.py:168-171 on the first n predictions, float32 like the kernel: uint8 [n,h,w,3]"""
    p = y[:n, :, :h, :w].permute(0, 2, 3, 1).numpy().astype(np.float32)
    return ((p + np.float32(1)) / np.float32(2) * np.float32(255)).astype(np.uint8)


def _full_np(calls, windows, L, h, w):
    """the blended predictions of test.py:172-179 with a mask of ones: float32 [L,h,w,3] -> uint8"""
    full = np.zeros((L, h, w, 3), np.float32)
    seen = [False] * L
    half = np.float32(0.5)
    assert len(calls) == len(windows)
    for (y, n, b), (nb, _) in zip(calls, windows):
        assert b == 1 and n == len(nb)
        v = _pred_u8(y, n, h, w).astype(np.float32)
        for i, j in enumerate(nb):
            full[j] = v[i] if not seen[j] else full[j] * half + v[i] * half
            seen[j] = True
    assert all(seen)
    return full.astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"in_flight": 2}, {"batch_windows": 2}, {"region": "hole"}, {"region": "track"}], ids=str)
def test_inpaint_video_feather(dev, kw):
    """inpaint_video(size, restore=True, feather=4) == the restatement applied to the predictions the model returned, kept
    everywhere and blended in window order, the masks the driver used and the caller's frames; outside the 2r ring around the
    pasted mask the caller's bytes"""
    L, size, r = 7, (108, 60), 4
    (w, h), (H, W) = size, (131, 250)
    f, m = _toy_video(L, H, W, seed=4)
    windows = video.plan_windows(L)
    calls = []
    out = video.inpaint_video(_net(dev, calls), f, m, device=dev, size=size, restore=True, feather=r, **kw)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == f.shape
    Mfull = np.zeros((L, H, W), bool)
    if kw.get("region") == "track":
        boxes = video.track_regions(m, (W, H), size, device=dev)
        assert all(b is not None for b in boxes) and len(calls) == len(windows)
        acc = f.astype(np.float32)
        seen = [False] * L
        half = np.float32(0.5)
        for (y, n, b), (nb, rf), box in zip(calls, windows, boxes):
            assert b == 1 and n == len(nb)
            m01 = video.prepare_masks(m, (h, w), dev, box=box, ids=nb + rf).cpu().numpy()[:n]
            img = feather_np(_pred_u8(y, n, h, w), m01, f[nb], r, box).astype(np.float32)
            left, upper, right, lower = box
            Mfull[nb, upper:lower, left:right] |= feather_parts(np.zeros((n, h, w, 3), np.uint8), m01, (right - left, lower - upper), 0)[1]
            for i, j in enumerate(nb):
                acc[j] = img[i] if not seen[j] else acc[j] * half + img[i] * half
                seen[j] = True
        ref = acc.astype(np.uint8)
    else:
        box = video.hole_region(m, (W, H), size, device=dev) if kw.get("region") == "hole" else None
        assert box != (0, 0, W, H)
        m01 = video.prepare_masks(m, (h, w), dev, box=box).cpu().numpy()
        ref = feather_np(_full_np(calls, windows, L, h, w), m01, f, r, box)
        left, upper, right, lower = box or (0, 0, W, H)
        Mfull[:, upper:lower, left:right] = feather_parts(np.zeros((L, h, w, 3), np.uint8), m01, (right - left, lower - upper), 0)[1]
    assert np.array_equal(out, ref), (kw, int((out != ref).sum()))
    far = far_from(Mfull, r)
    assert far.any() and np.array_equal(out[far], f[far]) and (out[Mfull] != f[Mfull]).any()
    ring = ~far & ~Mfull
    assert (out[ring] != f[ring]).any()                             # the ramp itself
    hard = video.inpaint_video(_net(dev), f, m, device=dev, size=size, restore=True, **kw)
    assert np.array_equal(hard[far], f[far]) and (hard != out).any()


@pytest.mark.gpu
def test_e2fgvi_feathers_a_larger_video(dev):
    """the fixed-size e2fgvi model on six 864x480 frames (the tennis clip, PIL-upscaled) with feather=8: the result is the
    restatement of the predictions the net returned (recorded by a thin wrapper), and the input outside the ring"""
    from PIL import Image
    from e2fgvi_amd.synth import synth_state_dict
    z = np.load(GOLD)
    big = np.stack([np.asarray(Image.fromarray(f).resize((864, 480))) for f in z["frames"][:6]])
    raw = z["masks_raw"][:6]
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
    net = net.to(dev).eval()
    calls = []

    def recording(x, n):
        y, aux = net(x, n)
        calls.append((y[:n].float().cpu(), n, x.shape[0]))
        return y, aux

    r = 8
    out = video.inpaint_video(recording, big, raw, device=dev, size=(432, 240), restore=True, feather=r)
    assert out.shape == big.shape and out.dtype == np.uint8
    m01 = video.prepare_masks(raw, (240, 432), dev).cpu().numpy()
    full = _full_np(calls, video.plan_windows(6), 6, 240, 432)
    ref = feather_np(full, m01, big, r)
    M = m01[:, video.nearest_table(240, 480)][:, :, video.nearest_table(432, 864)] != 0
    assert 0 < M.mean() < 0.5
    assert np.array_equal(out[M], ref[M]) and np.array_equal(out, ref), int((out != ref).sum())
    far = far_from(M, r)
    assert np.array_equal(out[far], big[far]) and (out[M] != big[M]).any() and (out[~far & ~M] != big[~far & ~M]).any()
