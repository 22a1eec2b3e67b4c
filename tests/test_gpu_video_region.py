"""inpaint_video(region=...) on the device: the hole's bounding box (csrc/video.hip hole_bbox_kernel), the box resize
(resample_u8_kernel with a row window), the paste-back into a box (restore_u8_kernel with an offset) and the driver around them,
against Pillow and the numpy restatements that tests/test_video_region.py pins to Pillow.  Every comparison is bit-exact."""
import importlib
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import ops, video
from tests.test_gpu_video_restore import _stand_in_model, _toy_video
from tests.test_video_region import CASES, nearest_box_np, pass_np, resize_box_np, restore_box_np
from tests.test_video_restore import frames, masks, restore_np

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tennis25.npz")


def _bbox_np(m):
    """(x0, y0, x1, y1) of the non-zero bytes of [L,Hm,Wm], upper ends exclusive; None without any"""
    hit = (m != 0).any(0)
    if not hit.any():
        return None
    ys, xs = np.nonzero(hit)
    return int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1


def _bbox_masks(L, Hm, Wm):
    """empty, full, one pixel in each corner, one pixel only in the last frame, a patch of the values 1 and 255"""
    out = [np.zeros((L, Hm, Wm), np.uint8) for _ in range(8)]
    out[1][:] = 255
    for k, (y, x) in enumerate(((0, 0), (0, Wm - 1), (Hm - 1, 0), (Hm - 1, Wm - 1))):
        out[2 + k][k % L, y, x] = 7
    out[6][L - 1, Hm // 2, Wm // 3] = 128
    out[7][0, Hm // 3, Wm // 4] = 1
    out[7][1, (2 * Hm) // 3, (3 * Wm) // 4] = 255
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("Hm,Wm", [(1, 1), (5, 7), (33, 130), (20, 64)])
def test_hole_bbox_is_numpy(dev, Hm, Wm):
    """a one-byte video, rows shorter than a 16-byte word, a pitch that is no multiple of 16 over more than one block (99 rows,
    four per block), and a pitch that is; every mask at a base as allocated and at one a byte further (no row 16-byte aligned,
    or, with the pitch of 64, every row with a 15-byte head)"""
    L = 3
    for k, m in enumerate(_bbox_masks(L, Hm, Wm)):
        for shift in (0, 1):
            buf = torch.zeros(m.size + shift, dtype=torch.uint8, device=dev)
            md = buf[shift:].view(L, Hm, Wm).copy_(torch.from_numpy(m))
            assert md.is_contiguous() and md.data_ptr() % 16 == shift
            got = ops.hole_bbox(md)
            assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (4,)
            got = tuple(got.cpu().tolist())
            ref = _bbox_np(m)
            if ref is None:
                assert got[2] <= got[0] and got[3] <= got[1], (k, shift, got)
            else:
                assert got == ref, (k, shift, got, ref)
    assert tuple(ops.hole_bbox(torch.zeros((0, Hm, Wm), dtype=torch.uint8, device=dev)).cpu().tolist())[2] == 0      # no launch
    with pytest.raises(TypeError):
        ops.hole_bbox(torch.zeros((L, Hm, Wm), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.hole_bbox(torch.zeros((L, Hm, Wm, 1), dtype=torch.uint8, device=dev))


@pytest.mark.gpu
def test_hole_region_maps_mask_pixels_to_frame_pixels(dev):
    """masks of another size than the frames: floor for the lower ends, ceil for the upper ends, then plan_region"""
    m = np.zeros((3, 60, 125), np.uint8)
    m[1, 21:30, 40:57] = 255
    m[2, 25:33, 38:50] = 1
    # x: 38 * 250 / 125 = 76, 57 * 2 = 114; y: floor(21 * 131 / 60) = 45, ceil(33 * 131 / 60) = ceil(72.05) = 73
    ref = video.plan_region((76, 45, 114, 73), (250, 131), (108, 60))
    assert video.hole_region(m, (250, 131), (108, 60), device=dev) == ref
    assert video.hole_region(torch.from_numpy(m).to(dev), (250, 131), (108, 60)) == ref
    assert video.hole_region(m, (250, 131), (108, 60), context=2, device=dev) == video.plan_region((76, 45, 114, 73), (250, 131), (108, 60), 2)
    assert video.hole_region(m * 0, (250, 131), (108, 60), device=dev) == (0, 0, 250, 131)
    same = np.zeros((2, 131, 250), np.uint8)
    same[1, 100:131, 0:9] = 3
    assert video.hole_region(same, (250, 131), (108, 60), device=dev) == video.plan_region((0, 100, 9, 131), (250, 131), (108, 60))


@pytest.mark.gpu
def test_resample_rows_is_the_restatement(dev):
    """the width pass over a row window, L = 2, row0 > 0, rows < H: frames are H rows apart in the source and `rows` apart in the
    result; with tables of a box (absolute columns) and with the one-tap tables of a crop"""
    f = frames(2, 200, 120, seed=3)
    fd = torch.from_numpy(f).to(dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    for (n_out, box, row0, rows) in ((108, (40, 150), 28, 75), (20, (10, 190), 1, 118), (57, (60, 90), 119, 1), (108, (0, 200), 0, 120)):
        b, c = video.bicubic_tables(200, n_out, box)
        got = ops.resample_rows_u8(fd, n_out, row0, rows, t(b), t(c))
        assert tuple(got.shape) == (2, rows, n_out, 3)
        assert np.array_equal(got.cpu().numpy(), pass_np(f[:, row0:row0 + rows], b, c, -2)), (n_out, box, row0, rows)
    b, c = video._axis_tables(200, 108, (50, 158))
    assert c.shape == (108, 1)
    assert np.array_equal(ops.resample_rows_u8(fd, 108, 40, 60, t(b), t(c)).cpu().numpy(), f[:, 40:100, 50:158])
    for row0, rows in ((-1, 5), (0, 0), (100, 21), (120, 1)):
        with pytest.raises(ValueError):
            ops.resample_rows_u8(fd, 108, row0, rows, t(b), t(c))
    with pytest.raises(ValueError):
        ops.resample_rows_u8(fd, 107, 0, 5, t(b), t(c))
    with pytest.raises(TypeError):
        ops.resample_rows_u8(fd.float(), 108, 0, 5, t(b), t(c))


def _check_resize(dev, case, seed):
    from PIL import Image
    (W, H), size, box = case
    f = frames(2, W, H, seed)
    got = video.resize_frames(f, size, dev, box=box)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (2, size[1], size[0], 3)
    got = got.cpu().numpy()
    for i in range(2):
        ref = np.asarray(Image.fromarray(f[i]).resize(size, box=box))
        assert np.array_equal(got[i], ref), (case, i, int((got[i] != ref).sum()))
    assert np.array_equal(got, resize_box_np(f, size, box))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(15))
def test_resize_frames_box_is_pillow(dev, k):
    """the fixed list of the CPU test: an interior box (its row window starts after row 0 of the frame and ends before its last
    row), a box at every edge, one pixel, the whole frame, crops along one or both axes, untouched axes, a 9x shrink, an upscale"""
    _check_resize(dev, CASES[k], seed=k)


@pytest.mark.gpu
def test_resize_frames_box_is_pillow_on_random_boxes(dev):
    for k in range(15, len(CASES)):
        _check_resize(dev, CASES[k], seed=k)
    f = torch.from_numpy(frames(2, 200, 120, 1)).to(dev)
    assert video.resize_frames(f, (200, 120), box=(0, 0, 200, 120)) is f             # nothing to do: no copy, as without a box
    assert torch.equal(video.resize_frames(f, (108, 60), box=(0, 0, 200, 120)), video.resize_frames(f, (108, 60)))


# the paste-back's tile (csrc/video.hip: RT_W, RT_H)
RT_W, RT_H = 128, 8
RESTORE_BOXES = [(1, 1, 300, 20), (127, 7, 390, 25), (129, 9, 260, 29),        # left / upper one past, one short of and one past a tile edge
                 (150, 10, 400, 30),                                            # flush with the right and bottom edges
                 (130, 9, 200, 15),                                             # inside one tile
                 (100, 3, 300, 12),                                             # three tiles across, two down
                 (129, 9, 165, 29)]                                             # the size of lo: where(mask, lo, src) at an offset


def _check_restore(dev, wh, WH, box, seed):
    (w, h), (W, H) = wh, WH
    left, upper, right, lower = box
    m = masks(h, w, seed)
    outside = np.ones((H, W), bool)
    outside[upper:lower, left:right] = False
    for k in range(0, len(m), 3):                                   # L = 3: two launches cover the six mask kinds
        lo, src = frames(3, w, h, seed + k), frames(3, W, H, seed + k + 50)
        got = video.restore_frames(lo, m[k:k + 3], src, dev, box=box)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, H, W, 3)
        got, ref = got.cpu().numpy(), restore_box_np(lo, m[k:k + 3], src, box)
        for i in range(3):
            assert np.array_equal(got[i], ref[i]), (wh, WH, box, k + i, int((got[i] != ref[i]).sum()))
        assert np.array_equal(got[:, outside], src[:, outside])
        if k == 0 and (right - left, lower - upper) != (w, h):
            assert (got[1] != src[1]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("box", RESTORE_BOXES, ids=str)
def test_restore_frames_box_is_the_restatement(dev, box):
    """a 400 x 30 frame (four tiles across, four down, the last ones partial), lo of 36 x 20; per box the six mask kinds: empty
    (every tile copied), full, one pixel in the first / the last corner of the box, random 30 %, a one-pixel diagonal"""
    assert (400 + RT_W - 1) // RT_W == 4 and (30 + RT_H - 1) // RT_H == 4
    _check_restore(dev, (36, 20), (400, 30), box, seed=sum(box))


@pytest.mark.gpu
def test_restore_frames_box_direct_path(dev):
    """300 rows to 47: the 27 taps of one output row already exceed the rows the LDS holds, and the clipped taps of the box's first
    and last rows reach all 400 columns (16 rows x 1200 bytes > the patch budget): every tile with a hole pixel recomputes its
    horizontal values from global memory"""
    assert video.bicubic_tables(300, 47)[1].shape[1] == 27 and video.bicubic_tables(300, 47)[0][0].tolist() == [0, 16]
    _check_restore(dev, (400, 300), (250, 131), (129, 9, 219, 56), seed=11)


@pytest.mark.gpu
def test_restore_whole_frame_box_is_no_box(dev):
    (w, h), (W, H) = (36, 20), (250, 131)
    m = masks(h, w, 9)[3:]
    lo, src = frames(3, w, h, 1), frames(3, W, H, 2)
    ref = video.restore_frames(lo, m, src, dev)
    assert torch.equal(video.restore_frames(lo, m, src, dev, box=(0, 0, W, H)), ref)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tabs = [t(video.nearest_table(h, H)), t(video.nearest_table(w, W))] + [t(x) for x in video.bicubic_tables(w, W)] \
        + [t(x) for x in video.bicubic_tables(h, H)]
    assert torch.equal(ops.restore_u8(t(lo), t(m), t(src), *tabs, box=(0, 0, W, H)), ref)       # the new entry, the same kernel
    assert np.array_equal(ref.cpu().numpy(), restore_np(lo, m, src))


@pytest.mark.gpu
def test_restore_box_checks_its_arguments(dev):
    """aliasing, dtypes, shapes, the box and the table lengths are refused before a launch"""
    from e2fgvi_amd.lib import HipError
    (w, h), (W, H), box = (36, 20), (160, 47), (30, 5, 113, 40)
    Bw, Bh = box[2] - box[0], box[3] - box[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lo, m, src = t(frames(2, w, h, 1)), t(masks(h, w, 2)[4:6]), t(frames(2, W, H, 3))
    tabs = [t(video.nearest_table(h, Bh)), t(video.nearest_table(w, Bw))] + [t(x) for x in video.bicubic_tables(w, Bw)] \
        + [t(x) for x in video.bicubic_tables(h, Bh)]
    full = [t(video.nearest_table(h, H)), t(video.nearest_table(w, W))] + [t(x) for x in video.bicubic_tables(w, W)] \
        + [t(x) for x in video.bicubic_tables(h, H)]
    ref = restore_box_np(lo.cpu().numpy(), m.cpu().numpy(), src.cpu().numpy(), box)
    out = torch.empty_like(src)
    assert ops.restore_u8(lo, m, src, *tabs, out=out, box=box) is out and np.array_equal(out.cpu().numpy(), ref)
    keep = src.clone()
    with pytest.raises(HipError, match="overlap"):
        ops.restore_u8(lo, m, src, *tabs, out=src, box=box)                 # out aliases src
    big = torch.empty(src.numel() + lo.numel(), dtype=torch.uint8, device=dev)
    lo2 = big[src.numel() - 1:src.numel() - 1 + lo.numel()].view(lo.shape).copy_(lo)
    with pytest.raises(HipError, match="overlap"):
        ops.restore_u8(lo2, m, src, *tabs, out=big[: src.numel()].view(src.shape), box=box)    # the last byte of out is the first of lo
    assert torch.equal(src, keep)
    with pytest.raises(TypeError):
        ops.restore_u8(lo.float(), m, src, *tabs, box=box)
    with pytest.raises(TypeError):
        ops.restore_u8(lo, m.bool(), src, *tabs, box=box)
    with pytest.raises(TypeError):
        ops.restore_u8(lo, m, src.cpu(), *tabs, box=box)
    with pytest.raises(ValueError):
        ops.restore_u8(lo[:1], m, src, *tabs, box=box)                      # L differs
    with pytest.raises(ValueError):
        ops.restore_u8(lo, m, src, *full, box=box)                          # tables of the frame's size, not of the box's
    with pytest.raises(ValueError):
        ops.restore_u8(lo, m, src, *tabs)                                   # ... and the other way round
    with pytest.raises(ValueError):
        ops.restore_u8(lo, m, src, *tabs, out=torch.empty((2, Bh, Bw, 3), dtype=torch.uint8, device=dev), box=box)
    for bad in ((30, 5, 161, 40), (30, 5, 113, 48), (-1, 5, 82, 40), (30, 5, 30, 40), (30, 40, 113, 5), (30, 5, 113)):
        with pytest.raises(ValueError):
            ops.restore_u8(lo, m, src, *tabs, box=bad)
        with pytest.raises(ValueError):
            video.restore_frames(lo, m, src, box=bad)
    with pytest.raises(ValueError):
        video.restore_frames(lo, m[:, :, :5], src, box=box)


def _pil_region(f, m, size, box, mask_box=None):
    from PIL import Image
    fr = np.stack([np.asarray(Image.fromarray(x).resize(size, box=box)) for x in f])
    mr = np.stack([np.asarray(Image.fromarray(x).resize(size, Image.NEAREST, box=mask_box or box)) for x in m])
    return fr, mr


@pytest.mark.gpu
@pytest.mark.parametrize("region", [(60, 20, 221, 110), "hole"], ids=str)
@pytest.mark.parametrize("kw", [{}, {"dilate": False}, {"in_flight": 2}, {"batch_windows": 2}], ids=str)
def test_inpaint_video_region(dev, kw, region):
    """inpaint_video(size, region) == the same call without region on the frames and masks PIL makes with resize(size, box=box);
    with restore=True the restatement's paste of that into the caller's frames; a device tensor of frames is left as it was"""
    L, size = 7, (108, 60)
    f, m = _toy_video(L, 131, 250, seed=4)
    net = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    box = region
    if region == "hole":
        assert _bbox_np(m) == (62, 32, 131, 67)
        box = video.plan_region(_bbox_np(m), (250, 131), size)
        assert box == (27, 11, 165, 88) and video.hole_region(m, (250, 131), size, device=dev) == box
    fr, mr = _pil_region(f, m, size, box)
    assert np.array_equal(fr, resize_box_np(f, size, box)) and np.array_equal(mr, nearest_box_np(m, size, box))
    lo = video.inpaint_video(net, fr, mr, device=dev, **kw)
    got = video.inpaint_video(net, f, m, device=dev, size=size, region=region, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (L, 60, 108, 3)
    assert np.array_equal(got, lo), int((got != lo).sum())
    assert (lo != fr).any() and not np.array_equal(lo, video.inpaint_video(net, f, m, device=dev, size=size, **kw))
    m01 = video.prepare_masks(mr, (60, 108), dev, kw.get("dilate", True)).cpu().numpy()
    ref = restore_box_np(lo, m01, f, box)
    fd = torch.from_numpy(f).to(dev)
    out = video.inpaint_video(net, fd, m, device=dev, size=size, region=region, restore=True, **kw)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == f.shape
    assert np.array_equal(out, ref), int((out != ref).sum())
    assert np.array_equal(fd.cpu().numpy(), f) and (out != f).any()


@pytest.mark.gpu
def test_inpaint_video_region_with_masks_of_another_size(dev):
    """the box goes to mask pixels with floor for the lower ends and ceil for the upper ends, and the masks are resized with it"""
    L, size, box = 7, (108, 60), (61, 21, 220, 110)
    f, m = _toy_video(L, 131, 250, seed=4)
    m = np.ascontiguousarray(m[:, ::2, ::3])                         # 66 x 84
    mask_box = (61 * 84 // 250, 21 * 66 // 131, -(-220 * 84 // 250), -(-110 * 66 // 131))
    assert mask_box == (20, 10, 74, 56)
    net = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    fr, mr = _pil_region(f, m, size, box, mask_box)
    lo = video.inpaint_video(net, fr, mr, device=dev)
    assert np.array_equal(video.inpaint_video(net, f, m, device=dev, size=size, region=box), lo) and (lo != fr).any()
    m01 = video.prepare_masks(mr, (60, 108), dev).cpu().numpy()
    assert np.array_equal(video.prepare_masks(m, (60, 108), dev, box=mask_box).cpu().numpy(), m01)
    out = video.inpaint_video(net, f, m, device=dev, size=size, region=box, restore=True)
    assert np.array_equal(out, restore_box_np(lo, m01, f, box))


@pytest.mark.gpu
def test_inpaint_video_region_without_a_hole_is_no_region(dev):
    L, size = 7, (108, 60)
    f, m = _toy_video(L, 131, 250, seed=4)
    net = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    for kw in ({}, {"restore": True}):
        ref = video.inpaint_video(net, f, m * 0, device=dev, size=size, **kw)
        assert np.array_equal(video.inpaint_video(net, f, m * 0, device=dev, size=size, region="hole", **kw), ref)
        # a hole as large as the frame plans the whole frame: the same path again
        ref = video.inpaint_video(net, f, m * 0 + 1, device=dev, size=size, **kw)
        assert np.array_equal(video.inpaint_video(net, f, m * 0 + 1, device=dev, size=size, region="hole", **kw), ref)
        assert np.array_equal(video.inpaint_video(net, f, m * 0 + 1, device=dev, size=size, region=(0, 0, 250, 131), **kw), ref)


@pytest.mark.gpu
def test_e2fgvi_inpaints_a_region_at_source_resolution(dev):
    """the fixed-size e2fgvi model on six 864x480 frames (the tennis clip, PIL-upscaled) with a hole small enough for a 432x240
    box: both resizes are the identity, so inside the box the result is inpaint_video on the numpy slice of the frames and masks
    (the same kernels on the same bytes), outside the hole it is the source, with and without reuse"""
    from PIL import Image
    from e2fgvi_amd.synth import synth_state_dict
    z = np.load(GOLD)
    big = np.stack([np.asarray(Image.fromarray(f).resize((864, 480))) for f in z["frames"][:6]])
    m = np.zeros((6, 480, 864), np.uint8)
    for i in range(6):
        m[i, 200 + 2 * i:260 + 2 * i, 380 + 3 * i:470 + 3 * i] = 255
    assert _bbox_np(m) == (380, 200, 485, 270)
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
    net = net.to(dev).eval()
    box = video.hole_region(m, (864, 480), (432, 240), device=dev)
    left, upper, right, lower = box
    assert box == video.plan_region((380, 200, 485, 270), (864, 480), (432, 240)) == (216, 115, 648, 355)
    assert (right - left, lower - upper) == (432, 240)
    M = np.zeros(m.shape, bool)
    M[:, upper:lower, left:right] = video.prepare_masks(m[:, upper:lower, left:right], (240, 432), dev).cpu().numpy() != 0
    assert M[m != 0].all() and 0 < M.mean() < 0.1
    for kw in ({}, {"reuse": True}):
        out = video.inpaint_video(net, big, m, size=(432, 240), region="hole", restore=True, **kw)
        assert out.shape == big.shape and out.dtype == np.uint8
        ref = video.inpaint_video(net, big[:, upper:lower, left:right], m[:, upper:lower, left:right], **kw)
        assert np.array_equal(out[:, upper:lower, left:right], ref), kw
        assert np.array_equal(out[~M], big[~M]) and (out[M] != big[M]).any()
        assert np.array_equal(video.inpaint_video(net, big, m, size=(432, 240), region="hole", **kw), ref)
