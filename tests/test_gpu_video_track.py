"""inpaint_video(region="track") on the device: the per-frame bounding boxes (hole_bbox_kernel with a grid row per frame), the
resizes of chosen frames (ids tables of resample_u8_kernel / mask_prepare_kernel), the paste-back with blend (restore_u8_kernel's
BLEND epilogue) and the driver around them, against numpy and the restatement tests/test_video_track.py pins to Pillow.  Every
comparison is bit-exact."""
import importlib

import numpy as np
import pytest
import torch

from e2fgvi_amd import ops, video
from oracle.video_ref import dilate_cross_np
from tests.test_gpu_video_region import RESTORE_BOXES, _bbox_masks, _bbox_np
from tests.test_gpu_video_restore import GOLD, _stand_in_model
from tests.test_video_region import CASES, resize_box_np, restore_box_np
from tests.test_video_restore import frames, masks
from tests.test_video_track import SIZE, example_boxes, moving_hole_video, stand_in, track_np

IDS = (2, 0, 2, 1)              # repeats an id and is out of order


def _t(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("Hm,Wm", [(1, 1), (5, 7), (33, 130), (20, 64)])
def test_hole_bbox_frames_is_numpy(dev, Hm, Wm):
    """the sizes, bases and mask kinds of test_hole_bbox_is_numpy, a box per frame: a frame's box must not see its neighbours' rows
    (the kinds with one pixel in one frame), and a video whose middle frame is empty"""
    L = 3
    gap = np.zeros((L, Hm, Wm), np.uint8)
    gap[0, Hm // 3, Wm // 4] = 9
    gap[2, : (Hm + 1) // 2, Wm // 2:] = 255
    for k, m in enumerate(_bbox_masks(L, Hm, Wm) + [gap]):
        for shift in (0, 1):
            buf = torch.zeros(m.size + shift, dtype=torch.uint8, device=dev)
            md = buf[shift:].view(L, Hm, Wm).copy_(torch.from_numpy(m))
            assert md.is_contiguous() and md.data_ptr() % 16 == shift
            got = ops.hole_bbox_frames(md)
            assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (L, 4)
            got = got.cpu().tolist()
            for i in range(L):
                ref = _bbox_np(m[i:i + 1])
                if ref is None:
                    assert got[i][2] <= got[i][0] and got[i][3] <= got[i][1], (k, shift, i, got[i])
                else:
                    assert tuple(got[i]) == ref, (k, shift, i, got[i], ref)
    assert _bbox_np(gap[1:2]) is None and _bbox_np(gap[:1]) is not None
    assert tuple(ops.hole_bbox_frames(torch.zeros((0, Hm, Wm), dtype=torch.uint8, device=dev)).shape) == (0, 4)      # no launch
    with pytest.raises(TypeError):
        ops.hole_bbox_frames(torch.zeros((L, Hm, Wm), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.hole_bbox_frames(torch.zeros((L, Hm, Wm, 1), dtype=torch.uint8, device=dev))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 7, 13])
def test_resizes_with_ids_equal_the_resizes_of_the_gathered_source(dev, k):
    """CASES[0] (an interior box), CASES[7] (a crop) and CASES[13] (an upscale): the width pass over a row window, the whole-axis
    pass along either axis and the mask preparation with ids == the same call on the numpy-gathered frames; then the two front
    ends, against the restatement"""
    (W, H), (w, h), box = CASES[k]
    left, upper, right, lower = box
    t = _t(dev)
    f = frames(3, W, H, seed=k)
    m = ((np.random.RandomState(k).rand(3, H, W) < 0.05) * 255).astype(np.uint8)
    fd, md, ids = t(f), t(m), torch.tensor(IDS, dtype=torch.int32, device=dev)
    fg, mg = t(f[list(IDS)]), t(m[list(IDS)])
    bx, cx = video._axis_tables(W, w, (left, right))
    got = ops.resample_rows_u8(fd, w, upper, lower - upper, t(bx), t(cx), ids=ids)
    assert tuple(got.shape) == (4, lower - upper, w, 3)
    assert torch.equal(got, ops.resample_rows_u8(fg, w, upper, lower - upper, t(bx), t(cx)))
    for axis, n_in, n_out in ((1, H, h), (2, W, w)):
        b, c = video.bicubic_tables(n_in, n_out)
        got = ops.resample_u8(fd, n_out, axis, t(b), t(c), ids=ids)
        assert got.shape[0] == 4 and got.shape[axis] == n_out
        assert torch.equal(got, ops.resample_u8(fg, n_out, axis, t(b), t(c)))
    b, c = video.bicubic_tables(H, h, (upper, lower))
    assert torch.equal(ops.resample_u8(fd, h, 1, t(b), t(c), span=lower - upper, ids=ids),
                       ops.resample_u8(fg, h, 1, t(b), t(c), span=lower - upper))
    ytab, xtab = t(video.nearest_table(H, h, (upper, lower))), t(video.nearest_table(W, w, (left, right)))
    for it in (0, 4):
        got = ops.mask_prepare(md, ytab, xtab, h, w, it, ids=ids)
        assert tuple(got.shape) == (4, h, w) and torch.equal(got, ops.mask_prepare(mg, ytab, xtab, h, w, it))
    assert got.any()
    # the front ends: a list of ids or a device table, with and without a box
    ref = resize_box_np(f[list(IDS)], (w, h), box)
    assert np.array_equal(video.resize_frames(f, (w, h), dev, box=box, ids=IDS).cpu().numpy(), ref)
    assert np.array_equal(video.resize_frames(fd, (w, h), box=box, ids=ids).cpu().numpy(), ref)
    assert torch.equal(video.resize_frames(fd, (w, h), ids=ids), video.resize_frames(fg, (w, h)))
    assert np.array_equal(video.resize_frames(fd, (W, H), ids=ids).cpu().numpy(), f[list(IDS)])         # the identity: a gather
    assert torch.equal(video.prepare_masks(m, (h, w), dev, box=box, ids=list(IDS)), video.prepare_masks(mg, (h, w), dev, box=box))
    assert torch.equal(video.prepare_masks(md, (h, w), dev, ids=ids), video.prepare_masks(mg, (h, w), dev))
    # without ids nothing changed
    assert np.array_equal(video.resize_frames(fd, (w, h), box=box).cpu().numpy(), resize_box_np(f, (w, h), box))
    # an id outside [0, L): refused from a list; in a device table the kernels keep in bounds and give an empty frame
    for bad in ([0, 3], [-1], [2, 0, 2, 1, 3]):
        with pytest.raises(ValueError):
            video.resize_frames(fd, (w, h), box=box, ids=bad)
        with pytest.raises(ValueError):
            video.prepare_masks(md, (h, w), dev, ids=bad)
    bad = torch.tensor([1, 3, -1, 0], dtype=torch.int32, device=dev)
    want = resize_box_np(f[[1, 0]], (w, h), box)
    got = video.resize_frames(fd, (w, h), box=box, ids=bad).cpu().numpy()
    assert np.array_equal(got[[0, 3]], want) and not got[1:3].any()
    got = ops.resample_u8(fd, h, 1, t(b), t(c), span=lower - upper, ids=bad)
    assert torch.equal(got[[0, 3]], ops.resample_u8(t(f[[1, 0]]), h, 1, t(b), t(c), span=lower - upper)) and not got[1:3].any()
    got = ops.mask_prepare(t(m * 0 + 1), ytab, xtab, h, w, 4, ids=bad)
    assert got[[0, 3]].all() and not got[1:3].any()
    with pytest.raises(TypeError):
        ops.resample_rows_u8(fd, w, upper, lower - upper, t(bx), t(cx), ids=ids.long())
    with pytest.raises(ValueError):
        ops.mask_prepare(md, ytab, xtab, h, w, 4, ids=ids[:0])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_blend(dev, wh, WH, box, seed, touch=None):
    """L = 4 source frames, a window of two: lo[0] -> frame 3 (its first paste), lo[1] -> frame 1 (blended).  acc starts with
    quarter fractions, so a blend shows in the bits (x.25 * 0.5 + v * 0.5 is exact in fp32) and so does any other write."""
    (w, h), (W, H) = wh, WH
    left, upper, right, lower = box
    L, ids, first = 4, (3, 1), (1, 0)
    t = _t(dev)
    m = masks(h, w, seed)
    src = frames(L, W, H, seed + 50)
    acc0 = ((np.arange(L * H * W * 3, dtype=np.int64) * 7 + seed) % 251).astype(np.float32).reshape(L, H, W, 3) + np.float32(0.25)
    tabs = video._restore_tables((h, w), (lower - upper, right - left), dev)
    tl, tu, tr, tb = touch or box
    for k in range(0, len(m), 2):                                   # three launches cover the six mask kinds
        lo = frames(2, w, h, seed + k)
        img = restore_box_np(lo, m[k:k + 2], src[list(ids)], box).astype(np.float32)
        want = acc0.copy()
        want[3, tu:tb, tl:tr] = img[0, tu:tb, tl:tr]
        want[1, tu:tb, tl:tr] = acc0[1, tu:tb, tl:tr] * np.float32(0.5) + img[1, tu:tb, tl:tr] * np.float32(0.5)
        acc = t(acc0)
        out = ops.restore_blend(t(lo), t(m[k:k + 2]), t(src), torch.tensor(ids, dtype=torch.int32, device=dev),
                                torch.tensor(first, dtype=torch.uint8, device=dev), acc, *tabs, box=box, touch=touch)
        assert out is acc
        got = acc.cpu().numpy()
        for fr in range(L):
            assert np.array_equal(_bits(got[fr]), _bits(want[fr])), (wh, WH, box, touch, k, fr, int((got[fr] != want[fr]).sum()))
        # said again, as the issue states it: frames 0 and 2 and everything outside the rectangle are bitwise untouched
        outside = np.ones((H, W), bool)
        outside[tu:tb, tl:tr] = False
        assert np.array_equal(_bits(got[[0, 2]]), _bits(acc0[[0, 2]]))
        assert np.array_equal(_bits(got[:, outside]), _bits(acc0[:, outside]))
        if k == 0:
            # the empty mask on a first paste: no tile has a hole pixel, and the box of acc still becomes the source
            assert np.array_equal(got[3, upper:lower, left:right], src[3, upper:lower, left:right].astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("box", RESTORE_BOXES, ids=str)
def test_restore_blend_is_the_restatement_plus_the_blend(dev, box):
    """the 400 x 30 frame (four tiles across, four down), lo of 36 x 20 and the boxes of the region test: tile edges one short of,
    on and one past the box's; per box the six mask kinds, among them the empty one (a tile without a hole still takes part in
    the blend: img is src there)"""
    _check_blend(dev, (36, 20), (400, 30), box, seed=sum(box))


@pytest.mark.gpu
def test_restore_blend_direct_path(dev):
    """the geometry of test_restore_frames_box_direct_path: every tile with a hole pixel recomputes its horizontal values from
    global memory"""
    _check_blend(dev, (400, 300), (250, 131), (129, 9, 219, 56), seed=11)


@pytest.mark.gpu
@pytest.mark.parametrize("box,touch", [((129, 9, 260, 29), (100, 3, 300, 30)), ((130, 9, 200, 15), (0, 0, 400, 30)),
                                       ((127, 7, 390, 25), (127, 7, 391, 26))], ids=str)
def test_restore_blend_touches_a_rectangle_around_the_box(dev, box, touch):
    """the update widened to a rectangle around the box -- tiles the box does not reach, up to the whole frame, and one pixel more
    than the box: between the box and the rim img is src, beyond the rim nothing is written"""
    _check_blend(dev, (36, 20), (400, 30), box, seed=sum(box), touch=touch)


@pytest.mark.gpu
def test_restore_blend_checks_its_arguments(dev):
    from e2fgvi_amd.lib import HipError
    (w, h), (W, H), box = (36, 20), (160, 47), (30, 5, 113, 40)
    t = _t(dev)
    lo, m, src = t(frames(2, w, h, 1)), t(masks(h, w, 2)[4:6]), t(frames(4, W, H, 3))
    ids, first = torch.tensor([3, 1], dtype=torch.int32, device=dev), torch.tensor([1, 0], dtype=torch.uint8, device=dev)
    tabs = video._restore_tables((h, w), (35, 83), dev)
    acc = ops.u8_to_float(src)
    assert acc.dtype == torch.float32 and np.array_equal(acc.cpu().numpy(), src.cpu().numpy().astype(np.float32))
    odd = t(frames(1, 5, 3, 1)).reshape(-1)[1:]                      # 44 bytes from a base that is no multiple of 4
    assert np.array_equal(ops.u8_to_float(odd).cpu().numpy(), odd.cpu().numpy().astype(np.float32))
    keep = acc.clone()
    # acc over the bytes of src, of lo: refused before a launch
    raw = torch.zeros(acc.numel() * 4 + lo.numel() + 16, dtype=torch.uint8, device=dev)
    a2 = raw[: acc.numel() * 4].view(torch.float32).view(acc.shape)
    lo2 = raw[acc.numel() * 4 - 1:acc.numel() * 4 - 1 + lo.numel()].view(lo.shape).copy_(lo)
    with pytest.raises(HipError, match="overlap"):
        ops.restore_blend(lo2, m, src, ids, first, a2, *tabs, box=box)          # the last byte of acc is the first of lo
    src2 = raw[: src.numel()].view(src.shape)
    with pytest.raises(HipError, match="overlap"):
        ops.restore_blend(lo, m, src2, ids, first, a2, *tabs, box=box)
    with pytest.raises(TypeError):
        ops.restore_blend(lo, m, src, ids, first, acc.double(), *tabs, box=box)
    with pytest.raises(TypeError):
        ops.restore_blend(lo, m, src, ids.long(), first, acc, *tabs, box=box)
    with pytest.raises(TypeError):
        ops.restore_blend(lo, m, src, ids, first.bool(), acc, *tabs, box=box)
    with pytest.raises(ValueError):
        ops.restore_blend(lo, m, src, ids[:1], first, acc, *tabs, box=box)
    with pytest.raises(ValueError):
        ops.restore_blend(lo, m, src, ids, first, acc[:3], *tabs, box=box)
    with pytest.raises(ValueError):
        ops.restore_blend(lo, m, src, ids, first, acc, *tabs)                   # tables of the box, no box
    for bad in ((30, 5, 161, 40), (-1, 5, 82, 40), (30, 5, 30, 40), (30, 5, 113)):
        with pytest.raises(ValueError):
            ops.restore_blend(lo, m, src, ids, first, acc, *tabs, box=bad)
    for bad in ((31, 5, 113, 40), (30, 5, 112, 40), (30, 6, 113, 40), (0, 0, 161, 47), (0, 0, 160)):
        with pytest.raises(ValueError):
            ops.restore_blend(lo, m, src, ids, first, acc, *tabs, box=box, touch=bad)
    assert torch.equal(acc, keep)
    # an id outside [0, L) is skipped
    ops.restore_blend(lo, m, src, torch.tensor([4, -1], dtype=torch.int32, device=dev), first, acc, *tabs, box=box)
    assert torch.equal(acc, keep)


def _jump_video():
    """frames 0 and 1: a hole at the far left; frames 2 ... 7: a 92 x 44 hole at the right, which context = 0 gives a box of
    exactly the model's size with the 8-pixel guard alone around it"""
    L, H, W = 8, 131, 250
    f = frames(L, W, H, 7)
    m = np.zeros((L, H, W), np.uint8)
    m[:2, 50:94, 2:12] = 255
    m[2:, 50:94, 150:242] = 200
    return f, m


def _run_track(dev, f, m, size, **kw):
    calls = []

    def net(x, n):
        calls.append((tuple(x.shape), n))
        return _stand_in_model(x.cpu(), n)[0].to(dev), None

    fd = torch.from_numpy(f).to(dev)
    out = video.inpaint_video(net, fd, m, device=dev, size=size, region="track", restore=True, **kw)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == f.shape
    assert np.array_equal(fd.cpu().numpy(), f)                      # a device tensor of frames is left as it was
    return out, calls


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{"neighbor_stride": 2}, {"neighbor_stride": 2, "dilate": False}, {"neighbor_stride": 2, "other": True},
                                {}, {"num_ref": 2, "context": 2}], ids=str)
def test_inpaint_video_track_is_the_restatement(dev, kw):
    """L = 12 at 131 x 250, a 20 x 12 hole that moves through frames 0 ... 7: with neighbor_stride = 2 the windows get four
    different boxes (one of exactly the model's size, the others scaled) and the last window none; with the default stride the
    windows carry reference frames; masks of another size; another context"""
    kw = dict(kw)
    size = (108, 60)
    f, m = moving_hole_video()
    if kw.pop("other", False):
        m = np.ascontiguousarray(m[:, ::2, ::3])                    # 66 x 84
    ref, boxes = track_np(stand_in, f, m, size, **kw)
    ran = [b for b in boxes if b is not None]
    if kw.get("neighbor_stride") == 2:
        assert len(boxes) == 6 and boxes[-1] is None and len(set(ran)) >= 2
        assert any((b[2] - b[0], b[3] - b[1]) != size for b in ran)
    out, calls = _run_track(dev, f, m, size, **kw)
    assert np.array_equal(out, ref), int((out != ref).sum())
    assert len(calls) == len(ran) and (out != f).any()              # one forward per window with a box
    windows = video.plan_windows(12, kw.get("neighbor_stride", 5), 10, kw.get("num_ref", -1))
    assert [c[1] for c in calls] == [len(nb) for (nb, _), b in zip(windows, boxes) if b is not None]
    tr = {k: v for k, v in kw.items() if k != "dilate"}
    assert video.track_regions(m, (250, 131), size, device=dev, **tr) == boxes
    assert video.track_regions(torch.from_numpy(m).to(dev), (250, 131), size, **tr) == boxes


@pytest.mark.gpu
def test_inpaint_video_track_blends_outside_a_later_box(dev):
    """context = 0: window 1 sees the holes at both ends of the frame and plans the whole frame, window 2 a box of the model's size
    -- the paste of window 1 (a 2.3x upscale of the dilated mask) reaches past the 8-pixel guard of window 2's box, where the
    contract still owes 0.5 acc + 0.5 src"""
    size = (108, 60)
    f, m = _jump_video()
    log = []
    ref, boxes = track_np(stand_in, f, m, size, neighbor_stride=2, context=0, log=log)
    assert boxes == [(0, 0, 250, 131), (0, 0, 250, 131), (142, 42, 250, 102), (142, 42, 250, 102)]
    beyond = 0
    for k1, j1, _, changed in log:
        for k2, j2, (left, upper, right, lower), _ in log:
            if j1 == j2 and k1 < k2:
                c = changed.copy()
                c[upper:lower, left:right] = False
                beyond += int(c.sum())
    assert beyond > 0
    out, calls = _run_track(dev, f, m, size, neighbor_stride=2, context=0)
    assert np.array_equal(out, ref), int((out != ref).sum())
    assert len(calls) == 4


@pytest.mark.gpu
def test_inpaint_video_track_without_a_hole_returns_the_source(dev):
    f, m = moving_hole_video()
    out, calls = _run_track(dev, f, m * 0, (108, 60))
    assert np.array_equal(out, f) and calls == []
    assert video.track_regions(m * 0, (250, 131), (108, 60), device=dev) == [None, None, None]


@pytest.mark.gpu
def test_e2fgvi_tracks_a_moving_hole_at_source_resolution(dev):
    """the worked example on the fixed-size e2fgvi model: 30 frames of 864 x 480 (the tennis clip, PIL-upscaled and repeated),
    frames 0 ... 14 with a 90 x 60 hole that moves 12 pixels right and 2 down per frame.  The four boxes are exactly 432 x 240, so
    both resizes are the identity and every window is the model on the numpy slice of its frames (the restatement with the same
    net: the same kernels on the same bytes); two of the six windows run no forward"""
    from PIL import Image
    from e2fgvi_amd.synth import synth_state_dict
    z = np.load(GOLD)
    small = z["frames"]
    up = [np.asarray(Image.fromarray(x).resize((864, 480))) for x in small]
    big = np.stack([up[i % len(up)] for i in range(30)])
    m = np.zeros((30, 480, 864), np.uint8)
    for i, b in enumerate(example_boxes()):
        if b is not None:
            m[i, b[1]:b[3], b[0]:b[2]] = 255
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
    net = net.to(dev).eval()
    calls = []

    def counted(x, n):
        calls.append(n)
        return net(x, n)

    want = [(0, 65, 432, 305), (0, 70, 432, 310), (43, 79, 475, 319), (73, 84, 505, 324), None, None]
    assert video.track_regions(m, (864, 480), SIZE, device=dev) == want
    assert video.hole_region(m, (864, 480), SIZE, device=dev) == (0, 50, 516, 337)         # region="hole": a 1.19x downscale
    windows = video.plan_windows(30)
    for (nb, rf), (left, upper, right, lower) in zip(windows, want[:4]):
        assert (right - left, lower - upper) == SIZE
        assert np.array_equal(resize_box_np(big[nb + rf], SIZE, (left, upper, right, lower)), big[nb + rf][:, upper:lower, left:right])
    out = video.inpaint_video(counted, big, m, device=dev, size=SIZE, region="track", restore=True)
    assert out.shape == big.shape and out.dtype == np.uint8
    assert calls == [6, 11, 11, 11]                                 # the engine is called four times
    ref, boxes = track_np(lambda x, n: net(x.to(dev), n)[0], big, m, SIZE)
    assert boxes == want
    assert np.array_equal(out, ref), int((out != ref).sum())
    M = np.stack([dilate_cross_np(x, 4) for x in m]) != 0           # at scale 1 the pasted mask is the dilated hole
    assert M[m != 0].all() and not M[15:].any()
    assert np.array_equal(out[~M], big[~M]) and (out[M] != big[M]).any()
