"""inpaint_video(region="track"): one crop box per window, the windows' results blended at source size.

    windows = plan_windows(L, ...);  boxes = plan_track(per-frame hole boxes, windows, (W, H), size, context)
    acc = float32(source)
    for every window k with a box, in the reference's order:
        fr, m01 = Image.resize(size, box=boxes[k]) of source[ids], NEAREST(box) -> != 0 -> dilate of masks[ids]
        lo      = test.py:146-174 at the model's size
        for every neighbour frame f:  img = restore_frames(lo, m01, source[f], box=boxes[k])
                                      acc[f] = img  (first time)  or  acc[f] * 0.5 + img * 0.5            (fp32, the whole frame)
    result = acc.astype(uint8)

``track_np`` below restates that around the restatements tests/test_video_region.py pins to Pillow; this file pins it against
Pillow on one window and plan_track against the worked example, and the device tests (tests/test_gpu_video_track.py) compare
the kernels and the driver with it."""
import numpy as np
import pytest
import torch

from e2fgvi_amd import video
from oracle.video_ref import dilate_cross_np
from tests.test_video_region import nearest_box_np, resize_box_np, restore_box_np
from tests.test_video_restore import frames

SIZE = (432, 240)


def frame_boxes_np(m, frame_wh):
    """every frame's hole box (x0, y0, x1, y1) in frame pixels, None without a hole: numpy per frame, then floor / ceil"""
    out = []
    for x in m:
        ys, xs = np.nonzero(x)
        if len(ys) == 0:
            out.append(None)
            continue
        box = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)
        out.append(video._scale_box(box, (m.shape[2], m.shape[1]), frame_wh))
    return out


def window_lo_np(model_fn, fr, m01, n, pad=True):
    """test.py:146-174 for ONE window at the model's size (oracle/video_ref.py's arithmetic): fr uint8 [t,h,w,3], m01 uint8 [t,h,w]
    of 0 / 1, the first n frames local -> uint8 [n,h,w,3]; model_fn(x[1,t,3,Hp,Wp], n) -> pred [>= n,3,Hp,Wp]"""
    t, h, w, _ = fr.shape
    imgs = torch.from_numpy(np.ascontiguousarray(fr)).permute(0, 3, 1, 2).float().div(255).unsqueeze(0) * 2 - 1
    x = imgs * (1 - torch.from_numpy(m01.astype(np.float32)).view(1, t, 1, h, w))
    Hp, Wp = video.padded_size(h, w) if pad else (h, w)
    x = torch.cat([x, torch.flip(x, [3])], 3)[:, :, :, :Hp, :]
    x = torch.cat([x, torch.flip(x, [4])], 4)[:, :, :, :, :Wp]
    pred = (model_fn(x, n)[:n, :, :h, :w] + 1) / 2
    pred = pred.cpu().permute(0, 2, 3, 1).numpy() * 255
    bm = m01[:n, :, :, None]
    return pred.astype(np.uint8) * bm + fr[:n] * (1 - bm)


def track_np(model_fn, f, m, size, neighbor_stride=5, ref_length=10, num_ref=-1, dilate=True, context=0.5, pad=True, log=None):
    """the contract of inpaint_video(region="track", restore=True) -> (uint8 [L,H,W,3], the boxes).  ``log`` (a list) receives
    (window, frame, box, [H,W] bool: where that paste differs from the source) for every paste."""
    L, H, W, _ = f.shape
    mask_wh = (m.shape[2], m.shape[1])
    windows = video.plan_windows(L, neighbor_stride, ref_length, num_ref)
    boxes = video.plan_track(frame_boxes_np(m, (W, H)), windows, (W, H), size, context)
    acc = f.astype(np.float32)
    seen = [False] * L
    half = np.float32(0.5)
    for k, (nb, rf) in enumerate(windows):
        if boxes[k] is None:
            continue
        ids = nb + rf
        fr = resize_box_np(f[ids], size, boxes[k])
        m01 = (nearest_box_np(m[ids], size, video._scale_box(boxes[k], (W, H), mask_wh)) != 0).astype(np.uint8)
        if dilate:
            m01 = np.stack([dilate_cross_np(x, 4) for x in m01])
        lo = window_lo_np(model_fn, fr, m01, len(nb), pad)
        for i, j in enumerate(nb):
            img = restore_box_np(lo[i:i + 1], m01[i:i + 1], f[j:j + 1], boxes[k])[0]
            if log is not None:
                log.append((k, j, boxes[k], (img != f[j]).any(-1)))
            img = img.astype(np.float32)
            acc[j] = img if not seen[j] else acc[j] * half + img * half
            seen[j] = True
    assert acc.dtype == np.float32
    return acc.astype(np.uint8), boxes


def stand_in(x, n_local):
    """tests/test_gpu_video_restore.py's stand-in model, the predictions alone"""
    b, t, c, H, W = x.shape
    return torch.tanh(x.reshape(b * t, c, H, W) * 0.7 + 0.1 * x.mean(dim=(1, 2, 3, 4)).view(1, 1, 1, 1))


def example_boxes(L=30):
    """the worked example: 864 x 480 frames, frames 0 ... 14 carry a 90 x 60 hole at (100 + 12 i, 150 + 2 i), the others none"""
    return [(100 + 12 * i, 150 + 2 * i, 190 + 12 * i, 210 + 2 * i) if i < 15 else None for i in range(L)]


def moving_hole_video(L=12, H=131, W=250, seed=4, last=8):
    """a 20 x 12 hole that moves 10 pixels right and 3 down per frame through frames 0 ... last - 1; none afterwards"""
    f = frames(L, W, H, seed)
    m = np.zeros((L, H, W), np.uint8)
    for i in range(last):
        m[i, 30 + 3 * i:42 + 3 * i, 40 + 10 * i:60 + 10 * i] = 1 + 36 * i
    return f, m


def test_plan_track_on_the_worked_example():
    windows = video.plan_windows(30)
    assert [(nb[0], nb[-1]) for nb, _ in windows] == [(0, 5), (0, 10), (5, 15), (10, 20), (15, 25), (20, 29)]
    fb = example_boxes()
    # the unions the table lists
    union = lambda nb: tuple(f([fb[j][i] for j in nb if fb[j]]) for i, f in enumerate((min, min, max, max)))
    assert [union(nb) for nb, _ in windows[:4]] == [(100, 150, 250, 220), (100, 150, 310, 230), (160, 160, 358, 238),
                                                    (220, 170, 358, 238)]
    assert video.plan_track(fb, windows, (864, 480), SIZE) == [(0, 65, 432, 305), (0, 70, 432, 310), (43, 79, 475, 319),
                                                               (73, 84, 505, 324), None, None]
    assert video.plan_region((100, 150, 358, 238), (864, 480), SIZE) == (0, 50, 516, 337)       # region="hole": a 1.19x downscale
    # an empty box in the device's convention (x1 <= x0) is a frame without a hole, like None
    raw = [b if b else (0x7f7f7f7f, 0x7f7f7f7f, 0, 0) for b in fb]
    assert video.plan_track(raw, windows, (864, 480), SIZE) == video.plan_track(fb, windows, (864, 480), SIZE)
    assert video.plan_track([None] * 30, windows, (864, 480), SIZE) == [None] * 6
    # context goes through to plan_region
    assert video.plan_track(fb, windows, (864, 480), SIZE, 2)[0] == video.plan_region((100, 150, 250, 220), (864, 480), SIZE, 2)
    assert video.plan_track(fb, windows, (864, 480), SIZE, 2)[0] != (0, 65, 432, 305)


def test_plan_track_takes_the_union_over_neighbours_only():
    L = 30
    windows = video.plan_windows(L)
    assert windows[2] == (list(range(5, 16)), [0, 20]) and windows[5] == (list(range(20, 30)), [0, 10])
    fb = [None] * L
    fb[0] = (700, 400, 800, 470)            # a reference frame of windows 2 ... 5, a neighbour of windows 0 and 1
    fb[10] = (100, 100, 150, 140)           # a neighbour of windows 1, 2 and 3, a reference frame of windows 4 and 5
    got = video.plan_track(fb, windows, (864, 480), SIZE)
    assert got[0] == video.plan_region(fb[0], (864, 480), SIZE)
    assert got[1] == video.plan_region((100, 100, 800, 470), (864, 480), SIZE)
    assert got[2] == got[3] == video.plan_region(fb[10], (864, 480), SIZE)                      # frame 0 does not widen them
    assert got[4] is None and got[5] is None                                                    # holes in reference frames only


def test_frame_boxes_of_masks_of_another_size_map_by_floor_and_ceil():
    m = np.zeros((3, 60, 125), np.uint8)
    m[0, 21:30, 40:57] = 255
    m[2, 25:33, 38:50] = 1
    # x: 40 * 250 / 125 = 80, 57 * 2 = 114; y: floor(21 * 131 / 60) = 45, ceil(30 * 131 / 60) = 66
    # x: 76, 100; y: floor(25 * 131 / 60) = 54, ceil(33 * 131 / 60) = ceil(72.05) = 73
    want = [(80, 45, 114, 66), None, (76, 54, 100, 73)]
    assert frame_boxes_np(m, (250, 131)) == want
    raw = [(40, 21, 57, 30), (0x7f7f7f7f, 0x7f7f7f7f, 0, 0), (38, 25, 50, 33)]                  # what ops.hole_bbox_frames returns
    assert video._map_frame_boxes(raw, (125, 60), (250, 131)) == want
    assert video._map_frame_boxes(raw, (125, 60), (125, 60)) == [raw[0], None, raw[2]]


def test_track_arguments_are_checked_before_any_device_work():
    f = np.zeros((3, 20, 36, 3), np.uint8)
    m = np.zeros((3, 20, 36), np.uint8)
    cpu = torch.device("cpu")

    def net(x, n):
        raise AssertionError("the model must not be called")

    with pytest.raises(ValueError, match="size"):
        video.inpaint_video(net, f, m, device=cpu, region="track", restore=True)
    with pytest.raises(ValueError, match="restore"):
        video.inpaint_video(net, f, m, device=cpu, size=(18, 10), region="track")
    with pytest.raises(ValueError, match="keep_float"):
        video.inpaint_video(net, f, m, device=cpu, size=(18, 10), region="track", restore=True, keep_float=True)
    with pytest.raises(ValueError, match="reuse"):
        video.inpaint_video(net, f, m, device=cpu, size=(18, 10), region="track", restore=True, reuse=True)
    with pytest.raises(ValueError, match="batch_windows"):
        video.inpaint_video(net, f, m, device=cpu, size=(18, 10), region="track", restore=True, batch_windows=2)
    with pytest.raises(ValueError, match="in_flight"):
        video.inpaint_video(net, f, m, device=cpu, size=(18, 10), region="track", restore=True, in_flight=2)
    with pytest.raises(ValueError, match="track"):
        video.inpaint_video(net, f, m, device=cpu, size=(18, 10), region="tracks", restore=True)
    # ids= of the two resizes: checked against the number of frames from the shapes alone
    for bad in ([3], [-1], [0, 3], []):
        with pytest.raises(ValueError):
            video.resize_frames(f, (18, 10), device=cpu, ids=bad)
        with pytest.raises(ValueError):
            video.prepare_masks(m, (10, 18), cpu, ids=bad)
    # a well-formed call gets as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="cuda"):
        video.inpaint_video(net, f, m, device=cpu, size=(18, 10), region="track", restore=True)


def test_restatement_is_pillow_on_one_window():
    """four frames are one window (all of them neighbours, no reference frame): every frame is pasted once, so the contract is the
    PIL lines of the resize, the mask and the paste-back around test.py:146-174"""
    from PIL import Image
    L, size = 4, (108, 60)
    f, m = moving_hole_video(L, 131, 250, seed=2, last=4)
    m[1] = 0                                                    # a frame without a hole inside the window
    assert video.plan_windows(L) == [([0, 1, 2, 3], [])]
    got, boxes = track_np(stand_in, f, m, size, context=1.5)
    box = boxes[0]
    left, upper, right, lower = box
    assert box == video.plan_region((40, 30, 90, 51), (250, 131), size, 1.5) and (right - left, lower - upper) != size
    fr = np.stack([np.asarray(Image.fromarray(x).resize(size, box=box)) for x in f])
    mr = np.stack([np.asarray(Image.fromarray(x).resize(size, Image.NEAREST, box=box)) for x in m])
    m01 = np.stack([dilate_cross_np(x != 0, 4) for x in mr])
    lo = window_lo_np(stand_in, fr, m01, L)
    assert lo.dtype == np.uint8 and (lo != fr).any()
    for i in range(L):
        ref = f[i].copy()
        up = np.asarray(Image.fromarray(lo[i]).resize((right - left, lower - upper)))
        M = np.asarray(Image.fromarray(m01[i] * 255).resize((right - left, lower - upper), Image.NEAREST))
        ref[upper:lower, left:right] = np.where(M[..., None] != 0, up, ref[upper:lower, left:right])
        assert np.array_equal(got[i], ref), i
    assert np.array_equal(got[1], f[1]) and (got[0] != f[0]).any()
    # no hole at all: the source, and the model is never called
    def net(x, n):
        raise AssertionError("the model must not be called")
    out, boxes = track_np(net, f, m * 0, size)
    assert np.array_equal(out, f) and boxes == [None]


def test_restatement_blends_overlapping_windows_over_the_whole_frame():
    """a frame two windows keep is the fp32 mean of its two pastes: of their two pasted values where both boxes paste, of a
    paste and the source where only one does"""
    f, m = moving_hole_video()
    log = []
    got, boxes = track_np(stand_in, f, m, (108, 60), neighbor_stride=2, log=log)
    assert len(set(b for b in boxes if b)) >= 2 and boxes[-1] is None
    per_frame = {}
    for k, j, box, changed in log:
        per_frame.setdefault(j, []).append(k)
    assert per_frame[0] == [0, 1] and per_frame[2] == [0, 1, 2] and 11 not in per_frame
    # frame 0: two pastes, blended once
    first = {}
    acc = f.astype(np.float32)
    windows = video.plan_windows(12, 2)
    for k in (0, 1):
        ids = windows[k][0] + windows[k][1]
        fr = resize_box_np(f[ids], (108, 60), boxes[k])
        m01 = np.stack([dilate_cross_np(x, 4) for x in nearest_box_np(m[ids], (108, 60), boxes[k]) != 0])
        lo = window_lo_np(stand_in, fr, m01, len(windows[k][0]))
        first[k] = restore_box_np(lo[:1], m01[:1], f[:1], boxes[k])[0].astype(np.float32)
    want = (first[0] * np.float32(0.5) + first[1] * np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(got[0], want) and (first[0] != first[1]).any()
    assert np.array_equal(got[8:], f[8:])


def test_new_entries_refuse_bad_arguments():
    """host side of e2fgvi_restore_blend, e2fgvi_hole_bbox_frames, e2fgvi_u8_to_float and the three ids variants: E2FGVI_EINVAL from
    the arguments alone (no launch, so this runs without a GPU; the addresses are never read)"""
    import os
    from e2fgvi_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    n, L, h, w, H, W = 2, 4, 20, 36, 47, 160
    n_src, n_lo = L * H * W * 3, n * h * w * 3
    base = 1 << 20
    good = dict(lo=base, mask=base + n_lo, src=base + 2 * n_lo, ids=64, first=128, acc=base + (1 << 22), n=n, L=L, h=h, w=w, H=H, W=W,
                left=30, upper=5, Bw=83, Bh=35, tl=30, tu=5, Tw=83, Th=35, ytab=256, xtab=256, bx=256, cx=256, kx=5, by=256, cy=256,
                ky=5)
    order = ("lo", "mask", "src", "ids", "first", "acc", "n", "L", "h", "w", "H", "W", "left", "upper", "Bw", "Bh", "tl", "tu", "Tw",
             "Th", "ytab", "xtab", "bx", "cx", "kx", "by", "cy", "ky")

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_restore_blend(*[a[k] for k in order], None)

    for k in ("lo", "mask", "src", "ids", "first", "acc", "ytab", "xtab", "bx", "cx", "by", "cy"):
        assert rc(**{k: None}) == -1, k
    for k in ("n", "L", "h", "w", "H", "W", "Bw", "Bh", "Tw", "Th", "kx", "ky"):
        assert rc(**{k: 0}) == -1 and rc(**{k: -3}) == -1, k
    assert rc(left=-1, tl=-1) == -1 and rc(upper=-1, tu=-1) == -1 and b"box" in so.e2fgvi_last_error()
    assert rc(left=78, tl=78) == -1 and rc(Bw=131, Tw=131) == -1 and rc(upper=13, tu=13) == -1 and rc(Bh=43, Th=43) == -1
    assert rc(left=0x7fffffff) == -1 and rc(Bw=0x7fffffff) == -1                                    # no overflow in the check
    # the touched rectangle: inside the frame, around the box
    assert rc(tl=31) == -1 and b"touched" in so.e2fgvi_last_error()
    assert rc(tu=6) == -1 and rc(Tw=82) == -1 and rc(Th=34) == -1 and rc(tl=0, Tw=112) == -1 and rc(tl=-1, Tw=200) == -1
    assert rc(tl=0, Tw=161) == -1 and rc(tu=0, Th=48) == -1 and rc(Tw=0x7fffffff) == -1
    # acc [L,H,W,3] fp32 must not overlap an input, and must be a float address
    assert rc(acc=good["src"]) == -1 and b"overlap" in so.e2fgvi_last_error()
    assert rc(acc=good["src"] + n_src - 4) == -1 and rc(acc=good["src"] - 4 * n_src + 4) == -1
    assert rc(acc=good["lo"] + n_lo - 4 + (4 - n_lo % 4) % 4) == -1 and rc(acc=good["mask"] - 4 * n_src + 4) == -1
    assert rc(ids=good["acc"] + 8) == -1 and rc(first=good["acc"] + 4 * n_src - 1) == -1
    assert rc(acc=good["acc"] + 2) == -1 and b"aligned" in so.e2fgvi_last_error()

    assert so.e2fgvi_hole_bbox_frames(base, 2, 5, 7, None, None) == -1
    assert so.e2fgvi_hole_bbox_frames(None, 2, 5, 7, base, None) == -1
    assert so.e2fgvi_hole_bbox_frames(base, -1, 5, 7, base, None) == -1 and so.e2fgvi_hole_bbox_frames(base, 2, 5, -7, base, None) == -1
    assert so.e2fgvi_hole_bbox_frames(None, 0, 5, 7, None, None) == 0                               # L = 0: nothing to do

    def rows(**kw):
        a = dict(dict(src=base, L=L, ids=64, n=n, dst=base + n_src, H=H, W=W, n_out=50, row0=3, rows=40, bounds=64, coeffs=64, ksize=9),
                 **kw)
        return so.e2fgvi_resample_rows_ids_u8(*[a[k] for k in ("src", "L", "ids", "n", "dst", "H", "W", "n_out", "row0", "rows",
                                                               "bounds", "coeffs", "ksize")], None)

    def axis(**kw):
        a = dict(dict(src=base, L=L, ids=64, n=n, dst=base + n_src, H=H, W=W, n_out=50, axis=1, bounds=64, coeffs=64, ksize=9), **kw)
        return so.e2fgvi_resample_ids_u8(*[a[k] for k in ("src", "L", "ids", "n", "dst", "H", "W", "n_out", "axis", "bounds", "coeffs",
                                                          "ksize")], None)

    def mask(**kw):
        a = dict(dict(masks=base, L=L, ids=64, n=n, Hin=H, Win=W, ytab=64, xtab=64, out=base + n_src, H=h, W=w, it=4), **kw)
        return so.e2fgvi_mask_prepare_ids(*[a[k] for k in ("masks", "L", "ids", "n", "Hin", "Win", "ytab", "xtab", "out", "H", "W",
                                                           "it")], None)

    for fn, ptrs, ints in ((rows, ("src", "ids", "dst", "bounds", "coeffs"), ("L", "n", "H", "W", "n_out", "rows", "ksize")),
                           (axis, ("src", "ids", "dst", "bounds", "coeffs"), ("L", "n", "H", "W", "n_out", "ksize")),
                           (mask, ("masks", "ids", "ytab", "xtab", "out"), ("L", "n", "Hin", "Win", "H", "W"))):
        for k in ptrs:
            assert fn(**{k: None}) == -1, (fn.__name__, k)
        for k in ints:
            assert fn(**{k: 0}) == -1 and fn(**{k: -2}) == -1, (fn.__name__, k)
    assert rows(row0=-1) == -1 and rows(row0=8) == -1 and rows(rows=45) == -1 and axis(axis=0) == -1 and axis(axis=3) == -1
    assert mask(it=-1) == -1 and mask(it=65) == -1
    assert so.e2fgvi_u8_to_float(None, base, 5, None) == -1 and so.e2fgvi_u8_to_float(base, None, 5, None) == -1
    assert so.e2fgvi_u8_to_float(base, base + 64, 0, None) == -1
    assert so.e2fgvi_abi_version() == 9
