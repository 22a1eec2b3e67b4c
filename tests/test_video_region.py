"""The crop region of inpaint_video(region=...): the model sees ``Image.resize(size, box=box)`` of the frames and
``resize(size, Image.NEAREST, box=box)`` of the masks, and the result is pasted back into that box.

``resize_box_np`` / ``nearest_box_np`` / ``restore_box_np`` below restate those around video.bicubic_tables(box=) /
video.nearest_table(box=) with Pillow's pass structure (the width pass over the rows the height pass reads, the height pass's
bounds shifted by the first of them); this file pins the restatements against Pillow and plan_region against its stated
properties, and the device tests (tests/test_gpu_video_region.py) compare the kernels with the restatements."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from e2fgvi_amd import video
from tests.test_video_restore import frames, masks, restore_np

# ((W, H) of the frame, (w, h) of the output, (left, upper, right, lower)), PIL order
CASES = [
    ((200, 120), (108, 60), (40, 30, 150, 100)),        # interior: the row window starts after row 0 and ends before the last row
    ((200, 120), (108, 60), (0, 30, 110, 100)),         # touching the left edge
    ((200, 120), (108, 60), (40, 0, 150, 70)),          # ... the top edge
    ((200, 120), (108, 60), (90, 30, 200, 100)),        # ... the right edge
    ((200, 120), (108, 60), (40, 50, 150, 120)),        # ... the bottom edge
    ((200, 120), (108, 60), (77, 33, 78, 34)),          # one pixel
    ((200, 120), (108, 60), (0, 0, 200, 120)),          # the whole frame
    ((200, 120), (108, 60), (50, 40, 158, 100)),        # the output's size at an offset: Pillow crops
    ((200, 120), (108, 60), (30, 40, 171, 100)),        # the height keeps its size (at an offset), the width shrinks
    ((200, 120), (108, 120), (20, 0, 180, 120)),        # the height is not touched at all: no height pass
    ((200, 120), (200, 60), (0, 10, 200, 110)),         # the width is not touched at all: no width pass
    ((200, 120), (200, 100), (0, 10, 200, 110)),        # ... and the height is a crop
    ((200, 120), (20, 12), (10, 6, 190, 114)),          # a 9x shrink
    ((200, 120), (108, 60), (60, 40, 90, 55)),          # an upscale
    ((131, 57), (37, 91), (3, 5, 129, 50)),             # one axis down, the other up
]
_rng = np.random.RandomState(31)
for _ in range(20):
    _W, _H = (int(v) for v in _rng.randint(2, 160, 2))
    _l, _u = int(_rng.randint(0, _W)), int(_rng.randint(0, _H))
    CASES.append(((_W, _H), tuple(int(v) for v in _rng.randint(1, 120, 2)),
                  (_l, _u, int(_rng.randint(_l + 1, _W + 1)), int(_rng.randint(_u + 1, _H + 1)))))


def pass_np(a, bounds, coeffs, axis):
    """one pass of Pillow's 8-bit resample along `axis` of uint8 [..., H, W, 3] (-3: rows, -2: columns) with the given tables:
    _pass_np of tests/test_video_restore.py with the tables as arguments, int32 like Pillow"""
    n_in, n_out = a.shape[axis], len(bounds)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    acc = np.full((n_out,) + a.shape[1:], 1 << 21, np.int64)
    for j in range(coeffs.shape[1]):
        idx = np.clip(bounds[:, 0] + j, 0, n_in - 1)            # coefficients past a row's tap count are zero
        acc += a[idx] * coeffs[:, j].reshape((n_out,) + (1,) * (a.ndim - 1))
    assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31
    return np.moveaxis(np.clip(acc >> 22, 0, 255).astype(np.uint8), 0, axis)


def resize_box_np(f, size, box):
    """``Image.resize(size, box=box)`` (BICUBIC) of uint8 [L,H,W,3] as Pillow's ImagingResample runs it"""
    (w, h), (H, W) = size, f.shape[1:3]
    left, upper, right, lower = box
    bx, cx = video.bicubic_tables(W, w, (left, right))
    by, cy = video.bicubic_tables(H, h, (upper, lower))
    need_w = w != W or left != 0 or right != w
    need_h = h != H or upper != 0 or lower != h
    if need_w:
        first, last = int(by[0, 0]), int(by[-1, 0] + by[-1, 1])
        f = pass_np(f[:, first:last], bx, cx, -2)              # the row window: frames H rows apart in, last - first rows apart out
        by = by - np.array([first, 0], np.int32)
    if need_h:
        f = pass_np(f, by, cy, -3)
    return f


def nearest_box_np(m, size, box):
    """``resize(size, Image.NEAREST, box=box)`` of uint8 [L,Hm,Wm]"""
    (w, h), (Hm, Wm) = size, m.shape[1:3]
    left, upper, right, lower = box
    return m[:, video.nearest_table(Hm, h, (upper, lower))][:, :, video.nearest_table(Wm, w, (left, right))]


def restore_box_np(lo, m, src, box):
    """restore_frames(box=): src outside the box, the three PIL lines of restore_np on the sub-image inside it"""
    left, upper, right, lower = box
    out = src.copy()
    out[:, upper:lower, left:right] = restore_np(lo, m, src[:, upper:lower, left:right])
    return out


def test_box_tables_are_pillow():
    from PIL import Image
    differs_from_crop = 0
    for k, ((W, H), size, box) in enumerate(CASES):
        f = frames(2, W, H, seed=k)
        m = (np.random.RandomState(k).rand(2, H, W) < 0.3).astype(np.uint8) * 255
        got, gotm = resize_box_np(f, size, box), nearest_box_np(m, size, box)
        assert got.shape == (2, size[1], size[0], 3) and got.dtype == np.uint8
        for i in range(2):
            ref = np.asarray(Image.fromarray(f[i]).resize(size, box=box))
            assert np.array_equal(got[i], ref), ((W, H), size, box, i, int((got[i] != ref).sum()))
            refm = np.asarray(Image.fromarray(m[i]).resize(size, Image.NEAREST, box=box))
            assert np.array_equal(gotm[i], refm), ((W, H), size, box, i)
            differs_from_crop += int(not np.array_equal(ref, np.asarray(Image.fromarray(f[i]).crop(box).resize(size))))
    # the taps at the box's edge reach into the surrounding image: a test against crop-then-resize would check something else
    (W, H), size, box = CASES[0]
    f = frames(1, W, H, seed=0)[0]
    from_crop = np.asarray(Image.fromarray(f).crop(box).resize(size))
    assert not np.array_equal(resize_box_np(f[None], size, box)[0], from_crop) and differs_from_crop >= len(CASES) // 2


def test_whole_axis_box_is_no_box():
    for n_in, n_out in ((36, 160), (160, 36), (20, 20), (1, 9), (300, 7)):
        for a, b in zip(video.bicubic_tables(n_in, n_out), video.bicubic_tables(n_in, n_out, (0, n_in))):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        a, b = video.nearest_table(n_in, n_out), video.nearest_table(n_in, n_out, (0, n_in))
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # the arrays of the parent commit's formulas, written out: the scale from n_in alone, the centres without an offset
    b, c = video.bicubic_tables(7, 3)
    assert b.tolist() == [[0, 6], [0, 7], [1, 6]] and c.shape == (3, 11) and abs(c.sum(1) - (1 << 22)).max() <= 2
    assert video.nearest_table(7, 3).tolist() == [1, 3, 5]
    # bounds are absolute and clipped to the image, not to the box; ksize follows the box
    b, c = video.bicubic_tables(100, 10, (40, 60))
    assert c.shape[1] == 2 * 4 + 1 and b[0].tolist() == [37, 8] and b[-1].tolist() == [55, 8]
    b, c = video.bicubic_tables(100, 10, (0, 20))
    assert b[0].tolist() == [0, 5]
    for bad in ((-1, 5), (5, 5), (7, 3), (0, 101)):
        with pytest.raises(ValueError):
            video.bicubic_tables(100, 10, bad)
        with pytest.raises(ValueError):
            video.nearest_table(100, 10, bad)


def test_restore_box_restatement_is_pil_on_the_sub_image():
    from PIL import Image
    (w, h), (W, H), box = (36, 20), (160, 90), (17, 9, 130, 71)
    m = masks(h, w, seed=5)
    lo, src = frames(len(m), w, h, seed=6), frames(len(m), W, H, seed=7)
    got = restore_box_np(lo, m, src, box)
    left, upper, right, lower = box
    for i in range(len(m)):
        ref = np.array(Image.fromarray(src[i]))
        up = np.asarray(Image.fromarray(lo[i]).resize((right - left, lower - upper)))
        M = np.asarray(Image.fromarray(m[i] * 255).resize((right - left, lower - upper), Image.NEAREST))
        ref[upper:lower, left:right] = np.where(M[..., None] != 0, up, ref[upper:lower, left:right])
        assert np.array_equal(got[i], ref)
    outside = np.ones((H, W), bool)
    outside[upper:lower, left:right] = False
    assert np.array_equal(got[:, outside], src[:, outside]) and (got[1] != src[1]).any()


G = 8
SIZE = (432, 240)
FRAMES = [(1920, 1080), (432, 240), (300, 200), (500, 200), (433, 1000)]      # larger than, equal to, smaller than size, mixed


def _bboxes(W, H):
    out = [(W // 2, H // 2, W // 2 + 1, H // 2 + 1), (0, 0, W, H)]                       # tiny, as large as the frame
    for bw, bh in ((1, 1), (min(50, W), min(30, H)), (min(300, W), min(31, H)), (max(1, W // 2), max(1, H - 1))):
        out += [(0, 0, bw, bh), (W - bw, 0, W, bh), (0, H - bh, bw, H), (W - bw, H - bh, W, H)]      # flush with each corner
    return out


def test_plan_region_properties():
    w, h = SIZE
    exact = 0
    for W, H in FRAMES:
        for bbox in _bboxes(W, H):
            for context in (0, 0.5, 2):
                left, upper, right, lower = box = video.plan_region(bbox, (W, H), SIZE, context)
                x0, y0, x1, y1 = bbox
                key = ((W, H), bbox, context, box)
                assert all(isinstance(v, int) for v in box), key
                assert 0 <= left < right <= W and 0 <= upper < lower <= H, key                  # inside the frame
                assert left <= x0 and x1 <= right and upper <= y0 and y1 <= lower, key          # contains the hole
                Bw, Bh = right - left, lower - upper
                assert Bw >= min(W, w) and Bh >= min(H, h), key                                 # no upscale the frame did not force
                bw, bh = x1 - x0, y1 - y0
                c = 1 + 2 * Fraction(context)
                s = max(Fraction(1), c * bw / w, c * bh / h, Fraction(bw, w - 2 * G), Fraction(bh, h - 2 * G))
                if Bw < W and Bh < H:
                    # neither axis clamped: Bw / w and Bh / h lie in [s, s + 1 / w) and [s, s + 1 / h): the aspect to one pixel
                    assert abs(Fraction(Bw, w) - Fraction(Bh, h)) < Fraction(1, min(w, h)), key
                    assert s * w <= Bw < s * w + 1 and s * h <= Bh < s * h + 1, key
                    # ... with the context the caller asked for and the guard, in box pixels
                    assert c * bw <= Bw and c * bh <= Bh and bw * w <= Bw * (w - 2 * G) and bh * h <= Bh * (h - 2 * G), key
                if s == 1 and W >= w and H >= h:
                    assert (Bw, Bh) == SIZE, key
                    exact += 1
                if 0 < (x0 + x1 - Bw) // 2 < W - Bw:
                    assert left == (x0 + x1 - Bw) // 2, key                                     # centred where the frame allows
                if 0 < (y0 + y1 - Bh) // 2 < H - Bh:
                    assert upper == (y0 + y1 - Bh) // 2, key
    assert exact > 10


def test_plan_region_by_hand():
    # 200 x 120 hole in a 1080p frame: twice its extent fits 432 x 240, so the box is the model's size, centred on (900, 460)
    assert video.plan_region((800, 400, 1000, 520), (1920, 1080), SIZE) == (684, 340, 1116, 580)
    assert video.plan_region((800, 400, 1000, 520), (1920, 1080), SIZE, context=0) == (684, 340, 1116, 580)
    # the same hole in the corner: the box is pushed inside
    assert video.plan_region((0, 0, 200, 120), (1920, 1080), SIZE) == (0, 0, 432, 240)
    assert video.plan_region((1720, 960, 1920, 1080), (1920, 1080), SIZE) == (1488, 840, 1920, 1080)
    # 600 x 200: the width with its context decides, s = 2 * 600 / 432 = 25 / 9; Bw = 1200, Bh = ceil(666.67) = 667
    assert video.plan_region((500, 300, 1100, 500), (1920, 1080), SIZE) == (200, 66, 1400, 733)
    # context 0: the guard decides, s = 600 / 416 = 75 / 52; Bw = ceil(623.08) = 624, Bh = ceil(346.15) = 347
    assert video.plan_region((500, 300, 1100, 500), (1920, 1080), SIZE, context=0) == (488, 226, 1112, 573)
    # a frame smaller than the model's size is taken whole; a hole as large as the frame too
    assert video.plan_region((100, 80, 140, 100), (300, 200), SIZE) == (0, 0, 300, 200)
    assert video.plan_region((0, 0, 1920, 1080), (1920, 1080), SIZE) == (0, 0, 1920, 1080)
    assert video.plan_region(None, (1920, 1080), SIZE) == (0, 0, 1920, 1080)
    # the context decides: twice the hole's 200 x 120 is the most that fits 432 x 240
    assert video.plan_region((800, 400, 1000, 520), (1920, 1080), SIZE, context=0.25) == (684, 340, 1116, 580)
    assert video.plan_region((800, 400, 1000, 520), (1920, 1080), SIZE, context=0.6)[2:] != (1116, 580)


def test_plan_region_refuses_bad_arguments():
    ok = ((800, 400, 1000, 520), (1920, 1080), SIZE)
    with pytest.raises(ValueError):
        video.plan_region(*ok, context=-0.1)
    with pytest.raises(ValueError):
        video.plan_region(*ok, context=float("nan"))
    for size in ((16, 240), (432, 16), (0, 0)):
        with pytest.raises(ValueError):
            video.plan_region(ok[0], ok[1], size)
    for bbox in ((800, 400, 800, 520), (800, 400, 1000, 1081), (-1, 0, 5, 5), (1, 2, 3), (1.5, 2, 30, 40)):
        with pytest.raises(ValueError):
            video.plan_region(bbox, ok[1], SIZE)
    with pytest.raises(ValueError):
        video.plan_region(None, ok[1], SIZE, context=-1)


def test_region_arguments_are_checked_before_any_device_work():
    f = np.zeros((3, 20, 36, 3), np.uint8)
    m = np.zeros((3, 20, 36), np.uint8)
    cpu = torch.device("cpu")

    def net(x, n):
        raise AssertionError("the model must not be called")

    for region in ("hole", (2, 2, 20, 12)):
        with pytest.raises(ValueError, match="size"):
            video.inpaint_video(net, f, m, device=cpu, region=region)
        with pytest.raises(ValueError, match="size"):
            video.inpaint_video(net, f, m, device=cpu, region=region, restore=True)
    for region in ((2, 2, 37, 12), (2, 2, 20, 21), (-1, 2, 20, 12), (5, 2, 5, 12), (5, 9, 20, 3), (2, 2, 20), (2, 2, 20, 12, 1), "box",
                   (2.5, 2, 20, 12), 7):
        with pytest.raises(ValueError):
            video.inpaint_video(net, f, m, device=cpu, size=(18, 10), region=region)
        if not isinstance(region, str):
            with pytest.raises(ValueError):
                video.resize_frames(f, (18, 10), device=cpu, box=region)
            with pytest.raises(ValueError):
                video.restore_frames(f[:, :10, :18], m[:, :10, :18], f, device=cpu, box=region)
            with pytest.raises(ValueError):
                video.prepare_masks(m, (10, 18), cpu, box=region)
    # a well-formed region gets as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="cuda"):
        video.inpaint_video(net, f, m, device=cpu, size=(18, 10), region=(2, 2, 20, 12))


def test_new_entries_refuse_bad_arguments():
    """host side of e2fgvi_restore_box_u8, e2fgvi_resample_rows_u8 and e2fgvi_hole_bbox: E2FGVI_EINVAL from the arguments alone
    (no launch, so this runs without a GPU; the addresses are never read)"""
    import os
    from e2fgvi_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    L, h, w, H, W = 2, 20, 36, 47, 160
    n_out, n_lo = L * H * W * 3, L * h * w * 3
    base = 1 << 20
    good = dict(lo=base, mask=base + n_lo, src=base + 2 * n_lo, out=base + 2 * n_lo + n_out, L=L, h=h, w=w, H=H, W=W, left=30, upper=5,
                Bw=83, Bh=35, ytab=64, xtab=64, bx=64, cx=64, kx=5, by=64, cy=64, ky=5)
    order = ("lo", "mask", "src", "out", "L", "h", "w", "H", "W", "left", "upper", "Bw", "Bh", "ytab", "xtab", "bx", "cx", "kx", "by",
             "cy", "ky")

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_restore_box_u8(*[a[k] for k in order], None)

    for k in ("lo", "mask", "src", "out", "ytab", "xtab", "bx", "cx", "by", "cy"):
        assert rc(**{k: None}) == -1, k
    for k in ("L", "h", "w", "H", "W", "Bw", "Bh", "kx", "ky"):
        assert rc(**{k: 0}) == -1 and rc(**{k: -3}) == -1, k
    assert rc(left=-1) == -1 and rc(upper=-1) == -1 and b"box" in so.e2fgvi_last_error()
    assert rc(left=78) == -1 and rc(Bw=131) == -1 and rc(upper=13) == -1 and rc(Bh=43) == -1       # one pixel past the frame
    assert rc(left=0x7fffffff) == -1 and rc(Bw=0x7fffffff) == -1                                    # no overflow in the check
    assert rc(out=good["src"]) == -1 and b"overlap" in so.e2fgvi_last_error()
    assert rc(out=good["lo"] + n_lo - 1) == -1

    def rows(**kw):
        a = dict(dict(src=base, dst=base + n_out, L=L, H=H, W=W, n_out=50, row0=3, rows=40, bounds=64, coeffs=64, ksize=9), **kw)
        return so.e2fgvi_resample_rows_u8(*[a[k] for k in ("src", "dst", "L", "H", "W", "n_out", "row0", "rows", "bounds", "coeffs",
                                                           "ksize")], None)

    for k in ("src", "dst", "bounds", "coeffs"):
        assert rows(**{k: None}) == -1, k
    for k in ("L", "H", "W", "n_out", "rows", "ksize"):
        assert rows(**{k: 0}) == -1 and rows(**{k: -2}) == -1, k
    assert rows(row0=-1) == -1 and rows(row0=8) == -1 and rows(rows=45) == -1 and rows(row0=0x7fffffff) == -1
    assert b"rows" in so.e2fgvi_last_error()
    assert so.e2fgvi_hole_bbox(base, 2, 5, 7, None, None) == -1
    assert so.e2fgvi_hole_bbox(None, 2, 5, 7, base, None) == -1
    assert so.e2fgvi_hole_bbox(base, -1, 5, 7, base, None) == -1 and so.e2fgvi_hole_bbox(base, 2, 5, -7, base, None) == -1
    assert so.e2fgvi_abi_version() == 9
