"""The 4:2:0 pixel formats on the device: ops.yuv420_to_rgb / ops.rgb_to_yuv420 (csrc/yuv.hip) against the numpy restatement of
tests/yuv_cases.py, and inpaint_video(pixel_format=) against the same call on the decoded frames, encoded by the paste form.  Every
comparison is torch.equal / np.array_equal: no tolerance and no exempted element."""
import numpy as np
import pytest
import torch

from e2fgvi_amd import ops, video
from tests import yuv_cases as Y
from tests.test_gpu_video_overlay import _up
from tests.test_gpu_video_restore import _stand_in_model

pytestmark = pytest.mark.gpu

# (L, H, W): the smallest frame, rows narrower than a strip of 8 pixels, one chroma row and one more than a thread's four, strips that
# end 2, 4 and 6 pixels into the last one, more than one workgroup (256 threads: 257 strips in one row; 3 x 8 x 14 strips); none of
# these widths divides by 8, so all of them take the byte-wise instantiation.  WIDE: widths that do, which take the 8-byte
# instantiation when the base is aligned (shift 0) and the byte-wise one when it is not -- one strip, several, two workgroups.
SHAPES = [(1, 2, 2), (2, 2, 6), (3, 4, 2), (2, 6, 10), (2, 34, 66), (1, 66, 130), (3, 60, 108), (1, 2, 2050)]
WIDE = [(2, 2, 8), (2, 10, 24), (3, 60, 104)]
PAIRS = [("bt709", False), ("bt601", True)]


def _coef(matrix, full):
    dec, enc = video.yuv_coefficients(matrix, full)
    yo = 0 if full else 16
    return dec, enc, yo


def _shifts(W, i):
    """how far the base is moved off an allocation's start: every case of a wide shape runs aligned and not, the others rotate 0 - 3"""
    return (0, 1 + i % 3) if W % 8 == 0 else (i % 4,)


@pytest.mark.parametrize("L,H,W", SHAPES + WIDE, ids=str)
def test_decode_is_the_restatement(dev, L, H, W):
    i = 0
    for layout in Y.LAYOUTS:
        for kind in Y.CONTENTS:
            x = Y.frames(kind, L, H, W, layout)
            for chroma in Y.CHROMAS:
                for matrix, full in PAIRS:
                    dec, _, yo = _coef(matrix, full)
                    want = torch.from_numpy(Y.decode_np(x, layout, chroma, dec, yo))
                    for shift in _shifts(W, i):
                        got = ops.yuv420_to_rgb(_up(x, dev, shift), layout, chroma, dec + (yo,))
                        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (L, H, W, 3)
                        assert torch.equal(got.cpu(), want), (layout, kind, chroma, matrix, full, shift, int((got.cpu() != want).sum()))
                    i += 1


@pytest.mark.parametrize("matrix,full,layout,chroma", [PAIRS[0] + ("nv12", "nearest"), PAIRS[1] + ("i420", "left")], ids=str)
def test_decode_of_every_triple_is_the_restatement(dev, matrix, full, layout, chroma):
    """the 4096 x 4096 frame of the CPU test, which is within one level of the float formula there; once with "left", where the
    chroma steps between the blocks meet every luma value"""
    dec, _, yo = _coef(matrix, full)
    x = Y.all_triples_yuv(layout)
    got = ops.yuv420_to_rgb(_up(x.copy(), dev), layout, chroma, dec + (yo,)).cpu()     # (the shared frame is read-only)
    assert torch.equal(got, torch.from_numpy(Y.decode_np(x, layout, chroma, dec, yo)))


@pytest.mark.parametrize("L,H,W", SHAPES + WIDE, ids=str)
def test_encode_is_the_restatement(dev, L, H, W):
    i = 0
    for kind in Y.CONTENTS:
        rgb = Y.rgb_frames(kind, L, H, W)
        for layout in Y.LAYOUTS:
            for matrix, full in PAIRS:
                _, enc, yo = _coef(matrix, full)
                want = torch.from_numpy(Y.encode_np(rgb, layout, enc, yo))
                for shift in _shifts(W, i):
                    got = ops.rgb_to_yuv420(_up(rgb, dev, shift), layout, enc + (yo,))
                    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (L, H // 2 * 3, W)
                    assert torch.equal(got.cpu(), want), (kind, layout, matrix, full, shift, int((got.cpu() != want).sum()))
                i += 1


def test_encode_of_every_triple_is_the_restatement(dev):
    """every (R, G, B) once in luma; the chroma of the frame's 2x2 blocks, whose sums step through B in fours and G in the rows"""
    rgb = Y.all_triples_rgb()
    d = _up(rgb.copy(), dev)
    for (matrix, full), layout in zip(PAIRS, Y.LAYOUTS):
        _, enc, yo = _coef(matrix, full)
        assert torch.equal(ops.rgb_to_yuv420(d, layout, enc + (yo,)).cpu(), torch.from_numpy(Y.encode_np(rgb, layout, enc, yo)))


def _edits(like_rgb):
    """like_rgb changed at: no pixel, one pixel in each corner, one pixel of every block, a whole frame of three, one channel of one
    pixel by one level"""
    L, H, W, _ = like_rgb.shape
    out = {"none": like_rgb.copy()}
    a = like_rgb.copy()
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        a[:, y, x] ^= 0xFF
    out["corners"] = a
    a = like_rgb.copy()
    by, bx = np.meshgrid(np.arange(H // 2), np.arange(W // 2), indexing="ij")
    a[:, 2 * by + (by + bx) % 2, 2 * bx + (by + 2 * bx) // 2 % 2] ^= 0x55
    out["every block"] = a
    a = like_rgb.copy()
    a[L // 2] = 255 - a[L // 2]
    out["a frame"] = a
    a = like_rgb.copy()
    a[L - 1, H // 2, W // 2, 1] = a[L - 1, H // 2, W // 2, 1] + 1 if a[L - 1, H // 2, W // 2, 1] < 255 else 254
    out["one level"] = a
    return out


@pytest.mark.parametrize("L,H,W", [(3, 2, 2), (3, 6, 10), (3, 34, 66), (3, 10, 24), (3, 60, 104)], ids=str)
def test_paste_encode_is_the_restatement(dev, L, H, W):
    i = 0
    for layout in Y.LAYOUTS:
        for (matrix, full), chroma in zip(PAIRS, Y.CHROMAS):
            dec, enc, yo = _coef(matrix, full)
            like = Y.frames("random", L, H, W, layout, seed=1)
            like_rgb = Y.decode_np(like, layout, chroma, dec, yo)
            for what, rgb in _edits(like_rgb).items():
                want = Y.encode_paste_np(rgb, like_rgb, like, layout, enc, yo)
                if what == "none":
                    assert np.array_equal(want, like)
                else:
                    assert not np.array_equal(want, like)
                for shift in _shifts(W, i):
                    got = ops.rgb_to_yuv420(_up(rgb, dev, shift), layout, enc + (yo,), like=_up(like, dev, shift),
                                            like_rgb=_up(like_rgb, dev, shift))
                    assert torch.equal(got.cpu(), torch.from_numpy(want)), (layout, matrix, what, shift)
                i += 1


def test_both_layouts_give_the_same_planes(dev):
    p = Y.planes("random", 2, 34, 66)
    dec, enc, yo = _coef("bt709", False)
    rgb = [ops.yuv420_to_rgb(_up(Y.join(*p, layout), dev), layout, "left", dec + (yo,)) for layout in Y.LAYOUTS]
    assert torch.equal(rgb[0], rgb[1])
    back = [Y.split(ops.rgb_to_yuv420(rgb[0], layout, enc + (yo,)).cpu().numpy(), layout) for layout in Y.LAYOUTS]
    assert all(np.array_equal(a, b) for a, b in zip(*back))
    # and through the public pair: numpy in, numpy out; a device tensor comes back as one
    x = Y.join(*p, "i420")
    r = video.yuv420_to_rgb(x, "i420", dev)
    assert isinstance(r, np.ndarray) and np.array_equal(r, rgb[0].cpu().numpy())
    rd = video.yuv420_to_rgb(torch.from_numpy(x).to(dev), video.yuv_format("i420"))
    assert rd.is_cuda and torch.equal(rd, rgb[0])
    assert np.array_equal(video.rgb_to_yuv420(r, "i420", dev, like=x), x)
    assert torch.equal(video.rgb_to_yuv420(rd, "i420", like=torch.from_numpy(x).to(dev)).cpu(), torch.from_numpy(x))


def test_wrappers_check_their_arguments(dev):
    dec, enc, yo = _coef("bt709", False)
    x = torch.zeros((2, 6, 8), dtype=torch.uint8, device=dev)
    rgb = torch.zeros((2, 4, 8, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError):
        ops.yuv420_to_rgb(x.cpu(), "nv12", "left", dec + (yo,))
    with pytest.raises(TypeError):
        ops.rgb_to_yuv420(rgb.float(), "nv12", enc + (yo,))
    for bad in (dict(layout="nv21"), dict(chroma="mid"), dict(coef=dec)):
        kw = dict(layout="nv12", chroma="left", coef=dec + (yo,))
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.yuv420_to_rgb(x, **kw)
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb(x[:, :, :7].contiguous(), "nv12", "left", dec + (yo,))
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420(rgb, "nv12", enc + (yo,), like=x)
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420(rgb, "nv12", enc + (yo,), like=x[:1], like_rgb=rgb)
    assert tuple(ops.yuv420_to_rgb(x[:0], "nv12", "left", dec + (yo,)).shape) == (0, 4, 8, 3)
    assert tuple(ops.rgb_to_yuv420(rgb[:0], "i420", enc + (yo,)).shape) == (0, 6, 8)


def _video(L, H, W, layout, holes, seed=3):
    """smooth moving content as YUV frames and masks [L,H,W] with the given (frames, box) holes"""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rgb = np.stack([np.stack([(yy * 2 + xx + 5 * l) % 256, (yy + 3 * xx + 3 * l) % 256, (2 * yy + 2 * xx + 7 * l) % 256], -1)
                    for l in range(L)]).astype(np.uint8)
    rgb ^= rng.randint(0, 8, rgb.shape).astype(np.uint8)
    _, enc = video.yuv_coefficients("bt709", False)
    x = Y.encode_np(rgb, layout, enc, 16)
    m = np.zeros((L, H, W), np.uint8)
    for fr, (left, upper, right, lower) in holes:
        m[fr, upper:lower, left:right] = 255
    return x, m


CASES = {
    "plain": (60, 108, dict(), [(slice(None), (40, 20, 60, 35))]),
    "size restore": (120, 216, dict(size=(108, 60), restore=True), [(slice(None), (80, 40, 120, 70))]),
    "holes": (120, 216, dict(size=(108, 60), restore=True, region="holes"), [(slice(None), (6, 6, 30, 22)), (slice(None), (170, 90, 206, 112))]),
    "feather": (120, 216, dict(size=(108, 60), restore=True, feather=4), [(slice(None), (80, 40, 120, 70))]),
    "track": (120, 216, dict(size=(108, 60), restore=True, region="track"), [(slice(0, 6), (20, 20, 50, 44)), (slice(6, 12), (150, 70, 180, 96))]),
    "size": (120, 216, dict(size=(108, 60)), [(slice(None), (80, 40, 120, 70))]),
    "in flight": (120, 216, dict(size=(108, 60), restore=True, in_flight=2), [(slice(None), (80, 40, 120, 70))]),
}


@pytest.mark.parametrize("case", list(CASES), ids=str)
def test_inpaint_video_in_yuv_is_the_rgb_call_between_the_conversions(dev, case):
    H, W, kw, holes = CASES[case]
    L = 12
    fmt = video.yuv_format("i420" if case in ("holes", "size") else "nv12", "bt601" if case == "feather" else "bt709",
                           chroma="nearest" if case == "track" else "left")
    x, m = _video(L, H, W, fmt.layout, holes)
    net = lambda t, n: (_stand_in_model(t.cpu(), n)[0].to(dev), None)
    got = video.inpaint_video(net, x, m, device=dev, pixel_format=fmt, **kw)
    rgb = video.inpaint_video(net, video.yuv420_to_rgb(x, fmt, dev), m, device=dev, **kw)
    pasted = "restore" in kw or "size" not in kw
    want = video.rgb_to_yuv420(rgb, fmt, dev, like=x if pasted else None)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == ((L, H // 2 * 3, W) if pasted else (L, 90, 108))
    assert np.array_equal(got, want), int((got != want).sum())
    if pasted:
        # the caller's bytes wherever the driver changed nothing within the 2x2 block; and it did change something
        changed = (rgb != video.yuv420_to_rgb(x, fmt, dev)).any(-1)
        block = changed.reshape(L, H // 2, 2, W // 2, 2).any((2, 4))
        for g, s, keep in zip(Y.split(got, fmt.layout), Y.split(x, fmt.layout), (~changed, ~block, ~block)):
            assert np.array_equal(g[keep], s[keep])
        assert changed.any() and not changed.all()
    # a layout string is that layout with the defaults; a device tensor of frames is left as it was
    if case == "plain":
        xd = torch.from_numpy(x).to(dev)
        assert np.array_equal(video.inpaint_video(net, xd, m, device=dev, pixel_format="nv12"), got)
        assert torch.equal(xd.cpu(), torch.from_numpy(x))


def test_without_a_hole_every_byte_is_the_callers(dev):
    def net(t, n):
        return _stand_in_model(t.cpu(), n)[0].to(dev), None
    for H, W, kw in ((60, 108, dict()), (120, 216, dict(size=(108, 60), restore=True))):
        for layout in Y.LAYOUTS:
            x = Y.frames("random", 12, H, W, layout)
            got = video.inpaint_video(net, x, np.zeros((12, H, W), np.uint8), device=dev, pixel_format=layout, **kw)
            assert np.array_equal(got, x)


def test_a_hole_in_three_frames_leaves_the_other_frames_bytes(dev):
    net = lambda t, n: (_stand_in_model(t.cpu(), n)[0].to(dev), None)
    for H, W, kw, box in ((60, 108, dict(), (40, 20, 60, 35)), (120, 216, dict(size=(108, 60), restore=True), (80, 40, 120, 70))):
        x, m = _video(12, H, W, "nv12", [(slice(3, 6), box)])
        got = video.inpaint_video(net, x, m, device=dev, pixel_format="nv12", **kw)
        assert np.array_equal(got[:3], x[:3]) and np.array_equal(got[6:], x[6:])
        assert all((got[l] != x[l]).any() for l in (3, 4, 5))
