"""The feathered paste-back of video.restore_frames(feather=r) / inpaint_video(restore=True, feather=r), defined in integers.  With
up = BICUBIC(lo) and M = NEAREST(m) at the box's size as in tests/test_video_restore.py, in box-relative pixels and with everything
outside the box counting as 0:

    D(p) = 1 iff some q with |q - p|_inf <= r has M(q) = 1              (M dilated by the (2r+1) x (2r+1) square)
    c(p) = #{q in the box : |q - p|_inf <= r, D(q) = 1},    n(p) = #{q in the box : |q - p|_inf <= r}
    out  = (c * up + (n - c) * src + n // 2) // n  inside the box,      src outside it

``feather_np`` below restates that with cumulative sums; this file pins it against scipy's filters, Pillow and the three guarantees
(r = 0 is the hard paste; a pixel of M gets exactly `up`; a pixel farther than 2r from M is src), and the device tests
(tests/test_gpu_video_feather.py) compare the kernel with it."""
import numpy as np
import pytest
import torch

from e2fgvi_amd import video
from tests.test_video_region import restore_box_np
from tests.test_video_restore import PAIRS, _pass_np, frames, masks, restore_np

RADII = (0, 1, 3, 16)
BOXES = [(0, 0, 72, 40), (88, 50, 160, 90), (10, 7, 150, 85), (40, 30, 76, 50)]        # of a 160 x 90 frame; the last has lo's size


def win_sum(a, r, axis):
    """sum over [i - r, i + r] along axis, zeros outside"""
    n = a.shape[axis]
    p = [(0, 0)] * a.ndim
    p[axis] = (r + 1, r)
    c = np.cumsum(np.pad(a.astype(np.int64), p), axis=axis)
    return np.take(c, np.arange(n) + 2 * r + 1, axis=axis) - np.take(c, np.arange(n), axis=axis)


def feather_parts(lo, m, box_wh, r):
    """(up, M, D, c, n) of the definition for a box of (Bw, Bh): up uint8 [L,Bh,Bw,3], M / D bool and c int64 [L,Bh,Bw], n [1,Bh,Bw]"""
    Bw, Bh = box_wh
    h, w = lo.shape[1:3]
    up = lo
    if Bw != w:
        up = _pass_np(up, Bw, -2)
    if Bh != h:
        up = _pass_np(up, Bh, -3)
    M = m[:, video.nearest_table(h, Bh)][:, :, video.nearest_table(w, Bw)] != 0
    D = win_sum(win_sum(M, r, 2), r, 1) > 0
    c = win_sum(win_sum(D, r, 2), r, 1)
    n = win_sum(win_sum(np.ones((1, Bh, Bw)), r, 2), r, 1)
    return up, M, D, c, n


def feather_np(lo, m, src, r, box=None):
    """the definition on whole videos: lo uint8 [L,h,w,3], m uint8 [L,h,w] of 0 / 1, src uint8 [L,H,W,3] -> uint8 [L,H,W,3]"""
    L, H, W, _ = src.shape
    left, upper, right, lower = box or (0, 0, W, H)
    up, _, _, c, n = feather_parts(lo, m, (right - left, lower - upper), r)
    c, n = c[..., None], n[..., None]
    sub = src[:, upper:lower, left:right].astype(np.int64)
    out = src.copy()
    out[:, upper:lower, left:right] = ((c * up.astype(np.int64) + (n - c) * sub + n // 2) // n).astype(np.uint8)
    return out


def far_from(M, r):
    """bool [L,H,W]: farther than 2r (Chebyshev) from every pixel of M"""
    return win_sum(win_sum(M, 2 * r, 2), 2 * r, 1) == 0


def _video(wh, WH):
    (w, h), (W, H) = wh, WH
    m = masks(h, w, seed=w + 3 * h)
    return frames(len(m), w, h, seed=w * 7 + h), m, frames(len(m), W, H, seed=W * 5 + H + 1)


@pytest.mark.parametrize("r", RADII)
def test_restatement_is_scipy_pillow_and_the_three_guarantees(r):
    from PIL import Image
    from scipy import ndimage
    ramp = 0
    for wh, (W, H) in PAIRS:
        lo, m, src = _video(wh, (W, H))
        got = feather_np(lo, m, src, r)
        assert got.shape == src.shape and got.dtype == np.uint8
        up, M, D, c, n = feather_parts(lo, m, (W, H), r)
        k = 2 * r + 1
        for i in range(len(m)):
            assert np.array_equal(up[i], np.asarray(Image.fromarray(lo[i]).resize((W, H))))
            assert np.array_equal(M[i], np.asarray(Image.fromarray(m[i] * 255).resize((W, H), Image.NEAREST)) != 0)
            assert np.array_equal(D[i], ndimage.maximum_filter(M[i].astype(np.uint8), size=k, mode="constant") != 0)
            assert np.array_equal(c[i], ndimage.convolve(D[i].astype(np.int64), np.ones((k, k), np.int64), mode="constant"))
        assert np.array_equal(n[0], ndimage.convolve(np.ones((H, W), np.int64), np.ones((k, k), np.int64), mode="constant"))
        assert n.max() <= k * k and (c <= n).all() and (c[M] == np.broadcast_to(n, c.shape)[M]).all()
        if r == 0:
            assert np.array_equal(got, restore_np(lo, m, src))                  # today's bytes
        assert np.array_equal(got[M], up[M])                                    # the pasted mask: exactly the pasted byte
        far = far_from(M, r)
        assert np.array_equal(got[far], src[far])                               # beyond the ring: the caller's byte
        assert np.array_equal(got[0], src[0])                                   # the empty mask
        ramp += int(((c > 0) & (c < n)).sum())
    assert (ramp > 0) == (r > 0)


@pytest.mark.parametrize("box", BOXES, ids=str)
def test_restatement_in_a_box_keeps_the_source_outside_and_cuts_the_ramp(box):
    (w, h), (W, H) = (36, 20), (160, 90)
    left, upper, right, lower = box
    lo, m, src = _video((w, h), (W, H))
    outside = np.ones((H, W), bool)
    outside[upper:lower, left:right] = False
    for r in RADII:
        got = feather_np(lo, m, src, r, box)
        assert np.array_equal(got[:, outside], src[:, outside])
        up, M, D, c, n = feather_parts(lo, m, (right - left, lower - upper), r)
        assert (c <= n).all() and n.min() == (min(r, right - left - 1) + 1) * (min(r, lower - upper - 1) + 1)     # a corner of the box
        # the same paste on the cropped source: the box is all the definition sees
        assert np.array_equal(got[:, upper:lower, left:right], feather_np(lo, m, src[:, upper:lower, left:right], r))
        if r == 0:
            assert np.array_equal(got, restore_box_np(lo, m, src, box))
        sub = got[:, upper:lower, left:right]
        assert np.array_equal(sub[M], up[M])
        far = far_from(M, r)
        assert np.array_equal(sub[far], src[:, upper:lower, left:right][far])
        # the full mask: c == n everywhere, so the box holds `up` right up to its edge -- no ramp past the box
        assert np.array_equal(got[1, upper:lower, left:right], up[1])


def test_feather_arguments_are_checked_before_any_device_work():
    f = np.zeros((3, 20, 36, 3), np.uint8)
    m = np.zeros((3, 20, 36), np.uint8)
    cpu = torch.device("cpu")

    def net(x, n):
        raise AssertionError("the model must not be called")

    assert video.FEATHER_MAX == 16
    with pytest.raises(ValueError, match="restore"):
        video.inpaint_video(net, f, m, device=cpu, size=(18, 10), feather=4)
    with pytest.raises(ValueError, match="restore"):
        video.inpaint_video(net, f, m, device=cpu, feather=1)
    for bad in (-1, video.FEATHER_MAX + 1, 2.5, "4", None):
        with pytest.raises(ValueError, match="feather"):
            video.inpaint_video(net, f, m, device=cpu, size=(18, 10), restore=True, feather=bad)
        with pytest.raises(ValueError, match="feather"):
            video.inpaint_video(net, f, m, device=cpu, size=(18, 10), restore=True, region="track", feather=bad)
        with pytest.raises(ValueError, match="feather"):
            video.restore_frames(f, m, f, device=cpu, feather=bad)
    # a well-formed call gets as far as the device check: there is no CPU path
    for kw in ({}, {"region": "hole"}, {"region": "track"}):
        with pytest.raises(RuntimeError, match="cuda"):
            video.inpaint_video(net, f, m, device=cpu, size=(18, 10), restore=True, feather=video.FEATHER_MAX, **kw)


def test_feather_entries_refuse_bad_arguments():
    """host side of e2fgvi_restore_feather_u8 and e2fgvi_restore_feather_blend: their siblings' refusals plus 1 <= feather <= 16,
    E2FGVI_EINVAL from the arguments alone (no launch, so this runs without a GPU; the addresses are never read)"""
    import os
    from e2fgvi_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    n, L, h, w, H, W = 2, 4, 20, 36, 47, 160
    n_src, n_lo = L * H * W * 3, n * h * w * 3
    base = 1 << 20
    tabs = dict(ytab=256, xtab=256, bx=256, cx=256, kx=5, by=256, cy=256, ky=5)
    tab_order = ("ytab", "xtab", "bx", "cx", "kx", "by", "cy", "ky", "feather")

    good_u8 = dict(tabs, lo=base, mask=base + L * h * w * 3, src=base + (1 << 21), out=base + (1 << 22), L=L, h=h, w=w, H=H, W=W, left=30,
                   upper=5, Bw=83, Bh=35, feather=4)
    order_u8 = ("lo", "mask", "src", "out", "L", "h", "w", "H", "W", "left", "upper", "Bw", "Bh") + tab_order

    def u8(**kw):
        a = dict(good_u8, **kw)
        return so.e2fgvi_restore_feather_u8(*[a[k] for k in order_u8], None)

    good_bl = dict(tabs, lo=base, mask=base + n_lo, src=base + 2 * n_lo, ids=64, first=128, acc=base + (1 << 22), n=n, L=L, h=h, w=w, H=H,
                   W=W, left=30, upper=5, Bw=83, Bh=35, tl=30, tu=5, Tw=83, Th=35, feather=4)
    order_bl = ("lo", "mask", "src", "ids", "first", "acc", "n", "L", "h", "w", "H", "W", "left", "upper", "Bw", "Bh", "tl", "tu", "Tw",
                "Th") + tab_order

    def bl(**kw):
        a = dict(good_bl, **kw)
        return so.e2fgvi_restore_feather_blend(*[a[k] for k in order_bl], None)

    for rc, ptrs, ints in ((u8, ("lo", "mask", "src", "out"), ("L", "h", "w", "H", "W", "Bw", "Bh", "kx", "ky")),
                           (bl, ("lo", "mask", "src", "ids", "first", "acc"), ("n", "L", "h", "w", "H", "W", "Bw", "Bh", "Tw", "Th", "kx",
                                                                               "ky"))):
        for k in ptrs + ("ytab", "xtab", "bx", "cx", "by", "cy"):
            assert rc(**{k: None}) == -1, (rc.__name__, k)
        for k in ints:
            assert rc(**{k: 0}) == -1 and rc(**{k: -3}) == -1, (rc.__name__, k)
        for bad in (0, 17, -1, 0x7fffffff):
            assert rc(feather=bad) == -1 and b"feather" in so.e2fgvi_last_error(), (rc.__name__, bad)
    # the box inside the frame; out / acc must not overlap an input
    assert u8(left=-1) == -1 and u8(left=78) == -1 and u8(Bh=43) == -1 and b"box" in so.e2fgvi_last_error()
    assert u8(out=good_u8["src"]) == -1 and b"overlap" in so.e2fgvi_last_error()
    assert u8(out=good_u8["src"] + n_src - 1) == -1 and u8(out=good_u8["lo"] - n_src + 1) == -1
    assert bl(left=-1, tl=-1) == -1 and bl(Bw=131, Tw=131) == -1 and b"box" in so.e2fgvi_last_error()
    assert bl(tl=31) == -1 and b"touched" in so.e2fgvi_last_error() and bl(Tw=82) == -1 and bl(tu=0, Th=48) == -1
    assert bl(acc=good_bl["src"]) == -1 and b"overlap" in so.e2fgvi_last_error()
    assert bl(acc=good_bl["src"] + n_src - 4) == -1 and bl(ids=good_bl["acc"] + 8) == -1
    assert bl(acc=good_bl["acc"] + 2) == -1 and b"aligned" in so.e2fgvi_last_error()
    assert so.e2fgvi_abi_version() == 9


def test_the_paste_back_kernels_use_no_scratch():
    """the build's own check (build.verify_no_scratch) over the four instantiations of restore_u8_kernel: hard edge and feathered,
    bytes and accumulator -- no private segment, no spilled vector register"""
    import os
    from e2fgvi_amd import build
    if not (os.path.exists(build.OBJDUMP) and os.path.exists(os.path.join(build.CSRC, "build", "video.o"))):
        pytest.skip("library not built here (python -m e2fgvi_amd.build)")
    assert build.verify_no_scratch(obj="video.o", marker="restore_u8_kernel", what="paste-back") == 4
    with pytest.raises(RuntimeError, match="no paste-back instantiation"):
        build.verify_no_scratch(obj="video.o", marker="restore_u9_kernel", what="paste-back")
