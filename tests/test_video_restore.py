"""The paste-back of video.restore_frames / inpaint_video(restore=True), defined by three PIL lines per frame:

    up  = Image.fromarray(lo).resize((W, H))                          # BICUBIC, Pillow's two passes: width, then height
    M   = Image.fromarray(m * 255).resize((W, H), Image.NEAREST)
    out = where(M != 0, up, src)

``restore_np`` below restates them around video.bicubic_tables / video.nearest_table with the two-pass integer arithmetic; this
file pins that restatement against Pillow, and the device tests (tests/test_gpu_video_restore.py) compare the kernel with it."""
import numpy as np
import pytest
import torch

from e2fgvi_amd import video

# (w, h) -> (W, H), PIL order: both axes up, by one pixel, one axis only, none, one axis shrinking, one-pixel and extreme shapes
PAIRS = [((36, 20), (160, 90)), ((36, 20), (37, 21)), ((36, 20), (36, 47)), ((36, 20), (83, 20)), ((36, 20), (36, 20)),
         ((36, 20), (30, 47)), ((1, 1), (9, 4)), ((7, 5), (300, 3))]
_rng = np.random.RandomState(23)
PAIRS = PAIRS + [(tuple(int(v) for v in _rng.randint(1, 60, 2)), tuple(int(v) for v in _rng.randint(1, 200, 2))) for _ in range(5)]


def _pass_np(a, n_out, axis):
    """one pass of Pillow's 8-bit resample along `axis` of uint8 [..., H, W, 3] (-3: rows, -2: columns), int32 like Pillow"""
    n_in = a.shape[axis]
    bounds, coeffs = video.bicubic_tables(n_in, n_out)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    acc = np.full((n_out,) + a.shape[1:], 1 << 21, np.int64)
    for j in range(coeffs.shape[1]):
        idx = np.minimum(bounds[:, 0] + j, n_in - 1)            # coefficients past a row's tap count are zero
        acc += a[idx] * coeffs[:, j].reshape((n_out,) + (1,) * (a.ndim - 1))
    assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31
    return np.moveaxis(np.clip(acc >> 22, 0, 255).astype(np.uint8), 0, axis)


def restore_np(lo, m, src):
    """the definition on whole videos: lo uint8 [L,h,w,3], m uint8 [L,h,w] of 0 / 1, src uint8 [L,H,W,3] -> uint8 [L,H,W,3]"""
    (h, w), (H, W) = lo.shape[1:3], src.shape[1:3]
    up = lo
    if W != w:
        up = _pass_np(up, W, -2)
    if H != h:
        up = _pass_np(up, H, -3)
    M = m[:, video.nearest_table(h, H)][:, :, video.nearest_table(w, W)]
    return np.where(M[..., None] != 0, up, src)


def frames(L, W, H, seed):
    """smooth gradients (no clamping) plus noise patches (large negative taps: the uint8 clamps of both passes)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.empty((L, H, W, 3), np.uint8)
    for i in range(L):
        for c in range(3):
            f[i, :, :, c] = (xx * (3 + c) + yy * (5 - c) + 40 * i) % 256
        f[i, : (H + 1) // 2, W // 3:] = rng.randint(0, 256, f[i, : (H + 1) // 2, W // 3:].shape)
    return f


def masks(h, w, seed):
    """one mask per kind: empty, full, the two corner pixels, a random 30 % mask, a one-pixel-wide diagonal"""
    rng = np.random.RandomState(seed)
    m = np.zeros((6, h, w), np.uint8)
    m[1] = 1
    m[2, 0, 0] = 1
    m[3, h - 1, w - 1] = 1
    m[4] = rng.rand(h, w) < 0.3
    for i in range(max(h, w)):
        m[5, min(i, h - 1), min(i, w - 1)] = 1
    return m


def _pil_restore(lo, m, src):
    from PIL import Image
    H, W = src.shape[:2]
    up = np.asarray(Image.fromarray(lo).resize((W, H)))
    M = np.asarray(Image.fromarray(m * 255).resize((W, H), Image.NEAREST))
    return np.where(M[..., None] != 0, up, src)


def test_restatement_is_the_three_pil_lines():
    for (w, h), (W, H) in PAIRS:
        m = masks(h, w, seed=w + 3 * h)
        lo = frames(len(m), w, h, seed=w * 7 + h)
        src = frames(len(m), W, H, seed=W * 5 + H + 1)
        got = restore_np(lo, m, src)
        assert got.shape == src.shape and got.dtype == np.uint8
        for i in range(len(m)):
            ref = _pil_restore(lo[i], m[i], src[i])
            assert np.array_equal(got[i], ref), ((w, h), (W, H), i, int((got[i] != ref).sum()))
        assert np.array_equal(got[0], src[0])                                       # empty mask: the source, untouched
        if m[4].any() and (W, H) != (w, h):
            assert (got[1] != src[1]).any()


def test_restore_needs_size_and_bytes():
    """both refusals of inpaint_video(restore=True) come before anything touches a device"""
    f = np.zeros((3, 20, 36, 3), np.uint8)
    m = np.zeros((3, 20, 36), np.uint8)

    def net(x, n):
        raise AssertionError("the model must not be called")

    with pytest.raises(ValueError, match="size"):
        video.inpaint_video(net, f, m, device=torch.device("cpu"), restore=True)
    with pytest.raises(ValueError, match="keep_float"):
        video.inpaint_video(net, f, m, device=torch.device("cpu"), size=(18, 10), keep_float=True, restore=True)


def test_restore_frames_refuses_mismatched_videos():
    """shape errors are raised from the shapes alone, before any upload"""
    lo, m = np.zeros((3, 20, 36, 3), np.uint8), np.zeros((3, 20, 36), np.uint8)
    with pytest.raises(ValueError):
        video.restore_frames(lo, m, np.zeros((4, 40, 72, 3), np.uint8), device=torch.device("cpu"))       # L differs
    with pytest.raises(ValueError):
        video.restore_frames(lo, m[:2], np.zeros((3, 40, 72, 3), np.uint8), device=torch.device("cpu"))
    with pytest.raises(ValueError):
        video.restore_frames(lo[..., 0], m, np.zeros((3, 40, 72, 3), np.uint8), device=torch.device("cpu"))  # not [L,.,.,3]
    with pytest.raises(ValueError):
        video.restore_frames(lo, m[:, :10], np.zeros((3, 40, 72, 3), np.uint8), device=torch.device("cpu"))


def test_restore_u8_abi_refuses_bad_arguments():
    """host side of e2fgvi_restore_u8: null pointers, non-positive sizes, ksize < 1 and an `out` that overlaps src, lo or the mask
    are E2FGVI_EINVAL, decided from the arguments alone (no launch, so this runs without a GPU; the addresses are never read)"""
    import os
    from e2fgvi_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    L, h, w, H, W = 2, 20, 36, 47, 83
    n_out, n_lo = L * H * W * 3, L * h * w * 3
    base = 1 << 20
    good = dict(lo=base, mask=base + n_lo, src=base + 2 * n_lo, out=base + 2 * n_lo + n_out, L=L, h=h, w=w, H=H, W=W,
                ytab=64, xtab=64, bx=64, cx=64, kx=5, by=64, cy=64, ky=5)
    order = ("lo", "mask", "src", "out", "L", "h", "w", "H", "W", "ytab", "xtab", "bx", "cx", "kx", "by", "cy", "ky")

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_restore_u8(*[a[k] for k in order], None)

    for k in ("lo", "mask", "src", "out", "ytab", "xtab", "bx", "cx", "by", "cy"):
        assert rc(**{k: None}) == -1, k
    for k in ("L", "h", "w", "H", "W", "kx", "ky"):
        assert rc(**{k: 0}) == -1 and rc(**{k: -3}) == -1, k
    assert rc(out=good["src"]) == -1 and b"overlap" in so.e2fgvi_last_error()
    assert rc(out=good["src"] + n_out - 1) == -1                    # the first byte of out is the last of src
    assert rc(out=good["src"] - n_out + 1) == -1                    # the last byte of out is the first of src (and inside lo)
    assert rc(out=good["lo"] + n_lo - 1) == -1                      # ... the last of lo
    assert rc(out=good["mask"] - n_out + 1, lo=base + (1 << 24)) == -1      # the last byte of out is the first of the mask
    assert lib.load().e2fgvi_abi_version() == 9
