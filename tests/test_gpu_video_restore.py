"""video.restore_frames / ops.restore_u8 (csrc/video.hip restore_u8_kernel) and inpaint_video(restore=True) on the device, against
the numpy restatement that tests/test_video_restore.py pins to Pillow.  Every comparison is bit-exact."""
import importlib
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import ops, video
from tests.test_video_restore import PAIRS, frames, masks, restore_np

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tennis25.npz")

# the kernel's tile and LDS budget (csrc/video.hip: RT_W, RT_H, RT_ROWS, RT_PATCH)
RT_W, RT_H, RT_ROWS, RT_PATCH = 128, 8, 24, 8192


def _staged_tiles(h, w, H, W):
    """per output tile, the kernel's own choice: True where the lo patch of the tile's taps fits the LDS budget
    (pr <= RT_ROWS and pr * pc * 3 <= RT_PATCH, pr / pc = rows / columns between the tile's first and last tap)"""
    def spans(n_in, n_out, tile):
        if n_in == n_out:
            first, cnt = np.arange(n_out), np.ones(n_out, np.int64)
        else:
            b, _ = video.bicubic_tables(n_in, n_out)
            first, cnt = b[:, 0].astype(np.int64), b[:, 1].astype(np.int64)
        return [int((first[o:o + tile] + cnt[o:o + tile]).max() - first[o:o + tile].min()) for o in range(0, n_out, tile)]
    return np.array([[pr <= RT_ROWS and pr * pc * 3 <= RT_PATCH for pc in spans(w, W, RT_W)] for pr in spans(h, H, RT_H)])


def _check(dev, wh, WH, seed):
    (w, h), (W, H) = wh, WH
    m = masks(h, w, seed)
    L = 3
    for k in range(0, len(m), L):                                   # L = 3: two launches cover the six mask kinds
        lo = frames(L, w, h, seed + k)
        src = frames(L, W, H, seed + k + 50)
        got = video.restore_frames(lo, m[k:k + L], src, dev)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (L, H, W, 3)
        ref = restore_np(lo, m[k:k + L], src)
        got = got.cpu().numpy()
        for i in range(L):
            assert np.array_equal(got[i], ref[i]), (wh, WH, k + i, int((got[i] != ref[i]).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("wh,WH", PAIRS + [((108, 60), (250, 131)), ((108, 60), (100, 75)), ((60, 34), (300, 170))])
def test_restore_frames_is_the_restatement(dev, wh, WH):
    """every size pair of the CPU test, a 750-byte row with sizes that are no multiple of the tile, the 432x240 -> 400x300 case
    in small (one axis shrinks), and more than one tile along both axes; per pair the six mask kinds: empty (every tile copied),
    full, one pixel in the first / the last tile corner, random 30 %, a one-pixel diagonal (tiles with and without a hole side by
    side).  All of them fit the LDS budget in every tile -- the staged path -- but one of the random pairs, whose 26 rows go to 7."""
    (w, h), (W, H) = wh, WH
    assert _staged_tiles(h, w, H, W).all() == ((wh, WH) != ((27, 26), (180, 7)))
    _check(dev, wh, WH, seed=w + 3 * h + 5 * W + 7 * H)


@pytest.mark.gpu
@pytest.mark.parametrize("wh,WH", [((400, 300), (90, 47)), ((300, 200), (310, 23))])
def test_restore_frames_direct_path(dev, wh, WH):
    """strong shrinking: the rows (and, for the first pair, the bytes) a tile's taps reach exceed the LDS budget in EVERY tile,
    so every tile with a hole pixel recomputes its horizontal values from global memory; the second pair shrinks rows only while
    the columns grow (three tiles across)"""
    (w, h), (W, H) = wh, WH
    assert not _staged_tiles(h, w, H, W).any()
    _check(dev, wh, WH, seed=w + H)


@pytest.mark.gpu
def test_restore_same_size_is_where(dev):
    f = frames(6, 140, 33, 1)
    src = frames(6, 140, 33, 2)
    m = masks(33, 140, 3)
    got = video.restore_frames(torch.from_numpy(f).to(dev), torch.from_numpy(m).to(dev), src).cpu().numpy()
    assert np.array_equal(got, np.where(m[..., None] != 0, f, src))


@pytest.mark.gpu
def test_restore_checks_its_arguments(dev):
    """aliasing, dtypes, devices and shapes are refused before a launch"""
    from e2fgvi_amd.lib import HipError
    (w, h), (W, H) = (36, 20), (83, 47)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lo, m, src = t(frames(2, w, h, 1)), t(masks(h, w, 2)[4:6]), t(frames(2, W, H, 3))
    tabs = [t(video.nearest_table(h, H)), t(video.nearest_table(w, W))] + [t(x) for x in video.bicubic_tables(w, W)] \
        + [t(x) for x in video.bicubic_tables(h, H)]
    ref = restore_np(lo.cpu().numpy(), m.cpu().numpy(), src.cpu().numpy())
    out = torch.empty_like(src)
    assert ops.restore_u8(lo, m, src, *tabs, out=out) is out and np.array_equal(out.cpu().numpy(), ref)
    keep = src.clone()
    with pytest.raises(HipError, match="overlap"):
        ops.restore_u8(lo, m, src, *tabs, out=src)                      # out aliases src
    big = torch.empty(src.numel() + lo.numel(), dtype=torch.uint8, device=dev)
    lo2 = big[src.numel() - 1:src.numel() - 1 + lo.numel()].view(lo.shape).copy_(lo)
    with pytest.raises(HipError, match="overlap"):
        ops.restore_u8(lo2, m, src, *tabs, out=big[: src.numel()].view(src.shape))     # the last byte of out is the first of lo
    assert torch.equal(src, keep)
    with pytest.raises(TypeError):
        ops.restore_u8(lo.float(), m, src, *tabs)
    with pytest.raises(TypeError):
        ops.restore_u8(lo, m.bool(), src, *tabs)
    with pytest.raises(TypeError):
        ops.restore_u8(lo, m, src, tabs[0].long(), *tabs[1:])
    with pytest.raises(TypeError):
        ops.restore_u8(lo, m, src.cpu(), *tabs)
    with pytest.raises(ValueError):
        ops.restore_u8(lo[:1], m, src, *tabs)                           # L differs
    with pytest.raises(ValueError):
        ops.restore_u8(lo, m, src, tabs[1], tabs[0], *tabs[2:])         # ytab / xtab swapped
    with pytest.raises(ValueError):
        ops.restore_u8(lo, m, src, tabs[0], tabs[1], tabs[4], tabs[5], tabs[2], tabs[3])    # x / y taps swapped
    with pytest.raises(ValueError):
        video.restore_frames(lo, m, src[:1])
    with pytest.raises(ValueError):
        video.restore_frames(lo, m[:, :, :5], src)


def _toy_video(L, h, w, seed):
    rng = np.random.RandomState(seed)
    f = frames(L, w, h, seed)
    m = np.zeros((L, h, w), np.uint8)
    for i in range(L):
        m[i, h // 4 + i % 3:h // 2 + i % 3, w // 4 + i:w // 2 + i] = rng.randint(1, 256)
    return f, m


def _stand_in_model(x, n_local):
    # deterministic, batch-free stand-in with the InpaintGenerator output convention, evaluated on the CPU
    b, t, c, H, W = x.shape
    y = torch.tanh(x.reshape(b * t, c, H, W) * 0.7 + 0.1 * x.mean(dim=(1, 2, 3, 4)).view(1, 1, 1, 1))
    return y, None


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{"dilate": True}, {"dilate": False}, {"in_flight": 2}, {"batch_windows": 2}], ids=str)
def test_inpaint_video_restore(dev, kw):
    """inpaint_video(size, restore=True) == the restatement applied to the same call without restore, the masks the driver
    used (dilated or not) and the caller's frames; a device tensor of frames is left as it was"""
    L, size = 7, (108, 60)
    f, m = _toy_video(L, 131, 250, seed=4)
    net = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    lo = video.inpaint_video(net, f, m, device=dev, size=size, **kw)
    m01 = video.prepare_masks(m, (size[1], size[0]), dev, kw.get("dilate", True)).cpu().numpy()
    ref = restore_np(lo, m01, f)
    fd = torch.from_numpy(f).to(dev)
    out = video.inpaint_video(net, fd, m, device=dev, size=size, restore=True, **kw)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == f.shape
    assert np.array_equal(out, ref), int((out != ref).sum())
    assert np.array_equal(fd.cpu().numpy(), f)
    assert (out != f).any() and np.array_equal(video.inpaint_video(net, f, m, device=dev, size=size, restore=True, **kw), ref)


@pytest.mark.gpu
def test_e2fgvi_restores_a_larger_video(dev):
    """the fixed-size e2fgvi model on six 864x480 frames (the tennis clip, PIL-upscaled): restore=True returns 864x480 frames
    that are the restatement of the 432x240 result, with and without reuse, and the input outside the scaled-up hole"""
    from PIL import Image
    from e2fgvi_amd.synth import synth_state_dict
    z = np.load(GOLD)
    big = np.stack([np.asarray(Image.fromarray(f).resize((864, 480))) for f in z["frames"][:6]])
    raw = z["masks_raw"][:6]
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
    net = net.to(dev).eval()
    m01 = video.prepare_masks(raw, (240, 432), dev).cpu().numpy()
    M = m01[:, video.nearest_table(240, 480)][:, :, video.nearest_table(432, 864)] != 0
    assert 0 < M.mean() < 0.5
    for kw in ({}, {"reuse": True}):
        lo = video.inpaint_video(net, big, raw, size=(432, 240), **kw)
        out = video.inpaint_video(net, big, raw, size=(432, 240), restore=True, **kw)
        assert out.shape == big.shape and out.dtype == np.uint8
        assert np.array_equal(out, restore_np(lo, m01, big)), kw
        assert np.array_equal(out[~M], big[~M]) and (out[M] != big[M]).any()
