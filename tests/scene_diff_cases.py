"""Scene cuts (e2fgvi_amd.video.scene_scores / detect_cuts, csrc/video.hip scene_hist_kernel): the numpy restatement of the
block-histogram difference and the inputs the CPU tests (test_video_scenes.py) and the GPU tests (test_gpu_video_scenes.py) share.

The definition, integers only.  For frame t and pixel (x, y) with bytes R, G, B:
    Y    = (77 R + 150 G + 29 B + 128) >> 8                 0 .. 255
    bin  = Y >> 2                                           64 bins
    cell = ((4 y) // H) * 4 + (4 x) // W                    a 4 x 4 grid; cells are empty when H < 4 or W < 4
    hist[t][cell][bin] = number of such pixels
    out[t] = sum over cell, bin of |hist[t][cell][bin] - hist[t + 1][cell][bin]|,  0 <= t < L - 1:  0 .. 2 H W
    score[t] = out[t] / (2 H W)
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tennis25.npz")
TENNIS_CUT = 12                 # tennis_join(): frames 12 .. are flipped horizontally


def bins_np(frames):
    """uint8 [..., 3] -> int64 [...] luma bins"""
    f = np.asarray(frames).astype(np.int64)
    return ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8) >> 2


def cells_np(H, W):
    """int64 [H, W]: the cell of every pixel"""
    y, x = np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64)
    return ((4 * y) // H)[:, None] * 4 + ((4 * x) // W)[None, :]


def hist_np(frames):
    """uint8 [L,H,W,3] -> int64 [L,16,64]"""
    frames = np.asarray(frames)
    L, H, W, _ = frames.shape
    idx = cells_np(H, W)[None] * 64 + bins_np(frames)
    return np.stack([np.bincount(i.reshape(-1), minlength=1024) for i in idx]).reshape(L, 16, 64).astype(np.int64)


def scene_diff_np(frames):
    """uint8 [L,H,W,3] -> int64 [L-1]"""
    h = hist_np(frames)
    return np.abs(h[1:] - h[:-1]).sum(axis=(1, 2))


def scores_np(frames):
    frames = np.asarray(frames)
    return scene_diff_np(frames).astype(np.float64) / (2.0 * frames.shape[1] * frames.shape[2])


def tennis():
    return np.load(GOLD)["frames"]


def tennis_join():
    """the fixture's 25 frames with frames TENNIS_CUT .. flipped horizontally: one shot joined with its own mirrored continuation"""
    f = tennis().copy()
    f[TENNIS_CUT:] = f[TENNIS_CUT:, :, ::-1]
    return f


CONTENTS = ("random", "zeros", "full", "mid", "gradient")


def content(kind, L, H, W, seed=0):
    """uint8 [L,H,W,3] of one kind.  The constant kinds put every pixel of a cell into one bin -- every add of a wave meets on one
    counter; the value changes at least once so that the differences are not all zero.  The gradient is smooth and
    moves by a pixel a frame."""
    rng = np.random.RandomState(seed + 7 * L + 13 * H + 17 * W)
    if kind == "random":
        return rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)
    if kind in ("zeros", "full", "mid"):
        f = np.full((L, H, W, 3), {"zeros": 0, "full": 255, "mid": 117}[kind], np.uint8)
        if kind == "mid":
            f[1::2] = (90, 140, 33)                     # another bin in every other frame: out = 2 H W
        else:
            f[-1] = 255 - f[-1]                         # the last frame is the other extreme: 0, ..., 0, 2 H W
        return f
    if kind == "gradient":
        t, y, x = np.meshgrid(np.arange(L), np.arange(H), np.arange(W), indexing="ij")
        r = (255 * (x + t)) // (W + L)
        g = (255 * (y + 2 * t)) // (H + 2 * L)
        b = (r + g) // 2
        return np.stack([r, g, b], -1).astype(np.uint8)
    raise KeyError(kind)


def toy_video(L, h, w, seed=0):
    """tests/test_video_driver.py's random-texture toy video: a window that slides over one random image, and a moving hole"""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, (h + 2 * L, w + 2 * L, 3)).astype(np.float32)
    frames = np.stack([np.clip(base[i:i + h, 2 * i:2 * i + w], 0, 255).astype(np.uint8) for i in range(L)])
    masks = np.zeros((L, h, w), np.uint8)
    for i in range(L):
        masks[i, h // 4 + i % 3:h // 2 + i % 3, w // 4 + i:w // 2 + i] = 255
    return frames, masks


def gradient_video(L, h, w):
    """a smooth shot: a diagonal colour ramp that moves by a pixel a frame"""
    t, y, x = np.meshgrid(np.arange(L), np.arange(h), np.arange(w), indexing="ij")
    r = (200 * (x + t)) // (w + L) + 20
    g = (200 * (y + t)) // (h + L) + 30
    b = (100 * (x + y)) // (w + h) + 60
    return np.stack([r, g, b], -1).astype(np.uint8)
