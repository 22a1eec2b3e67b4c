"""Static overlays (e2fgvi_amd.video.overlay_mask, csrc/video.hip overlay_stats_kernel / overlay_edges_kernel): the numpy restatement
of the definition and the inputs the CPU tests (test_video_overlay.py) and the GPU tests (test_gpu_video_overlay.py) share.

The definition, integers only.  Frames are uint8 [L,H,W,3]; per frame, with clamped borders,
    Y  = (77 R + 150 G + 29 B + 128) >> 8                                  the scene detector's luma
    gx = Y[y, min(x+1, W-1)] - Y[y, max(x-1, 0)],   gy = Y[min(y+1, H-1), x] - Y[max(y-1, 0), x]
and per pixel over the L frames   Sx = sum gx,  Sy = sum gy,  M = sum (|gx| + |gy|)          int32 [3,H,W].
    persistent edge:  M >= g_min L  and  256 (|Sx| + |Sy|) >= coherence M                    (64-bit)
    D    = the edge map dilated by the (2 r + 1) x (2 r + 1) box, outside the frame counting as no edge
    mask = D, plus every 8-connected component of the complement of D whose bounding box touches no frame edge, minus every
           8-connected component of that with fewer than min_area pixels; uint8 [H,W] of 0 / 255.
count(D) > max_fraction H W raises ValueError: the scenery itself is static.
"""
import functools

import numpy as np

from tests import hole_label_cases as C
from tests import scene_diff_cases as S

DEFAULTS = dict(g_min=32, coherence=224, radius=3, min_area=256, max_fraction=0.25)


def luma_np(frames):
    """uint8 [..., 3] -> int64 [...]"""
    f = np.asarray(frames).astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def stats_np(frames):
    """uint8 [L,H,W,3] -> int32 [3,H,W] = (Sx, Sy, M)"""
    Y = luma_np(frames)
    px = np.pad(Y, ((0, 0), (0, 0), (1, 1)), mode="edge")
    py = np.pad(Y, ((0, 0), (1, 1), (0, 0)), mode="edge")
    gx, gy = px[:, :, 2:] - px[:, :, :-2], py[:, 2:, :] - py[:, :-2, :]
    out = np.stack([gx.sum(0), gy.sum(0), (np.abs(gx) + np.abs(gy)).sum(0)])
    assert np.abs(out).max(initial=0) < 1 << 31
    return out.astype(np.int32)


def edges_np(stats, L, g_min, coherence):
    """int32 [3,H,W] -> bool [H,W]: the persistent edges, before the dilation"""
    sx, sy, m = (np.asarray(p).astype(np.int64) for p in stats)
    return (m >= int(g_min) * int(L)) & (256 * (np.abs(sx) + np.abs(sy)) >= int(coherence) * m)


def dilate_np(E, r):
    """bool [H,W] -> bool [H,W]: OR over the (2 r + 1) x (2 r + 1) box, outside the map counting as False"""
    E = np.asarray(E, bool)
    H, W = E.shape
    p = np.pad(E, r, mode="constant")
    out = np.zeros((H, W), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def dilated_np(stats, L, g_min, coherence, radius):
    """what ops.overlay_edges returns: (D uint8 [H,W] of 0 / 1, count)"""
    D = dilate_np(edges_np(stats, L, g_min, coherence), radius)
    return D.astype(np.uint8), int(D.sum())


def fill_and_filter_np(D, min_area):
    """D bool [H,W] -> uint8 [H,W] of 0 / 255: the enclosed components of the complement added, the small components dropped"""
    D = np.asarray(D, bool)
    H, W = D.shape
    if not D.any():
        return np.zeros((H, W), np.uint8)
    labels, boxes = C.components_np(~D)
    inner = [k + 1 for k, (x0, y0, x1, y1, _) in enumerate(boxes.tolist()) if x0 > 0 and y0 > 0 and x1 < W and y1 < H]
    filled = D | np.isin(labels, inner)
    labels, boxes = C.components_np(filled)
    keep = [k + 1 for k, b in enumerate(boxes.tolist()) if b[4] >= min_area]
    return np.isin(labels, keep).astype(np.uint8) * 255


def mask_np(frames, g_min=32, coherence=224, radius=3, min_area=256, max_fraction=0.25):
    """video.overlay_mask restated; ValueError when more than max_fraction of the frame is set after the dilation"""
    frames = np.asarray(frames)
    L, H, W, _ = frames.shape
    D, n = dilated_np(stats_np(frames), L, g_min, coherence, radius)
    if n > max_fraction * H * W:
        raise ValueError("%d of %d pixels are static" % (n, H * W))
    return fill_and_filter_np(D, min_area)


# ------------------------------------------------------------------------------------------------ contents for the kernels
CONTENTS = ("random", "zeros", "vstep", "checker", "step255", "toy")


def content(kind, L, H, W, seed=0):
    """uint8 [L,H,W,3] of one kind:
      random   random bytes: every sum is some mid value of either sign
      zeros    no gradient at all: M = 0 fails M >= g_min L for every g_min >= 1
      vstep    a static vertical step between two mid greys: gy = 0 and gx keeps its sign, so |Sx| = M and 256 (|Sx| + |Sy|) equals
               256 M exactly -- coherence = 256 is met with equality
      checker  2 x 2 cells of 0 / 255 that invert every frame: |gx| = |gy| = 255 away from the borders, M = 510 L, the largest there
               is, while Sx = Sy = 0 for an even L (one frame's gradient is left for an odd one)
      step255  rows of 255 above rows of 0 (and a 0 / 255 column step in the lower half) held for all frames: |Sy| = 255 L, the
               largest |S| there is
      toy      tests/scene_diff_cases.py's sliding random texture"""
    rng = np.random.RandomState(seed + 5 * L + 11 * H + 19 * W)
    if kind == "random":
        return rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)
    if kind == "zeros":
        return np.zeros((L, H, W, 3), np.uint8)
    if kind == "vstep":
        f = np.full((L, H, W, 3), 60, np.uint8)
        f[:, :, (W + 1) // 2:] = 180
        return f
    if kind == "checker":
        t, y, x = np.meshgrid(np.arange(L), np.arange(H), np.arange(W), indexing="ij")
        v = ((y // 2 + x // 2 + t) % 2) * 255
        return np.repeat(v[..., None], 3, -1).astype(np.uint8)
    if kind == "step255":
        f = np.zeros((L, H, W, 3), np.uint8)
        f[:, :H // 2] = 255
        f[:, H // 2:, W // 2:] = 255
        return f
    if kind == "toy":
        return S.toy_video(L, H, W, seed)[0]
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------ the fixture and its overlay
RING = (375, 36, 12, 24)        # centre x, centre y, inner radius, outer radius
BARS = [(30 + 14 * k, 205, 8, 18) for k in range(8)]    # left, top, width, height: rows 205 .. 222


def tennis():
    return S.tennis()


def overlay_truth(H=240, W=432):
    """(truth, inside): bool [H,W] maps of the drawn overlay's own pixels and of the disc the ring encloses"""
    y, x = np.mgrid[0:H, 0:W]
    cx, cy, r0, r1 = RING
    d2 = (x - cx) ** 2 + (y - cy) ** 2
    truth = (d2 >= r0 * r0) & (d2 <= r1 * r1)
    for left, top, w, h in BARS:
        truth[top:top + h, left:left + w] = True
    return truth, d2 < r0 * r0


def draw_overlay(frames, alpha):
    """the white overlay blended into every frame: uint8(frame * (1 - alpha) + 255 * alpha + 0.5) on the overlay's pixels"""
    frames = np.asarray(frames)
    truth, _ = overlay_truth(frames.shape[1], frames.shape[2])
    out = frames.copy()
    out[:, truth] = (frames[:, truth].astype(np.float64) * (1.0 - alpha) + 255.0 * alpha + 0.5).astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def clip(name):
    """the shared clips, built once: "plain", "alpha1.0", "alpha0.5" (25 frames) and "still" (frame 0 repeated 25 times)"""
    f = tennis()
    if name == "plain":
        out = f
    elif name == "still":
        out = np.repeat(f[:1], 25, 0)
    else:
        out = draw_overlay(f, {"alpha1.0": 1.0, "alpha0.5": 0.5}[name])
    return out


@functools.lru_cache(maxsize=None)
def clip_mask(name):
    """mask_np of a shared clip with the defaults, computed once and left unchanged"""
    m = mask_np(clip(name))
    m.setflags(write=False)
    return m


def patch_video(L=12, h=131, w=250, seed=4):
    """tests/test_video_restore.py's sliding toy frames with a static patch drawn into every frame: a bright 40 x 24 block with a
    dark frame around it, far from the frame's edges"""
    from tests.test_video_restore import frames
    f = frames(L, w, h, seed).copy()
    f[:, 40:72, 150:198] = 20
    f[:, 44:68, 154:194] = 235
    return f
