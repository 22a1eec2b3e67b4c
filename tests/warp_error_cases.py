"""E_warp (e2fgvi_amd.metrics.warp_error, csrc/metrics.hip): the float64 numpy reference of its definition and the inputs the CPU
tests (test_warp_error.py) and the GPU tests (test_gpu_warp_error.py) share.

The definition (Lai et al., ECCV 2018; occlusion test of Ruder et al. 2016) for pair t with A = frames[t], B = frames[t+1],
f = fwd[t], g = bwd[t], pixel p = (x, y), everything in float64:
  q = (x + f_x, y + f_y);  inside = 0 <= q_x <= W-1 and 0 <= q_y <= H-1;
  bil(T, q) = 4-corner bilinear sample, corners outside the image contribute 0;  g_w = bil(g, q), B_w = bil(B, q);
  occluded        |f + g_w|^2 > 0.01 (|f|^2 + |g_w|^2) + 0.5;
  motion boundary |dx f|^2 + |dy f|^2 > 0.01 |f|^2 + 0.002, forward differences, 0 on the last column / row;
  M = inside, not occluded, no motion boundary, valid[t] != 0, and f(p), the neighbours of f used and g_w finite;
  n = sum M,  e = sum_p M sum_c ((A_c - B_w,c) / 255)^2 / n  (0 when n = 0).

`variant` names one deliberately WRONG reading of that text (VARIANTS): test_warp_error.py shows that each of them moves e or n on
at least one case, i.e. that the reference the kernel is held to tells them apart.
"""
import functools

import numpy as np

VARIANTS = ("swap_channels", "border", "bwd_unwarped", "no_half", "no_rel", "central_diff", "ignore_valid", "div_hw")


def bilinear(T, qx, qy, border=False):
    """T [H,W,C] float64 sampled at (qx, qy) [H,W] (finite, inside [0,W-1] x [0,H-1]): corners outside the image contribute 0
    (border=True: they repeat the edge pixel -- the wrong variant).  The plain weighted sum of the in-image corners: a corner
    with weight 0 still enters it."""
    H, W, _ = T.shape
    x0 = np.floor(qx).astype(np.int64)
    y0 = np.floor(qy).astype(np.int64)
    wx1, wy1 = qx - x0, qy - y0
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    out = np.zeros(qx.shape + (T.shape[2],), np.float64)
    with np.errstate(all="ignore"):
        for dy, dx, w in ((0, 0, wy0 * wx0), (0, 1, wy0 * wx1), (1, 0, wy1 * wx0), (1, 1, wy1 * wx1)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
            v = T[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]
            term = w[..., None] * v
            out = out + (term if border else np.where(ok[..., None], term, 0.0))
    return out


def reference_pair(A, B, f, g, valid=None, variant=None):
    """one pair: A, B [H,W,3], f, g [H,W,2], valid [H,W] or None -> dict(e, n, outside, occluded, boundary, keep, margin, warped)
    -- outside / occluded / boundary / keep are boolean maps (occluded and boundary among the inside pixels with finite flows),
    margin the smallest |lhs - rhs| of the two threshold tests over the pixels no other condition excludes, warped = B_w
    (zeros outside)."""
    assert variant is None or variant in VARIANTS, variant
    A, B, f, g = (np.asarray(v, np.float64) for v in (A, B, f, g))
    if variant == "swap_channels":
        f, g = f[..., ::-1], g[..., ::-1]
    H, W, _ = A.shape
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        fx, fy = f[..., 0], f[..., 1]
        qx, qy = xs + fx, ys + fy
        inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
        sx, sy = np.where(inside, qx, 0.0), np.where(inside, qy, 0.0)
        border = variant == "border"
        if border:                   # border padding: every position is sampled, clamped into the image
            inside = np.isfinite(qx) & np.isfinite(qy)
            sx = np.clip(np.where(inside, qx, 0.0), 0, W - 1)
            sy = np.clip(np.where(inside, qy, 0.0), 0, H - 1)
        g_w = g if variant == "bwd_unwarped" else bilinear(g, sx, sy, border)
        B_w = bilinear(B, sx, sy, border)
        dxf, dyf = np.zeros_like(f), np.zeros_like(f)
        fin = np.isfinite(f).all(-1)
        fin_n = fin.copy()
        if variant == "central_diff":
            dxf[:, 1:-1] = (f[:, 2:] - f[:, :-2]) / 2
            dyf[1:-1, :] = (f[2:, :] - f[:-2, :]) / 2
        else:
            dxf[:, :-1] = f[:, 1:] - f[:, :-1]
            dyf[:-1, :] = f[1:, :] - f[:-1, :]
        fin_n[:, :-1] &= fin[:, 1:]
        fin_n[:-1, :] &= fin[1:, :]
        rel = 0.0 if variant == "no_rel" else 0.01
        ff = fx * fx + fy * fy
        mb_l = (dxf ** 2).sum(-1) + (dyf ** 2).sum(-1)
        mb_r = rel * ff + 0.002
        s = f + g_w
        oc_l = (s ** 2).sum(-1)
        oc_r = rel * (ff + (g_w ** 2).sum(-1)) + (0.0 if variant == "no_half" else 0.5)
        finite = fin_n & np.isfinite(g_w).all(-1)
        base = inside & finite
        if valid is not None and variant != "ignore_valid":
            base = base & (np.asarray(valid) != 0)
        occluded = inside & finite & (oc_l > oc_r)
        boundary = inside & finite & (mb_l > mb_r)
        keep = base & ~(oc_l > oc_r) & ~(mb_l > mb_r)
        m_oc = np.where(base & ~(mb_l > mb_r), np.abs(oc_l - oc_r), np.inf).min()
        m_mb = np.where(base & ~(oc_l > oc_r), np.abs(mb_l - mb_r), np.inf).min()
        per = (((A - B_w) / 255.0) ** 2).sum(-1)
    n = int(keep.sum())
    den = H * W if variant == "div_hw" else n
    e = float(per[keep].sum() / den) if n else 0.0
    return dict(e=e, n=n, outside=~inside, occluded=occluded, boundary=boundary, keep=keep, margin=float(min(m_oc, m_mb)),
                warped=np.where(inside[..., None], B_w, 0.0))


def reference(frames, fwd, bwd, valid=None, variant=None):
    """every pair of a video: list of reference_pair() results"""
    return [reference_pair(frames[t], frames[t + 1], fwd[t], bwd[t], None if valid is None else valid[t], variant)
            for t in range(len(frames) - 1)]


def rows(ref):
    """reference() as warp_error's [L-1, 2] array"""
    return np.array([[r["e"], r["n"]] for r in ref], np.float64)


# ------------------------------------------------------------------------------------------------ inputs
SCENE_HW, SCENE_L = (48, 72), 5


def _bg(x, y):
    return 127 + 60 * np.sin(x / 6) * np.cos(y / 5) + 30 * np.sin((x + y) / 11)


def _ob(x, y):
    return 127 + 70 * np.cos(x / 3.5) * np.sin(y / 4.5)


def _rgb(g):
    return np.stack([g, 0.8 * g + 20, 255 - g], -1)


def scene(flicker=False, zero_flows=False):
    """a textured rectangle moving by (3, 1) per frame over a background moving by (1.5, -0.75), with their true flows: frames
    float32 [5,48,72,3], fwd / bwd float32 [4,48,72,2].  flicker: frame 2 brighter by 8 on rows 10:30, columns 10:40."""
    H, W = SCENE_HW
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    frames, rects = [], []
    for t in range(SCENE_L):
        rect = (xs >= 20 + 3 * t) & (xs <= 42 + 3 * t) & (ys >= 12 + t) & (ys <= 28 + t)
        frames.append(_rgb(np.where(rect, _ob(xs - 3 * t, ys - t), _bg(xs - 1.5 * t, ys + 0.75 * t))))
        rects.append(rect)
    frames = np.stack(frames)
    if flicker:
        frames[2, 10:30, 10:40] += 8
    fwd = np.stack([np.where(rects[t][..., None], (3.0, 1.0), (1.5, -0.75)) for t in range(SCENE_L - 1)])
    bwd = np.stack([np.where(rects[t + 1][..., None], (-3.0, -1.0), (-1.5, 0.75)) for t in range(SCENE_L - 1)])
    if zero_flows:
        fwd, bwd = np.zeros_like(fwd), np.zeros_like(bwd)
    return dict(frames=frames.astype(np.float32), fwd=fwd.astype(np.float32), bwd=bwd.astype(np.float32), valid=None)


def _waves(rng, H, W, n, amp, lam=(8, 40)):
    """sum of n sines of random direction, wavelength lam[0] .. lam[1] pixels and phase; peak about amp"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((H, W))
    for _ in range(n):
        a, lam_, ph = rng.uniform(0, 2 * np.pi), rng.uniform(*lam), rng.uniform(0, 2 * np.pi)
        out += np.sin((np.cos(a) * xs + np.sin(a) * ys) * 2 * np.pi / lam_ + ph)
    return out * (amp / n)


def smooth(H, W, L, seed, valid=False):
    """smooth random frames and flows: flows of up to about 3 pixels (less along an axis too short for them: an image one pixel
    high keeps a sample inside only with f_y = 0), bwd = -fwd plus a perturbation of 0.3 .. 0.6 pixels"""
    rng = np.random.RandomState(seed)
    ax, ay = min(3.0, (W - 1) / 4.0), min(3.0, (H - 1) / 4.0)
    frames = np.stack([_rgb(np.clip(127 + _waves(rng, H, W, 4, 100), 0, 255)) for _ in range(L)])
    # long waves on a constant drift: the gradients sit around the motion-boundary threshold, so that test cuts through the image
    flow = lambda a: rng.uniform(-0.6, 0.6) * a + _waves(rng, H, W, 3, 0.4 * a, (50, 200))
    fwd = np.stack([np.stack([flow(ax), flow(ay)], -1) for _ in range(L - 1)])
    pert = np.stack([np.stack([_waves(rng, H, W, 2, min(ax, rng.uniform(0.3, 0.6))),
                               _waves(rng, H, W, 2, min(ay, rng.uniform(0.3, 0.6)))], -1) for _ in range(L - 1)])
    case = dict(frames=frames.astype(np.float32), fwd=fwd.astype(np.float32), bwd=(-fwd + pert).astype(np.float32), valid=None)
    if valid:
        v = (rng.uniform(size=(L, H, W)) < 0.7).astype(np.uint8) * rng.randint(1, 256, (L, H, W)).astype(np.uint8)
        v[:, H // 4:H // 2, W // 3:W // 2] = 0
        case["valid"] = v
    return case


def nonfinite():
    """smooth flows with inf, nan and +-1e30 entries at interior, last-column and last-row pixels of fwd and at interior pixels
    of bwd (which the warp reads through up to four samples)"""
    c = smooth(24, 40, 3, 11)
    H, W = 24, 40
    bad = [np.inf, -np.inf, np.nan, 1e30, -1e30]
    spots = [(5, 7), (12, 20), (9, W - 1), (15, W - 1), (H - 1, 6), (H - 1, 30), (H - 1, W - 1), (0, 0), (10, 33), (18, 3)]
    for t in range(2):
        for k, (y, x) in enumerate(spots):
            c["fwd"][t, y, x, (k + t) % 2] = bad[(k + t) % len(bad)]
        for k, (y, x) in enumerate([(6, 12), (7, 13), (14, 25), (20, 20), (3, 30), (11, 5)]):
            c["bwd"][t, y, x, k % 2] = bad[(k + 2 * t) % len(bad)]
    c["fwd"][1, 8, 8] = (1e30, -1e30)
    c["fwd"][1, 16, 16] = (np.nan, np.inf)
    return c


# name -> builder.  Sizes: (1, 9) / (9, 1) put every gradient on the last row / column, (7, 5) is smaller than a wave,
# (33, 65) and (17, 300) cross wave (64) and block (256) edges with a ragged last block.
_BUILDERS = {
    "scene": lambda: scene(),
    "scene_flicker": lambda: scene(flicker=True),
    "scene_zero_flows": lambda: scene(zero_flows=True),
    "smooth_1x9": lambda: smooth(1, 9, 3, 1),
    "smooth_9x1": lambda: smooth(9, 1, 3, 2),
    "smooth_7x5": lambda: smooth(7, 5, 3, 3),
    "smooth_33x65": lambda: smooth(33, 65, 3, 4),
    "smooth_17x300": lambda: smooth(17, 300, 2, 5),
    "smooth_valid_40x56": lambda: smooth(40, 56, 3, 6, valid=True),
    "nonfinite": nonfinite,
    "eval_70x90": lambda: smooth(70, 90, 13, 7),
}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of a case (shared, read-only): frames fp32 [L,H,W,3], fwd / bwd fp32 [L-1,H,W,2], valid uint8 [L,H,W] or None"""
    c = _BUILDERS[name]()
    for v in c.values():
        if v is not None:
            v.setflags(write=False)
    return c


def frames_u8(name):
    """the case's frames rounded to uint8"""
    return np.clip(np.rint(case(name)["frames"]), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_reference(name, u8=False, variant=None):
    """reference() of a case, computed once (read-only)"""
    c = case(name)
    return reference(frames_u8(name) if u8 else c["frames"], c["fwd"], c["bwd"], c["valid"], variant)
