"""The temporal denoiser restated in numpy (video.denoise, ops.denoise; the definition is in include/e2fgvi_hip.h), the named
cases the device code is compared with byte for byte, mutated restatements (VARIANTS) that must each differ from the definition on
a case named for them -- which is what shows that the cases can see such a mistake -- and the planted clips the definition is
judged on.  Integers after one floor: there is no tolerance anywhere.  Written unlike the kernel on purpose: all frames at once,
index arrays for the taps, every candidate's weight as a whole plane."""
import os

import numpy as np

DEFAULTS = dict(strength=8, search=1, max_change=255)
# (flag, the case that must see it, the (h, s, limit) it is seen at)
CAUGHT_BY = (
    ("floor_q", "halves_17x23", (8, 0, 255)),              # r = floor(q) instead of floor(q + 0.5)
    ("inside_after_round", "edges_17x23", (8, 1, 255)),    # inside tested on r, not on q
    ("taps_unclamped", "tiny_3x5", (64, 1, 255)),          # taps off the frame read as 0 instead of the border pixel
    ("candidate_clamped", "corners_17x23", (64, 2, 255)),  # a candidate off the frame clamped to it instead of dropped
    ("flows_swapped", "soft_33x70", (8, 1, 255)),          # A reached along fwd, B along bwd
    ("across_cut", "cut2_17x23", (8, 1, 255)),             # a neighbour is taken across a cut
    ("per_channel", "soft_33x70", (8, 1, 255)),            # the weights from each channel's own bytes, not from luma
    ("no_centre_weight", "soft_33x70", (8, 1, 255)),       # Wsum without the centre's 256
    ("round_full", "soft_33x70", (8, 1, 255)),             # + Wsum instead of + (Wsum >> 1)
    ("m_floor", "soft_33x70", (64, 1, 255)),               # m = 65536 // (9 h), rounded down
    ("limit_first", "soft_33x70", (64, 1, 3)),             # the neighbours' bytes clamped to C +- limit, not the result
    ("centre_at_r", "soft_33x70", (8, 1, 255)),            # the centre's patch taken around r, not around p
)
VARIANTS = tuple((name, {name: True}) for name, _, _ in CAUGHT_BY)


def luma(frames):
    a = np.asarray(frames).astype(np.int64)
    return (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8


def scene_of_np(length, scenes=None):
    """int32 [L]: the number of cuts at or in front of each frame"""
    s = np.zeros(length, np.int32)
    for c in scenes or []:
        s[int(c):] += 1
    return s


def weight_scale(h, **f):
    return 65536 // (9 * h) if f.get("m_floor") else (65536 + (9 * h) // 2) // (9 * h)


def _tap(P, tt, yy, xx, f):
    """P[tt, yy, xx] with the coordinates clamped to the frame"""
    H, W = P.shape[1:3]
    v = P[tt, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    if f.get("taps_unclamped"):
        v = np.where((yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1), v, 0)
    return v


def reference(frames, fwd, bwd, scene, h, s, limit, **f):
    """the definition: frames uint8 [L,H,W,3]; fwd, bwd fp32 [L-1,H,W,2]; scene int32 [L] -> uint8 [L,H,W,3]"""
    fr = np.asarray(frames).astype(np.int64)
    L, H, W = fr.shape[:3]
    if L < 2 or H * W == 0:
        return np.array(frames, np.uint8)
    scene = np.asarray(scene)
    m = weight_scale(h, **f)
    planes = [fr[..., k] for k in range(3)] if f.get("per_channel") else [luma(fr)]
    tt, yy, xx = np.meshgrid(np.arange(L), np.arange(H), np.arange(W), indexing="ij")
    wsum = np.full((L, H, W), 0 if f.get("no_centre_weight") else 256, np.int64)
    acc = 256 * fr
    if f.get("per_channel"):
        wsum = np.repeat(wsum[..., None], 3, axis=-1)
    A, B = (np.asarray(bwd), np.asarray(fwd)) if not f.get("flows_swapped") else (np.asarray(fwd), np.asarray(bwd))
    for step, flows in ((-1, A), (1, B)):
        tn = np.arange(L) + step
        there = (tn >= 0) & (tn <= L - 1)
        tn = np.clip(tn, 0, L - 1)
        if not f.get("across_cut"):
            there &= scene[tn] == scene
        g = flows[np.clip(np.arange(L) + min(step, 0), 0, L - 2)].astype(np.float64)       # bwd[t - 1] or fwd[t]
        with np.errstate(invalid="ignore", over="ignore"):
            qx, qy = xx + g[..., 0], yy + g[..., 1]
            finite = np.isfinite(g[..., 0]) & np.isfinite(g[..., 1])
            if f.get("floor_q"):
                rx, ry = np.floor(qx), np.floor(qy)
            else:
                rx, ry = np.floor(qx + 0.5), np.floor(qy + 0.5)
            if f.get("inside_after_round"):
                inside = finite & (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
            else:
                inside = finite & (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
        inside &= there[:, None, None]
        rx = np.where(inside, rx, 0).astype(np.int64)
        ry = np.where(inside, ry, 0).astype(np.int64)
        tnn = np.broadcast_to(tn[:, None, None], (L, H, W))
        px, py = (rx, ry) if f.get("centre_at_r") else (xx, yy)
        for j in range(-s, s + 1):
            for i in range(-s, s + 1):
                cx, cy = rx + i, ry + j
                ok = inside & (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
                if f.get("candidate_clamped"):
                    ok = inside
                cx, cy = np.clip(cx, 0, W - 1), np.clip(cy, 0, H - 1)
                ws = []
                for P in planes:
                    sad = sum(np.abs(_tap(P, tt, py + v, px + u, f) - _tap(P, tnn, cy + v, cx + u, f))
                              for v in (-1, 0, 1) for u in (-1, 0, 1))
                    ws.append(np.where(ok, np.maximum(0, 256 - ((sad * m) >> 8)), 0))
                w = np.stack(ws, axis=-1) if f.get("per_channel") else ws[0][..., None]
                nb = fr[tnn, cy, cx]
                if f.get("limit_first"):
                    nb = np.clip(nb, fr - limit, fr + limit)
                acc = acc + w * nb
                wsum = wsum + (w if f.get("per_channel") else w[..., 0])
    ws3 = wsum if f.get("per_channel") else wsum[..., None]
    safe = np.maximum(ws3, 1)
    o = (acc + (safe if f.get("round_full") else (safe >> 1))) // safe
    o = np.where(ws3 > 0, o, fr)
    if not f.get("limit_first"):
        o = np.clip(o, fr - limit, fr + limit)
    return np.clip(o, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ named cases
def noise(L, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (L, H, W, 3)).astype(np.uint8)


def soft(L, H, W, seed, sigma=4.0):
    """one smooth picture, the same in every frame up to noise of a few levels: patches match, so weights are neither 0 nor 256"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (H + 4, W + 4, 3)).astype(np.float64)
    base = sum(a[j:j + H, k:k + W] for j in range(5) for k in range(5)) / 25.0
    base = 128 + (base - 128) * 3
    return np.clip(np.rint(base[None] + sigma * rng.standard_normal((L, H, W, 3))), 0, 255).astype(np.uint8)


def const_flows(L, H, W, fx, fy):
    """fwd = (fx, fy) everywhere, bwd = its negative"""
    fwd = np.zeros((max(L - 1, 0), H, W, 2), np.float32)
    fwd[..., 0], fwd[..., 1] = fx, fy
    return fwd, -fwd


def random_flows(L, H, W, seed, amp=6.0):
    rng = np.random.RandomState(seed)
    return tuple((amp * (2 * rng.random_sample((max(L - 1, 0), H, W, 2)) - 1)).astype(np.float32) for _ in range(2))


def _case(frames, flows, scenes=None):
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    fwd, bwd = (np.ascontiguousarray(a, dtype=np.float32) for a in flows)
    for a in (frames, fwd, bwd):
        a.setflags(write=False)
    L, H, W = frames.shape[:3]
    return dict(frames=frames, fwd=fwd, bwd=bwd, scenes=list(scenes or []), L=L, H=H, W=W)


def _halves(L, H, W, seed):
    """flows on exact halves, positive and negative: q + 0.5 is an integer, and floor(q) differs from floor(q + 0.5)"""
    rng = np.random.RandomState(seed)
    return tuple((rng.randint(-3, 4, (L - 1, H, W, 2)) + 0.5).astype(np.float32) for _ in range(2))


def _edges(L, H, W):
    """per column a flow that lands exactly on column W - 1 / row H - 1, just outside them, on -0.5 and just inside 0, and the
    non-finite ones"""
    fwd, bwd = np.zeros((L - 1, H, W, 2), np.float32), np.zeros((L - 1, H, W, 2), np.float32)
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    kinds = (lambda n, at: n - 1 - at, lambda n, at: np.nextafter(np.float32(n - 1), np.float32(n)) - at, lambda n, at: -0.5 - at,
             lambda n, at: -at, lambda n, at: n - 1 + 0.4 - at, lambda n, at: -0.4 - at, lambda n, at: n - 0.5 - at)
    for x in range(W):
        fwd[:, :, x, 0] = kinds[x % len(kinds)](W, xs[x])
        bwd[:, :, x, 0] = kinds[(x + 3) % len(kinds)](W, xs[x])
    for y in range(H):
        fwd[:, y, :, 1] = kinds[(y + 1) % len(kinds)](H, ys[y])
        bwd[:, y, :, 1] = kinds[(y + 4) % len(kinds)](H, ys[y])
    return fwd, bwd


def _nonfinite(L, H, W, seed):
    fwd, bwd = random_flows(L, H, W, seed, 2.0)
    fwd, bwd = fwd.copy(), bwd.copy()
    bad = (np.nan, np.inf, -np.inf, 1e30, -1e30)
    rng = np.random.RandomState(seed + 1)
    for a in (fwd, bwd):
        hit = rng.randint(0, 4, a.shape[:3] + (2,))
        which = rng.randint(0, len(bad), a.shape)
        a[hit == 0] = np.asarray(bad, np.float32)[which[hit == 0]]
    return fwd, bwd


def _corners(L, H, W):
    """every pixel points at one of the four corners: candidates fall off the frame on two sides"""
    yy, xx = np.mgrid[0:H, 0:W]
    tx = np.where((xx + yy) % 2 == 0, 0, W - 1)
    ty = np.where((xx // 2 + yy) % 2 == 0, 0, H - 1)
    f = np.stack([tx - xx, ty - yy], axis=-1).astype(np.float32)
    b = np.stack([(W - 1 - tx) - xx, (H - 1 - ty) - yy], axis=-1).astype(np.float32)      # the opposite corner
    return np.repeat(f[None], L - 1, axis=0), np.repeat(b[None], L - 1, axis=0)


def _steps(L, H, W):
    """frame t is flat at 100 + t d: with zero flows a candidate's SAD is 9 d, which puts SAD m right at a multiple of 256"""
    base = np.zeros((L, H, W, 3), np.int64) + 100
    yy, xx = np.mgrid[0:H, 0:W]
    for t in range(L):
        base[t] += t * ((xx + yy) % 7)[..., None]
    return base


SIZES = ((1, 1), (1, 7), (2, 2), (3, 5), (17, 23), (33, 70), (64, 128))
_BUILDERS = {}
for _H, _W in SIZES:
    # random bytes along random flows of +-6 px, three frames; and softened frames, where the weights take every value
    _BUILDERS["random_%dx%d" % (_H, _W)] = lambda H=_H, W=_W: _case(noise(3, H, W, 10 * H + W), random_flows(3, H, W, H + W))
    _BUILDERS["soft_%dx%d" % (_H, _W)] = lambda H=_H, W=_W: _case(soft(3, H, W, 11 * H + W), random_flows(3, H, W, H + W + 1, 1.5))
_BUILDERS.update({
    "tiny_3x5": lambda: _case(soft(2, 3, 5, 3), const_flows(2, 3, 5, 0, 0)),
    "single_17x23": lambda: _case(noise(1, 17, 23, 20), const_flows(1, 17, 23, 0, 0)),
    "pair_17x23": lambda: _case(soft(2, 17, 23, 21), random_flows(2, 17, 23, 22, 2.0)),
    "five_33x70": lambda: _case(soft(5, 33, 70, 23), random_flows(5, 33, 70, 24, 3.0)),
    "halves_17x23": lambda: _case(soft(3, 17, 23, 25), _halves(3, 17, 23, 26)),
    "edges_17x23": lambda: _case(soft(3, 17, 23, 27), _edges(3, 17, 23)),
    "edges_3x5": lambda: _case(soft(3, 3, 5, 28), _edges(3, 3, 5)),
    "nonfinite_17x23": lambda: _case(soft(3, 17, 23, 29), _nonfinite(3, 17, 23, 30)),
    "corners_17x23": lambda: _case(soft(3, 17, 23, 31, 2.0), _corners(3, 17, 23)),
    "corners_2x2": lambda: _case(soft(3, 2, 2, 32, 2.0), _corners(3, 2, 2)),
    # a cut at every place of five frames, and at all of them
    "cut1_17x23": lambda: _case(soft(5, 17, 23, 33), random_flows(5, 17, 23, 34, 1.5), [1]),
    "cut2_17x23": lambda: _case(soft(5, 17, 23, 33), random_flows(5, 17, 23, 34, 1.5), [2]),
    "cut4_17x23": lambda: _case(soft(5, 17, 23, 33), random_flows(5, 17, 23, 34, 1.5), [4]),
    "cuts_17x23": lambda: _case(soft(5, 17, 23, 33), random_flows(5, 17, 23, 34, 1.5), [1, 2, 3, 4]),
    # 0 and 255 alone: every clamp is reached, and |a - b| is 0 or 255
    "extremes_17x23": lambda: _case(255 * np.random.RandomState(35).randint(0, 2, (3, 17, 23, 3)), random_flows(3, 17, 23, 36, 2.0)),
    "extremes_64x128": lambda: _case(255 * (np.random.RandomState(37).randint(0, 8, (3, 64, 128, 1)) > 0) + np.zeros((1, 1, 1, 3)),
                                     random_flows(3, 64, 128, 38, 2.0)),
    "flat_17x23": lambda: _case(np.full((3, 17, 23, 3), 90), random_flows(3, 17, 23, 39)),
    "steps_17x23": lambda: _case(_steps(3, 17, 23), const_flows(3, 17, 23, 0, 0)),
})
NAMES = tuple(_BUILDERS)
# every setting a case is run with on the device: (h, s, limit)
SETTINGS = ((8, 1, 255), (1, 0, 255), (64, 2, 255), (8, 2, 3), (64, 1, 3), (1, 2, 255), (8, 0, 0), (64, 0, 255), (1, 1, 3))
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def want(name, setting, **f):
    """the output bytes of a case at (h, s, limit) under the definition (or a variant's flags); computed once, read-only"""
    key = (name, tuple(setting)) + tuple(sorted(f))
    if key not in _WANT:
        c = case(name)
        w = reference(c["frames"], c["fwd"], c["bwd"], scene_of_np(c["L"], c["scenes"]), *setting, **f)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ planted clips
def tennis25(root):
    with np.load(os.path.join(root, "tests", "golden", "tennis25.npz")) as z:
        return np.asarray(z["frames"], np.uint8)


def pan_clip(f):
    """(the clean clip of 8 frames of 120 x 160: a window that pans over f[0] by (2, 1) px a frame, fwd, bwd)"""
    clean = np.stack([f[0][40 + t:160 + t, 100 + 2 * t:260 + 2 * t] for t in range(8)])
    fwd, bwd = const_flows(8, 120, 160, -2.0, -1.0)
    return clean, fwd, bwd


def noisy_clips(clean):
    """the clean clip under Gaussian noise of sigma 5 and of sigma 10, drawn in that order from default_rng(1)"""
    rng = np.random.default_rng(1)
    return tuple(np.clip(np.rint(clean + sigma * rng.standard_normal(clean.shape)), 0, 255).astype(np.uint8) for sigma in (5.0, 10.0))


def psnr(a, b):
    err = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(10 * np.log10(255.0 ** 2 / np.mean(err ** 2)))


def still_clip(f, blotch=False):
    """5 copies of f[0][60:100, 120:180] with its bytes capped at 170; with ``blotch`` frame 2 carries a 5 x 5 patch of + 80 on
    every channel, which is + 80 luma levels"""
    one = np.minimum(f[0][60:100, 120:180], 170)
    clip = np.repeat(one[None], 5, axis=0).copy()
    if blotch:
        clip[2, 17:22, 30:35] += 80
    return clip
