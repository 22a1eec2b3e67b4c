"""The dust-and-dirt detector restated in numpy (video.detect_defects, ops.defect_candidates, ops.defect_clean; the definition is in
include/e2fgvi_hip.h), the named cases the device code is compared with byte for byte, and mutated restatements (VARIANTS) that
must each differ from the definition on some case -- which is what shows that the cases can see such a mistake.

The restatement drops the envelope pixels that lie outside the frame where the kernel clamps their coordinates; the two forms have
the same min / max, and stating it the other way makes the comparison a test of that claim too.  Everything is integers after one
floor of a float64 sum, so there is no tolerance anywhere."""
import math

import numpy as np

FLAGS = ("neg_fwd", "swap_xy", "ge", "either", "mixed", "nearest", "outside_zero", "no_centre", "dilate_first", "counts_after")
VARIANTS = tuple((name, {name: True}) for name in FLAGS)
#   neg_fwd        the previous neighbour is pulled along -fwd[t-1] in place of bwd[t-1]
#   swap_xy        channel 1 of a flow is taken for x
#   ge             >= in place of >
#   either         one neighbour suffices
#   mixed          brighter than one neighbour and darker than the other counts
#   nearest        the envelope starts at the nearest pixel, not at the floor
#   outside_zero   envelope pixels outside the frame count as luma 0
#   no_centre      the support count leaves the centre out
#   dilate_first   the dilation runs before the support test
#   counts_after   the counts are taken after the frame guard


def luma(frames):
    f = np.asarray(frames).astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def plan_np(length, scenes=None):
    """the eligible centre frames: t-1, t, t+1 in one scene"""
    bounds = [0] + [int(c) for c in (scenes or [])] + [length]
    out = []
    for s, e in zip(bounds[:-1], bounds[1:]):
        out += list(range(s + 1, e - 1))
    return out


def _envelope(Y, g, slack, f):
    """(inside, lo, hi) of one neighbour's luma Y [H,W] under the flow g [H,W,2]"""
    H, W = Y.shape
    ys, xs = np.mgrid[0:H, 0:W]
    gx, gy = (g[..., 1], g[..., 0]) if f.get("swap_xy") else (g[..., 0], g[..., 1])
    gx, gy = gx.astype(np.float64), gy.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = xs + gx, ys + gy
        inside = np.isfinite(gx) & np.isfinite(gy) & (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    qx, qy = np.where(inside, qx, 0.0), np.where(inside, qy, 0.0)
    if f.get("nearest"):
        x0, y0 = np.floor(qx + 0.5).astype(np.int64), np.floor(qy + 0.5).astype(np.int64)
    else:
        x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    lo, hi = np.full((H, W), 1 << 20, np.int64), np.full((H, W), -1, np.int64)
    for j in range(-slack, 2 + slack):
        for i in range(-slack, 2 + slack):
            yy, xx = y0 + j, x0 + i
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = Y[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            if f.get("outside_zero"):
                v, ok = np.where(ok, v, 0), np.ones_like(ok)
            lo = np.where(ok & (v < lo), v, lo)
            hi = np.where(ok & (v > hi), v, hi)
    return inside, lo, hi


def candidates_np(frames, fwd, bwd, ids, tau, slack, **f):
    """uint8 [L,H,W] of 0 / 1, set for the listed centre frames in [1, L-2] only"""
    Y = luma(frames)
    L, H, W = Y.shape
    out = np.zeros((L, H, W), np.uint8)
    for t in ids:
        if not 1 <= t <= L - 2:
            continue
        gA = -np.asarray(fwd[t - 1]) if f.get("neg_fwd") else np.asarray(bwd[t - 1])
        inA, loA, hiA = _envelope(Y[t - 1], gA, slack, f)
        inB, loB, hiB = _envelope(Y[t + 1], np.asarray(fwd[t]), slack, f)
        c = Y[t]
        if f.get("ge"):
            bA, bB, dA, dB = c >= hiA + tau, c >= hiB + tau, c <= loA - tau, c <= loB - tau
        else:
            bA, bB, dA, dB = c > hiA + tau, c > hiB + tau, c < loA - tau, c < loB - tau
        if f.get("either"):
            cand = (inA & (bA | dA)) | (inB & (bB | dB))
        elif f.get("mixed"):
            cand = inA & inB & (bA | dA) & (bB | dB)
        else:
            cand = inA & inB & ((bA & bB) | (dA & dB))
        out[t] = cand
    return out


def _box_sum(a, r):
    """sum over the (2 r + 1)-pixel box clipped at the frame"""
    H, W = a.shape
    p = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    p[r:r + H, r:r + W] = a
    return sum(p[j:j + H, i:i + W] for j in range(2 * r + 1) for i in range(2 * r + 1))


def clean_np(cand, ids, support, radius, **f):
    """(masks uint8 [L,H,W] of 0 / 255, counts int64 [L]) for the listed centre frames in [1, L-2]; nothing elsewhere"""
    cand = np.asarray(cand)
    L, H, W = cand.shape
    masks, counts = np.zeros((L, H, W), np.uint8), np.zeros(L, np.int64)
    for t in ids:
        if not 1 <= t <= L - 2:
            continue
        c = (cand[t] != 0).astype(np.int64)
        if f.get("dilate_first"):
            c = (_box_sum(c, radius) > 0).astype(np.int64)
        n3 = _box_sum(c, 1) - (c if f.get("no_centre") else 0)
        k = (c > 0) & (n3 >= support)
        d = k if f.get("dilate_first") else _box_sum(k.astype(np.int64), radius) > 0
        masks[t] = 255 * d
        counts[t] = int(d.sum())
    return masks, counts


def detect_np(frames, fwd, bwd, scenes=None, threshold=16, slack=0, support=3, radius=1, max_fraction=0.02, **f):
    """(masks, counts): the frames over the guard cleared, the counts as they were before it"""
    L, H, W = np.asarray(frames).shape[:3]
    ids = plan_np(L, scenes)
    cand = candidates_np(frames, fwd, bwd, ids, threshold, slack, **f)
    masks, counts = clean_np(cand, ids, support, radius, **f)
    over = counts > int(math.floor(max_fraction * H * W))
    masks[over] = 0
    if f.get("counts_after"):
        counts = np.where(over, 0, counts)
    return masks, counts


# ------------------------------------------------------------------------------------------------ the cases
def _grey(a):
    return np.repeat(np.asarray(a, np.uint8)[..., None], 3, axis=-1)


def _const_flows(L, H, W, f, b):
    fwd = np.empty((L - 1, H, W, 2), np.float32)
    bwd = np.empty_like(fwd)
    fwd[...], bwd[...] = f, b
    return fwd, bwd


def _case(frames, fwd, bwd, **kw):
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    c = dict(frames=frames, fwd=np.ascontiguousarray(fwd, dtype=np.float32), bwd=np.ascontiguousarray(bwd, dtype=np.float32),
             L=frames.shape[0], H=frames.shape[1], W=frames.shape[2], scenes=None, threshold=16, slack=0, support=3, radius=1,
             max_fraction=0.02)
    c.update(kw)
    for k in ("frames", "fwd", "bwd"):
        c[k].setflags(write=False)
    return c


def _zero_7x5():
    rng = np.random.RandomState(11)
    fr = rng.randint(0, 256, (3, 7, 5, 3)).astype(np.uint8)
    # exact ties at (x, y) = (1, 1) and (3, 4): the envelope of both neighbours is the 2 x 2 block from there, grey, top value 100 /
    # bottom value 150; the centre pixel is grey 116 = hi + tau (not brighter) and 134 = lo - tau (not darker); one level further
    # at (1, 4) and (3, 1) they are
    for (x, y), env, centre in (((1, 1), (100, 90), 116), ((3, 4), (150, 160), 134), ((1, 4), (100, 90), 117), ((3, 1), (150, 160), 133)):
        for n in (0, 2):
            fr[n, y:y + 2, x:x + 2] = env[1]
            fr[n, y, x] = env[0]
        fr[1, y, x] = centre
    return _case(fr, *_const_flows(3, 7, 5, 0.0, 0.0), support=1, radius=0, max_fraction=1.0)


def _shift_17x301():
    rng = np.random.RandomState(12)
    fr = rng.randint(0, 256, (3, 17, 301, 3)).astype(np.uint8)
    return _case(fr, *_const_flows(3, 17, 301, (90.0, 2.0), (-90.0, -2.0)), support=1, radius=1, max_fraction=1.0)


def _half_9x13():
    rng = np.random.RandomState(13)
    fr = rng.randint(0, 256, (4, 9, 13, 3)).astype(np.uint8)
    return _case(fr, *_const_flows(4, 9, 13, (-0.5, -0.5), (-0.5, -0.5)), threshold=4, support=1, radius=0, max_fraction=1.0)


def _wave_70x90():
    """a smooth texture under a smooth, non-rigid motion with a little noise on top, flows solved to a fixed point in each
    direction (so bwd is not -fwd), bright and dark blotches on frames 1 and 2, and frame 4 a flash: over the guard"""
    L, H, W = 6, 70, 90
    rng = np.random.RandomState(14)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)

    def disp(t, x, y):
        return 2.5 * t + 4.0 * np.sin(y / 9.0 + 0.7 * t), -1.5 * t + 3.0 * np.cos(x / 11.0 - 0.5 * t)

    def tex(u, v):
        return 128 + 55 * np.sin(u / 3.1) * np.cos(v / 2.7) + 30 * np.sin((u + v) / 7.0)

    fr = np.empty((L, H, W), np.float64)
    for t in range(L):
        dx, dy = disp(t, xs, ys)
        fr[t] = tex(xs + dx, ys + dy)
    fr = np.clip(np.rint(fr + rng.randint(-6, 7, fr.shape)), 0, 255)

    def solve(src, dst):                                 # the flow from frame src to frame dst on src's grid
        dx, dy = disp(src, xs, ys)
        qx, qy = xs.copy(), ys.copy()
        for _ in range(30):
            ex, ey = disp(dst, qx, qy)
            qx, qy = xs + dx - ex, ys + dy - ey
        return np.stack([qx - xs, qy - ys], -1)

    fwd = np.stack([solve(t, t + 1) for t in range(L - 1)])
    bwd = np.stack([solve(t + 1, t) for t in range(L - 1)])
    for t, n in ((1, 6), (2, 6)):
        for _ in range(n):
            h, w = rng.randint(2, 8, 2)
            y, x = rng.randint(0, H - h), rng.randint(0, W - w)
            fr[t, y:y + h, x:x + w] = 235 if rng.rand() < 0.5 else 20
    fr[4] = np.clip(fr[4] + 120, 0, 255)
    return _case(_grey(fr), fwd, bwd, max_fraction=0.2)


def _nonfinite_33x64():
    rng = np.random.RandomState(15)
    L, H, W = 4, 33, 64
    fr = rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)
    fwd = rng.uniform(-3, 3, (L - 1, H, W, 2)).astype(np.float32)
    bwd = rng.uniform(-3, 3, (L - 1, H, W, 2)).astype(np.float32)
    bad = (np.nan, np.inf, -np.inf, 1e30, -1e30)
    for k, v in enumerate(bad):
        for fl, ch, y in ((fwd, 0, 2), (fwd, 1, 8), (bwd, 0, 14), (bwd, 1, 20)):
            fl[:, y + k % 3:y + k % 3 + 2, 6 * k + 3:6 * k + 9, ch] = v
    fwd[:, 28:, 40:, :] = np.nan
    bwd[:, :3, 50:, :] = np.inf
    return _case(fr, fwd, bwd, threshold=2, support=2, radius=1, max_fraction=1.0)


def _cuts_L7():
    rng = np.random.RandomState(16)
    fr = rng.randint(0, 256, (7, 6, 9, 3)).astype(np.uint8)
    return _case(fr, *_const_flows(7, 6, 9, 0.0, 0.0), scenes=[3], threshold=8, support=1, radius=0, max_fraction=1.0)


def _corner_slack2():
    rng = np.random.RandomState(17)
    fr = rng.randint(90, 170, (3, 5, 6, 3)).astype(np.uint8)
    fr[1] = rng.randint(0, 256, (5, 6, 3))
    fwd = rng.uniform(-1.5, 1.5, (2, 5, 6, 2)).astype(np.float32)
    bwd = rng.uniform(-1.5, 1.5, (2, 5, 6, 2)).astype(np.float32)
    return _case(fr, fwd, bwd, threshold=0, slack=2, support=1, radius=0, max_fraction=1.0)


def _planted(shape, blotches, seed):
    rng = np.random.RandomState(seed)
    fr = rng.randint(96, 105, (3,) + shape).astype(np.uint8)
    for y, x, h, w, v in blotches:
        fr[1, y:y + h, x:x + w] = v
    return _grey(fr)


def _radius16_20x20():
    fr = _planted((20, 20), [(3, 4, 2, 2, 235), (15, 17, 1, 1, 20), (10, 9, 1, 2, 235)], 18)
    return _case(fr, *_const_flows(3, 20, 20, 0.0, 0.0), support=3, radius=16, max_fraction=1.0)


def _support9():
    fr = _planted((8, 9), [(0, 0, 3, 3, 235), (3, 4, 4, 4, 20)], 19)
    return _case(fr, *_const_flows(3, 8, 9, 0.0, 0.0), support=9, radius=0, max_fraction=1.0)


def _short(L):
    rng = np.random.RandomState(20 + L)
    fr = rng.randint(0, 256, (L, 4, 6, 3)).astype(np.uint8)
    fwd = np.zeros((max(L - 1, 0), 4, 6, 2), np.float32)
    return _case(fr, fwd, fwd.copy(), threshold=0, support=1, radius=0, max_fraction=1.0)


_BUILDERS = {"zero_7x5": _zero_7x5, "shift_17x301": _shift_17x301, "half_9x13": _half_9x13, "wave_70x90": _wave_70x90,
             "nonfinite_33x64": _nonfinite_33x64, "cuts_L7": _cuts_L7, "corner_slack2": _corner_slack2,
             "radius16_20x20": _radius16_20x20, "support9": _support9, "short_L1": lambda: _short(1), "short_L2": lambda: _short(2)}
NAMES = tuple(_BUILDERS)
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def settings(c):
    return dict(scenes=c["scenes"], threshold=c["threshold"], slack=c["slack"], support=c["support"], radius=c["radius"],
                max_fraction=c["max_fraction"])


def want(name, **f):
    """(cand, masks before the guard, masks, counts) of a case under the definition (or a variant's flags); computed once, read-only"""
    key = (name,) + tuple(sorted(f))
    if key not in _WANT:
        c = case(name)
        ids = plan_np(c["L"], c["scenes"])
        cand = candidates_np(c["frames"], c["fwd"], c["bwd"], ids, c["threshold"], c["slack"], **f)
        raw, _ = clean_np(cand, ids, c["support"], c["radius"], **f)
        masks, counts = detect_np(c["frames"], c["fwd"], c["bwd"], **dict(settings(c), **f))
        for a in (cand, raw, masks, counts):
            a.setflags(write=False)
        _WANT[key] = (cand, raw, masks, counts)
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ the statistics video
STATS_BORDER = 12


def tennis_video(root, planted=False, seed=0, length=7, step=(1.5, 0.5)):
    """The video the defaults were measured on: frame 0 of tests/golden/tennis25.npz translated by ``step`` pixels per frame with
    PIL's BICUBIC affine transform, with the ideal flows -> (frames [L,H,W,3], fwd, bwd, planted bool [L,H,W]).  ``planted``: 30
    grey rectangles per centre frame, luma 20 or 235, sides 2-7 px, inside the judged region."""
    import os

    from PIL import Image
    with np.load(os.path.join(root, "tests", "golden", "tennis25.npz")) as z:
        base = np.asarray(z[[k for k in z.files if z[k].ndim == 4][0]][0], np.uint8)
    H, W = base.shape[:2]
    img = Image.fromarray(base)
    fr = np.stack([np.asarray(img.transform((W, H), Image.AFFINE, (1, 0, -step[0] * t, 0, 1, -step[1] * t), resample=Image.BICUBIC))
                   for t in range(length)])
    fwd, bwd = _const_flows(length, H, W, step, (-step[0], -step[1]))
    marks = np.zeros((length, H, W), bool)
    if planted:
        fr = fr.copy()
        rng = np.random.RandomState(seed)
        b = STATS_BORDER
        for t in range(1, length - 1):
            for _ in range(30):
                h, w = rng.randint(2, 8, 2)
                y, x = rng.randint(b, H - b - h + 1), rng.randint(b, W - b - w + 1)
                fr[t, y:y + h, x:x + w] = 235 if rng.rand() < 0.5 else 20
                marks[t, y:y + h, x:x + w] = True
    return fr, fwd, bwd, marks
