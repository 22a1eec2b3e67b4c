"""The weave stabiliser restated in numpy (video.stabilize, ops.weave_profiles, ops.weave_match, ops.weave_path, ops.weave_apply;
the definition is in include/e2fgvi_hip.h), the named cases the device code is compared with word for word and byte for byte,
mutated restatements (VARIANTS) that must each differ from the definition on a case named for them -- which is what shows that
the cases can see such a mistake -- and the planted weave the definition is judged on.  Integers throughout: there is no
tolerance anywhere.  Written unlike the kernels on purpose: slices and sums for the profiles, a sort over (cost, |s|, s) for the
best shift, Python ints, absolute paths summed segment by segment (the kernel works on differences around each frame)."""
import os

import numpy as np

NB = 8
SHIFT_LIMIT = 16 * 64                      # apply clamps a shift to +-64 px
DEFAULTS = dict(span=4, radius=16, max_shift=16, tex=2, subpixel=True)
KEYS = ("col", "row", "motion", "shift", "out", "mask")
# (flag, the case that must see it)
CAUGHT_BY = (
    ("shift_sign", "weave_40x52"),         # the frames are moved by -c: X = 16 x + cx
    ("tie_positive", "periodic_tie"),      # of two equal costs at -s and +s the positive shift wins
    ("no_c0_rule", "exact_edge"),          # delta from the parabola even when the best cost is 0
    ("upper_median", "two_motions"),       # the upper median of the valid bands
    ("asym_window", "weave_40x52"),        # the window is cut at the segment's ends, not shrunk on both sides
    ("across_cut", "cut_mid"),             # a cut does not break the segment
    ("across_untrusted", "flat_mid"),      # an untrusted pair does not break the segment
    ("mask_clamped", "sub_37x53"),         # the mask is taken from the taps after clamping: never set
    ("trunc_q", "sub_37x53"),              # q = floor(S / n), not rounded
    ("delta_trunc", "sub_37x53"),          # delta rounded toward zero, not down
    ("no_clamp", "clamp"),                 # c is not clamped to +-16 max_shift
    ("window_from_R", "weave_40x52"),      # the window starts at R, not R + 1
)
VARIANTS = tuple((name, {name: True}) for name, _ in CAUGHT_BY)


def luma(frames):
    a = np.asarray(frames).astype(np.int64)
    return (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8


def scene_of_np(length, scenes=None):
    """int32 [L]: the number of cuts at or in front of each frame"""
    s = np.zeros(length, np.int32)
    for c in scenes or []:
        s[int(c):] += 1
    return s


def profiles_np(frames):
    """(col int32 [L,8,W], row int32 [L,8,H])"""
    Y = luma(frames)
    L, H, W = Y.shape
    col = np.stack([Y[:, b * H // NB:(b + 1) * H // NB].sum(axis=1) for b in range(NB)], axis=1)
    row = np.stack([Y[:, :, b * W // NB:(b + 1) * W // NB].sum(axis=2) for b in range(NB)], axis=1)
    return col.astype(np.int32), row.astype(np.int32)


def gradient_np(P):
    P = np.asarray(P).astype(np.int64)
    g = np.zeros(len(P), np.int64)
    if len(P) > 2:
        g[1:-1] = P[2:] - P[:-2]
    return g


def band_motion_np(Pp, Pc, R, tex, **f):
    """the motion of one band in 1/16 px from the profiles of frames t - 1 and t, or None when the band is not valid (the caller
    has dropped empty bands)"""
    n = len(Pp)
    lo, hi = (R if f.get("window_from_R") else R + 1), n - R - 1
    if hi - lo < 2 * R:
        return None
    gp, gc = gradient_np(Pp), gradient_np(Pc)
    i = np.arange(lo, hi)
    cost = {s: int(np.abs(gc[i + s] - gp[i]).sum()) for s in range(-R, R + 1)}
    s = sorted(cost, key=lambda s: (cost[s], abs(s), -s if f.get("tie_positive") else s))[0]
    if not -R < s < R:
        return None
    cm, c0, cp = cost[s - 1], cost[s], cost[s + 1]
    den = cm - 2 * c0 + cp
    if den <= 0 or int(np.abs(gp[i]).sum()) < tex * (hi - lo):
        return None
    num = 16 * (cm - cp) + den
    if c0 == 0 and not f.get("no_c0_rule"):
        delta = 0
    elif f.get("delta_trunc"):
        delta = -((-num) // (2 * den)) if num < 0 else num // (2 * den)
    else:
        delta = num // (2 * den)
    return 16 * s + delta


def match_np(col, row, scene_of, radius, tex, **f):
    """int32 [L,4]: mx, my, nx, ny"""
    L, _, W = col.shape
    H = row.shape[2]
    motion = np.zeros((L, 4), np.int32)
    for t in range(1, L):
        if scene_of[t] != scene_of[t - 1]:
            continue
        for axis, (P, other) in enumerate(((col, H), (row, W))):
            vals = []
            for b in range(NB):
                if b * other // NB == (b + 1) * other // NB:
                    continue
                v = band_motion_np(P[t - 1, b], P[t, b], radius, tex, **f)
                if v is not None:
                    vals.append(v)
            vals.sort()
            if len(vals) >= NB // 2:
                motion[t, axis] = vals[len(vals) // 2 if f.get("upper_median") else (len(vals) - 1) // 2]
            motion[t, 2 + axis] = len(vals)
    return motion


def path_np(motion, scene_of, span, max_shift, subpixel=True, **f):
    """int32 [L,2]: cx, cy in 1/16 px"""
    L = len(motion)
    shift = np.zeros((L, 2), np.int32)
    for axis in range(2):
        starts = []
        for t in range(L):
            cut = t == 0 or scene_of[t] != scene_of[t - 1]
            untrusted = not cut and int(motion[t, 2 + axis]) < NB // 2
            if t == 0 or (cut and not f.get("across_cut")) or (untrusted and not f.get("across_untrusted")):
                starts.append(t)
        for first, nxt in zip(starts, starts[1:] + [L]):
            last = nxt - 1
            p, run = {}, 0
            for t in range(first, nxt):
                if t > first:
                    run += int(motion[t, axis])
                p[t] = run
            for t in range(first, nxt):
                if f.get("asym_window"):
                    us = range(max(first, t - span), min(last, t + span) + 1)
                else:
                    k = min(span, t - first, last - t)
                    us = range(t - k, t + k + 1)
                S, n = sum(p[u] for u in us), len(us)
                q = S // n if f.get("trunc_q") else (2 * S + n) // (2 * n)
                c = q - p[t]
                if not f.get("no_clamp"):
                    c = max(-16 * max_shift, min(16 * max_shift, c))
                if not subpixel:
                    c = ((c + 8) >> 4) << 4
                shift[t, axis] = c
    return shift


def apply_np(frames, shift, **f):
    """(out uint8 like frames -- [L,H,W,3] or [L,H,W] --, mask uint8 [L,H,W])"""
    a = np.asarray(frames)
    flat = a.ndim == 3
    src = (a[..., None] if flat else a).astype(np.int64)
    L, H, W, _ = src.shape
    out = np.zeros(src.shape, np.uint8)
    mask = np.zeros((L, H, W), np.uint8)
    if H * W == 0:
        return (out[..., 0] if flat else out), mask
    for t in range(L):
        cx, cy = (max(-SHIFT_LIMIT, min(SHIFT_LIMIT, int(v))) for v in shift[t])
        if f.get("shift_sign"):
            cx, cy = -cx, -cy
        X, Y = 16 * np.arange(W) - cx, 16 * np.arange(H) - cy
        x0, fx, y0, fy = X >> 4, X & 15, Y >> 4, Y & 15
        xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
        ya, yb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
        wx, wy = fx[None, :, None], fy[:, None, None]
        A, B, C, D = src[t][ya][:, xa], src[t][ya][:, xb], src[t][yb][:, xa], src[t][yb][:, xb]
        out[t] = ((16 - wx) * (16 - wy) * A + wx * (16 - wy) * B + (16 - wx) * wy * C + wx * wy * D + 128) >> 8
        if f.get("mask_clamped"):
            ox, oy = (xa < 0) | (xb > W - 1), (ya < 0) | (yb > H - 1)
        else:
            ox = (x0 < 0) | (x0 > W - 1) | ((fx > 0) & ((x0 + 1 < 0) | (x0 + 1 > W - 1)))
            oy = (y0 < 0) | (y0 > H - 1) | ((fy > 0) & ((y0 + 1 < 0) | (y0 + 1 > H - 1)))
        mask[t] = 255 * (oy[:, None] | ox[None, :])
    return (out[..., 0] if flat else out), mask


def stabilize_np(frames, scenes=None, span=4, radius=16, max_shift=16, tex=2, subpixel=True, **f):
    """every stage of the definition (or of a variant, by its flags) as a dict of KEYS"""
    frames = np.asarray(frames)
    L = frames.shape[0]
    so = scene_of_np(L, scenes)
    col, row = profiles_np(frames)
    if frames.shape[1] * frames.shape[2] == 0:
        motion = np.zeros((L, 4), np.int32)
    else:
        motion = match_np(col, row, so, radius, tex, **f)
    shift = path_np(motion, so, span, max_shift, subpixel, **f)
    out, mask = apply_np(frames, shift, **f)
    return dict(col=col, row=row, motion=motion, shift=shift, out=out, mask=mask)


# ------------------------------------------------------------------------------------------------ the cases
def texture(H, W, seed):
    """a colour image of random texture, softened once so that a sub-pixel move changes it smoothly: uint8 [H,W,3]"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (H + 1, W + 1, 3)).astype(np.int64)
    return ((a[:-1, :-1] + a[1:, :-1] + a[:-1, 1:] + a[1:, 1:] + 2) >> 2).astype(np.uint8)


MARGIN = 40


def crops(L, H, W, seed, plant_x=None, plant_y=None, pan=(0, 0), image=None):
    """a video cut from one larger image: frame t shows the image moved by t * pan + (plant_x[t], plant_y[t]) / 16 px -- whole
    pixels are crops, a fraction is apply_np's bilinear blend of a crop with a border that is cut off afterwards.  uint8
    [L,H,W,3]; |move| <= MARGIN - 8"""
    px = [0] * L if plant_x is None else [int(v) for v in plant_x]
    py = [0] * L if plant_y is None else [int(v) for v in plant_y]
    big = texture(H + 2 * MARGIN, W + 2 * MARGIN, seed) if image is None else image
    out = []
    for t in range(L):
        mx, my = 16 * pan[0] * t + px[t], 16 * pan[1] * t + py[t]
        wx, wy = mx >> 4, my >> 4                                   # the content moves by +m: the crop starts at MARGIN - m
        x0, y0 = MARGIN - wx, MARGIN - wy
        assert 8 <= x0 <= 2 * MARGIN - 8 and 8 <= y0 <= 2 * MARGIN - 8
        crop = big[y0 - 2:y0 + H + 2, x0 - 2:x0 + W + 2]
        if (mx & 15) or (my & 15):
            crop = apply_np(crop[None], np.array([[mx & 15, my & 15]]))[0][0]
        out.append(crop[2:2 + H, 2:2 + W])
    return np.stack(out)


def _case(frames, scenes=None, **kw):
    frames = np.ascontiguousarray(np.asarray(frames).astype(np.uint8))
    frames.setflags(write=False)
    c = dict(DEFAULTS, frames=frames, L=frames.shape[0], H=frames.shape[1], W=frames.shape[2], scenes=scenes)
    c.update(kw)
    return c


WEAVE9_X = (0, 16, -32, 16, 32, -16, 0, 32, -16)                    # whole pixels, in 1/16 px
WEAVE9_Y = (0, -16, 16, 32, -32, 0, 16, -16, 16)
SUB9_X = (0, 7, -21, 13, 30, -9, -3, 25, -14)                       # fractions of either sign
SUB9_Y = (0, -11, 5, -27, 19, 2, -6, 14, -1)


def _periodic_tie():
    """period 4 along x, the second frame two columns on: the costs at -2 and +2 are both 0"""
    rng = np.random.RandomState(41)
    base = np.array([20, 90, 200, 140])[np.arange(52) % 4][None, :] + rng.randint(0, 40, 40)[:, None]
    fr = np.stack([base, np.roll(base, 2, axis=1)])
    return _case(np.repeat(fr[..., None], 3, axis=-1), radius=4)


def _exact_edge():
    """two equal frames -- an exact match, c0 = 0 -- of faint texture with one strong edge between columns 3 and 4, just in front
    of the window [5, 47): it is in the cost at s - 1 alone, so the parabola's minimum is far from 0"""
    fr = 100 + (texture(40, 52, 47).astype(np.int64) >> 5)
    fr[:, :4] += 120
    return _case(np.stack([fr, fr]), radius=4)


def _two_motions():
    """the upper four bands move by +1, the lower four by +3 columns: the lower median is 16, the upper 48"""
    big = texture(40 + 2 * MARGIN, 56 + 2 * MARGIN, 42)
    top = crops(3, 40, 56, 0, plant_x=(0, 16, 32), image=big)
    low = crops(3, 40, 56, 0, plant_x=(0, 48, 96), image=big)
    return _case(np.concatenate([top[:, :20], low[:, 20:]], axis=1), radius=4, span=1)


def _flat_mid():
    fr = crops(9, 40, 52, 43, WEAVE9_X, WEAVE9_Y).copy()
    fr[4] = 117
    return _case(fr, radius=6, span=2)


_BUILDERS = {
    # whole-pixel weave on both axes; 40 x 52: W is a multiple of 4, the frames start on a dword
    "weave_40x52": lambda: _case(crops(9, 40, 52, 30, WEAVE9_X, WEAVE9_Y), radius=6, span=2),
    # fractions of either sign; neither side a multiple of 4 or 8, frames 1 .. start off a dword
    "sub_37x53": lambda: _case(crops(9, 37, 53, 31, SUB9_X, SUB9_Y), radius=4),
    "whole_37x53": lambda: _case(crops(9, 37, 53, 31, SUB9_X, SUB9_Y), radius=4, subpixel=False),
    # H < 8: row band 0 is empty and the y axis has no window
    "rows_7x64": lambda: _case(crops(2, 7, 64, 32, (0, 32)), radius=4),
    "one_1x1": lambda: _case(np.array([[[[10, 20, 30]]], [[[200, 100, 50]]]])),
    # a window shorter than 2 R on both axes: nothing is trusted
    "short_64x9": lambda: _case(crops(3, 64, 9, 33, None, (0, 16, -16))),
    "single": lambda: _case(crops(1, 40, 52, 34)),
    "pair": lambda: _case(crops(2, 40, 52, 35, (0, 32), (0, -16)), radius=4),
    "r1": lambda: _case(crops(3, 40, 52, 36, (0, 4, -3), (0, -5, 2)), radius=1),
    # R = 32 needs 130 elements: x alone; motions of up to 25 px
    "r32_8x141": lambda: _case(crops(3, 8, 141, 37, (0, 16 * 25, -16 * 3)), radius=32, max_shift=64),
    "span0": lambda: _case(crops(3, 40, 52, 38, (0, 32, -16), (0, 16, 16)), radius=4, span=0),
    "span1": lambda: _case(crops(9, 40, 52, 30, WEAVE9_X, WEAVE9_Y), radius=6, span=1),
    "span16": lambda: _case(crops(9, 40, 52, 30, WEAVE9_X, WEAVE9_Y), radius=6, span=16),
    "cut_mid": lambda: _case(crops(9, 40, 52, 39, WEAVE9_X, WEAVE9_Y), scenes=[4], radius=6, span=2),
    "flat_mid": _flat_mid,
    "flat": lambda: _case(np.full((3, 40, 52, 3), 90), radius=4),
    # +-6 px of weave along x under max_shift = 1 (R = 12: the y axis has no window)
    "clamp": lambda: _case(crops(9, 40, 52, 40, [3 * v for v in WEAVE9_X[:5]] + [0, 48, -48, 0], None), radius=12, max_shift=1),
    "periodic_tie": _periodic_tie,
    "exact_edge": _exact_edge,
    "two_motions": _two_motions,
    "pan": lambda: _case(crops(9, 40, 52, 44, pan=(2, -1)), radius=4),
    # more than 32 rows a band: two workgroups a band; and a row of more than 1024 pixels
    "tall_300x20": lambda: _case(crops(2, 300, 20, 45, None, (0, 32)), radius=4),
    "wide_9x1100": lambda: _case(crops(2, 9, 1100, 46, (0, -48)), radius=8),
}
NAMES = tuple(_BUILDERS)
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def settings(c):
    return {k: c[k] for k in ("scenes",) + tuple(DEFAULTS)}


def want(name, **f):
    """the dict of KEYS of a case under the definition (or a variant's flags); computed once, read-only"""
    key = (name,) + tuple(sorted(f))
    if key not in _WANT:
        w = stabilize_np(case(name)["frames"], **dict(settings(case(name)), **f))
        for a in w.values():
            a.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


# shift tables for the apply entry alone: beyond the frame, beyond the clamp, fractions of either sign, one axis at a time
APPLY_SHIFTS = np.array([[0, 0], [16, 0], [0, -16], [-5, 0], [0, 9], [-37, 43], [16 * 60, -16 * 70], [-2000, 2000], [15, 15]], np.int32)


# ------------------------------------------------------------------------------------------------ planted weave
def tennis25(root):
    with np.load(os.path.join(root, "tests", "golden", "tennis25.npz")) as z:
        return np.asarray(z["frames"], np.uint8)


def plant(frames, seed, amplitude=3):
    """whole-pixel weave: frame t moved by (dx, dy) drawn from [-amplitude, amplitude], the border replicated -> (planted, d int64
    [L,2] in px)"""
    d = np.random.default_rng(seed).integers(-amplitude, amplitude + 1, (len(frames), 2))
    return apply_np(frames, (16 * d).astype(np.int32))[0], d


def residual_rms(shift, d):
    """rms in px of the weave left in a video planted with ``d`` px and moved by ``shift`` 1/16 px, the mean taken out per axis"""
    left = np.asarray(d, np.float64) + np.asarray(shift, np.float64) / 16
    return float(np.sqrt(((left - left.mean(axis=0)) ** 2).mean()))
