"""The line-scratch detector restated in numpy (video.detect_line_scratches, ops.line_sums, ops.line_columns, ops.line_paint; the
definition is in include/e2fgvi_hip.h), the named cases the device code is compared with entry for entry and byte for byte, mutated
restatements (VARIANTS) that must each differ from the definition on some case -- which is what shows that the cases can see such
a mistake -- and the planted videos the defaults were measured on.  Integers throughout: there is no tolerance anywhere."""
import os

import numpy as np

DEFAULTS = dict(rows=16, tau=6, gap=2, side=3, drift=1, coverage=50, span=2, persist=3, radius=2)
FLAGS = ("ge", "sides_with_gap", "merged", "across_cut", "persist_fixed", "no_remainder", "no_drift_near", "no_drift_vote",
         "coverage_floor")
VARIANTS = tuple((name, {name: True}) for name in FLAGS)
#   ge               >= and <= in place of > and <
#   sides_with_gap   the side columns start right beside the centre: the gap is compared with too
#   merged           bright and dark candidates are counted together
#   across_cut       frames of another scene vote
#   persist_fixed    `persist` is not reduced to the number of frames that can vote
#   no_remainder     the H mod rows rows at the bottom are never painted
#   no_drift_near    the height count looks at the column alone
#   no_drift_vote    the votes look at the column alone
#   coverage_floor   cnt >= floor(coverage nb / 100) in place of cnt 100 >= coverage nb
KEYS = ("S", "cand", "cnt", "col", "b0", "b1", "keep", "counts", "masks")


def luma(frames):
    f = np.asarray(frames).astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def scene_of_np(length, scenes=None):
    """int32 [L]: the number of cuts at or in front of each frame"""
    s = np.zeros(length, np.int32)
    for c in scenes or []:
        s[int(c):] += 1
    return s


def sums_np(frames, rows):
    """S int32 [L,nb,W]: the luma summed over each band of `rows` rows; the H mod rows rows at the bottom are in no band"""
    Y = luma(frames)
    L, H, W = Y.shape
    nb = H // rows
    return Y[:, :nb * rows].reshape(L, nb, rows, W).sum(axis=2).astype(np.int32)


def candidates_np(S, rows, tau, gap, side, **f):
    """uint8 [L,nb,W]: bit 0 bright, bit 1 dark"""
    S = np.asarray(S).astype(np.int64)
    L, nb, W = S.shape
    bits = np.zeros((L, nb, W), np.uint8)
    m = gap + side
    if W < 2 * m + 1:
        return bits
    xs = np.arange(m, W - m)                            # the columns whose side columns all lie in the frame
    first = 1 if f.get("sides_with_gap") else gap + 1
    sides = [S[..., xs + s * d] for d in range(first, m + 1) for s in (-1, 1)]
    hi, lo = np.maximum.reduce(sides), np.minimum.reduce(sides)
    c = S[..., xs]
    if f.get("ge"):
        bright, dark = c >= hi + tau * rows, c <= lo - tau * rows
    else:
        bright, dark = c > hi + tau * rows, c < lo - tau * rows
    bits[..., xs] = bright.astype(np.uint8) | (dark.astype(np.uint8) << 1)
    return bits


def _spread(a, d):
    """OR over the columns x-d .. x+d, clipped at the frame (the last axis)"""
    out = a.copy()
    for k in range(1, d + 1):
        out[..., k:] |= a[..., :-k]
        out[..., :-k] |= a[..., k:]
    return out


def columns_np(bits, drift, coverage, **f):
    """(near bool [L,2,nb,W], cnt int32 [L,2,W], col uint8 [L,2,W], b0, b1 int32 [L,2,W]); polarity 0 bright, 1 dark; a column
    without a near band has b0 = nb and b1 = -1"""
    bits = np.asarray(bits)
    L, nb, W = bits.shape
    pol = np.stack([(bits & 1) != 0, (bits & 2) != 0], axis=1)
    if f.get("merged"):
        pol = np.stack([pol[:, 0] | pol[:, 1]] * 2, axis=1)
    near = pol if f.get("no_drift_near") else _spread(pol, drift)
    cnt = near.sum(axis=2).astype(np.int64)
    col = cnt >= (coverage * nb) // 100 if f.get("coverage_floor") else cnt * 100 >= coverage * nb
    some = near.any(axis=2)
    if nb == 0:
        col = np.zeros_like(some)                       # no band: nothing is judged (a variant's 0 >= 0 included)
    band = np.arange(nb)[None, None, :, None]
    b0 = np.where(near, band, nb).min(axis=2, initial=nb)
    b1 = np.where(near, band, -1).max(axis=2, initial=-1)
    return near, cnt.astype(np.int32), col.astype(np.uint8), b0.astype(np.int32), b1.astype(np.int32)


def keep_np(col, scene_of, drift, span, persist, **f):
    """(keep uint8 [L,2,W], counts int32 [L])"""
    col = np.asarray(col) != 0
    L = col.shape[0]
    coln = col if f.get("no_drift_vote") else _spread(col, drift)
    keep = np.zeros(col.shape, np.uint8)
    for t in range(L):
        us = [u for u in range(max(0, t - span), min(L, t + span + 1)) if f.get("across_cut") or scene_of[u] == scene_of[t]]
        votes = coln[us].sum(axis=0)
        need = persist if f.get("persist_fixed") else min(persist, len(us))
        keep[t] = col[t] & (votes >= need)
    return keep, keep.reshape(L, -1).sum(axis=1).astype(np.int32)


def paint_np(keep, b0, b1, H, rows, radius, **f):
    """uint8 [L,H,W] of 0 / 255"""
    L, _, W = keep.shape
    nb = H // rows
    P = np.zeros((L, nb, W), bool)
    for t, p, x in np.argwhere(np.asarray(keep) != 0):
        P[t, b0[t, p, x]:b1[t, p, x] + 1, max(0, x - radius):x + radius + 1] = True
    masks = np.zeros((L, H, W), np.uint8)
    masks[:, :nb * rows] = np.repeat(P, rows, axis=1) * 255
    if nb and not f.get("no_remainder"):
        masks[:, nb * rows:] = P[:, nb - 1:nb] * 255
    return masks


def detect_np(frames, scenes=None, rows=16, tau=6, gap=2, side=3, drift=1, coverage=50, span=2, persist=3, radius=2, **f):
    """every stage of the definition (or of a variant, by its flags) as a dict of KEYS"""
    frames = np.asarray(frames)
    L, H, W = frames.shape[:3]
    nb = H // rows
    S = sums_np(frames, rows)
    cand = candidates_np(S, rows, tau, gap, side, **f)
    _, cnt, col, b0, b1 = columns_np(cand, drift, coverage, **f)
    keep, counts = keep_np(col, scene_of_np(L, scenes), drift, span, persist, **f)
    masks = paint_np(keep, b0, b1, H, rows, radius, **f)
    return dict(S=S, cand=cand, cnt=cnt, col=col, b0=b0, b1=b1, keep=keep, counts=counts, masks=masks)


# ------------------------------------------------------------------------------------------------ the cases
def _grey(a):
    return np.repeat(np.asarray(a, np.uint8)[..., None], 3, axis=-1)


def _ground(L, H, W, seed, flat=None):
    """grey 118 .. 124, noise that no column stands out of; ``flat``: that grey level everywhere"""
    if flat is not None:
        return np.full((L, H, W), flat, np.int64)
    return np.random.RandomState(seed).randint(118, 125, (L, H, W)).astype(np.int64)


def _stripe(g, x, amp, profile=(1.0,), frames=None, rows=slice(None)):
    """adds amp * profile to the columns from x on, on the frames listed (all) and the rows given"""
    for t in (range(g.shape[0]) if frames is None else frames):
        for k, w in enumerate(profile):
            g[t, rows, x + k] += int(round(amp * w))
    return g


def _case(g, scenes=None, **kw):
    frames = np.ascontiguousarray(_grey(np.clip(g, 0, 255)))
    frames.setflags(write=False)
    c = dict(DEFAULTS, frames=frames, L=frames.shape[0], H=frames.shape[1], W=frames.shape[2], scenes=scenes)
    c.update(kw)
    return c


def _bright_w1():
    return _case(_stripe(_ground(5, 64, 50, 1), 20, 40))


def _dark_w2():
    return _case(_stripe(_ground(5, 64, 50, 2), 27, -40, (1.0, 1.0)))


def _both_w3():
    g = _stripe(_ground(5, 64, 50, 3), 11, 45, (0.5, 1.0, 0.5))
    return _case(_stripe(g, 35, -50))


def _edges(inside):
    """a scratch at the first and at the last column whose side columns lie in the frame (x = 5 and W - 6 at the defaults), or one
    column outside each"""
    W = 41
    g = _stripe(_ground(3, 48, W, 4), 5 if inside else 4, 40)
    return _case(_stripe(g, W - 6 if inside else W - 5, -40))


def _remainder():
    return _case(_stripe(_ground(4, 75, 46, 5), 22, 40))             # 4 bands and 11 rows more


def _mixed_column():
    """bands 0-1 bright and bands 2-3 dark in one column, band 4 clean: 40 % of the height each way"""
    g = _ground(4, 40, 37, 6)
    _stripe(g, 18, 40, rows=slice(0, 16))
    _stripe(g, 18, -40, rows=slice(16, 32))
    return _case(g, rows=8)


def _partial(bands):
    """a scratch over the top `bands` of five bands"""
    return _case(_stripe(_ground(4, 43, 37, 7), 15, 40, rows=slice(0, 8 * bands)), rows=8)


def _wander(step):
    """the scratch moves between bands: columns x0-1, x0, x0+1 in turn (step 1), or `step` columns further in every band"""
    g = _ground(4, 72, 60, 8)
    for b in range(9):
        _stripe(g, 20 + (b % 3 - 1 if step == 1 else b * step), 40, rows=slice(8 * b, 8 * b + 8))
    return _case(g, rows=8)


def _two_of_five():
    return _case(_stripe(_ground(5, 48, 40, 9), 17, 40, frames=(1, 3)))


def _cut():
    """frames 1-3 of the first scene and 4-5 of the second carry it: three votes in front of the cut, two of three behind it"""
    return _case(_stripe(_ground(8, 48, 40, 10), 17, 40, frames=(1, 2, 3, 4, 5)), scenes=[4])


def _single():
    return _case(_stripe(_ground(1, 48, 40, 11), 17, 40))


def _jitter2():
    """columns x0 and x0 + 2 in turn from frame to frame: the votes for x0 need the drift window"""
    g = _ground(5, 48, 40, 12)
    for t in range(5):
        _stripe(g, 17 + 2 * (t % 2), 40, frames=(t,))
    return _case(g)


def _strokes():
    """a texture of short vertical strokes, each one band high and on every frame: candidates, but no column has the height"""
    g = _ground(4, 64, 90, 13)
    rng = np.random.RandomState(14)
    for x in range(6, 84, 6):
        b = rng.randint(0, 4)
        _stripe(g, x, 40 if x % 12 else -40, rows=slice(16 * b, 16 * b + 16))
    return _case(g)


def _ties():
    """flat grey 100 (its luma is 100): 106 and 94 are exactly tau away and are no candidates, 107 and 93 are"""
    g = _ground(3, 32, 60, 0, flat=100)
    for x, v in ((10, 6), (22, 7), (36, -6), (48, -7)):
        _stripe(g, x, v)
    return _case(g)


def _nondefault():
    """every parameter off its default, W mod 4 = 2, twelve frames, two cuts, five scratches that come and go"""
    L, H, W = 12, 75, 110
    g = _ground(L, H, W, 15)
    _stripe(g, 30, 30, (1.0, 0.7))
    _stripe(g, 61, -35, frames=range(0, 7))
    _stripe(g, 85, 28, frames=(2, 3, 8), rows=slice(0, 56))
    _stripe(g, 4, 40)
    _stripe(g, 104, -40, (0.5, 1.0, 0.5), frames=range(5, 12))
    for t in range(L):
        _stripe(g, 45 + (t % 3), 33, frames=(t,), rows=slice(8, 75))
    return _case(g, scenes=[5, 9], rows=8, tau=10, gap=1, side=2, drift=2, coverage=60, span=1, persist=2, radius=3)


def _small():
    """less than one workgroup of anything: 9 x 13, rows = 4, W mod 4 = 1"""
    return _case(_stripe(_ground(2, 9, 13, 16), 6, 40), rows=4, gap=0, side=2, radius=16)


def _wide():
    """two tiles of the paint pass and two of the column pass: a scratch on either side of column 256 and one across it"""
    g = _ground(2, 20, 300, 17)
    for x, a in ((250, 40), (253, -40), (258, 40), (140, -40)):
        _stripe(g, x, a)
    return _case(g, rows=4, persist=2)


_BUILDERS = {"bright_w1": _bright_w1, "dark_w2": _dark_w2, "both_w3": _both_w3, "edges_in": lambda: _edges(True),
             "edges_out": lambda: _edges(False), "remainder_75": _remainder, "short_H": lambda: _case(_stripe(_ground(3, 12, 40, 18), 17, 40)),
             "narrow_W": lambda: _case(_stripe(_ground(3, 48, 10, 19), 5, 40)), "mixed_column": _mixed_column,
             "partial_40": lambda: _partial(2), "partial_60": lambda: _partial(3), "wander_drift": lambda: _wander(1),
             "wander_far": lambda: _wander(3), "two_of_five": _two_of_five, "cut_L8": _cut, "single_L1": _single, "jitter2": _jitter2,
             "strokes": _strokes, "ties": _ties, "nondefault_12x75x110": _nondefault, "small_9x13": _small, "wide_20x300": _wide}
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
        c = case(name)
        w = detect_np(c["frames"], **dict(settings(c), **f))
        for a in w.values():
            a.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ the statistics videos
def stats_video(root, which):
    """The clean videos the defaults were measured on: "translated" -- defect_cases.tennis_video(length=12), frame 0 of
    tests/golden/tennis25.npz moved (1.5, 0.5) px per frame -- and "raw", the 25 frames of that file as they are"""
    if which == "translated":
        from tests import defect_cases
        return defect_cases.tennis_video(root, length=12)[0]
    with np.load(os.path.join(root, "tests", "golden", "tennis25.npz")) as z:
        return np.asarray(z["frames"], np.uint8)


PLANT_PROFILES = ((1.0,), (0.6, 1.0), (0.5, 1.0, 0.5))


def plant(frames, seed, n=3, amplitude=None, width=None):
    """``n`` full-height scratches on every frame -> (frames, planted bool [L,H,W]): x0 uniform in [20, W - 20), width 1 to 3 with
    the profiles above, amplitude +-25 .. +-59 grey levels added to all channels and clipped, wandering as
    x0 + round(1.5 sin(0.7 t + i)).  ``amplitude`` / ``width``: fixed in place of drawn."""
    rng = np.random.RandomState(seed)
    L, H, W = frames.shape[:3]
    out = frames.astype(np.int64)
    marks = np.zeros((L, H, W), bool)
    for i in range(n):
        x0 = rng.randint(20, W - 20)
        wd = rng.randint(1, 4)
        amp = rng.randint(25, 60) * (1 if rng.rand() < 0.5 else -1)
        wd, amp = (wd if width is None else width), (amp if amplitude is None else amplitude)
        for t in range(L):
            x = x0 + int(round(1.5 * np.sin(0.7 * t + i)))
            for k, w in enumerate(PLANT_PROFILES[wd - 1]):
                out[t, :, x + k] += int(round(amp * w))
                marks[t, :, x + k] = True
    return np.clip(out, 0, 255).astype(np.uint8), marks


def recall_and_strays(masks, marks, reach=4):
    """(the share of planted pixels that are set, the number of set pixels farther than `reach` columns from a planted one)"""
    near = _spread(marks, reach)
    return float(((masks > 0) & marks).sum()) / max(int(marks.sum()), 1), int(((masks > 0) & ~near).sum())
