"""The deflicker restated in numpy (video.deflicker, ops.flicker_hist, ops.flicker_curves, ops.flicker_apply; the definition is in
include/e2fgvi_hip.h), the named cases the device code is compared with word for word and byte for byte, mutated restatements
(VARIANTS) that must each differ from the definition on some case -- which is what shows that the cases can see such a mistake --
and the planted flicker the defaults are judged on.  Integers throughout: there is no tolerance anywhere.  Written unlike the
kernels on purpose: np.bincount for the counts, Python ints and one walk up the levels for the nodes (the kernel bisects a scan),
plain loops for the windows."""
import os

import numpy as np

DEFAULTS = dict(span=4, max_shift=32)
NODES = 32
FLAGS = ("exclusive_cdf", "no_fraction", "across_cut", "trunc_mean", "no_clamp", "c2_no_hist", "d_toward_zero", "luma_no_round",
         "wrap", "per_channel")
VARIANTS = tuple((name, {name: True}) for name in FLAGS)
#   exclusive_cdf    the node's level is looked up in the exclusive sum C[v-1]: one level too high
#   no_fraction      Q = 16 v, the position inside the bin is dropped
#   across_cut       frames of another scene are averaged
#   trunc_mean       T = sum // n in place of the rounded mean
#   no_clamp         s is not clamped to +-16 max_shift
#   c2_no_hist       a level sits at the lower end of its bin: c2 = 2 C[y-1]
#   d_toward_zero    d = d16 / 16 rounded toward zero
#   luma_no_round    Y = (77 R + 150 G + 29 B) >> 8
#   wrap             the sum wraps modulo 256 in place of being clipped
#   per_channel      every byte is moved by the shift of its own value, not by that of its pixel's luma
KEYS = ("hist", "Q", "d", "out")


def luma(frames, **f):
    a = np.asarray(frames).astype(np.int64)
    return (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + (0 if f.get("luma_no_round") else 128)) >> 8


def scene_of_np(length, scenes=None):
    """int32 [L]: the number of cuts at or in front of each frame"""
    s = np.zeros(length, np.int32)
    for c in scenes or []:
        s[int(c):] += 1
    return s


def hist_np(frames, **f):
    """int32 [L,256]: the pixels of each frame per luma level"""
    Y = luma(frames, **f)
    return np.stack([np.bincount(y.ravel(), minlength=256) for y in Y]).astype(np.int32) if len(Y) else np.zeros((0, 256), np.int32)


def nodes_np(hist, **f):
    """int32 [L,32]: the quantile nodes of every row, in 1/16 levels; one walk up the levels per row, Python ints"""
    Q = np.zeros((len(hist), NODES), np.int32)
    for t, row in enumerate(np.asarray(hist)):
        h = [int(x) for x in row]
        N = sum(h)
        v, below = 0, 0                                  # below = C[v-1]
        for k in range(NODES):
            r = ((2 * k + 1) * N) // (2 * NODES)
            while below + h[v] <= r:                     # r < N: the walk ends at a level with pixels
                below += h[v]
                v += 1
            frac = 0 if f.get("no_fraction") else (16 * (r - below)) // h[v]
            Q[t, k] = 16 * (min(v + 1, 255) if f.get("exclusive_cdf") else v) + frac
    return Q


def nodes_sorted_np(frames):
    """the nodes again, from the sorted lumas and without a histogram: the level of node k is the r_k-th smallest luma"""
    Y = luma(frames)
    Q = np.zeros((len(Y), NODES), np.int32)
    for t, y in enumerate(Y):
        ys = np.sort(y.ravel())
        N = len(ys)
        for k in range(NODES):
            r = ((2 * k + 1) * N) // (2 * NODES)
            v = int(ys[r])
            lo, hi = int(np.searchsorted(ys, v, "left")), int(np.searchsorted(ys, v, "right"))
            Q[t, k] = 16 * v + (16 * (r - lo)) // (hi - lo)
    return Q


def windows_np(scene_of, span, **f):
    """for every frame the list of the frames it is averaged over"""
    L = len(scene_of)
    return [[u for u in range(L) if abs(u - t) <= span and (f.get("across_cut") or scene_of[u] == scene_of[t])] for t in range(L)]


def curves_np(hist, scene_of, span, max_shift, **f):
    """(Q int32 [L,32], d int16 [L,256]) of the rows of ``hist``, every one of which sums to the same N >= 1"""
    hist = np.asarray(hist)
    L = len(hist)
    Q = nodes_np(hist, **f)
    d = np.zeros((L, 256), np.int16)
    K = NODES
    for t, us in enumerate(windows_np(scene_of, span, **f)):
        n = len(us)
        s = []
        for k in range(K):
            total = sum(int(Q[u, k]) for u in us)
            T = total // n if f.get("trunc_mean") else (2 * total + n) // (2 * n)
            v = T - int(Q[t, k])
            s.append(v if f.get("no_clamp") else max(-16 * max_shift, min(16 * max_shift, v)))
        h = [int(x) for x in hist[t]]
        N, below = sum(h), 0
        for y in range(256):
            c2 = 2 * below + (0 if f.get("c2_no_hist") else h[y])
            phi = max(0, min((K - 1) * 256, (c2 * K * 128) // N - 128))
            k0, fr = phi >> 8, phi & 255
            k1 = min(k0 + 1, K - 1)
            d16 = (s[k0] * (256 - fr) + s[k1] * fr + 128) >> 8
            if f.get("d_toward_zero"):
                d[t, y] = -((-d16) // 16) if d16 < 0 else d16 // 16
            else:
                d[t, y] = (d16 + 8) >> 4
            below += h[y]
    return Q, d


def apply_np(frames, d, **f):
    """uint8 [L,H,W,3]: every pixel moved by the shift of its luma, clipped"""
    a = np.asarray(frames).astype(np.int64)
    d = np.asarray(d).astype(np.int64)
    out = np.empty_like(a)
    for t in range(len(a)):
        out[t] = a[t] + (d[t][a[t]] if f.get("per_channel") else d[t][luma(a[t], **f)][..., None])
    return (out & 255 if f.get("wrap") else np.clip(out, 0, 255)).astype(np.uint8)


def deflicker_np(frames, scenes=None, span=4, max_shift=32, **f):
    """every stage of the definition (or of a variant, by its flags) as a dict of KEYS"""
    frames = np.asarray(frames)
    L, H, W = frames.shape[:3]
    hist = hist_np(frames, **f)
    if H * W == 0:
        Q, d = np.zeros((L, NODES), np.int32), np.zeros((L, 256), np.int16)
    else:
        Q, d = curves_np(hist, scene_of_np(L, scenes), span, max_shift, **f)
    return dict(hist=hist, Q=Q, d=d, out=apply_np(frames, d, **f))


# ------------------------------------------------------------------------------------------------ the cases
def _image(H, W, seed):
    """a colour image with a wide luma range: two ramps and noise, int64 [H,W,3]"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    g = 30 + (150 * yy) // max(H - 1, 1) + (40 * xx) // max(W - 1, 1)
    return np.clip(g[..., None] + rng.randint(-25, 26, (H, W, 3)), 0, 255).astype(np.int64)


def _flickered(L, H, W, seed, gains, offsets):
    """one image moving two pixels a frame, frame t at gains[t] / 256 and offsets[t]"""
    base = _image(H, W, seed)
    return np.stack([np.clip((np.roll(base, 2 * t, axis=1) * gains[t % len(gains)]) // 256 + offsets[t % len(offsets)], 0, 255)
                     for t in range(L)])


def _case(frames, scenes=None, **kw):
    frames = np.ascontiguousarray(np.asarray(frames).astype(np.uint8))
    frames.setflags(write=False)
    c = dict(DEFAULTS, frames=frames, L=frames.shape[0], H=frames.shape[1], W=frames.shape[2], scenes=scenes)
    c.update(kw)
    return c


GAINS, OFFSETS = (256, 282, 231, 270, 240), (0, -7, 6, 3, -5)


def _black_white():
    return _case(np.stack([np.zeros((6, 9, 3)), np.full((6, 9, 3), 255)]))


def _flat():
    """260 x 260 = 67 600 pixels in one bin: more than 16 bits"""
    return _case(np.stack([np.full((260, 260, 3), 90), np.full((260, 260, 3), 130)]))


def _two_level():
    """levels 40 and 200 only, in three proportions: most nodes of a frame share a bin"""
    fr = np.full((3, 13, 17, 3), 40)
    for t, rows in enumerate((3, 6, 10)):
        fr[t, :rows] = 200
    return _case(fr)


def _clip():
    """saturated colours -- channels at 0 and 255 beside mid-grey lumas -- under strong flicker: the sums leave [0, 255] at both ends"""
    rng = np.random.RandomState(31)
    fr = _flickered(4, 19, 22, 30, (256, 330, 190, 300), (0, 20, -25, 10))
    for t in range(4):
        for c in range(3):
            m = rng.rand(19, 22)
            fr[t, :, :, c] = np.where(m < 0.15, 0, np.where(m > 0.85, 255, fr[t, :, :, c]))
    return _case(fr)


def _rolled():
    base = _image(16, 18, 32)
    return _case(np.stack([np.roll(base, (3 * t, 5 * t), axis=(0, 1)) for t in range(5)]))


def _big_N():
    """curves alone, N = 2^26: a flat row, an even row, and a two-level row with odd counts"""
    N = 1 << 26
    hist = np.zeros((3, 256), np.int32)
    hist[0, 200] = N
    hist[1, :] = N // 256
    hist[2, 3], hist[2, 250] = N - 12345677, 12345677
    hist.setflags(write=False)
    return dict(DEFAULTS, frames=None, hist=hist, L=3, N=N, scenes=None, max_shift=64)


_BUILDERS = {
    "5x7": lambda: _case(_flickered(3, 5, 7, 20, GAINS, OFFSETS)),                       # W mod 4 = 3, 35 pixels: no multiple of 64
    "3x70x300": lambda: _case(_flickered(3, 70, 300, 21, GAINS, OFFSETS)),               # 21 000 pixels: several workgroups a frame
    "w1_33x41": lambda: _case(_flickered(4, 33, 41, 22, GAINS, OFFSETS)),                # W mod 4 = 1; frames 1 .. 3 start off a dword
    "w2_30x42": lambda: _case(_flickered(4, 30, 42, 23, GAINS, OFFSETS)),                # W mod 4 = 2, N mod 4 = 0
    "black_white": _black_white,
    "flat_260": _flat,
    "two_level": _two_level,
    "single": lambda: _case(_flickered(1, 9, 11, 24, GAINS, OFFSETS)),
    "span_gt_L": lambda: _case(_flickered(3, 10, 11, 25, GAINS, OFFSETS), span=8),
    "cuts_ends": lambda: _case(_flickered(6, 12, 14, 26, GAINS, OFFSETS), scenes=[1, 5]),
    "nondefault": lambda: _case(_flickered(9, 20, 23, 27, (256, 320, 200, 290), (0, 12, -14)), scenes=[4], span=2, max_shift=5),
    "clip": _clip,
    "rolled": _rolled,
    "big_N": _big_N,
}
NAMES = tuple(_BUILDERS)
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def settings(c):
    return {k: c[k] for k in ("scenes",) + tuple(DEFAULTS)}


def keys(name):
    """the KEYS a case has: a case without frames (curves alone) has Q and d"""
    return KEYS if case(name)["frames"] is not None else ("Q", "d")


def want(name, **f):
    """the dict of keys(name) of a case under the definition (or a variant's flags); computed once, read-only"""
    key = (name,) + tuple(sorted(f))
    if key not in _WANT:
        c = case(name)
        if c["frames"] is None:
            Q, d = curves_np(c["hist"], scene_of_np(c["L"], c["scenes"]), c["span"], c["max_shift"], **f)
            w = dict(Q=Q, d=d)
        else:
            w = deflicker_np(c["frames"], **dict(settings(c), **f))
        for a in w.values():
            a.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ planted flicker
def tennis25(root):
    with np.load(os.path.join(root, "tests", "golden", "tennis25.npz")) as z:
        return np.asarray(z["frames"], np.uint8)


def plant(frames, seed):
    """exposure flicker: frame t times a gain drawn from [0.9, 1.1] plus an offset drawn from [-8, 8], rounded and clipped"""
    rng = np.random.RandomState(seed)
    L = len(frames)
    gain, off = rng.uniform(0.9, 1.1, L), rng.uniform(-8.0, 8.0, L)
    out = np.asarray(frames).astype(np.float64) * gain[:, None, None, None] + off[:, None, None, None]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def roughness(frames):
    """the mean |second difference| along time of the frames' mean luma"""
    m = luma(frames).reshape(len(frames), -1).mean(axis=1)
    return float(np.abs(m[2:] - 2 * m[1:-1] + m[:-2]).mean())
