"""The deinterlacer restated in numpy (video.deinterlace, video.detect_interlace, ops.deinterlace, ops.interlace_scores; the
definition is in include/e2fgvi_hip.h), the named cases the device code is compared with byte for byte and word for word, mutated
restatements (VARIANTS) that must each differ from the definition on a case named for them -- which is what shows that the cases
can see such a mistake -- and the planted clips the definition is judged on.  Integers throughout: there is no tolerance anywhere.
Written unlike the kernels on purpose: whole planes at once, index arrays for the rows and the columns, every picture computed in
full and the missing rows picked out of it afterwards."""
import itertools
import os

import numpy as np

DEFAULTS = dict(order="tff", rate="field", keep="first", guard=True, edges=0)
# every setting a case is run with: (tff, mode, guard, edges)
SETTINGS = tuple(itertools.product((1, 0), (0, 1, 2), (1, 0), (0, 1, 2)))
# (flag, the case that must see it, the settings it is seen at)
CAUGHT_BY = (
    ("t0_not_halved", "noise_37x53", (1, 0, 0, 0)),        # diff = max(t0, t1, t2)
    ("guard_clamped", "tiny_4x5", (1, 0, 1, 0)),           # rows y - 2, y + 2 clamped to the frame instead of the guard skipped
    ("two_without_one", "noise_37x53", (1, 0, 1, 2)),      # score(2 sgn) tried although score(sgn) was not taken
    ("plus_vs_zero", "noise_37x53", (1, 0, 1, 1)),         # the + side compared against score(0) - 1, not against the best so far
    ("no_minus_one", "smooth_37x53", (1, 0, 1, 1)),        # best = score(0): a direction is taken for a gain of 1
    ("second_field_pair", "noise_37x53", (1, 0, 1, 0)),    # the second picture takes A = P, B = C like the first
    ("missing_zero", "single_6x7", (1, 0, 1, 0)),          # a missing neighbour frame reads as zeros
    ("across_cut", "cut2_6x7", (1, 0, 1, 0)),              # a neighbour is taken across a cut
    ("wrap_columns", "tiny_4x5", (1, 0, 1, 2)),            # columns wrapped instead of clamped
    ("per_channel", "noise_37x53", (1, 0, 1, 0)),          # the decisions taken per channel, not on luma
    ("updn_border", "tiny_4x5", (0, 0, 1, 0)),             # up / dn clamped at the border rows, not mirrored
    ("round_up", "noise_37x53", (1, 0, 1, 0)),             # (a + b + 1) >> 1 in place of >> 1
    ("score_rows_odd", "tiny_5x4", None),                  # the scores over rows [1, H - 2] on odd H
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


def _half(a, b, f):
    return (a + b + (1 if f.get("round_up") else 0)) >> 1


def _columns(W, off, f):
    x = np.arange(W) + off
    return x % W if f.get("wrap_columns") else np.clip(x, 0, W - 1)


def _decide(YP, YC, YN, YA, YB, guard, edges, f):
    """(diff, J, up, dn) for every row of a picture as if it were missing: planes [H,W] and row tables [H]; H >= 2"""
    H, W = YC.shape
    y = np.arange(H)
    if f.get("updn_border"):
        up, dn = np.clip(y - 1, 0, H - 1), np.clip(y + 1, 0, H - 1)
    else:
        up, dn = np.where(y - 1 >= 0, y - 1, y + 1), np.where(y + 1 <= H - 1, y + 1, y - 1)
    c, e = YC[up], YC[dn]
    dY = _half(YA, YB, f)
    t0 = np.abs(YA - YB)
    t1 = _half(np.abs(YP[up] - c), np.abs(YP[dn] - e), f)
    t2 = _half(np.abs(YN[up] - c), np.abs(YN[dn] - e), f)
    diff = np.maximum(t0 if f.get("t0_not_halved") else t0 >> 1, np.maximum(t1, t2))

    def score(j):
        return sum(np.abs(c[:, _columns(W, k + j, f)] - e[:, _columns(W, k - j, f)]) for k in (-1, 0, 1))

    s0 = score(0)
    best = s0 - (0 if f.get("no_minus_one") else 1)
    J = np.zeros((H, W), np.int64)
    for sgn in (-1, 1):
        if edges >= 1:
            s1 = score(sgn)
            take = s1 < ((s0 - 1) if (sgn == 1 and f.get("plus_vs_zero")) else best)
            best = np.where(take, s1, best)
            J = np.where(take, sgn, J)
            if edges >= 2:
                s2 = score(2 * sgn)
                take2 = (take | bool(f.get("two_without_one"))) & (s2 < best)
                best = np.where(take2, s2, best)
                J = np.where(take2, 2 * sgn, J)
    if guard:
        ok = (y - 2 >= 0) & (y + 2 <= H - 1)
        if f.get("guard_clamped"):
            ok = np.ones(H, bool)
        ym, yp = np.clip(y - 2, 0, H - 1), np.clip(y + 2, 0, H - 1)
        b, fv = _half(YA[ym], YB[ym], f), _half(YA[yp], YB[yp], f)
        mx = np.maximum(np.maximum(dY - e, dY - c), np.minimum(b - c, fv - e))
        mn = np.minimum(np.minimum(dY - e, dY - c), np.maximum(b - c, fv - e))
        diff = np.where(ok[:, None], np.maximum(diff, np.maximum(mn, -mx)), diff)
    return diff, J, up, dn


def picture_np(P, C, N, A, B, p, guard, edges, **f):
    """one picture uint8 [H,W,3]: the rows of parity p of C kept, the others interpolated; P, C, N, A, B int64 [H,W,3]"""
    H, W, _ = C.shape
    out = C.copy()
    miss = (np.arange(H) & 1) != p
    if H == 1:
        if miss[0]:
            out[0] = _half(A[0], B[0], f)
        return out.astype(np.uint8)
    if f.get("per_channel"):
        planes = [tuple(a[..., ch] for a in (P, C, N, A, B)) for ch in range(3)]
    else:
        planes = [tuple(luma(a) for a in (P, C, N, A, B))] * 3
    rows = np.arange(H)[:, None]
    for ch in range(3):
        diff, J, up, dn = _decide(*planes[ch], guard, edges, f)
        x = np.arange(W)[None, :]
        if f.get("wrap_columns"):
            xa, xb = (x + J) % W, (x - J) % W
        else:
            xa, xb = np.clip(x + J, 0, W - 1), np.clip(x - J, 0, W - 1)
        sp = _half(C[..., ch][up[:, None] + 0 * rows, xa], C[..., ch][dn[:, None] + 0 * rows, xb], f)
        d = _half(A[..., ch], B[..., ch], f)
        full = np.minimum(np.maximum(sp, d - diff), d + diff)
        out[miss, :, ch] = full[miss]
    return out.astype(np.uint8)


def deinterlace_np(frames, scenes=None, tff=1, mode=0, guard=1, edges=0, **f):
    """uint8 [2L,H,W,3] (mode 0) or [L,H,W,3] (mode 1: the first field kept, mode 2: the second)"""
    fr = np.asarray(frames).astype(np.int64)
    L, H, W, _ = fr.shape
    so = scene_of_np(L, scenes)
    first = 0 if tff else 1
    O = np.zeros((2 * L, H, W, 3), np.uint8)
    if H * W == 0:
        return O if mode == 0 else O[:L]

    def neighbour(t, step):
        u = t + step
        if 0 <= u < L and (so[u] == so[t] or f.get("across_cut")):
            return fr[u]
        return np.zeros_like(fr[t]) if f.get("missing_zero") else fr[t]

    for t in range(L):
        P, C, N = neighbour(t, -1), fr[t], neighbour(t, 1)
        O[2 * t] = picture_np(P, C, N, P, C, first, guard, edges, **f)
        A, B = (P, C) if f.get("second_field_pair") else (C, N)
        O[2 * t + 1] = picture_np(P, C, N, A, B, 1 - first, guard, edges, **f)
    return O if mode == 0 else np.ascontiguousarray(O[mode - 1::2])


def scores_np(frames, scenes=None, **f):
    """D int64 [L,2]"""
    Y = luma(frames)
    L, H, W = Y.shape
    so = scene_of_np(L, scenes)
    D = np.zeros((L, 2), np.int64)
    m = (H - 2) // 2
    ys = np.arange(1, (H - 2 if f.get("score_rows_odd") else 2 * m) + 1)
    if H < 4 and not f.get("score_rows_odd"):
        ys = ys[:0]
    for t in range(L - 1):
        if so[t] != so[t + 1]:
            continue
        for q in (0, 1):
            r = ys[(ys & 1) == q]
            D[t, q] = np.abs(2 * Y[t + 1][r] - Y[t][r - 1] - Y[t][r + 1]).sum()
    return D


def field_order_np(D, scenes=None, margin=5):
    """(verdict, votes int8 [L]) from the scores, in Python integers"""
    L = len(D)
    so = scene_of_np(L, scenes)
    votes, pairs = np.zeros(L, np.int8), 0
    for t in range(L - 1):
        if so[t] != so[t + 1]:
            continue
        pairs += 1
        d0, d1 = int(D[t][0]), int(D[t][1])
        votes[t] = 1 if 100 * d0 < (100 - margin) * d1 else (-1 if 100 * d1 < (100 - margin) * d0 else 0)
    up, down = int((votes == 1).sum()), int((votes == -1).sum())
    if pairs == 0 or 4 * (up + down) < pairs:
        return "progressive", votes
    return ("tff" if up > 2 * down else "bff" if down > 2 * up else "mixed"), votes


# ------------------------------------------------------------------------------------------------ the cases
def _case(frames, scenes=None):
    frames = np.ascontiguousarray(np.asarray(frames).astype(np.uint8))
    frames.setflags(write=False)
    return dict(frames=frames, L=frames.shape[0], H=frames.shape[1], W=frames.shape[2], scenes=scenes)


def noise(L, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (L, H, W, 3))


def smooth(L, H, W, seed):
    """noise softened over 3 x 3 pixels and three frames, with a diagonal edge that moves: neighbouring scores differ by little, so
    that the order of the direction search matters"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (L + 2, H + 2, W + 2, 3)).astype(np.int64)
    s = sum(a[i:i + L, j:j + H, k:k + W] for i in range(3) for j in range(3) for k in range(3)) // 27
    yy, xx = np.mgrid[0:H, 0:W]
    for t in range(L):
        s[t][(xx + yy + 2 * t) % 11 < 5] += 60
    return np.clip(s, 0, 255)


TINY = tuple((H, W) for H in range(1, 7) for W in (1, 2, 3, 4, 5, 7))
_BUILDERS = {"tiny_%dx%d" % hw: (lambda hw=hw: _case(noise(3, hw[0], hw[1], 100 + 10 * hw[0] + hw[1]))) for hw in TINY}
_BUILDERS.update({
    # neither side a multiple of 4: every row but one in four starts off a dword
    "noise_37x53": lambda: _case(noise(3, 37, 53, 1)),
    "smooth_37x53": lambda: _case(smooth(3, 37, 53, 2)),
    # rows of more than 1024 pixels: five tiles a row, the last one short; and a tall narrow frame: five groups a row
    "wide_9x1100": lambda: _case(noise(2, 9, 1100, 3)),
    "tall_300x20": lambda: _case(noise(2, 300, 20, 4)),
    "single_6x7": lambda: _case(noise(1, 6, 7, 5)),
    "pair_6x7": lambda: _case(noise(2, 6, 7, 6)),
    "single_40x52": lambda: _case(noise(1, 40, 52, 7)),
    # a cut at every place of four frames, and at all of them
    "cut1_6x7": lambda: _case(noise(4, 6, 7, 8), [1]),
    "cut2_6x7": lambda: _case(noise(4, 6, 7, 8), [2]),
    "cut3_6x7": lambda: _case(noise(4, 6, 7, 8), [3]),
    "cuts_6x7": lambda: _case(noise(4, 6, 7, 8), [1, 2, 3]),
    "cut2_40x52": lambda: _case(noise(4, 40, 52, 9), [2]),
    # 0 and 255 alone: every clamp is reached
    "extremes_12x13": lambda: _case(255 * np.random.RandomState(10).randint(0, 2, (3, 12, 13, 3))),
    "extremes_40x52": lambda: _case(255 * np.random.RandomState(11).randint(0, 2, (3, 40, 52, 3))),
    # every score ties: J must stay 0
    "flat_8x9": lambda: _case(np.full((3, 8, 9, 3), 90)),
    "steps_8x9": lambda: _case(np.arange(3)[:, None, None, None] * 40 + np.arange(8)[None, :, None, None] * 9 + np.zeros((3, 8, 9, 3))),
})
NAMES = tuple(_BUILDERS)
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def want(name, setting, **f):
    """the output bytes of a case at (tff, mode, guard, edges) under the definition (or a variant's flags); computed once, read-only"""
    key = (name, tuple(setting)) + tuple(sorted(f))
    if key not in _WANT:
        tff, mode, guard, edges = setting
        c = case(name)
        if mode != 0 and not f:                                     # the frame-rate modes are the pictures of the field-rate result
            w = np.ascontiguousarray(want(name, (tff, 0, guard, edges))[mode - 1::2])
        else:
            w = deinterlace_np(c["frames"], c["scenes"], tff, mode, guard, edges, **f)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def want_scores(name, **f):
    key = (name, "scores") + tuple(sorted(f))
    if key not in _WANT:
        c = case(name)
        _WANT[key] = scores_np(c["frames"], c["scenes"], **f)
        _WANT[key].setflags(write=False)
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ planted clips
def tennis25(root):
    with np.load(os.path.join(root, "tests", "golden", "tennis25.npz")) as z:
        return np.asarray(z["frames"], np.uint8)


def interlace(source, tff=True):
    """2n progressive frames -> n interlaced ones: the pair (a, b) gives the even rows of a and the odd rows of b for
    top-field-first, the other way round for bottom-field-first"""
    a, b = source[0::2], source[1::2]
    out = np.array(a if tff else b)
    out[:, 1::2] = (b if tff else a)[:, 1::2]
    return out


def pan_clip(f, tff=True):
    """(12 interlaced frames, the 24 source frames)"""
    return interlace(f[:24], tff), f[:24]


def locked_off_clip(f):
    """16 copies of f[0]; copy k carries the patch f[12, 100:164, 200:264] at rows 60 + k, columns 40 + 3 k -> (8 interlaced frames,
    top field first, the 16 source frames)"""
    src = np.repeat(f[:1], 16, axis=0).copy()
    for k in range(16):
        src[k, 60 + k:124 + k, 40 + 3 * k:104 + 3 * k] = f[12, 100:164, 200:264]
    return interlace(src, True), src


def missing_rows(n_pictures, H, tff=True):
    """bool [n,H]: the rows that picture i of a field-rate result does not keep"""
    first = 0 if tff else 1
    kept = np.array([first if i % 2 == 0 else 1 - first for i in range(n_pictures)])
    return (np.arange(H)[None, :] & 1) != kept[:, None]


def psnr_missing(pictures, source, tff=True):
    """PSNR in dB over the missing rows alone"""
    miss = missing_rows(len(pictures), pictures.shape[1], tff)
    err = (np.asarray(pictures, np.float64) - np.asarray(source, np.float64))[miss]
    return float(10 * np.log10(255.0 ** 2 / np.mean(err ** 2)))


def line_average(frames, tff=True):
    """the field-rate yardstick: a missing row is (C[up] + C[dn]) >> 1"""
    fr = np.repeat(np.asarray(frames).astype(np.int64), 2, axis=0)
    H = fr.shape[1]
    y = np.arange(H)
    up, dn = np.where(y - 1 >= 0, y - 1, y + 1), np.where(y + 1 <= H - 1, y + 1, y - 1)
    avg = (fr[:, up] + fr[:, dn]) >> 1
    miss = missing_rows(len(fr), H, tff)
    out = fr.copy()
    out[miss] = avg[miss]
    return out.astype(np.uint8)


def weave_fields(frames):
    """the other yardstick: both pictures of a frame are the frame"""
    return np.repeat(np.asarray(frames), 2, axis=0)
