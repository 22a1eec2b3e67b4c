"""The colour restoration restated in numpy (video.restore_color, video.apply_color, ops.color_hist, ops.color_nodes, ops.color_lut,
ops.color_apply; the definition is in include/e2fgvi_hip.h), the named cases the device code is compared with word for word and
byte for byte, mutated restatements (VARIANTS) that must each differ from the definition on some case -- which is what shows that
the cases can see such a mistake -- and the planted fades the tool is judged on.  Integers throughout: there is no tolerance
anywhere.  Written unlike the kernels on purpose: np.bincount for the counts, Python ints and one walk up the levels for the
nodes (the kernel bisects a 64-bit scan), plain loops for the tables, one fancy index for the apply."""
import os

import numpy as np

DEFAULTS = dict(clip=(5, 5), target=None, min_range=32, max_gain=768, strength=256)
NODES = 32
NQ = NODES + 2
KEEP, LEVELS, MATCH = 0, 1, 2
FLAGS = ("exclusive_cdf", "no_fraction", "white_off_by_one", "across_cut", "next_channel", "no_gain_limit", "usability_ignored",
         "div_toward_zero", "strength_trunc", "first_tied", "ends_by_slope")
VARIANTS = tuple((name, {name: True}) for name in FLAGS)
#   exclusive_cdf      the node's level is looked up in the exclusive sum C[v-1]: one level too high
#   no_fraction        node = 16 v, the position inside the bin is dropped
#   white_off_by_one   the white point is node(N - (hi N) // 1000)
#   across_cut         a scene's own frames are pooled with those of the other scenes
#   next_channel       byte c is looked up in the table of channel (c + 1) mod 3
#   no_gain_limit      num = Wt - B
#   usability_ignored  every channel with w > b takes part in the levels
#   div_toward_zero    the divisions of the tables round toward zero
#   strength_trunc     o' = x + (((o - x) strength) >> 8)
#   first_tied         of several equal nodes q[k] <= x the first is taken (and its empty segment divides by 1)
#   ends_by_slope      beyond the first and the last node the curve goes on with the end segment's slope
KEYS = ("hist", "Q", "T", "lut", "out")


# ------------------------------------------------------------------------------------------------ the definition
def hist_np(frames):
    """int32 [L,3,256]: the pixels of each frame per channel and byte value; one bincount"""
    a = np.asarray(frames)
    L = a.shape[0]
    if a.size == 0:
        return np.zeros((L, 3, 256), np.int32)
    a = a.reshape(L, -1, 3).astype(np.int64)
    idx = (np.arange(L, dtype=np.int64)[:, None, None] * 3 + np.arange(3)[None, None, :]) * 256 + a
    return np.bincount(idx.ravel(), minlength=L * 768).reshape(L, 3, 256).astype(np.int32)


def csr(groups):
    """lists of frame numbers -> (starts int32 [G+1], ids int32 [M])"""
    return (np.cumsum([0] + [len(g) for g in groups]).astype(np.int32), np.array([t for g in groups for t in g], np.int32).reshape(-1))


def _node(P, r, **f):
    """node(r) of one pooled row of Python ints: one walk up the levels"""
    v, below = 0, 0                                      # below = C[v-1]
    while v < 255 and below + P[v] <= r:
        below += P[v]
        v += 1
    frac = 0 if f.get("no_fraction") else max(0, min(15, (16 * (r - below)) // max(P[v], 1)))
    return 16 * (min(v + 1, 255) if f.get("exclusive_cdf") else v) + frac


def nodes_np(hist, starts, ids, clip=(5, 5), **f):
    """int32 [G,3,34]: per group and channel 32 quantiles, the black and the white point of the pooled histogram, in 1/16 levels"""
    hist, starts, ids = np.asarray(hist), [int(s) for s in np.asarray(starts)], np.asarray(ids).astype(np.int64)
    L, M, G = len(hist), len(ids), len(starts) - 1
    lo, hi = clip
    Q = np.zeros((G, 3, NQ), np.int32)
    for g in range(G):
        mine = ids[min(max(starts[g], 0), M):min(max(starts[g + 1], 0), M)]
        mine = mine[(mine >= 0) & (mine < L)]
        if not len(mine):
            continue
        pool = hist[mine].sum(axis=0, dtype=np.int64)
        for c in range(3):
            P = [int(x) for x in pool[c]]
            N = sum(P)
            if N == 0:
                continue
            rs = [((2 * k + 1) * N) // 64 for k in range(NODES)] + [(lo * N) // 1000]
            rs.append(N - (hi * N) // 1000 - (0 if f.get("white_off_by_one") else 1))
            Q[g, c] = [_node(P, r, **f) for r in rs]
    return Q


def nodes_sorted_np(values, clip=(5, 5)):
    """the 34 nodes of one channel again, from its pooled bytes sorted and without a histogram: the level of a node is the r-th
    smallest byte"""
    ys = np.sort(np.asarray(values).ravel())
    N = len(ys)
    rs = [((2 * k + 1) * N) // 64 for k in range(NODES)] + [(clip[0] * N) // 1000, N - 1 - (clip[1] * N) // 1000]
    out = []
    for r in rs:
        v = int(ys[r])
        lo, hi = int(np.searchsorted(ys, v, "left")), int(np.searchsorted(ys, v, "right"))
        out.append(16 * v + (16 * (r - lo)) // (hi - lo))
    return np.array(out, np.int32)


def _div(a, b, **f):
    if f.get("div_toward_zero"):
        return -((-a) // b) if a < 0 else a // b
    return a // b


def lut_np(Q, mode, T=None, target=None, min_range=32, max_gain=768, strength=256, **f):
    """uint8 [G,3,256]: the byte tables of the groups"""
    Q = np.asarray(Q)
    T = Q if T is None else np.asarray(T)
    G = len(Q)
    lut = np.zeros((G, 3, 256), np.uint8)
    for g in range(G):
        b = [int(Q[g, c, NODES]) for c in range(3)]
        w = [int(Q[g, c, NODES + 1]) for c in range(3)]
        usable = [(w[c] > b[c]) if f.get("usability_ignored") else (w[c] - b[c] >= 16 * min_range) for c in range(3)]
        if target is None:
            B = min([b[c] for c in range(3) if usable[c]], default=0)
            Wt = max([w[c] for c in range(3) if usable[c]], default=0)
        else:
            B, Wt = 16 * target[0], 16 * target[1]
        for c in range(3):
            q = [int(v) for v in Q[g, c, :NODES]]
            t = [max(0, min(4095, int(v))) for v in T[g, c, :NODES]]
            for v in range(256):
                x = 16 * v
                o = x
                if int(mode[g]) == LEVELS and usable[c]:
                    den = w[c] - b[c]
                    num = Wt - B if f.get("no_gain_limit") else min(Wt - B, (max_gain * den) >> 8)
                    o = _div((B + Wt) * den + (2 * x - b[c] - w[c]) * num + den, 2 * den, **f)
                elif int(mode[g]) == MATCH:
                    if x <= q[0]:
                        o = x + t[0] - q[0]
                        if f.get("ends_by_slope"):
                            o = t[0] + _div((x - q[0]) * (t[1] - t[0]), max(q[1] - q[0], 1))
                    elif x >= q[NODES - 1]:
                        o = x + t[NODES - 1] - q[NODES - 1]
                        if f.get("ends_by_slope"):
                            o = t[NODES - 1] + _div((x - q[NODES - 1]) * (t[NODES - 1] - t[NODES - 2]), max(q[NODES - 1] - q[NODES - 2], 1))
                    else:
                        k = max(i for i in range(NODES - 1) if q[i] <= x)
                        if f.get("first_tied"):
                            k = min(i for i in range(NODES - 1) if q[i] == q[k])
                        den = max(q[k + 1] - q[k], 1)
                        o = t[k] + _div(2 * (x - q[k]) * (t[k + 1] - t[k]) + den, 2 * den, **f)
                o2 = x + (((o - x) * strength + (0 if f.get("strength_trunc") else 128)) >> 8)
                lut[g, c, v] = max(0, min(255, (o2 + 8) >> 4))
    return lut


def apply_np(frames, lut, group, **f):
    """uint8 [L,H,W,3]: byte c of frame t through lut[group[t]][c]; a frame whose group is outside [0, G) is copied"""
    a = np.asarray(frames)
    lut, group = np.asarray(lut), np.asarray(group).astype(np.int64)
    G = len(lut)
    full = np.concatenate([lut, np.tile(np.arange(256, dtype=np.uint8), (1, 3, 1))])          # table G: the identity
    gi = np.where((group >= 0) & (group < G), group, G)
    ch = (np.arange(3) + (1 if f.get("next_channel") else 0)) % 3
    return full[gi[:, None, None, None], ch[None, None, None, :], a]


def plan_np(L, scenes=None, n_graded=None, keys=None, otherwise="levels", **f):
    """what restore_color pools and does per scene -> (groups of frames, groups of graded frames or None, mode, group of every
    frame): a scene without ``graded`` pools its own frames (mode LEVELS); with ``graded`` alone its own frames against all graded
    ones (MATCH); with keys its key frames against their graded versions (MATCH), and a scene without a key follows ``otherwise``"""
    bounds = [0] + [int(c) for c in scenes or []] + [L]
    S = len(bounds) - 1
    own = [list(range(L)) if f.get("across_cut") else list(range(bounds[s], bounds[s + 1])) for s in range(S)]
    group = np.zeros(L, np.int32)
    for s in range(S):
        group[bounds[s]:bounds[s + 1]] = s
    if n_graded is None:
        return own, None, np.full(S, LEVELS, np.int32), group
    if keys is None:
        return own, [list(range(n_graded)) for _ in range(S)], np.full(S, MATCH, np.int32), group
    held = [[i for i, k in enumerate(keys) if group[k] == s] for s in range(S)]
    mode = np.array([MATCH if h else (LEVELS if otherwise == "levels" else KEEP) for h in held], np.int32)
    return [[keys[i] for i in h] if h else o for h, o in zip(held, own)], held, mode, group


def restore_np(frames, scenes=None, graded=None, keys=None, otherwise="levels", clip=(5, 5), target=None, min_range=32,
               max_gain=768, strength=256, **f):
    """every stage of the definition (or of a variant, by its flags) as a dict of KEYS (T: None without ``graded``) and the tables
    the entries take"""
    frames = np.asarray(frames)
    L = frames.shape[0]
    groups, ggroups, mode, group = plan_np(L, scenes, None if graded is None else len(graded), keys, otherwise, **f)
    w = dict(hist=hist_np(frames), mode=mode, group=group, T=None)
    w["starts"], w["ids"] = csr(groups)
    w["Q"] = nodes_np(w["hist"], w["starts"], w["ids"], clip, **f)
    if graded is not None:
        w["ghist"] = hist_np(graded)
        w["gstarts"], w["gids"] = csr(ggroups)
        w["T"] = nodes_np(w["ghist"], w["gstarts"], w["gids"], clip, **f)
    w["lut"] = lut_np(w["Q"], mode, w["T"], target, min_range, max_gain, strength, **f)
    if strength == 0 or frames.size == 0:
        w["lut"] = np.tile(np.arange(256, dtype=np.uint8), (len(mode), 3, 1))
    w["out"] = apply_np(frames, w["lut"], group, **f)
    return w


# ------------------------------------------------------------------------------------------------ the cases
def _image(H, W, seed, lo=(20, 40, 10), span=(150, 120, 200)):
    """a colour image whose channels have different ranges: two ramps and noise, int64 [H,W,3]"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = (3 * yy * 256) // max(H - 1, 1) // 4 + (xx * 256) // max(W - 1, 1) // 4          # 0 .. 255
    img = np.stack([lo[c] + (ramp * span[c]) // 256 for c in range(3)], axis=-1)
    return np.clip(img + rng.randint(-6, 7, (H, W, 3)), 0, 255).astype(np.int64)


def _moving(L, H, W, seed, **kw):
    base = _image(H, W, seed, **kw)
    return np.stack([np.roll(base, 2 * t, axis=1) for t in range(L)])


def _case(frames, **kw):
    frames = np.ascontiguousarray(np.asarray(frames).astype(np.uint8))
    frames.setflags(write=False)
    c = dict(DEFAULTS, kind="video", frames=frames, scenes=None, graded=None, keys=None, otherwise="levels")
    if kw.get("graded") is not None:
        kw["graded"] = np.ascontiguousarray(np.asarray(kw["graded"]).astype(np.uint8))
        kw["graded"].setflags(write=False)
    c.update(kw)
    return c


def _flat():
    """260 x 260 = 67 600 pixels in one bin per channel: more than 16 bits, every group of four merged, no usable channel"""
    return _case(np.stack([np.full((260, 260, 3), 1) * (90, 40, 200), np.full((260, 260, 3), 1) * (90, 40, 200)]))


def _two_level():
    """two levels per channel in three proportions, matched onto two other levels: most nodes share a bin, in Q and in T"""
    fr = np.full((3, 13, 17, 3), 1) * (48, 64, 80)
    for t, rows in enumerate((3, 6, 10)):
        fr[t, :rows] = (192, 160, 208)
    gr = np.full((2, 8, 16, 3), 1) * (32, 32, 16)
    gr[0, :4], gr[1, :2] = (224, 240, 208), (224, 240, 208)
    return _case(fr, graded=gr, scenes=[2])


def _one_flat_channel():
    fr = _moving(3, 18, 22, 41)
    fr[..., 1] = 100 + (fr[..., 1] % 3)
    return _case(fr)


def _saturated():
    rng = np.random.RandomState(42)
    fr = _moving(3, 19, 22, 43, lo=(60, 70, 50), span=(120, 110, 140))
    for c in range(3):
        m = rng.rand(3, 19, 22)
        fr[..., c] = np.where(m < 0.12, 0, np.where(m > 0.88, 255, fr[..., c]))
    return _case(fr, target=(0, 255), clip=(150, 150))


def _narrow():
    """one channel 20 levels wide beside two wide ones: its gain would be about ten, max_gain = 3 binds"""
    fr = _moving(3, 18, 22, 44)
    fr[..., 2] = 120 + (fr[..., 2] * 24) // 256                   # 4 .. 216 -> 120 .. 140
    return _case(fr, min_range=16)


def _keys9(otherwise):
    """9 frames of 20 x 23 in three scenes, graded 11 x 13: two keys pooled in the first scene, no key in the second, one in the
    third"""
    fr = _moving(9, 20, 23, 45)
    fr[4:7] = _moving(3, 20, 23, 46, lo=(50, 20, 60), span=(90, 160, 100))
    fr[7:] = _moving(2, 20, 23, 47, lo=(70, 70, 30), span=(100, 100, 150))
    gr = np.stack([_image(11, 13, 48, lo=(5, 5, 5), span=(240, 240, 240)), _image(11, 13, 49, lo=(10, 0, 8), span=(230, 250, 235)),
                   _image(11, 13, 50, lo=(0, 12, 0), span=(250, 225, 245))])
    return _case(fr, scenes=[4, 7], keys=[1, 2, 8], graded=gr, otherwise=otherwise)


def _graded_n2():
    gr = np.stack([_image(9, 14, 52, lo=(5, 5, 5), span=(240, 240, 240)), _image(9, 14, 53, lo=(0, 10, 0), span=(250, 230, 240))])
    return _case(_moving(4, 17, 19, 51), graded=gr, scenes=[3])


def _big_N():
    """nodes alone: 40 rows of 2^26 pixels in three bins with odd counts, pooled -- N = 40 2^26 is past 2^31"""
    N = 1 << 26
    hist = np.zeros((40, 3, 256), np.int32)
    for t in range(40):
        for c in range(3):
            a, b = 12345677 + 2 * t + 4 * c, 23456789 - 2 * c
            hist[t, c, 3 + c], hist[t, c, 130], hist[t, c, 250] = a, N - a - b, b
    hist.setflags(write=False)
    starts, ids = csr([list(range(40)), list(range(0, 40, 2)), [39]])
    return dict(DEFAULTS, kind="nodes", hist=hist, starts=starts, ids=ids)


def _bad_ids():
    """nodes alone: ids of -1 and L are skipped, a reversed pair of starts and starts past M are empty"""
    hist = hist_np(_moving(4, 9, 11, 54).astype(np.uint8))
    hist.setflags(write=False)
    ids = np.array([0, -1, 1, 4, 2, 3, 3, 1 << 30, -(1 << 31)], np.int32)
    starts = np.array([0, 4, 2, 7, 9, 12, -3, 5], np.int32)           # 4 > 2: reversed; 12: clamped to M = 9; -3: clamped to 0
    return dict(DEFAULTS, kind="nodes", hist=hist, starts=starts, ids=ids)


def _group_out():
    """apply alone: frames whose group is -1 or G are copied"""
    fr = _moving(5, 7, 9, 55).astype(np.uint8)
    fr.setflags(write=False)
    rng = np.random.RandomState(56)
    lut = np.sort(rng.randint(0, 256, (2, 3, 256)), axis=-1).astype(np.uint8)
    return dict(DEFAULTS, kind="apply", frames=fr, lut=lut, group=np.array([1, -1, 0, 2, 1 << 30], np.int32))


def _lut_ties():
    """tables alone: hand-made nodes with ties that sit on whole levels, in Q and in T, in every mode"""
    q = np.array(sorted([160] * 6 + [800] * 5 + [1600] * 4 + list(range(1700, 1700 + 17 * 60, 60))), np.int64)
    t = np.array(sorted([64] * 3 + [480] * 8 + [2400] * 6 + list(range(2500, 2500 + 15 * 90, 90))), np.int64)
    Q = np.zeros((4, 3, NQ), np.int32)
    T = np.zeros((4, 3, NQ), np.int32)
    for g in range(4):
        for c in range(3):
            Q[g, c, :NODES], T[g, c, :NODES] = q + 16 * c, np.minimum(t + 48 * g + 5 * c, 5000)
            Q[g, c, NODES:], T[g, c, NODES:] = (100 + 200 * c, 2500 + 300 * c), (0, 4095)
    T[0, 2, 0], T[0, 2, NODES - 1] = -40, 5000                        # clamped to 0 and 4095
    return dict(DEFAULTS, kind="lut", Q=Q, T=T, mode=np.array([MATCH, LEVELS, KEEP, 7], np.int32), strength=200)


def _slabs():
    """65 540 frames of 2 x 3 with a cut at 65 537 and a key on either side: two launches of frames in the histogram and the apply
    pass"""
    rng = np.random.RandomState(57)
    fr = rng.randint(30, 200, (65540, 2, 3, 3))
    fr[65537:] += 40
    gr = rng.randint(0, 256, (2, 2, 3, 3))
    return _case(fr, scenes=[65537], keys=[5, 65538], graded=gr)


_BUILDERS = {
    "5x7": lambda: _case(_moving(3, 5, 7, 30)),                                          # W mod 4 = 3, 35 pixels: fewer than a workgroup
    "3x70x300": lambda: _case(_moving(3, 70, 300, 31), scenes=[2]),                      # 21 000 pixels: several workgroups a frame
    "w1_33x41": lambda: _case(_moving(4, 33, 41, 32)),                                   # W mod 4 = 1; frames 1 .. 3 start off a dword
    "w2_30x42": lambda: _case(_moving(4, 30, 42, 33), scenes=[1]),                       # W mod 4 = 2, N mod 4 = 0
    "flat_260": _flat,
    "black_white": lambda: _case(np.stack([np.zeros((6, 9, 3)), np.full((6, 9, 3), 255)])),
    "two_level": _two_level,
    "one_flat_channel": _one_flat_channel,
    "saturated": _saturated,
    "narrow_gain": _narrow,
    "clip_0": lambda: _case(_moving(3, 12, 15, 34), clip=(0, 0)),
    "clip_250": lambda: _case(_moving(3, 12, 15, 35), clip=(250, 250)),
    "strength_128": lambda: _case(_moving(3, 12, 15, 36, lo=(60, 90, 70), span=(90, 60, 110)), strength=128, target=(0, 255)),
    "target_16_235": lambda: _case(_moving(3, 12, 15, 37), target=(16, 235)),
    "keys_9": lambda: _keys9("levels"),
    "keys_9_keep": lambda: _keys9("keep"),
    "graded_n2": _graded_n2,
    "big_N": _big_N,
    "bad_ids": _bad_ids,
    "group_out": _group_out,
    "lut_ties": _lut_ties,
    "slabs_65540": _slabs,
}
NAMES = tuple(_BUILDERS)
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def settings(c):
    """the keyword arguments of video.restore_color (and of restore_np) of a video case"""
    return {k: c[k] for k in ("scenes", "graded", "keys", "otherwise") + tuple(DEFAULTS)}


def lut_settings(c):
    return {k: c[k] for k in ("target", "min_range", "max_gain", "strength")}


def keys(name):
    """the KEYS a case has"""
    c = case(name)
    if c["kind"] == "video":
        return tuple(k for k in KEYS if k != "T" or c["graded"] is not None)
    return dict(nodes=("Q",), lut=("lut",), apply=("out",))[c["kind"]]


def want(name, **f):
    """the dict of a case under the definition (or a variant's flags): keys(name) and, for a video, the tables the entries take;
    computed once, read-only"""
    key = (name,) + tuple(sorted(f))
    if key not in _WANT:
        c = case(name)
        if c["kind"] == "video":
            w = restore_np(c["frames"], **dict(settings(c), **f))
        elif c["kind"] == "nodes":
            w = dict(Q=nodes_np(c["hist"], c["starts"], c["ids"], c["clip"], **f))
        elif c["kind"] == "lut":
            w = dict(lut=lut_np(c["Q"], c["mode"], c["T"], **dict(lut_settings(c), **f)))
        else:
            w = dict(out=apply_np(c["frames"], c["lut"], c["group"], **f))
        for a in w.values():
            if a is not None:
                a.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ planted fades
FADES = {"affine": dict(lift=(60, 20, 35), gain=(0.70, 0.60, 0.55), gamma=(1.0, 1.0, 1.0)),
         "gamma": dict(lift=(60, 20, 35), gain=(0.70, 0.60, 0.55), gamma=(1.0, 1.3, 0.8))}


def tennis25(root):
    with np.load(os.path.join(root, "tests", "golden", "tennis25.npz")) as z:
        return np.asarray(z["frames"], np.uint8)


def plant_fade(frames, lift, gain, gamma):
    """a faded print: per channel clip(rint(255 (v / 255)^gamma gain + lift))"""
    v = np.asarray(frames).astype(np.float64) / 255.0
    out = 255.0 * v ** np.asarray(gamma, np.float64) * np.asarray(gain, np.float64) + np.asarray(lift, np.float64)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def psnr(a, b):
    """dB over all bytes; per frame with ``axis``"""
    e = (np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)) ** 2
    return float(10 * np.log10(255.0 ** 2 / e.mean()))


def psnr_frames(a, b):
    return [psnr(x, y) for x, y in zip(a, b)]
