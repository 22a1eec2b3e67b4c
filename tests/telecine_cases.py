"""The inverse telecine restated in numpy and plain Python (video.telecine_scores, video.matches_from_scores,
video.plan_inverse_telecine, video.inverse_telecine, ops.telecine_scores, ops.field_weave; the definition is in
include/e2fgvi_hip.h and in the docstrings of video.py), the named cases the device code is compared with word for word and byte
for byte, mutated restatements (CAUGHT_BY) that must each differ from the definition on a case named for them -- which is what
shows that the cases can see such a mistake -- and the planted clips the rules are judged on.  Integers throughout: there is no
tolerance anywhere.  Written unlike the kernels and unlike video.py on purpose: the scores from whole luma planes with the cell of
every pixel as an index plane, the rules frame by frame in Python integers."""
import numpy as np

from tests import interlace_cases as I

luma, scene_of_np, noise, tennis25 = I.luma, I.scene_of_np, I.noise, I.tennis25
PATTERN = (0, 0, 1, 1, 0)
# (flag, the case that must see it): the scores on a named case, the rules on a named table
CAUGHT_BY = (
    ("missing_zero", "single_6x7"),            # a missing neighbour frame reads as zeros
    ("across_cut", "cut2_6x7"),                # a neighbour is taken across a cut
    ("score_rows_odd", "tiny_5x4"),            # the rows [1, H - 2] on odd H
    ("cell_row_above", "noise_37x53"),         # the cell taken from row y - 1
    ("no_margin", "table_margin"),             # a gain without the margin test: every cell where x < c counts
    ("tie_break", "table_tie"),                # ties to the larger phi
    ("drop_orphans", "table_orphan"),          # the drop rule without the orphan exception
    ("drop_across_cut", "table_cut"),          # a drop across a cut
)
SCORE_FLAGS = ("missing_zero", "across_cut", "score_rows_odd", "cell_row_above")


# ------------------------------------------------------------------------------------------------ the two entries
def scores_np(frames, scenes=None, **f):
    """M int64 [L,2,3,16]"""
    Y = luma(frames)
    L, H, W = Y.shape
    so = scene_of_np(L, scenes)
    M = np.zeros((L, 2, 3, 16), np.int64)
    if H * W == 0:
        return M
    m = (H - 2) // 2
    ys = np.arange(1, (H - 2 if f.get("score_rows_odd") else 2 * m) + 1)
    if H < 4 and not f.get("score_rows_odd"):
        ys = ys[:0]
    yy, xx = np.mgrid[0:H, 0:W]
    cell = (4 * (yy - 1 if f.get("cell_row_above") else yy) // H) * 4 + (4 * xx) // W
    for t in range(L):
        for j, step in enumerate((-1, 0, 1)):
            s = t + step
            if 0 <= s < L and (so[s] == so[t] or f.get("across_cut")):
                S = Y[s]
            else:
                S = np.zeros_like(Y[t]) if f.get("missing_zero") else Y[t]
            for q in (0, 1):
                r = ys[(ys & 1) == q]
                np.add.at(M[t, q, j], cell[r].ravel(), np.abs(2 * S[r] - Y[t][r - 1] - Y[t][r + 1]).ravel())
    return M


def weave_np(frames, jobs, keep):
    """uint8 [n,H,W,3]: the rows of parity keep of out[i] from frames[a_i], the others from frames[b_i]"""
    fr = np.asarray(frames)
    jobs = np.asarray(jobs, np.int64).reshape(-1, 2)
    kept = ((np.arange(fr.shape[1]) & 1) == keep)[None, :, None, None]
    return np.where(kept, fr[jobs[:, 0]], fr[jobs[:, 1]]).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the rules
def spans(length, scenes=None):
    edges = [0] + [int(c) for c in scenes or []] + [length]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def raw_matches_np(M, keep="top", margin=10, **f):
    """the match of every frame on its own, a list of -1, 0, +1"""
    q = 1 if keep == "top" else 0
    out = []
    for t in range(len(M)):
        gains = []
        for j in (0, 2):
            g = 0
            for cell in range(16):
                c, x = int(M[t][q][1][cell]), int(M[t][q][j][cell])
                if (x < c) if f.get("no_margin") else (100 * x < (100 - margin) * c):
                    g += c - x
            gains.append(g)
        out.append(-1 if gains[0] > gains[1] else 1 if gains[1] > gains[0] else 0)
    return out


def matches_np(M, keep="top", scenes=None, margin=10, cadence="3:2", **f):
    """(k int8 [L], orphan bool [L], locks)"""
    k = raw_matches_np(M, keep, margin, **f)
    orphan, locks = [False] * len(k), []
    for s, e in spans(len(k), scenes):
        ranked = []
        for d in (-1, 1):
            for phi in range(5):
                pattern = [d * PATTERN[(t - s + phi) % 5] for t in range(s, e)]
                agree = sum(1 for t in range(s, e) if k[t] != 0 and k[t] == pattern[t - s])
                disagree = sum(1 for t in range(s, e) if k[t] != 0 and k[t] != pattern[t - s])
                # the best sorts first: the largest agree - disagree, then the largest agree, then d = -1, then the smaller phi
                ranked.append((-(agree - disagree), -agree, d, -phi if f.get("tie_break") else phi, phi, agree, disagree, pattern))
        ranked.sort(key=lambda r: r[:4])
        _, _, d, _, phi, agree, disagree, pattern = ranked[0]
        if cadence == "3:2" and agree >= 4 and 10 * disagree <= agree:
            locks.append((d, phi, agree, disagree))
            k[s:e] = pattern
            if k[s] == -1:
                orphan[s] = True
            if k[e - 1] == 1:
                orphan[e - 1] = True
        else:
            locks.append(None)
        if k[s] == -1:
            k[s] = 0
        if k[e - 1] == 1:
            k[e - 1] = 0
    return np.array(k, np.int8).reshape(-1), np.array(orphan, bool).reshape(-1), locks


def plan_np(k, orphan, scenes=None, **f):
    """(jobs [(t, t + k[t])], cuts_out)"""
    so = scene_of_np(len(k), scenes)
    jobs, kept_before = [], []
    for t in range(len(k)):
        kept_before.append(len(jobs))
        same = t > 0 and (so[t - 1] == so[t] or f.get("drop_across_cut"))
        clean = f.get("drop_orphans") or not (orphan[t - 1] or orphan[t])
        if same and int(k[t - 1]) - int(k[t]) == 1 and clean:
            continue
        jobs.append((t, t + int(k[t])))
    return jobs, [kept_before[int(c)] for c in scenes or []]


def verdict_np(k, locks, scenes=None):
    failed = any(lock is None and sum(1 for t in range(s, e) if k[t] != 0) >= 4 for lock, (s, e) in zip(locks, spans(len(k), scenes)))
    if any(lock is not None for lock in locks) and not failed:
        return "3:2"
    return "mixed" if any(int(v) != 0 for v in k) else "none"


def inverse_telecine_np(frames, scenes=None, keep="top", margin=10, cadence="3:2", M=None):
    """(the frames, the plan) of video.inverse_telecine with orphans="keep"; M: the scores when they are at hand"""
    M = scores_np(frames, scenes) if M is None else M
    k, orphan, locks = matches_np(M, keep, scenes, margin, cadence)
    jobs, cuts = plan_np(k, orphan, scenes)
    return weave_np(frames, jobs, 0 if keep == "top" else 1), dict(matches=k, orphan=orphan, source=np.array(jobs, np.int32).reshape(-1, 2),
                                                                    cuts=cuts, locks=locks)


# ------------------------------------------------------------------------------------------------ the named cases
TINY = tuple((H, W) for H in range(1, 7) for W in range(1, 8))
_BUILDERS = {"tiny_%dx%d" % hw: (lambda hw=hw: I._case(noise(3, hw[0], hw[1], 300 + 10 * hw[0] + hw[1]))) for hw in TINY}
_BUILDERS.update({
    # neither side a multiple of 4 or 16: cells of 13 and 14 columns, every group short
    "noise_37x53": lambda: I._case(noise(3, 37, 53, 21)),
    # a tall narrow frame: runs of 19 rows, four chunks of rows a cell row; and rows of more than 1024 pixels: 72 groups a row
    "tall_300x20": lambda: I._case(noise(2, 300, 20, 24)),
    "wide_9x1100": lambda: I._case(noise(2, 9, 1100, 23)),
    # whole groups and short ones side by side, more than one run a cell row
    "noise_70x150": lambda: I._case(noise(3, 70, 150, 22)),
    "single_6x7": lambda: I._case(noise(1, 6, 7, 25)),
    "pair_6x7": lambda: I._case(noise(2, 6, 7, 26)),
    "single_40x52": lambda: I._case(noise(1, 40, 52, 27)),
    # a cut at every place of four frames, and at all of them
    "cut1_6x7": lambda: I._case(noise(4, 6, 7, 28), [1]),
    "cut2_6x7": lambda: I._case(noise(4, 6, 7, 28), [2]),
    "cut3_6x7": lambda: I._case(noise(4, 6, 7, 28), [3]),
    "cuts_6x7": lambda: I._case(noise(4, 6, 7, 28), [1, 2, 3]),
    "cut2_40x52": lambda: I._case(noise(4, 40, 52, 29), [2]),
    # 0 and 255 alone: the largest terms
    "extremes_12x13": lambda: I._case(255 * np.random.RandomState(30).randint(0, 2, (3, 12, 13, 3))),
    "extremes_40x52": lambda: I._case(255 * np.random.RandomState(31).randint(0, 2, (3, 40, 52, 3))),
    "flat_8x9": lambda: I._case(np.full((3, 8, 9, 3), 90)),
    "steps_8x9": lambda: I._case(np.arange(3)[:, None, None, None] * 40 + np.arange(8)[None, :, None, None] * 9 + np.zeros((3, 8, 9, 3))),
})
NAMES = tuple(_BUILDERS)
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def want_scores(name, **f):
    """the scores of a case under the definition (or a variant's flags); computed once, read-only"""
    key = (name, "scores") + tuple(sorted(f))
    if key not in _WANT:
        c = case(name)
        _WANT[key] = scores_np(c["frames"], c["scenes"], **f)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def case_jobs(name):
    """the jobs a case is woven with: every frame with itself, with each neighbour, and the last with the first"""
    L = case(name)["L"]
    return [(t, u) for t in range(L) for u in (t - 1, t, t + 1) if 0 <= u < L] + [(L - 1, 0)]


def want_weave(name, keep):
    key = (name, "weave", keep)
    if key not in _WANT:
        _WANT[key] = weave_np(case(name)["frames"], case_jobs(name), keep)
        _WANT[key].setflags(write=False)
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ the named tables of the rules
def _table(rows):
    """M int64 [L,2,3,16] from rows of (x of k = -1, c, x of k = +1) in cell 0 of q = 1 (keep="top"); every other cell holds 100 thrice"""
    M = np.full((len(rows), 2, 3, 16), 100, np.int64)
    for t, row in enumerate(rows):
        M[t, 1, :, 0] = row
    return M


def _table_of(k):
    return _table([(50, 100, 100) if v == -1 else (100, 100, 50) if v == 1 else (100, 100, 100) for v in k])


TABLES = {
    # x = 95 against c = 100: inside the margin of 10, so no match -- a gain without the margin test takes it
    "table_margin": dict(M=_table([(100, 100, 100), (95, 100, 100), (100, 100, 95), (94, 100, 95), (100, 100, 100)]), scenes=None),
    # four decided frames at t = 3 mod 5: phi = 0 and phi = 4 agree with all of them, the smaller phi wins
    "table_tie": dict(M=_table_of([-1 if t % 5 == 3 else 0 for t in range(20)]), scenes=None),
    # a scene that starts two frames into the cadence: its first frame is an orphan and must not swallow its successor
    "table_orphan": dict(M=_table_of([-1, -1, 0, 0, 0, -1, -1, 0, 0, 0, -1, -1]), scenes=None),
    # plan only: a k that points across the cut in front of frame 2
    "table_cut": dict(k=[0, 0, -1, 0], orphan=[False] * 4, scenes=[2]),
}


def table_result(name, **f):
    """what a table gives under the definition or a variant: (k, orphan, jobs, cuts_out) as lists"""
    t = TABLES[name]
    if "M" in t:
        k, orphan, _ = matches_np(t["M"], "top", t["scenes"], 10, "3:2", **f)
    else:
        k, orphan = np.array(t["k"], np.int8), np.array(t["orphan"], bool)
    jobs, cuts = plan_np(k, orphan, t["scenes"], **f)
    return k.tolist(), orphan.tolist(), jobs, cuts


# ------------------------------------------------------------------------------------------------ planted clips
def telecine_origin(n, tff=True, phase=0):
    """3:2 pulldown of n film frames: film frame i lasts two fields when (i + phase) is even and three when it is odd, the fields
    alternate in parity from the first one's (top when tff), and every two fields are a video frame -> origin int [m,2]: the film
    frame behind the top and the bottom field of every video frame"""
    fields = [i for i in range(n) for _ in range(2 if (i + phase) % 2 == 0 else 3)]
    fields = fields[:len(fields) // 2 * 2]
    first = 0 if tff else 1
    origin = np.zeros((len(fields) // 2, 2), np.int64)
    origin[:, first], origin[:, 1 - first] = fields[0::2], fields[1::2]
    return origin


def telecine(film, tff=True, phase=0):
    """(video uint8 [m,H,W,3], origin) of film frames [n,H,W,3] under telecine_origin's pulldown"""
    origin = telecine_origin(len(film), tff, phase)
    video = np.array(film[origin[:, 0]])
    video[:, 1::2] = film[origin[:, 1]][:, 1::2]
    return video, origin


def noisy(video, sigma=5, seed=0):
    """Gaussian noise of `sigma` grey levels on every byte, rounded and clipped"""
    g = np.random.RandomState(seed).normal(0.0, sigma, video.shape)
    return np.clip(np.rint(video.astype(np.float64) + g), 0, 255).astype(np.uint8)


def noise_seed(film, tff, phase):
    """the seed of the noise of a planted arm (the kept field does not change the video, so it does not change the noise)"""
    return 1000 + 100 * int(tff) + 10 * phase + {"pan": 25, "locked": 16}[film]


def pan_film(f):
    return f[:25]


def locked_off_film(f):
    return I.locked_off_clip(f)[1]


def film_of(plan, origin, keep="top"):
    """the film frame behind the kept field and behind the other field of every output frame: int [n,2]"""
    p = 0 if keep == "top" else 1
    src = np.asarray(plan["source"]).reshape(-1, 2)
    return np.stack([origin[src[:, 0], p], origin[src[:, 1], 1 - p]], axis=1)


ARMS = tuple((tff, phase, keep) for tff in (True, False) for phase in (0, 1) for keep in ("top", "bottom"))
