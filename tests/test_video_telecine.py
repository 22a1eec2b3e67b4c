"""The host side of the inverse telecine (video.matches_from_scores, video.plan_inverse_telecine, video.telecine_scores,
video.detect_telecine, video.inverse_telecine) without a device: the host rules against the restatement of tests/telecine_cases.py
and on the planted clips with the restatement's scores, every mutated restatement moving the case named for it, every refusal
before the device, the signatures, the header and the binding, and the C entries' refusals."""
import inspect
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import interlace_cases as I
from tests import telecine_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"e2fgvi_telecine_scores": ["frames", "scene", "M", "L", "H", "W", "stream"],
           "e2fgvi_field_weave": ["frames", "jobs", "out", "L", "n", "H", "W", "keep", "stream"]}
TOOLS = (video.telecine_scores, video.detect_telecine, video.inverse_telecine)        # what the restatement restates


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_telecine_scores_device", touched)
    monkeypatch.setattr(video, "_inverse_telecine_device", touched)


@pytest.fixture(scope="module")
def tennis():
    return C.tennis25(ROOT)


@pytest.fixture(scope="module")
def planted(tennis):
    """{(film, tff, phase): (film frames, video, origin, M of the clean video, M of the video with noise of sigma 5)}: the scores
    of the restatement, computed once"""
    out = {}
    for name, film in (("pan", C.pan_film(tennis)), ("locked", C.locked_off_film(tennis))):
        for tff in (True, False):
            for phase in (0, 1):
                video_, origin = C.telecine(film, tff, phase)
                out[name, tff, phase] = (film, video_, origin, C.scores_np(video_),
                                         C.scores_np(C.noisy(video_, 5, C.noise_seed(name, tff, phase))))
    return out


def _same_rules(M, keep, scenes, margin, cadence):
    """video's rules on M against the restatement's; returns the restatement's (k, orphan, locks, jobs, cuts)"""
    k, orphan, locks = video.matches_from_scores(M, keep, scenes, margin, cadence)
    wk, wo, wl = C.matches_np(M, keep, scenes, margin, cadence)
    assert k.dtype == np.int8 and orphan.dtype == np.bool_ and k.shape == orphan.shape == (len(M),)
    assert (k.tolist(), orphan.tolist(), locks) == (wk.tolist(), wo.tolist(), wl), (keep, scenes, margin, cadence)
    jobs, cuts = video.plan_inverse_telecine(k, orphan, scenes)
    assert (jobs, cuts) == C.plan_np(wk, wo, scenes), (keep, scenes, margin, cadence)
    return wk, wo, wl, jobs, cuts


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name,case", C.CAUGHT_BY, ids=[v[0] for v in C.CAUGHT_BY])
def test_every_variant_differs_from_the_definition_on_its_case(name, case):
    if name in C.SCORE_FLAGS:
        a, b = C.want_scores(case), C.want_scores(case, **{name: True})
        print(name, case, int((a != b).sum()))
        assert a.shape == b.shape and not np.array_equal(a, b)
    else:
        a, b = C.table_result(case), C.table_result(case, **{name: True})
        print(name, case, a, b)
        assert a != b


def test_cases_hold_what_they_are_named_for():
    shapes = {(C.case(n)["H"], C.case(n)["W"]) for n in C.NAMES}
    assert {(H, W) for H in range(1, 7) for W in range(1, 8)} <= shapes and {(37, 53), (9, 1100), (300, 20)} <= shapes
    assert {C.case(n)["L"] for n in C.NAMES} >= {1, 2, 3, 4}
    assert [C.case(n)["scenes"] for n in ("cut1_6x7", "cut2_6x7", "cut3_6x7", "cuts_6x7")] == [[1], [2], [3], [1, 2, 3]]
    assert all(C.case(n)["H"] * C.case(n)["W"] <= 10500 for n in C.NAMES)
    for n in ("extremes_12x13", "extremes_40x52"):
        assert set(np.unique(C.case(n)["frames"]).tolist()) == {0, 255}
    for n in C.NAMES:
        c, M = C.case(n), C.want_scores(n)
        so = C.scene_of_np(c["L"], c["scenes"])
        assert M.shape == (c["L"], 2, 3, 16) and M.dtype == np.int64 and (M >= 0).all()
        if c["H"] < 4:
            assert not M.any()
        # the identity with the interlace scores: the cells of candidate t + 1 sum to D[t][q] wherever t has a successor in its scene
        D = I.scores_np(c["frames"], c["scenes"])
        for t in range(c["L"]):
            if t + 1 < c["L"] and so[t + 1] == so[t]:
                assert np.array_equal(M[t, :, 2].sum(axis=1), D[t]), (n, t)
            else:
                assert np.array_equal(M[t, :, 2], M[t, :, 1]), (n, t)         # a candidate replaced by t
            if not (t > 0 and so[t - 1] == so[t]):
                assert np.array_equal(M[t, :, 0], M[t, :, 1]), (n, t)
    # a flat video combs nowhere; every cell of a frame of more than four rows and columns is reached
    assert not C.want_scores("flat_8x9").any()
    assert C.want_scores("noise_37x53").all() and C.want_scores("tall_300x20").all() and C.want_scores("wide_9x1100")[:, :, :, :].any()
    # H = 5: rows 1 and 2 alone (m = 1), row 3 is not scored; cells by (4 y) / 5 and (4 x) / 4
    Y = C.luma(C.case("tiny_5x4")["frames"])
    M = C.want_scores("tiny_5x4")
    assert M[0, 1, 2].tolist() == [int(abs(2 * Y[1][1][x] - Y[0][0][x] - Y[0][2][x])) for x in range(4)] + [0] * 12
    assert M[0, 0, 2].tolist() == [0] * 4 + [int(abs(2 * Y[1][2][x] - Y[0][1][x] - Y[0][3][x])) for x in range(4)] + [0] * 8
    # the weave: the rows of the kept parity are those of a, the others those of b
    for n in ("noise_37x53", "tiny_1x1", "tiny_2x3", "cut2_6x7", "single_6x7"):
        c, jobs = C.case(n), C.case_jobs(n)
        for keep in (0, 1):
            out = C.want_weave(n, keep)
            assert out.shape == (len(jobs),) + c["frames"].shape[1:] and out.dtype == np.uint8
            for i, (a, b) in enumerate(jobs):
                assert np.array_equal(out[i, keep::2], c["frames"][a, keep::2]) and np.array_equal(out[i, 1 - keep::2], c["frames"][b, 1 - keep::2])


def test_scene_by_scene_is_the_call_with_scenes():
    c = C.case("cut2_40x52")
    assert np.array_equal(np.concatenate([C.scores_np(c["frames"][:2]), C.scores_np(c["frames"][2:])]), C.want_scores("cut2_40x52"))
    assert not np.array_equal(C.scores_np(c["frames"]), C.want_scores("cut2_40x52"))


# ------------------------------------------------------------------------------------------------ the rules
def test_rules_are_the_restatement_on_tables():
    rng = np.random.RandomState(5)
    for name, t in C.TABLES.items():
        if "M" in t:
            for keep in ("top", "bottom"):
                for cadence in ("3:2", None):
                    _same_rules(t["M"], keep, t["scenes"], 10, cadence)
    # random tables: candidates near their frame's own field, so that the margin decides; with and without cuts
    for trial in range(40):
        L = int(rng.randint(1, 24))
        c = rng.randint(0, 1000, (L, 2, 1, 16))
        M = (c + rng.randint(-300, 100, (L, 2, 3, 16)) * (rng.rand(L, 2, 3, 1) < 0.5)).clip(0).astype(np.int64)
        M[:, :, 1] = c[:, :, 0]
        scenes = sorted(set(rng.randint(1, L, rng.randint(0, 3)).tolist())) if L > 1 else None
        for keep in ("top", "bottom"):
            _same_rules(M, keep, scenes or None, int(rng.randint(1, 51)), "3:2" if trial % 2 else None)
    # cadence tables in every phase and direction, from three frames on, with a cut: the lock, the orphans, the drops
    for d in (-1, 1):
        for phi in range(5):
            for L in (3, 7, 11, 20):
                ks = [d * C.PATTERN[(t + phi) % 5] for t in range(L)]
                _same_rules(C._table_of(ks), "top", None, 10, "3:2")
                _same_rules(C._table_of(ks + ks), "top", [L], 10, "3:2")


def test_rules_on_hand_made_tables():
    rule = video.matches_from_scores
    # 100 x < 90 c: 89 against 100 matches, 90 does not; both sides at once: the larger gain, a tie is no match
    k, orphan, locks = rule(C._table([(100, 100, 100), (89, 100, 100), (90, 100, 100), (100, 100, 89), (50, 100, 60), (60, 100, 50), (50, 100, 50)]))
    assert (k.tolist(), orphan.tolist(), locks) == ([0, -1, 0, 1, -1, 1, 0], [False] * 7, [None])
    assert rule(C._table([(100, 100, 100), (51, 100, 100), (49, 100, 100), (100, 100, 100)]), margin=50)[0].tolist() == [0, 0, -1, 0]
    # the bottom field kept reads q = 0: these tables have their evidence in q = 1
    assert not rule(C._table_of([0, -1, -1, 0, 0] * 3), keep="bottom")[0].any()
    # entries that point outside the video or the scene: 0 without a flag when there is no lock
    k, orphan, locks = rule(C._table_of([-1, 0, 1, -1, 0, 1]), scenes=[3])
    assert (k.tolist(), orphan.any(), locks) == ([0, 0, 0, 0, 0, 0], False, [None, None])
    # the lock: four agreeing frames lock, three do not; one dissenter in ten is allowed, one in nine is not
    cyc = [0, 0, -1, -1, 0]
    assert rule(C._table_of(cyc * 2))[2] == [(-1, 0, 4, 0)] and rule(C._table_of(cyc + [0, 0, -1]))[2] == [None]
    ten = cyc * 5
    odd = list(ten)
    odd[0] = 1
    assert rule(C._table_of(odd))[2] == [(-1, 0, 10, 1)] and rule(C._table_of(odd))[0].tolist() == ten
    assert rule(C._table_of(odd[:23]))[2] == [None] and rule(C._table_of(odd[:23]))[0].tolist() == odd[:23]
    # a locked scene takes the pattern where there was no evidence; d = +1 and the orphan at the scene's last frame
    blank = [0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1]
    k, orphan, locks = rule(C._table_of(blank))
    assert k.tolist() == [0, 0, 1, 1, 0] * 3 + [0, 0, 0] and orphan.tolist() == [False] * 17 + [True] and locks == [(1, 0, 5, 0)]
    assert rule(C._table_of(blank), cadence=None)[0].tolist() == blank[:17] + [0] and rule(C._table_of(blank), cadence=None)[2] == [None]
    # exact at the size of the scores: 2^36 a word
    u = (1 << 36) // 100
    assert rule(C._table([(90 * u - 1, 100 * u, 100 * u), (90 * u, 100 * u, 100 * u)]))[0].tolist() == [0, 0]       # frame 0 points outside
    assert rule(C._table([(100 * u, 100 * u, 100 * u), (90 * u - 1, 100 * u, 100 * u), (90 * u, 100 * u, 100 * u)]))[0].tolist() == [0, -1, 0]
    for bad in (np.zeros((3, 2, 3, 16), np.int32), np.zeros((3, 2, 3, 16), np.float64), np.zeros((3, 2, 3, 15), np.int64), np.zeros((3, 96), np.int64), None):
        with pytest.raises(ValueError, match="M must"):
            rule(bad)
    M = C._table_of(cyc * 2)
    for name, values in dict(margin=(0, 51, 5.5, True, None, "5"), keep=("first", "", None, 0, True), cadence=("2:2", "", 5, True),
                             scenes=([0], [10], "auto", [2, 1])).items():
        for v in values:
            with pytest.raises(ValueError, match=name):
                rule(M, **{name: v})
    # the plan: one frame in five of a cadence, none of progressive video or of 2:2 with a field shift; the cuts of the result
    plan = video.plan_inverse_telecine
    assert plan(np.array(cyc * 2, np.int8), np.zeros(10, bool)) == ([(0, 0), (1, 1), (3, 2), (4, 4), (5, 5), (6, 6), (8, 7), (9, 9)], [])
    assert plan(np.zeros(6, np.int8), np.zeros(6, bool), [2, 4]) == ([(t, t) for t in range(6)], [2, 4])
    assert plan(np.array([0, -1, -1, -1, -1], np.int8), np.zeros(5, bool))[0] == [(0, 0), (2, 1), (3, 2), (4, 3)]
    assert plan(np.array([0, 0, 1, 1, 0] * 2, np.int8), np.zeros(10, bool), [5]) == ([(0, 0), (1, 1), (2, 3), (3, 4), (5, 5), (6, 6), (7, 8), (8, 9)], [4])
    assert plan(np.zeros(0, np.int8), np.zeros(0, bool)) == ([], [])
    for k, orphan, what in ((np.zeros(3), np.zeros(3, bool), "k must"), (np.array([0, 2, 0]), np.zeros(3, bool), "k must"),
                            (np.zeros((3, 1), np.int8), np.zeros((3, 1), bool), "k must"), (np.zeros(3, np.int8), np.zeros(2, bool), "orphan"),
                            (np.zeros(3, np.int8), np.zeros(3, np.int8), "orphan")):
        with pytest.raises(ValueError, match=what):
            plan(k, orphan)
    with pytest.raises(ValueError, match="scenes"):
        plan(np.zeros(3, np.int8), np.zeros(3, bool), "auto")
    assert video.TELECINE_MARGIN == 10 and inspect.signature(rule).parameters["margin"].default == 10


# ------------------------------------------------------------------------------------------------ the planted clips
def test_planted_clips_come_back_byte_for_byte(planted):
    """The pan (25 film frames) and the locked-off clip (16 frames, a moving 64 x 64 patch) under 3:2 pulldown in both field orders
    and both starting phases, either field kept, the matches taken from the clean video and from the video with noise of sigma 5:
    at the default margin every film frame comes back once, in order, byte for byte, with the lock and without it.  The ratios
    x / c of the best cell: a right match shows 0.094 .. 0.293 on the pan and 0.438 .. 0.899 on the locked-off clip;
    on whole frames no cell falls below 0.954."""
    for (name, tff, phase), (film, clip, origin, clean, noisy) in planted.items():
        for keep in ("top", "bottom"):
            for M in (clean, noisy):
                for cadence in ("3:2", None):
                    k, orphan, locks, jobs, cuts = _same_rules(M, keep, None, 10, cadence)
                    out = C.weave_np(clip, jobs, 0 if keep == "top" else 1)
                    assert out.shape == film.shape and np.array_equal(out, film), (name, tff, phase, keep, cadence)
                    assert not orphan.any() and cuts == [] and (locks[0] is not None) == (cadence == "3:2")
                    src = C.film_of(dict(source=jobs), origin, keep)
                    assert src[:, 0].tolist() == src[:, 1].tolist() == list(range(len(film)))
                assert C.verdict_np(*C.matches_np(M, keep)[::2]) == "3:2"


def test_margin_20_is_too_wide_for_the_noisy_locked_off_clip(planted):
    """Why the margin is 10 and why there is a lock.  At margin 20 and sigma 5 the raw matches on the locked-off clip find the first
    cycle or two and little after: without the lock all eight arms give 17 or 18 frames for 16.  The lock completes seven of them
    (agree 4 or 5, disagree 0); in the eighth (bottom field first, phase 0, top kept) it has three agreeing frames, does not lock
    and 18 frames come back.  On the clean video one arm (top field first, phase 0, top kept) misses a match without the lock and
    is completed with it."""
    wrong_raw, wrong_locked, rescued = [], [], []
    for (name, tff, phase), (film, clip, origin, clean, noisy) in planted.items():
        if name != "locked":
            continue
        for keep in ("top", "bottom"):
            n = {}
            for cadence in ("3:2", None):
                k, orphan, locks, jobs, cuts = _same_rules(noisy, keep, None, 20, cadence)
                n[cadence] = len(jobs), np.array_equal(C.weave_np(clip, jobs, 0 if keep == "top" else 1), film) if len(jobs) == len(film) else False
            print(tff, phase, keep, n)
            if not n[None][1]:
                wrong_raw.append((tff, phase, keep, n[None][0]))
            if not n["3:2"][1]:
                wrong_locked.append((tff, phase, keep, n["3:2"][0]))
            elif not n[None][1]:
                rescued.append((tff, phase, keep))
    assert len(wrong_raw) == 8 and {w[3] for w in wrong_raw} == {17, 18}
    assert wrong_locked == [(False, 0, "top", 18)] and len(rescued) == 7
    film, clip, origin, clean, noisy = planted["locked", True, 0]
    assert len(_same_rules(clean, "top", None, 20, None)[3]) == 16 and not np.array_equal(C.weave_np(clip, _same_rules(clean, "top", None, 20, None)[3], 0), film)
    assert np.array_equal(C.weave_np(clip, _same_rules(clean, "top", None, 20, "3:2")[3], 0), film)


def test_progressive_and_static_video_come_back_as_they_were(tennis):
    static = np.repeat(tennis[:1], 10, axis=0)
    for name, clip in (("progressive", tennis[:12]), ("static", static)):
        for src in (clip, C.noisy(clip, 5, 77)):
            M = C.scores_np(src)
            for keep in ("top", "bottom"):
                k, orphan, locks, jobs, cuts = _same_rules(M, keep, None, 10, "3:2")
                assert not k.any() and not orphan.any() and locks == [None] and jobs == [(t, t) for t in range(len(clip))], (name, keep)
                assert C.verdict_np(k, locks) == "none"
            assert np.array_equal(C.inverse_telecine_np(src, M=M)[0], src)


def test_joined_clips_give_every_film_frame_once_per_scene(tennis):
    """two telecined clips joined at a cut, the first started 0, 2, 3 and 4 frames into the cadence: every film frame once per scene;
    an orphan only at a scene's first frame (top kept) or last frame (bottom kept)"""
    second, origin_b = C.telecine(tennis[12:25], True, 1)
    for start in (0, 2, 3, 4):
        first, origin_a = C.telecine(tennis[:12], True, 0)
        first, origin_a = first[start:], origin_a[start:]
        clip, cut = np.concatenate([first, second]), len(first)
        origin = np.concatenate([origin_a, 100 + origin_b])
        M = C.scores_np(clip, [cut])
        for keep in ("top", "bottom"):
            p = 0 if keep == "top" else 1
            k, orphan, locks, jobs, cuts = _same_rules(M, keep, [cut], 10, "3:2")
            assert all(locks), (start, keep)
            film = C.film_of(dict(source=jobs), origin, keep)
            for (s, e), (a, b) in zip(C.spans(len(clip), [cut]), C.spans(len(jobs), cuts)):
                assert film[a:b, 0].tolist() == sorted(set(origin[s:e, p].tolist())), (start, keep)
            assert [t for t, _ in jobs] == sorted(t for t, _ in jobs) and all(0 <= b_ < len(clip) for _, b_ in jobs)
            where = np.flatnonzero(orphan).tolist()
            assert set(where) <= ({0, cut} if keep == "top" else {cut - 1, len(clip) - 1}), (start, keep, where)
            for i, (t, u) in enumerate(jobs):                          # every frame but an orphan is one film frame
                assert (film[i, 0] == film[i, 1]) == (not orphan[t]), (start, keep, t)
            print(start, keep, "orphans", where, "locks", locks, "frames", len(jobs), "cuts", cuts)
        # started two frames in, the top field of the first frame has lost its partner
        if start == 2:
            assert video.matches_from_scores(M, "top", [cut])[1].tolist()[0] is True


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_tools_check_before_the_device(no_device):
    f = np.zeros((7, 32, 40, 3), np.uint8)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(1, 8193, 8192, 3), strides=(0, 0, 0, 0))
    calls = TOOLS
    for call in calls:
        for bad in (f[0], f[..., :2], np.zeros((5, 32, 40), np.uint8), f.astype(np.float32), f.astype(np.int32), [[1, 2, 3]], None, big):
            with pytest.raises(ValueError, match="frames"):
                call(bad)
        for scenes in ([0], [7], [2, 2], [3, 1], "auto", "", [True], 3):
            with pytest.raises(ValueError, match="scenes"):
                call(f, scenes=scenes)
    for call in calls[1:]:
        for v in (0, 51, 2.5, True, False, None, "5", np.bool_(True)):
            with pytest.raises(ValueError, match="margin"):
                call(f, margin=v)
        for v in ("first", "TOP", "", None, 0, True):
            with pytest.raises(ValueError, match="keep"):
                call(f, keep=v)
    for v in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="return_scores"):
            video.detect_telecine(f, return_scores=v)
        with pytest.raises(ValueError, match="return_plan"):
            video.inverse_telecine(f, return_plan=v)
    for v in ("2:2", "", 32, True, False):
        with pytest.raises(ValueError, match="cadence"):
            video.inverse_telecine(f, cadence=v)
    for v in ("drop", "", None, True, 1):
        with pytest.raises(ValueError, match="orphans"):
            video.inverse_telecine(f, orphans=v)
    for kw in (dict(orphans="deinterlace"), dict(orphans="deinterlace", order=None), dict(orphans="deinterlace", order="auto"),
               dict(order="auto"), dict(order=""), dict(order=1), dict(order=True), dict(orphans="deinterlace", order="TFF")):
        with pytest.raises(ValueError, match="order"):
            video.inverse_telecine(f, **kw)
    good = {video.telecine_scores: ({}, dict(scenes=[2]), dict(scenes=[])),
            video.detect_telecine: ({}, dict(scenes=[2]), dict(keep="bottom", margin=1), dict(margin=50, return_scores=True), dict(margin=np.int64(7))),
            video.inverse_telecine: ({}, dict(scenes=[2, 5]), dict(keep="bottom", cadence=None), dict(orphans="deinterlace", order="bff"),
                                     dict(order="tff"), dict(return_plan=True, margin=20))}
    for call, kws in good.items():
        for kw in kws:
            with pytest.raises(AssertionError, match="device work"):
                call(f, **kw)
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(f, device="cpu", **kw)
    # the deinterlacer's mode for the orphans: the kept field is the first one under tff when it is the top field
    modes = [video._check_inverse_telecine_args(f, None, keep, 10, "3:2", "deinterlace", order, False)[4]
             for keep, order in (("top", "tff"), ("top", "bff"), ("bottom", "tff"), ("bottom", "bff"))]
    assert modes == [1, 2, 2, 1] and video._check_inverse_telecine_args(f, [3], "bottom", 10, None, "keep", None, True)[1:] == ([3], 1, 10, None)


def test_defaults_and_signatures():
    sig = inspect.signature(video.inverse_telecine).parameters
    assert list(sig) == ["frames_u8", "scenes", "keep", "margin", "cadence", "orphans", "order", "return_plan", "device"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, "top", 10, "3:2", "keep", None, False, None]
    sig = inspect.signature(video.detect_telecine).parameters
    assert list(sig) == ["frames_u8", "scenes", "keep", "margin", "return_scores", "device"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, "top", 10, False, None]
    assert [(k, v.default) for k, v in list(inspect.signature(video.telecine_scores).parameters.items())[1:]] == [("scenes", None), ("device", None)]
    sig = inspect.signature(video.matches_from_scores).parameters
    assert list(sig) == ["M", "keep", "scenes", "margin", "cadence"] and [sig[k].default for k in list(sig)[1:]] == ["top", None, 10, "3:2"]
    assert list(inspect.signature(video.plan_inverse_telecine).parameters) == ["k", "orphan", "scenes"]
    assert list(inspect.signature(ops.telecine_scores).parameters) == ["frames", "scene"]
    assert list(inspect.signature(ops.field_weave).parameters) == ["frames", "jobs", "keep", "out"]
    # the driver is untouched: no new parameter, the record as it was; the deinterlacer's words stand
    assert len(video._Call._fields) == 21 and video._Call._fields[-1] == "defects"
    assert not any("telecine" in k or "cadence" in k for k in inspect.signature(video.inpaint_video).parameters)
    assert "3:2 pulldown is not undone (inverse telecine is another tool)" in " ".join(video.deinterlace.__doc__.split())
    assert "3:2 pulldown votes in a pattern of its own" in " ".join(video.detect_interlace.__doc__.split())
    doc = " ".join(video.inverse_telecine.__doc__.split())
    for word in ("a progressive or static video comes back as it was", "every output row is a caller's row", "scene by scene and joined",
                 "only 3:2 locks", "2:3:3:2", "field-blended", "stays combed", "video-originated inserts", "not on real tape", "There is no CPU path"):
        assert word in doc, word


# ------------------------------------------------------------------------------------------------ header, binding, C entries
def _declared(header, name):
    decl = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert decl, name
    return [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")]


def test_header_and_binding_declare_the_entries():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    ints = {"L", "n", "H", "W", "keep"}
    for name, args in ENTRIES.items():
        assert _declared(header, name) == args, name
        res, types = lib.SYMBOLS[name]
        assert res is lib.C.c_int and len(types) == len(args)
        assert [t is lib._i32 for t in types] == [a in ints for a in args] and all(t in (lib._i32, lib._fp) for t in types), name
    assert "M[t][q][j][cell] = the sum of |2 Y_s[y][x] - Y_t[y-1][x] - Y_t[y+1][x]|" in header
    assert lib.ABI_VERSION == 9                          # symbols were only added
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "telecine.hip"]
    assert len(unit) == 1 and unit[0][1] == "telecine.o" and unit[0][1] in build.NOPK_OBJECTS and unit[0][2] == build.NOPK
    # the row of the table build() walks: verify_no_scratch over the unit's kernels on every build
    assert ("telecine.o", "telecine_", "inverse telecine", False) in build.KERNEL_CHECKS and "for obj, marker, what, _ in KERNEL_CHECKS" in inspect.getsource(build.build)


def test_source_has_no_floating_point():
    src = open(os.path.join(ROOT, "e2fgvi_amd", "csrc", "telecine.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double|half)\b", code) and not re.search(r"\d\.\d*f?\b", code)


def test_built_object_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "telecine.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("object or llvm-objdump not present (python -m e2fgvi_amd.build)")
    assert build.verify_no_scratch(obj="telecine.o", marker="telecine_", what="inverse telecine") == 2     # the scores and the weave


def test_entries_refuse_bad_arguments_and_return_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    ptrs = dict(frames=base + 1, scene=base + (1 << 16), jobs=base + (1 << 16), M=base + (2 << 16), out=base + (8 << 16) + 3)
    good = dict(ptrs, L=4, n=5, H=40, W=30, keep=1)
    for name, args in ENTRIES.items():
        who = name[len("e2fgvi_"):].encode()
        table = "scene" if "scene" in args else "jobs"
        no_work = (dict(L=0), dict(H=0), dict(W=0), dict(L=0, H=0, W=0)) if "M" in args else (dict(n=0), dict(H=0), dict(W=0), dict(n=0, L=0))

        def rc(**kw):
            a = dict(good, **kw)
            return getattr(so, name)(*[a[k] for k in args[:-1]], None)

        mine = [k for k in args if k in ptrs]
        null = {k: None for k in mine}
        for k in mine:
            assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), (name, k)
        assert rc(**{table: ptrs[table] + 2}) == -1 and b"aligned" in so.e2fgvi_last_error()
        if "M" in args:
            assert rc(M=ptrs["M"] + 4) == -1 and b"aligned" in so.e2fgvi_last_error()
        for k in [k for k in ("L", "n", "H", "W") if k in args]:
            assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), (name, k)
        assert rc(**dict(null, H=8193, W=8192)) == -1 and b"2^26" in so.e2fgvi_last_error()
        assert rc(**dict(null, H=0x7fffffff, W=0x7fffffff)) == -1
        assert rc(**dict(null, H=8192, W=8192)) == -1 and b"null" in so.e2fgvi_last_error()
        if "keep" in args:
            for v in (-1, 2, -(1 << 30), 1 << 30):
                assert rc(keep=v) == -1 and b"keep" in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), v
                assert rc(**dict(null, keep=v, n=0)) == -1               # decided from the arguments alone, work or not
            assert rc(L=0) == -1 and b"no frame" in so.e2fgvi_last_error()
        # no work: nothing is launched and the pointers are not looked at
        for kw in no_work:
            assert rc(**kw) == 0 and rc(**dict(null, **kw)) == 0, (name, kw)
    # any overlap of out with frames is refused, out == frames too; the result has n frames, the source L
    run = lambda frames, out, L, n: so.e2fgvi_field_weave(frames, ptrs["jobs"], out, L, n, 40, 30, 0, None)
    size = 3 * 40 * 30
    for frames, out, L, n in ((base, base, 4, 4), (base, base + 1, 4, 1), (base, base + 4 * size - 1, 4, 1), (base + 6 * size - 1, base, 1, 6),
                              (base + 5, base, 4, 4)):
        assert run(frames, out, L, n) == -1 and b"overlap" in so.e2fgvi_last_error(), (frames, out, L, n)
    assert so.e2fgvi_abi_version() == 9
