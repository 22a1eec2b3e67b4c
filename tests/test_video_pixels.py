"""Real pixels for restored holes, host side: the numpy restatement of the step, the chains and the fill
(tests/pixel_track_cases.py) on its named cases -- the exact-truth case, the sharpness bound that must not depend on a pixel's age
-- the planner video.plan_pixel_chains over an exhaustive sweep of small videos, paste_mask's tables against PIL, the argument
checks of propagate_pixels that need no device, and the C entries' error paths on the loaded library.  The kernels and the driver
are compared with the restatement in tests/test_gpu_video_pixels.py."""
import itertools
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import mask_key_cases as K
from tests import pixel_track_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("variant", P.VARIANTS)
def test_every_wrong_reading_changes_some_case(variant):
    changed = []
    for n in P.NAMES:
        out, source = P.propagate_np(P.case(n), True, variant)[:2]
        if not (np.array_equal(out, P.reference(n)[0]) and np.array_equal(source, P.reference(n)[1])):
            changed.append(n)
    print(variant, "changes", changed)
    assert changed


@pytest.mark.parametrize("name", P.NAMES)
def test_guarantees_hold_in_every_case(name):
    """a byte outside the hole and a hole byte of source 3 are filled's; source is 0 exactly outside the hole; a reached pixel's
    origin frame lies in the video and in the pixel's scene"""
    c = P.case(name)
    out, source, age, origin = P.reference(name)
    hole = c["hole"] == 1
    assert np.array_equal(source == 0, ~hole) and set(np.unique(source).tolist()) <= {0, 1, 2, 3}
    keep = ~hole | (source == 3)
    assert np.array_equal(out[keep], c["filled"][keep])
    assert np.array_equal(age[:, ~hole], np.zeros_like(age[:, ~hole])) and (age[:, hole] != 0).all()
    cuts = c.get("scenes") or []
    scene_of = lambda f: sum(1 for x in cuts if f >= x)
    for t in range(c["L"]):
        for pl in (0, 1):
            a = age[pl, t][hole[t] & (age[pl, t] != 255)].astype(int)
            assert (a <= (c.get("reach") or 254)).all()
            for f in set((t + a if pl else t - a).tolist()):
                assert 0 <= f < c["L"] and scene_of(f) == scene_of(t), (t, pl, f)


def test_static_hole_under_zero_flow_reaches_nothing():
    c = P.case("zero_7x5")
    out, source, age, _ = P.reference("zero_7x5")
    assert c["hole"].any() and (source[c["hole"] == 1] == 3).all() and np.array_equal(out, c["filled"])
    assert (age[:, c["hole"] == 1] == 255).all()


def test_integer_shift_returns_the_truth_exactly():
    c = P.case("int_shift_24x61")
    out, source, age, origin = P.reference("int_shift_24x61")
    got = (source == 1) | (source == 2)
    assert got.sum() > 1000 and np.array_equal(out[got], c["truth"][got])
    assert (c["src"][got] != c["truth"][got]).any()                     # the caller's frames hold something else there
    hole = c["hole"] == 1
    for t in range(6, 10):                              # a condition on the case: in the middle everything can be fetched
        assert hole[t].any() and not (source[t][hole[t]] == 3).any(), t
    # the origins are the pixel minus (plus) age times the shift, whole numbers
    ys, xs = np.mgrid[0:c["H"], 0:c["W"]]
    for pl, sign in ((0, -1.0), (1, 1.0)):
        m = hole & (age[pl] != 255)
        a = age[pl].astype(np.float64)
        assert np.array_equal(origin[pl, ..., 0][m], (xs[None] + sign * a * P.INT_SHIFT[0])[m])
        assert np.array_equal(origin[pl, ..., 1][m], (ys[None] + sign * a * P.INT_SHIFT[1])[m])


def _half_errors(out, source, age):
    """|out - analytic truth| at the propagated pixels of half_shift_40x60 and the age each was fetched over"""
    c = P.case("half_shift_40x60")
    truth = np.stack([P.half_truth(t) for t in range(c["L"])])
    got = (source == 1) | (source == 2)
    a = np.where(source == 1, age[0], age[1])
    return np.abs(out.astype(np.float64) - truth).max(-1)[got], a[got]


def test_half_shift_origins_are_exact_and_sharpness_does_not_depend_on_age():
    """A = (40, 30), k = ((0.9, 0.3), (-0.4, 0.8)): the bound is 4.5 + 3.0 + 1 = 8.5 grey levels (pixel_track_cases.HALF_WAVES)"""
    c = P.case("half_shift_40x60")
    out, source, age, origin = P.reference("half_shift_40x60")
    hole = c["hole"] == 1
    ys, xs = np.mgrid[0:c["H"], 0:c["W"]]
    for pl, sign in ((0, -1.0), (1, 1.0)):
        m = hole & (age[pl] != 255)
        a = age[pl].astype(np.float64)
        assert m.sum() > 500 and age[pl][m].max() >= 6
        assert np.array_equal(origin[pl, ..., 0][m], (xs[None] + sign * a * P.HALF_SHIFT[0])[m])
        assert np.array_equal(origin[pl, ..., 1][m], (ys[None] + sign * a * P.HALF_SHIFT[1])[m])
    assert P.HALF_BOUND == 8.5
    err, a = _half_errors(out, source, age)
    old = a >= 6
    print("half shift: %d propagated pixels, worst error %.2f; %d of age >= 6, worst %.2f; bound %.2f"
          % (len(err), err.max(), old.sum(), err[old].max(), P.HALF_BOUND))
    assert len(err) > 500 and err.max() <= P.HALF_BOUND
    assert old.sum() > 100 and err[old].max() <= P.HALF_BOUND
    # colours dragged along frame by frame are blurred once per step: that reading breaks the bound, and most at the old pixels
    bo, bs, ba, _ = P.propagate_np(c, True, "carry_colours")
    berr, bage = _half_errors(bo, bs, ba)
    print("carrying colours: worst error %.2f, at age >= 6 %.2f" % (berr.max(), berr[bage >= 6].max()))
    assert berr[bage >= 6].max() > 2 * P.HALF_BOUND


def test_moving_hole_is_reached_at_its_distance_in_frames():
    c = P.case("square_40x60")
    out, source, age, origin = P.reference("square_40x60")
    hole = c["hole"] == 1
    L = c["L"]
    for t in range(L):
        wants = []
        for pl in (0, 1):
            frames = range(t - 1, -1, -1) if pl == 0 else range(t + 1, L)
            want = np.full(hole[t].shape, 255)
            for f in frames:                            # the nearest frame of that direction in which the square is off the pixel
                want = np.where((want == 255) & ~hole[f], abs(t - f), want)
            assert np.array_equal(age[pl, t][hole[t]], want[hole[t]]), (t, pl)
            wants.append(want)
        # a pixel the square covers in every frame of a direction is not reached from there; from neither: it is left as it was
        never = hole[t] & (wants[0] == 255) & (wants[1] == 255)
        assert np.array_equal(source[t] == 3, never), t
        assert np.array_equal(source[t] == 2, hole[t] & (wants[1] < wants[0])), t
    got = hole & (source != 3)
    assert got.sum() > 500 and (source == 3).any() and np.array_equal(out[got], c["truth"][got])


def test_reach_cut_and_borders_in_the_smooth_case():
    c = P.case("smooth_70x90")
    out, source, age, origin = P.reference("smooth_70x90")
    hole = c["hole"] == 1
    assert (age[:, hole][age[:, hole] != 255] <= 2).all() and (age[:, hole] == 2).any()
    assert (age[:, 5][:, hole[5]] == 255).all() and (age[1, 4][hole[4]] == 255).all()     # nothing comes over the cut at 5
    assert hole[:, -1, -1].all() and (source == 3).any() and (source == 1).any() and (source == 2).any()
    loose = P.propagate_np(c, check=False)
    assert ((loose[1] != 3) & (source == 3)).sum() > 50       # the consistency test drops what is pulled from the patches


@pytest.mark.parametrize("v, lo, hi", [(0.4, 0.0, 0.0), (1.0, 1.0, 1.0), (1.4, 1.0, 1.0), (1.6, 0.2, 0.5), (2.0, 1.0, 1.0)])
def test_the_walk_advances_by_the_rounded_flow(v, lo, hi):
    """A known limit of the nearest-pixel rule, pinned so that it stays visible: through a static hole the walk moves
    by the flow rounded to whole pixels and the origin by the flow itself.  A pan of 0.4 px per frame never leaves the hole; one of
    1.6 leaves it before its origin does, and the fill refuses an origin whose corners are hole pixels; 1.0, 1.4 and 2.0 fill all."""
    L, H, W = 16, 24, 61
    rng = np.random.RandomState(3)
    fwd, bwd = K._uniform(L, H, W, v, 0.0)
    c = P._finish(dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, hole=P._static_hole(L, H, W, 8, 17, 24, 36),
                       truth=rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)), 4)
    source = P.propagate_np(c)[1]
    share = ((source == 1) | (source == 2)).sum() / float((c["hole"] == 1).sum())
    print("pan %.1f px per frame: %.3f of the hole pixels filled" % (v, share))
    assert lo <= share <= hi


# ------------------------------------------------------------------------------------------------ the planner
def _check_plan(length, cuts):
    steps = video.plan_pixel_chains(length, scenes=cuts or None)
    bounds = list(zip([0] + cuts, cuts + [length]))
    scene_of = lambda f: sum(1 for c in cuts if f >= c)
    assert len(steps) == max(b - a for a, b in bounds) - 1
    written, seen = {}, []
    for s, step in enumerate(steps):
        assert step, "an empty step"
        reads = [(d, t if d == 0 else t + 1) for t, d in step]
        writes = [(d, t + 1 if d == 0 else t) for t, d in step]
        assert len(set(writes)) == len(writes) and not set(writes) & set(reads)
        for (t, d), r, w in zip(step, reads, writes):
            assert 0 <= t < length - 1 and d in (0, 1)
            assert scene_of(r[1]) == scene_of(w[1])     # nothing crosses a cut
            first = [a if d == 0 else b - 1 for a, b in bounds if a <= r[1] < b][0]
            assert r[1] == first or written.get(r) is not None and written[r] < s
            assert w not in written
            written[w] = s
            seen.append((t, d))
    pairs = [t for a, b in bounds for t in range(a, b - 1)]
    assert sorted(seen) == sorted((t, d) for t in pairs for d in (0, 1))
    assert sorted(j for s in steps for j in s) == sorted(j for ch in P.chains_np(length, cuts) for j in ch)
    return steps


def test_planner_invariants_exhaustively():
    n = 0
    for length in range(1, 11):
        for k in (0, 1, 2, 3):
            for cuts in itertools.combinations(range(1, length), k):
                _check_plan(length, list(cuts))
                n += 1
    assert n > 300
    assert _check_plan(7, [4]) == [[(0, 0), (2, 1), (4, 0), (5, 1)], [(1, 0), (1, 1), (5, 0), (4, 1)], [(2, 0), (0, 1)]]
    assert video.plan_pixel_chains(1) == [] and video.plan_pixel_chains(3, scenes=[1, 2]) == []
    assert len(video.plan_pixel_chains(100)) == 99 and len(video.plan_pixel_chains(100, scenes=list(range(10, 100, 10)))) == 9
    assert video.plan_pixel_chains(np.int64(3), scenes=[]) == [[(0, 0), (1, 1)], [(1, 0), (0, 1)]]
    for bad in ([0], [6], [3, 3], [2.5], [4, 2]):
        with pytest.raises(ValueError, match="scenes"):
            video.plan_pixel_chains(6, scenes=bad)
    for bad in (0, -3, 2.0, True, "4"):
        with pytest.raises(ValueError, match="length"):
            video.plan_pixel_chains(bad)


# ------------------------------------------------------------------------------------------------ paste_mask's tables
@pytest.mark.parametrize("frame_hw, size", [((37, 53), (20, 11)), ((48, 64), (16, 12)), ((30, 30), (30, 30)), ((1080 // 8, 1920 // 8), (54, 30))])
def test_paste_tables_are_pils_nearest_upscale(frame_hw, size):
    from PIL import Image
    H, W = frame_hw
    w, h = size
    rng = np.random.RandomState(H + w)
    m = (rng.rand(h, w) < 0.5).astype(np.uint8)
    ytab, xtab = video._paste_tables(frame_hw, size)
    assert ytab.shape == (H,) and xtab.shape == (W,)
    want = np.array(Image.fromarray(m).resize((W, H), Image.NEAREST))
    assert np.array_equal(m[ytab][:, xtab], want)
    assert np.array_equal(ytab, video.nearest_table(h, H)) and np.array_equal(xtab, video.nearest_table(w, W))


# ------------------------------------------------------------------------------------------------ argument checks, no device
def _no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work before the argument checks were done")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_propagate_pixels_device", touched)


class _Gen:
    def engine(self):
        raise AssertionError("the engine was asked for")


def test_propagate_pixels_checks_its_arguments_before_the_device(monkeypatch):
    _no_device(monkeypatch)
    f = np.zeros((5, 6, 8, 3), np.uint8)
    m = np.zeros((5, 3, 4), np.uint8)
    fl = (np.zeros((4, 6, 8, 2), np.float32),) * 2
    call = lambda *a, **k: video.propagate_pixels(None, *a, **dict(dict(flows=fl), **k))
    for bad in (f[0], f[..., :2], f[:0]):
        with pytest.raises(ValueError, match="frames"):
            call(bad, m, f)
    for filled in (f[:4], f[:, :5], f[0], None, [[1]]):
        with pytest.raises(ValueError, match="filled_u8"):
            call(f, m, filled)
    for masks in (m[:4], m[0], np.zeros((5, 3, 4, 1), np.uint8), None):
        with pytest.raises(ValueError, match="masks"):
            call(f, masks, f)
    for flows in ((fl[0],), fl + fl[:1], (fl[0], fl[1][:3]), (fl[0][..., :1], fl[1]), 7, (None, None)):
        with pytest.raises(ValueError, match="flows"):
            call(f, m, f, flows=flows)
    call_ok = dict(size=(4, 3))                         # size= is the model's: the flows keep the frames' size
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(f, m, f, device="cpu", **call_ok)
    for size in ((0, 4), (8,), (8.5, 6), 8, (8, 6, 3)):
        with pytest.raises(ValueError, match="size"):
            call(f, m, f, size=size)
    for scenes in ([0], [5], [2, 2], "auto"):
        with pytest.raises(ValueError, match="scenes"):
            call(f, m, f, scenes=scenes)
    for reach in (0, -1, 1.5, False, 255):
        with pytest.raises(ValueError, match="reach"):
            call(f, m, f, reach=reach)
    for name in ("check", "dilate", "return_source"):
        for bad in (None, 1, "yes"):
            with pytest.raises(ValueError, match=name):
                call(f, m, f, **{name: bad})
    for model in (None, lambda x, n: (x, None)):        # without flows the generator is needed
        with pytest.raises(TypeError, match="InpaintGenerator"):
            video.propagate_pixels(model, f, m, f)
    # good arguments pass the checks: on a host without a device the call gets as far as the refusal of the CPU device
    for kw in ({}, dict(scenes=[2]), dict(reach=254, check=False, dilate=False, return_source=True), dict(flows=None)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            video.propagate_pixels(_Gen(), f, m, f, device="cpu", **dict(dict(flows=fl), **kw))


# ------------------------------------------------------------------------------------------------ header, binding, C entries
def test_header_and_binding_declare_the_entries():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    names = {}
    for entry in ("e2fgvi_pixel_track_step", "e2fgvi_pixel_fill"):
        decl = re.search(r"int %s\(([^;]*)\);" % entry, header)
        assert decl, entry
        names[entry] = [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")]
    assert names["e2fgvi_pixel_track_step"] == ["hole", "age", "origin", "fwd", "bwd", "jobs", "n", "L", "H", "W", "reach", "check", "stream"]
    assert names["e2fgvi_pixel_fill"] == ["src", "hole", "age", "origin", "out", "source", "L", "H", "W", "stream"]
    res, args = lib.SYMBOLS["e2fgvi_pixel_track_step"]
    assert len(args) == 13 and args[-1] is lib._fp and args[:6] == [lib._fp] * 6 and args[6:12] == [lib._i32] * 6
    res, args = lib.SYMBOLS["e2fgvi_pixel_fill"]
    assert len(args) == 10 and args[-1] is lib._fp and args[:6] == [lib._fp] * 6 and args[6:9] == [lib._i32] * 3
    assert lib.ABI_VERSION == 9                          # symbols were only added
    assert callable(ops.pixel_track_step) and callable(ops.pixel_fill) and ops.PIXEL_REACH_MAX == 254 == P.REACH_MAX
    assert callable(video.paste_mask) and callable(video.plan_pixel_chains) and callable(video.propagate_pixels)
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "pixel_track.hip"]
    assert len(unit) == 1 and unit[0][1] == "pixel_track.o" and "-ffp-contract=off" in unit[0][2] and unit[0][1] in build.NOPK_OBJECTS
    assert all(f in unit[0][2] for f in build.NOPK)


def test_entries_refuse_bad_arguments_and_return_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    ptrs = ("hole", "age", "origin", "fwd", "bwd", "jobs")
    good = dict({k: base + (i << 16) for i, k in enumerate(ptrs)}, n=2, L=3, H=7, W=5, reach=254, check=1)
    order = ptrs + ("n", "L", "H", "W", "reach", "check")

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_pixel_track_step(*[a[k] for k in order], None)

    for k in ptrs:
        assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
    for L in (1, 0, -4):
        assert rc(L=L) == -1 and b"L >= 2" in so.e2fgvi_last_error()
        assert rc(L=L, n=0) == -1
    for k in ("n", "H", "W"):
        assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error(), k
    for v in (2, -1, 256):
        assert rc(check=v) == -1 and b"check" in so.e2fgvi_last_error()
    for v in (0, -1, 255, 1 << 20):
        assert rc(reach=v) == -1 and b"reach" in so.e2fgvi_last_error()
        assert rc(reach=v, n=0) == -1
    assert rc(H=46341, W=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
    assert rc(H=1, W=2147483647 - 256) == -1 and rc(H=0x7fffffff, W=0x7fffffff) == -1
    for k in ("fwd", "bwd", "origin"):
        assert rc(**{k: good[k] + 4}) == -1 and b"aligned" in so.e2fgvi_last_error(), k
    assert rc(jobs=good["jobs"] + 2) == -1 and b"aligned" in so.e2fgvi_last_error()
    null = {k: None for k in ptrs}
    assert rc(n=0) == 0 and rc(H=0) == 0 and rc(W=0) == 0
    assert rc(n=0, **null) == 0 and rc(H=0, **null) == 0 and rc(W=0, H=0, n=0, **null) == 0
    assert rc(n=0, check=0, L=2, reach=1) == 0

    fptrs = ("src", "hole", "age", "origin", "out", "source")
    fgood = dict({k: base + (i << 16) for i, k in enumerate(fptrs)}, L=3, H=7, W=5)

    def frc(**kw):
        a = dict(fgood, **kw)
        return so.e2fgvi_pixel_fill(*[a[k] for k in fptrs + ("L", "H", "W")], None)

    for k in fptrs[:5]:
        assert frc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
    for k in ("L", "H", "W"):
        assert frc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error(), k
    assert frc(H=46341, W=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
    assert frc(origin=fgood["origin"] + 4) == -1 and b"aligned" in so.e2fgvi_last_error()
    fnull = {k: None for k in fptrs}
    assert frc(L=0) == 0 and frc(H=0) == 0 and frc(W=0) == 0
    assert frc(L=0, **fnull) == 0 and frc(H=0, **fnull) == 0 and frc(W=0, H=0, L=0, **fnull) == 0
    assert so.e2fgvi_abi_version() == 9


def test_the_object_rounds_every_operation_and_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "pixel_track.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("pixel_track.o not built here (python -m e2fgvi_amd.build)")
    assert build.verify_no_fma64(obj="pixel_track.o") > 10
    assert build.verify_no_scratch(obj="pixel_track.o", marker="pixel_", what="pixel propagation") == 2
