"""Masks from keyframes, host side: the numpy restatement of the step and of the propagation (tests/mask_key_cases.py) on its named
cases, the planner video.plan_mask_chains over an exhaustive sweep of small videos, the argument checks of plan_mask_chains,
propagate_masks and inpaint_video(mask_keys=) that need no device, and the C entry's error paths on the loaded library.  The kernel
and the driver are compared with the restatement in tests/test_gpu_video_mask_keys.py."""
import itertools
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import mask_key_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shift_zero_fill(m, dx, dy):
    """np.roll by (dx, dy) with what wraps around set to zero"""
    out = np.roll(m, (dy, dx), (0, 1))
    if dy > 0:
        out[:dy] = 0
    elif dy < 0:
        out[dy:] = 0
    if dx > 0:
        out[:, :dx] = 0
    elif dx < 0:
        out[:, dx:] = 0
    return out


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("variant", K.VARIANTS)
def test_every_wrong_reading_changes_some_case(variant):
    changed = [n for n in K.NAMES if not np.array_equal(K.propagate_np(K.case(n), True, variant)[0], K.reference(n)[0])]
    print(variant, "changes", changed)
    assert changed


def test_no_case_decides_near_the_threshold():
    """every comparison of the consistency test is decided by at least 1e-9 (the bound of tests/test_gpu_warp_error.py), so the
    kernel's answer does not hang on its last bit; the tie case is all dyadic and exempt"""
    for n in K.NAMES:
        margin = min(r[3] for r in K.reference(n)[1])
        print("%s: margin %.3e over %d candidates" % (n, margin, sum(r[4] for r in K.reference(n)[1])))
        assert n in K.TIE_CASES or margin >= 1e-9, (n, margin)


def test_zero_flows_return_the_key_mask():
    c = K.case("zero_7x5")
    key = K.binarise(c["key_masks"])[0]
    for check in (True, False):
        masks = K.reference("zero_7x5", check)[0]
        assert key.any() and all(np.array_equal(masks[t], key) for t in range(c["L"]))


def test_shift_is_roll_with_zero_fill():
    c = K.case("shift_17x301")
    key, k = K.binarise(c["key_masks"])[0], c["keys"][0]
    masks = K.reference("shift_17x301")[0]
    for t in range(c["L"]):
        want = _shift_zero_fill(key, (t - k) * K.SHIFT[0], (t - k) * K.SHIFT[1])
        assert np.array_equal(masks[t], want), t
    assert masks[3].any() and masks[3].sum() < key.sum() and not masks[4].any()          # it leaves through the border and vanishes
    assert masks[0].any() and masks[0].sum() < key.sum()


def test_tie_case_is_exact_and_holds_ties():
    c = K.case("tie_9x13")
    M = K.binarise(c["key_masks"])[1].astype(np.float64)
    s = 0.25 * (M[:-1, :-1] + M[:-1, 1:] + M[1:, :-1] + M[1:, 1:])                       # q = p + (0.5, 0.5)
    assert (s == 0.5).any()
    want = np.zeros_like(M, dtype=np.uint8)
    want[:-1, :-1] = s >= 0.5
    assert np.array_equal(K.reference("tie_9x13")[0][2], want)


@pytest.mark.parametrize("key", [0, 7])
def test_square_keeps_inside_the_object_and_holds(key):
    c = K.square_case(key)
    masks, _ = K.propagate_np(c)
    loose, _ = K.propagate_np(c, check=False)
    order = list(range(8)) if key == 0 else list(range(7, -1, -1))
    counts = [int(masks[t].sum()) for t in order]
    trail = [int((loose[t].astype(bool) & ~K.square_truth(t)).sum()) for t in order]
    print("key %d: counts %s, pixels outside the object without the test %s" % (key, counts, trail))
    for t in range(8):
        assert not (masks[t].astype(bool) & ~K.square_truth(t)).any(), t
    assert counts[0] == 120 and len(set(counts[2:])) == 1 and 90 <= counts[2] <= 120
    assert trail[-1] >= 90 and trail == sorted(trail)                                   # and without it the trail keeps growing


def test_smooth_case_frames():
    """keys 0, 4, 5, a cut at 5, reach 2: frame 1 from key 0, frame 3 from key 4, frame 2 the union of both"""
    c = K.case("smooth_70x90")
    masks = K.reference("smooth_70x90")[0]
    for k, m in zip(c["keys"], K.binarise(c["key_masks"])):
        assert np.array_equal(masks[k], m)
    only = lambda keys: K.propagate_np(dict(c, keys=keys, key_masks=c["key_masks"][[c["keys"].index(k) for k in keys]]))[0]
    a, b = only([0]), only([4])
    assert np.array_equal(masks[1], a[1]) and np.array_equal(masks[3], b[3]) and np.array_equal(masks[2], a[2] | b[2])
    assert a[2].any() and b[2].any() and not a[3].any() and not b[1].any() and not b[5].any()


# ------------------------------------------------------------------------------------------------ the planner
def _check_plan(length, keys, cuts, reach):
    steps = video.plan_mask_chains(length, keys, scenes=cuts or None, reach=reach)
    scene_of = lambda f: sum(1 for c in cuts if f >= c)
    written = {}
    for s, step in enumerate(steps):
        assert step, "an empty step"
        reads = [(d, t if d == 0 else t + 1) for t, d in step]
        writes = [(d, t + 1 if d == 0 else t) for t, d in step]
        assert len(set(writes)) == len(writes) and not set(writes) & set(reads)
        for (t, d), r, w in zip(step, reads, writes):
            assert 0 <= t < length - 1 and d in (0, 1)
            assert scene_of(r[1]) == scene_of(w[1]) and w[1] not in keys
            # what a job reads is a key or was written by an earlier step
            assert r[1] in keys or written.get(r) is not None and written[r] < s
            assert w not in written
            written[w] = s
    want = set()
    for f in range(length):
        for d in (0, 1):
            before = [k for k in keys if (k < f if d == 0 else k > f) and scene_of(k) == scene_of(f)]
            if not before or f in keys:
                continue
            k = max(before) if d == 0 else min(before)
            if reach is None or abs(f - k) <= reach:
                want.add((d, f))
                assert written[(d, f)] == abs(f - k) - 1
    assert set(written) == want
    return steps


def test_planner_invariants_exhaustively():
    n = 0
    for length in range(1, 10):
        for nk in (1, 2, 3):
            for keys in itertools.combinations(range(length), nk):
                for cuts in [[]] + [[c] for c in range(1, length)]:
                    for reach in (None, 1, 2, 3):
                        _check_plan(length, list(keys), cuts, reach)
                        n += 1
    assert n > 5000
    steps = _check_plan(9, [2, 7], [5], None)
    assert steps == [[(2, 0), (1, 1), (7, 0), (6, 1)], [(3, 0), (0, 1), (5, 1)]]
    assert video.plan_mask_chains(4, [0, 1, 2, 3]) == [] and video.plan_mask_chains(1, [0]) == []
    assert len(video.plan_mask_chains(100, [50])) == 50 and len(video.plan_mask_chains(100, list(range(0, 100, 10)))) == 9
    assert video.plan_mask_chains(6, np.array([1, 4]), scenes=[], reach=np.int64(1)) == [[(1, 0), (0, 1), (4, 0), (3, 1)]]


def test_planner_is_the_reference_walk():
    for name in K.NAMES:
        c = K.case(name)
        steps = video.plan_mask_chains(c["L"], c["keys"], c.get("scenes"), c.get("reach"))
        chains = K.chains_np(c["L"], c["keys"], c.get("scenes"), c.get("reach"))
        assert sorted(j for s in steps for j in s) == sorted(j for ch in chains for j in ch)
        assert len(steps) == max(len(ch) for ch in chains)


def test_plan_mask_chains_checks_its_arguments():
    for bad in ([], None, [3, 3], [4, 2], [-1], [6], [1.5], [True], "ab", 3):
        with pytest.raises(ValueError, match="keys"):
            video.plan_mask_chains(6, bad)
    for bad in (0, -1, 2.5, True, "2"):
        with pytest.raises(ValueError, match="reach"):
            video.plan_mask_chains(6, [2], reach=bad)
    for bad in ([0], [6], [3, 3], [2.5]):
        with pytest.raises(ValueError, match="scenes"):
            video.plan_mask_chains(6, [2], scenes=bad)
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="length"):
            video.plan_mask_chains(bad, [0])


# ------------------------------------------------------------------------------------------------ argument checks, no device
class _Gen:
    """what the checks take for the generator: an object with engine()"""
    def engine(self):
        raise AssertionError("the engine was asked for")


def _no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work before the argument checks were done")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_propagate_masks_device", touched)


def test_propagate_masks_checks_its_arguments_before_the_device(monkeypatch):
    _no_device(monkeypatch)
    f = np.zeros((5, 6, 8, 3), np.uint8)
    m = np.zeros((2, 6, 8), np.uint8)
    fl = (np.zeros((4, 6, 8, 2), np.float32),) * 2
    call = lambda *a, **k: video.propagate_masks(None, *a, **dict(dict(flows=fl), **k))
    for bad in (f[0], f[..., :2], f[:0]):
        with pytest.raises(ValueError, match="frames"):
            call(bad, m, [0, 3])
    for keys in ([], [3, 0], [0, 5], [0, 0], [1.0, 2.0], None):
        with pytest.raises(ValueError, match="keys"):
            call(f, m, keys)
    for masks in (m[:1], m[0], np.zeros((3, 6, 8), np.uint8), [[1]], None):
        with pytest.raises(ValueError, match="key_masks"):
            call(f, masks, [0, 3])
    for flows in ((fl[0],), fl + fl[:1], (fl[0], fl[1][:3]), (fl[0][..., :1], fl[1]), 7, (None, None)):
        with pytest.raises(ValueError, match="flows"):
            call(f, m, [0, 3], flows=flows)
    with pytest.raises(ValueError, match="flows"):      # the flows must have the size the frames are resized to
        call(f, m, [0, 3], size=(16, 12))
    for size in ((0, 4), (8,), (8.5, 6), 8, (8, 6, 3)):
        with pytest.raises(ValueError, match="size"):
            call(f, m, [0, 3], size=size)
    for scenes in ([0], [5], [2, 2], "auto"):
        with pytest.raises(ValueError, match="scenes"):
            call(f, m, [0, 3], scenes=scenes)
    for reach in (0, -1, 1.5, False):
        with pytest.raises(ValueError, match="reach"):
            call(f, m, [0, 3], reach=reach)
    for check in (None, 1, "yes"):
        with pytest.raises(ValueError, match="check"):
            call(f, m, [0, 3], check=check)
    # without flows the generator is needed
    for model in (None, lambda x, n: (x, None)):
        with pytest.raises(TypeError, match="InpaintGenerator"):
            video.propagate_masks(model, f, m, [0, 3])


def test_inpaint_video_mask_keys_checks_before_the_device(monkeypatch):
    _no_device(monkeypatch)
    f = np.zeros((12, 8, 8, 3), np.uint8)
    m = np.zeros((2, 8, 8), np.uint8)
    gen = _Gen()
    for keys in ([], [5, 2], [0, 12], [1, 1], [0.5, 2], 4):
        with pytest.raises(ValueError, match="mask_keys"):
            video.inpaint_video(gen, f, m, mask_keys=keys, device="cpu")
    for masks in (m[:1], np.zeros((12, 8, 8), np.uint8), m[0]):
        with pytest.raises(ValueError, match="mask_keys"):
            video.inpaint_video(gen, f, masks, mask_keys=[2, 9], device="cpu")
    with pytest.raises(ValueError, match="overlay"):
        video.inpaint_video(gen, f, "overlay", mask_keys=[2, 9], device="cpu")
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.inpaint_video(lambda x, n: (x, None), f, m, mask_keys=[2, 9], device="cpu")
    with pytest.raises(ValueError, match="scenes"):
        video.inpaint_video(gen, f, m, mask_keys=[2, 9], scenes=[12], device="cpu")
    # good arguments pass the checks: on a host without a device the call gets as far as the refusal of the CPU device
    for kw in ({}, dict(scenes="auto"), dict(scenes=[4]), dict(size=(108, 60), restore=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            video.inpaint_video(gen, f, m, mask_keys=[2, 9], device="cpu", **kw)
    # and without mask_keys nothing has changed: K masks for L frames are not looked at here
    with pytest.raises(RuntimeError, match="no CPU path"):
        video.inpaint_video(gen, f, np.zeros((12, 8, 8), np.uint8), device="cpu")


# ------------------------------------------------------------------------------------------------ header, binding, C entry
def test_header_and_binding_declare_the_entry():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    decl = re.search(r"int e2fgvi_mask_track_step\(([^;]*)\);", header)
    assert decl
    names = [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")]
    assert names == ["planes", "fwd", "bwd", "jobs", "n", "L", "H", "W", "check", "stream"]
    res, args = lib.SYMBOLS["e2fgvi_mask_track_step"]
    assert len(args) == 10 and args[-1] is lib._fp and args[:4] == [lib._fp] * 4 and args[4:9] == [lib._i32] * 5
    assert lib.ABI_VERSION == 9                          # a symbol was only added
    assert callable(ops.mask_track_step) and callable(video.plan_mask_chains) and callable(video.propagate_masks)
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "mask_track.hip"]
    assert len(unit) == 1 and "-ffp-contract=off" in unit[0][2] and unit[0][1] in build.NOPK_OBJECTS


def test_entry_refuses_bad_arguments_and_returns_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    good = dict(planes=base, fwd=base + (1 << 16), bwd=base + (1 << 17), jobs=base + (1 << 18), n=2, L=3, H=7, W=5, check=1)
    order = ("planes", "fwd", "bwd", "jobs", "n", "L", "H", "W", "check")

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_mask_track_step(*[a[k] for k in order], None)

    for k in ("planes", "fwd", "bwd", "jobs"):
        assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
    for L in (1, 0, -4):
        assert rc(L=L) == -1 and b"L >= 2" in so.e2fgvi_last_error()
        assert rc(L=L, n=0) == -1
    for k in ("n", "H", "W"):
        assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error(), k
    for v in (2, -1, 256):
        assert rc(check=v) == -1 and b"check" in so.e2fgvi_last_error()
    assert rc(H=46341, W=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
    assert rc(H=1, W=2147483647 - 256) == -1 and rc(H=0x7fffffff, W=0x7fffffff) == -1
    assert rc(fwd=good["fwd"] + 4) == -1 and b"aligned" in so.e2fgvi_last_error()
    assert rc(jobs=good["jobs"] + 2) == -1 and b"aligned" in so.e2fgvi_last_error()
    # no work: 0, whatever the pointers are
    null = dict(planes=None, fwd=None, bwd=None, jobs=None)
    assert rc(n=0) == 0 and rc(H=0) == 0 and rc(W=0) == 0
    assert rc(n=0, **null) == 0 and rc(H=0, **null) == 0 and rc(W=0, H=0, n=0, **null) == 0
    assert rc(n=0, check=0, L=2) == 0
    assert so.e2fgvi_abi_version() == 9
