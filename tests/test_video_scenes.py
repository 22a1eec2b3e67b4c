"""Scene cuts in the video driver, host side: plan_windows(scenes=) and plan_reuse on its list, cuts_from_scores, the numpy
restatement of the block-histogram difference (tests/scene_diff_cases.py) against hand-counted frames and the tennis fixture, and
the argument checks of the C entries and of inpaint_video that need no device.  The kernel and the drivers are compared with
these in tests/test_gpu_video_scenes.py."""
import numpy as np
import pytest
import torch

from e2fgvi_amd import video
from tests import scene_diff_cases as S

PLANS = [(23, [9]), (41, [5, 6, 30]), (12, [11]), (7, [])]
ARGS = [(5, 10, -1), (3, 7, 4), (2, 4, 2)]                     # (neighbor_stride, ref_length, num_ref)


def _scene_bounds(L, scenes):
    return list(zip([0] + list(scenes), list(scenes) + [L]))


@pytest.mark.parametrize("L,scenes", PLANS, ids=str)
@pytest.mark.parametrize("args", ARGS, ids=str)
def test_window_plan_with_scenes_is_the_per_scene_plans_shifted(L, scenes, args):
    got = video.plan_windows(L, *args, scenes=scenes)
    if not scenes:
        assert got == video.plan_windows(L, *args)                                  # today's list, whatever it holds
        return
    want, dropped = [], 0
    for s, e in _scene_bounds(L, scenes):
        for nb, rf in video.plan_windows(e - s, *args):
            # test.py:47-48 with num_ref != -1 can name frame `length` itself, one past the end: not a frame of the scene
            dropped += sum(j >= e - s for j in rf)
            want.append(([j + s for j in nb], [j + s for j in rf if j < e - s]))
    assert got == want
    assert dropped == 0 or args[2] != -1
    # no window's ids cross a cut, every frame is some window's neighbour
    for nb, rf in got:
        home = [(s, e) for s, e in _scene_bounds(L, scenes) if s <= nb[0] < e]
        assert len(home) == 1 and all(home[0][0] <= j < home[0][1] for j in nb + rf)
    assert sorted(set(j for nb, _ in got for j in nb)) == list(range(L))


def test_window_plan_without_scenes_is_unchanged():
    for L, stride, ref_length, num_ref in ((23, 5, 10, -1), (12, 5, 10, 2), (7, 3, 10, -1), (41, 5, 7, 4)):
        today = video.plan_windows(L, stride, ref_length, num_ref)
        assert video.plan_windows(L, stride, ref_length, num_ref, scenes=None) == today
        assert video.plan_windows(L, stride, ref_length, num_ref, scenes=[]) == today
        assert video.plan_windows(L, stride, ref_length, num_ref, None) == today
    # a cut does change the plan: the first window of the one-shot plan crosses frame 9
    assert video.plan_windows(23, scenes=[9]) != video.plan_windows(23)


@pytest.mark.parametrize("bad", [[9, 5], [5, 5], [0], [23], [0, 9], [9, 23], [-1], [9.5], ["9"], [None], 9, [[9]], [True]], ids=str)
def test_window_plan_refuses_a_bad_scene_list(bad):
    with pytest.raises(ValueError):
        video.plan_windows(23, scenes=bad)


def test_scene_list_accepts_integers_of_any_kind():
    want = video.plan_windows(23, scenes=[9, 15])
    assert video.plan_windows(23, scenes=(9, 15)) == want
    assert video.plan_windows(23, scenes=np.array([9, 15])) == want
    assert video.plan_windows(23, scenes=[np.int64(9), 15]) == want


@pytest.mark.parametrize("L,scenes", PLANS[:3] + [(60, [17, 40])], ids=str)
@pytest.mark.parametrize("args", ARGS[:2], ids=str)
def test_reuse_plan_on_a_scene_plan(L, scenes, args):
    plan = video.plan_reuse(video.plan_windows(L, *args, scenes=scenes))
    encoded = [j for p in plan.windows for j in p["encode"]]
    assert sorted(encoded) == list(range(L))                                        # every frame once
    pairs = [pr for p in plan.windows for pr in p["pairs"]]
    assert len(pairs) == len(set(pairs)) and all(b == a + 1 for a, b in pairs)
    assert not any(a < c <= b for a, b in pairs for c in scenes)                    # none straddles a cut
    assert sorted(pairs) == [(j, j + 1) for j in range(L - 1) if j + 1 not in scenes]
    k = 0
    for s, e in _scene_bounds(L, scenes):
        alone = video.plan_reuse(video.plan_windows(e - s, *args)).windows
        for a in alone:
            p = plan.windows[k]
            assert p["encode"] == [j + s for j in a["encode"] if j < e - s] and p["pairs"] == [(x + s, y + s) for x, y in a["pairs"]]
            k += 1
    assert k == len(plan.windows)


def test_cuts_from_scores():
    z = lambda n, hot: np.array([0.9 if i in hot else 0.05 for i in range(n)])
    assert video.cuts_from_scores(z(19, {9})) == [10]                               # L = 20
    assert video.cuts_from_scores(z(19, ())) == []
    assert video.cuts_from_scores(np.zeros(0)) == [] and video.cuts_from_scores([]) == []
    # a one-frame flash at frame 10 raises pairs 9 and 10: the second half is dropped
    assert video.cuts_from_scores(z(19, {9, 10})) == [10]
    # ... and both when the flash is among the first min_scene frames; a later cut is still found
    assert video.cuts_from_scores(z(19, {2, 3})) == []
    assert video.cuts_from_scores(z(19, {2, 3, 11})) == [12]
    # ends closer than min_scene: L = 20, the last scene would have 4 frames; 5 is enough
    assert video.cuts_from_scores(z(19, {15})) == [] and video.cuts_from_scores(z(19, {14})) == [15]
    assert video.cuts_from_scores(z(19, {3})) == [] and video.cuts_from_scores(z(19, {4})) == [5]
    # the distance counts from the previous ACCEPTED cut: 5, (8 dropped), 10
    assert video.cuts_from_scores(z(19, {4, 7, 9})) == [5, 10]
    assert video.cuts_from_scores(z(19, {4, 7, 9}), min_scene=3) == [5, 8]          # 10 is 2 after 8
    assert video.cuts_from_scores(z(19, {4, 7, 9}), min_scene=1) == [5, 8, 10]
    assert video.cuts_from_scores(z(3, {0, 1, 2}), min_scene=1) == [1, 2, 3]
    # the threshold is inclusive
    assert video.cuts_from_scores([0.1, 0.35, 0.1] * 4, 0.35, 1) == [2, 5, 8, 11]
    assert video.cuts_from_scores([0.1, 0.35, 0.1] * 4, 0.36, 1) == []
    assert video.cuts_from_scores([1.0] * 11, 1) == [5]                             # threshold 1 is allowed; L = 12: 5, (10: 2 left)
    out = video.cuts_from_scores(z(19, {9}))
    assert all(type(c) is int for c in out)
    for bad in (0, -0.1, 1.01, 2):
        with pytest.raises(ValueError):
            video.cuts_from_scores(z(19, {9}), threshold=bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            video.cuts_from_scores(z(19, {9}), min_scene=bad)
    # what it returns is a list plan_windows accepts
    assert video.plan_windows(20, scenes=video.cuts_from_scores(z(19, {9}))) == video.plan_windows(20, scenes=[10])


def test_restatement_on_hand_counted_frames():
    # the luma extremes
    assert S.bins_np(np.array([255, 255, 255], np.uint8)) == 63 and S.bins_np(np.array([0, 0, 0], np.uint8)) == 0
    assert S.bins_np(np.array([255, 0, 0], np.uint8)) == ((77 * 255 + 128) >> 8) >> 2 == 19
    # a 2 x 2 frame: (4 y) // 2 and (4 x) // 2 are 0 and 2, so the pixels sit in cells 0, 2, 8 and 10, the others stay empty
    assert S.cells_np(2, 2).tolist() == [[0, 2], [8, 10]]
    a = np.zeros((2, 2, 2, 3), np.uint8)
    a[1, 0, 0] = 255                                                                # one pixel of four moves from bin 0 to bin 63
    h = S.hist_np(a)
    assert h.sum() == 8 and h[0, [0, 2, 8, 10], 0].tolist() == [1, 1, 1, 1] and h[1, 0, 63] == 1 and h[1, 0, 0] == 0
    assert S.scene_diff_np(a).tolist() == [2] and S.scores_np(a).tolist() == [0.25]
    a[1] = 255
    assert S.scene_diff_np(a).tolist() == [8] and S.scores_np(a).tolist() == [1.0]  # the largest value, 2 H W
    # H < 4: 3 rows sit in cell rows 0, 1, 2 ((4 y) // 3); 5 columns in cell columns 0, 0, 1, 2, 3
    assert S.cells_np(3, 5).tolist() == [[0, 0, 1, 2, 3], [4, 4, 5, 6, 7], [8, 8, 9, 10, 11]]
    b = np.zeros((2, 3, 5, 3), np.uint8)
    b[1, 0, :2] = (0, 255, 0)                                                       # both pixels of cell 0: bin ((150 * 255 + 128) >> 8) >> 2 = 37
    assert S.bins_np(b[1, 0, 0]) == 37
    assert S.scene_diff_np(b).tolist() == [4]
    # 1 x 1: one pixel in cell 0
    c = np.array([[[[10, 20, 30]]], [[[10, 20, 30]]], [[[200, 20, 30]]]], np.uint8)
    assert S.scene_diff_np(c).tolist() == [0, 2]
    # permuted pixels inside one cell: the same counters, score 0; the same permutation across cells: not 0
    rng = np.random.RandomState(1)
    f = rng.randint(0, 256, (8, 8, 3)).astype(np.uint8)
    inside = f.copy()
    inside[:2, :2] = f[:2, :2][::-1, ::-1]                                          # cell 0 is rows 0-1 x columns 0-1
    assert (inside != f).any() and S.scene_diff_np(np.stack([f, inside])).tolist() == [0]
    across = f.copy()
    across[:2, :4] = f[:2, :4][:, ::-1]                                             # cells 0 and 1 swap their pixels
    assert np.array_equal(np.sort(S.bins_np(across).ravel()), np.sort(S.bins_np(f).ravel()))
    assert S.scene_diff_np(np.stack([f, across]))[0] > 0


def test_restatement_on_the_tennis_fixture():
    f = S.tennis()
    s = S.scores_np(f)
    assert s.shape == (24,) and round(float(s.max()), 4) == 0.0944 and s.max() < video.SCENE_THRESHOLD == 0.35
    assert video.cuts_from_scores(s) == []
    j = S.scores_np(S.tennis_join())
    assert round(float(j[11]), 3) == 0.470 and np.delete(j, 11).max() <= 0.0944 + 5e-5
    assert video.cuts_from_scores(j) == [S.TENNIS_CUT] == [12]
    # the toy shots of the GPU tests: the random texture stays far below the threshold, the join with the gradient at twice the threshold and more
    toy, _ = S.toy_video(23, 50, 70)
    assert S.scores_np(toy).max() <= 0.111
    g = S.gradient_video(14, 50, 70)
    two = np.concatenate([toy[:9], g])
    t = S.scores_np(two)
    assert t[8] >= 2 * video.SCENE_THRESHOLD and np.delete(t, 8).max() < video.SCENE_THRESHOLD / 2 and video.cuts_from_scores(t) == [9]


def test_new_entries_refuse_bad_arguments():
    """host side of e2fgvi_scene_diff and e2fgvi_scene_diff_workspace: E2FGVI_EINVAL from the arguments alone (no launch, so this
    runs without a GPU; the addresses are never read)"""
    import os
    from e2fgvi_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    good = dict(frames=base, L=3, H=7, W=5, work=base + (1 << 16), out=base + (1 << 18))
    order = ("frames", "L", "H", "W", "work", "out")

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_scene_diff(*[a[k] for k in order], None)

    for k in ("frames", "work", "out"):
        assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
    for L in (1, 0, -2):
        assert rc(L=L) == -1 and b"two frames" in so.e2fgvi_last_error()
        assert so.e2fgvi_scene_diff_workspace(L, 7, 5) == -1
    for v in (0, -1):
        assert rc(H=v) == -1 and rc(W=v) == -1
        assert so.e2fgvi_scene_diff_workspace(3, v, 5) == -1 and so.e2fgvi_scene_diff_workspace(3, 7, v) == -1
    # H * W >= 2^31, and the check itself does not overflow: 46341^2 = 2^31 + 4633, (2^31 - 1)^2 wraps to 1 in 32 bits
    assert 46341 * 46341 >= 1 << 31 > 46340 * 46340
    assert rc(H=46341, W=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
    assert rc(H=0x7fffffff, W=0x7fffffff) == -1 and rc(H=65536, W=32768) == -1
    assert so.e2fgvi_scene_diff_workspace(3, 46341, 46341) == -1 and so.e2fgvi_scene_diff_workspace(3, 0x7fffffff, 0x7fffffff) == -1
    assert rc(work=good["work"] + 2) == -1 and rc(out=good["out"] + 4) == -1 and b"aligned" in so.e2fgvi_last_error()
    # a table of 16 x 64 32-bit counters per frame
    assert so.e2fgvi_scene_diff_workspace(3, 7, 5) == 3 * 1024 * 4
    assert so.e2fgvi_scene_diff_workspace(2, 46340, 46340) == 2 * 1024 * 4
    assert so.e2fgvi_scene_diff_workspace(0x7fffffff, 1, 1) == 0x7fffffff * 4096
    assert so.e2fgvi_abi_version() == 9 == lib.ABI_VERSION
    assert "e2fgvi_scene_diff" in lib.SYMBOLS and "e2fgvi_scene_diff_workspace" in lib.SYMBOLS


def test_inpaint_video_refuses_bad_scenes_before_any_device_work():
    """the scenes= checks come from the shapes alone: they raise on a host without a GPU, in front of the CPU-device refusal"""
    f, m = np.zeros((12, 8, 8, 3), np.uint8), np.zeros((12, 8, 8), np.uint8)

    def model(x, n):
        raise AssertionError("no forward")

    for bad in ("other", "Auto", "", [5, 5], [7, 3], [0], [12], [3.5], 5):
        with pytest.raises(ValueError, match="scenes"):
            video.inpaint_video(model, f, m, device=torch.device("cpu"), scenes=bad)
    with pytest.raises(ValueError, match="scenes"):
        video.track_regions(m, (8, 8), (108, 60), scenes=[12])
    with pytest.raises(ValueError):
        video.detect_cuts(f, threshold=0)
    with pytest.raises(ValueError):
        video.detect_cuts(f, min_scene=0)
    # a good list passes the check and reaches the device test
    with pytest.raises(RuntimeError, match="cuda"):
        video.inpaint_video(model, f, m, device=torch.device("cpu"), scenes=[5])
    with pytest.raises(RuntimeError, match="cuda"):
        video.inpaint_video(model, f, m, device=torch.device("cpu"), scenes="auto")
    # fewer than two frames: no pair, no launch
    assert video.scene_scores(f[:1]).shape == (0,) and video.scene_scores(f[:0]).shape == (0,) and video.detect_cuts(f[:1]) == []
    with pytest.raises(ValueError):
        video.scene_scores(f[..., :2])
