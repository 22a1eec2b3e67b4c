"""inpaint_video(region="holes"), host side: the restatement of the component labelling (tests/hole_label_cases.py) against
scipy.ndimage.label, video.plan_holes on hand-computed regions, and the argument checks of the C entries and of inpaint_video that
need no device.  The kernels and the driver are compared with these in tests/test_gpu_video_holes.py."""
import itertools

import numpy as np
import pytest
import torch

from e2fgvi_amd import ops, video
from tests import hole_label_cases as C

TW, TH = ops.LABEL_TILE_W, ops.LABEL_TILE_H
SIZES = [(1, 1), (1, 200), (130, 1), (5, 7), (33, 130), (2 * TH + 3, 2 * TW + 5)]
FRAME, SIZE = (250, 131), (108, 60)
A, B, C3 = (8, 10, 40, 30), (200, 95, 240, 120), (60, 12, 75, 25)


@pytest.mark.parametrize("Hm,Wm", SIZES, ids=str)
def test_restatement_is_scipy_label(Hm, Wm):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, U in C.footprints(Hm, Wm, TH, TW).items():
        labels, boxes = C.components_np(U)
        ref, K = ndimage.label(U, np.ones((3, 3)))
        assert labels.dtype == np.int32 and boxes.dtype == np.int32 and boxes.shape == (K, 5), name
        assert np.array_equal(labels, ref), name
        for k, sl in enumerate(ndimage.find_objects(ref), 1):
            assert boxes[k - 1].tolist() == [sl[1].start, sl[0].start, sl[1].stop, sl[0].stop, int((ref == k).sum())], (name, k)
        v = C.video_of(U, name, seed=Hm + Wm)
        assert v.dtype == np.uint8 and v.shape == (3, Hm, Wm) and np.array_equal(C.footprint_np(v), U), name
        assert set(np.unique(v).tolist()) <= {0, 1, 255}


def test_restatement_on_hand_counted_masks():
    U = np.array([[0, 1, 0, 0, 0, 1, 1, 0],
                  [0, 0, 1, 0, 0, 0, 0, 0],
                  [1, 0, 0, 0, 0, 0, 1, 0],
                  [1, 0, 0, 0, 0, 1, 0, 0],
                  [0, 1, 0, 1, 1, 0, 0, 0],
                  [0, 0, 0, 0, 0, 0, 0, 1]], bool)
    labels, boxes = C.components_np(U)
    assert labels.tolist() == [[0, 1, 0, 0, 0, 2, 2, 0],
                               [0, 0, 1, 0, 0, 0, 0, 0],
                               [3, 0, 0, 0, 0, 0, 4, 0],
                               [3, 0, 0, 0, 0, 4, 0, 0],
                               [0, 3, 0, 4, 4, 0, 0, 0],
                               [0, 0, 0, 0, 0, 0, 0, 5]]
    assert boxes.tolist() == [[1, 0, 3, 2, 2], [5, 0, 7, 1, 2], [0, 2, 2, 5, 3], [3, 2, 7, 5, 4], [7, 5, 8, 6, 1]]
    big = (2 * TH + 3, 2 * TW + 5)
    f = C.footprints(*big, TH, TW)
    count = lambda name: len(C.components_np(f[name])[1])
    assert count("checkerboard") == 1 and count("spiral") == 1 and count("comb_bottom") == 1 and count("comb_top") == 1
    assert count("two_combs") == 2 and count("corners") == 4 and count("empty") == 0 and count("full") == 1
    assert count("isolated") == ((big[0] + 1) // 2) * ((big[1] + 1) // 2) > 1024          # the numbering crosses scan blocks
    assert f["spiral"].sum() > big[0] * big[1] // 3
    for name, (U, k) in C.corner_cases(*big, TH, TW).items():
        assert len(C.components_np(U)[1]) == k, name
    assert len(C.corner_cases(*big, TH, TW)) == 3 and not C.corner_cases(5, 7, TH, TW)


def _overlap(r, s):
    return r[0] < s[2] and s[0] < r[2] and r[1] < s[3] and s[1] < r[3]


def test_plan_holes_on_hand_computed_regions():
    assert video.plan_holes([A, B], FRAME, SIZE) == [((0, 0, 108, 60), [1]), ((142, 71, 250, 131), [2])]
    # the third component's own region overlaps the first one's: those two share a pass, the second is left alone
    assert video.plan_region(C3, FRAME, SIZE) == (13, 0, 121, 60)
    assert video.plan_holes([A, B, C3], FRAME, SIZE) == [((0, 0, 134, 75), [1, 3]), ((142, 71, 250, 131), [2])]
    assert video.plan_region((8, 10, 75, 30), FRAME, SIZE) == (0, 0, 134, 75)
    for boxes in ([A, B], [A, B, C3]):
        union = (min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), max(b[3] for b in boxes))
        assert video.plan_holes(boxes, FRAME, SIZE, max_regions=1) == [(video.plan_region(union, FRAME, SIZE), list(range(1, len(boxes) + 1)))]
    assert video.plan_holes([], FRAME, SIZE) == []
    assert video.plan_holes([A], FRAME, SIZE) == [(video.plan_region(A, FRAME, SIZE), [1])]
    assert video.plan_holes([A, B], FRAME, SIZE, context=2) == [(video.plan_region((8, 10, 240, 120), FRAME, SIZE, 2), [1, 2])]
    out = video.plan_holes([list(A), np.array(B)], FRAME, SIZE, max_regions=np.int64(4))
    assert out == video.plan_holes([A, B], FRAME, SIZE) and all(type(v) is int for r, _ in out for v in r)


def test_plan_holes_merges_a_chain_in_one_round():
    """three small holes 80 pixels apart in a wide frame: the regions of P and Q overlap, those of Q and R do, those of P and R do
    not -- one group; a fourth far away keeps its own"""
    frame = (2000, 200)
    P, Q, R, S = (100, 90, 110, 100), (180, 90, 190, 100), (260, 90, 270, 100), (1500, 90, 1510, 100)
    rp, rq, rr = (video.plan_region(b, frame, SIZE) for b in (P, Q, R))
    assert _overlap(rp, rq) and _overlap(rq, rr) and not _overlap(rp, rr)
    got = video.plan_holes([P, Q, R, S], frame, SIZE)
    assert got == [(video.plan_region((100, 90, 270, 100), frame, SIZE), [1, 2, 3]), (video.plan_region(S, frame, SIZE), [4])]
    # numbered otherwise, the groups come in the order of their lowest component
    got = video.plan_holes([S, R, Q, P], frame, SIZE)
    assert [g for _, g in got] == [[1], [2, 3, 4]]


def test_plan_holes_cap_picks_the_smallest_union():
    frame = (4000, 3000)
    sq = lambda x, y: (x, y, x + 10, y + 10)
    # four holes no two of whose regions overlap; unions: (1,2) 610 x 10, (3,4) 10 x 610, every other pair far larger
    boxes = [sq(100, 100), sq(700, 100), sq(3000, 2000), sq(3000, 2600)]
    assert len(video.plan_holes(boxes, frame, SIZE, max_regions=4)) == 4
    got = video.plan_holes(boxes, frame, SIZE, max_regions=3)
    assert [g for _, g in got] == [[1, 2], [3], [4]]                                   # the tie 6100 = 6100: the lowest g
    assert got[0][0] == video.plan_region((100, 100, 710, 110), frame, SIZE)
    got = video.plan_holes(boxes, frame, SIZE, max_regions=2)
    assert [g for _, g in got] == [[1, 2], [3, 4]]
    # ... then the lowest h: 1 is as near to 2 as to 3
    boxes = [sq(1000, 1000), sq(1600, 1000), sq(1000, 1600), sq(3500, 2800)]
    assert [g for _, g in video.plan_holes(boxes, frame, SIZE, max_regions=3)] == [[1, 2], [3], [4]]
    # a smaller union elsewhere wins over a lower number
    boxes = [sq(100, 100), sq(900, 100), sq(3000, 2000), sq(3000, 2500)]
    assert [g for _, g in video.plan_holes(boxes, frame, SIZE, max_regions=3)] == [[1], [2], [3, 4]]
    assert len(video.plan_holes(boxes, frame, SIZE, max_regions=1)) == 1


def test_plan_holes_plans_one_group_beyond_the_component_limit():
    assert video.HOLE_COMPONENTS_MAX == 1024
    frame = (40000, 40000)
    boxes = [(1000 * (k % 33), 1000 * (k // 33), 1000 * (k % 33) + 5, 1000 * (k // 33) + 5) for k in range(1025)]
    got = video.plan_holes(boxes, frame, SIZE, max_regions=1000)
    assert got == [(video.plan_region((0, 0, 32005, 31005), frame, SIZE), list(range(1, 1026)))]
    assert len(video.plan_holes(boxes[:1024], frame, SIZE, max_regions=2000)) == 1024


def test_plan_holes_refuses_bad_arguments():
    for bad in (0, -1, True, False, 1.5, "2", None, [2]):
        with pytest.raises(ValueError, match="max_regions"):
            video.plan_holes([A, B], FRAME, SIZE, max_regions=bad)
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="context"):
            video.plan_holes([A, B], FRAME, SIZE, context=bad)
    with pytest.raises(ValueError):
        video.plan_holes([A, (200, 95, 251, 120)], FRAME, SIZE)                          # a box outside the frame
    with pytest.raises(ValueError):
        video.plan_holes([A, (40, 10, 40, 30)], FRAME, SIZE)                             # an empty one
    with pytest.raises(ValueError):
        video.plan_holes([A], FRAME, (16, 60))                                          # no room for the guard
    with pytest.raises(ValueError, match="context"):
        video.plan_holes([], FRAME, SIZE, context=-1)                                   # checked without a box too


def test_plan_holes_regions_are_disjoint_on_random_boxes():
    rng = np.random.RandomState(11)
    for trial in range(200):
        W, H = int(rng.randint(120, 900)), int(rng.randint(70, 600))
        K = int(rng.randint(1, 12))
        boxes = []
        for _ in range(K):
            x0, y0 = int(rng.randint(0, W - 1)), int(rng.randint(0, H - 1))
            boxes.append((x0, y0, int(rng.randint(x0 + 1, min(W, x0 + 40) + 1)), int(rng.randint(y0 + 1, min(H, y0 + 40) + 1))))
        cap = int(rng.randint(1, 6))
        got = video.plan_holes(boxes, (W, H), SIZE, context=float(rng.choice([0, 0.5, 1])), max_regions=cap)
        assert 1 <= len(got) <= cap
        assert sorted(k for _, g in got for k in g) == list(range(1, K + 1))
        assert [g[0] for _, g in got] == sorted(g[0] for _, g in got) and all(g == sorted(g) for _, g in got)
        for r, g in got:
            assert 0 <= r[0] < r[2] <= W and 0 <= r[1] < r[3] <= H
            for k in g:
                b = boxes[k - 1]
                assert r[0] <= b[0] and r[1] <= b[1] and b[2] <= r[2] and b[3] <= r[3], (trial, r, b)
        for (r, _), (s, _) in itertools.combinations(got, 2):
            assert not _overlap(r, s), (trial, r, s)


def test_new_entries_refuse_bad_arguments():
    """host side of e2fgvi_hole_label, e2fgvi_hole_label_workspace and e2fgvi_label_boxes: E2FGVI_EINVAL from the arguments alone
    (no launch, so this runs without a GPU; the addresses are never read)"""
    import os
    from e2fgvi_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    good = dict(masks=base, L=3, Hm=7, Wm=5, work=base + (1 << 16), labels=base + (1 << 18), count=base + (1 << 19))
    order = ("masks", "L", "Hm", "Wm", "work", "labels", "count")

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_hole_label(*[a[k] for k in order], None)

    for k in ("masks", "work", "labels", "count"):
        assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
    assert rc(L=-1) == -1 and b"frames" in so.e2fgvi_last_error()
    for v in (0, -1):
        assert rc(Hm=v) == -1 and rc(Wm=v) == -1
        assert so.e2fgvi_hole_label_workspace(v, 5) == -1 and so.e2fgvi_hole_label_workspace(7, v) == -1
        assert so.e2fgvi_label_boxes(base, v, 5, 2, base + 4096, None) == -1 and so.e2fgvi_label_boxes(base, 7, v, 2, base + 4096, None) == -1
    # Hm * Wm >= 2^31, and the check itself does not overflow: 46341^2 = 2^31 + 4633, (2^31 - 1)^2 wraps to 1 in 32 bits
    assert rc(Hm=46341, Wm=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
    assert rc(Hm=0x7fffffff, Wm=0x7fffffff) == -1 and rc(Hm=65536, Wm=32768) == -1
    assert so.e2fgvi_hole_label_workspace(46341, 46341) == -1 and so.e2fgvi_hole_label_workspace(0x7fffffff, 0x7fffffff) == -1
    assert so.e2fgvi_hole_label_workspace(65536, 32768) == -1 and b"2^31" in so.e2fgvi_last_error()
    assert so.e2fgvi_label_boxes(base, 46341, 46341, 2, base + 4096, None) == -1
    for shift in (2, 4, 8):
        assert rc(work=good["work"] + shift) == -1 and b"aligned" in so.e2fgvi_last_error()
    assert rc(labels=good["labels"] + 2) == -1 and rc(count=good["count"] + 1) == -1 and b"aligned" in so.e2fgvi_last_error()
    assert so.e2fgvi_label_boxes(None, 7, 5, 2, base, None) == -1 and so.e2fgvi_label_boxes(base, 7, 5, 2, None, None) == -1
    assert so.e2fgvi_label_boxes(base, 7, 5, -1, base + 4096, None) == -1
    assert so.e2fgvi_label_boxes(base + 2, 7, 5, 2, base + 4096, None) == -1 and so.e2fgvi_label_boxes(base, 7, 5, 2, base + 4098, None) == -1
    assert so.e2fgvi_label_boxes(None, 7, 5, 0, None, None) == 0                         # no component: nothing to do
    # per pixel an int32 rank and a footprint byte, a counter per 1024 pixels; every part a multiple of 16 bytes
    assert so.e2fgvi_hole_label_workspace(7, 5) == 144 + 48 + 16
    assert so.e2fgvi_hole_label_workspace(1080, 1920) == 4 * 1080 * 1920 + 1080 * 1920 + 4 * 2025 + 12
    assert so.e2fgvi_hole_label_workspace(46340, 46340) > 5 * 46340 * 46340
    assert so.e2fgvi_abi_version() == 9 == lib.ABI_VERSION
    assert all(n in lib.SYMBOLS for n in ("e2fgvi_hole_label_workspace", "e2fgvi_hole_label", "e2fgvi_label_boxes"))


def test_inpaint_video_refuses_bad_holes_arguments_before_any_device_work():
    f, m = np.zeros((12, 8, 8, 3), np.uint8), np.zeros((12, 8, 8), np.uint8)

    def model(x, n):
        raise AssertionError("no forward")

    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="size"):
        video.inpaint_video(model, f, m, device=cpu, region="holes", restore=True)
    with pytest.raises(ValueError, match="restore"):
        video.inpaint_video(model, f, m, device=cpu, region="holes", size=(108, 60))
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError, match="max_regions"):
            video.inpaint_video(model, f, m, device=cpu, region="holes", size=(108, 60), restore=True, max_regions=bad)
    with pytest.raises(ValueError, match="region"):
        video.inpaint_video(model, f, m, device=cpu, region="hole s", size=(108, 60), restore=True)
    # good arguments reach the device test
    with pytest.raises(RuntimeError, match="cuda"):
        video.inpaint_video(model, f, m, device=cpu, region="holes", size=(108, 60), restore=True, max_regions=2)
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError, match="max_regions"):
            video.hole_regions(m, (8, 8), (108, 60), max_regions=bad)
    with pytest.raises(ValueError, match="context"):
        video.hole_regions(m, (8, 8), (108, 60), context=-1)
