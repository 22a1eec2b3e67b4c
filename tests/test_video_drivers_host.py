"""The host side of video.inpaint_video's drivers, piece by piece and without a device: the checked options record
(_check_call), the per-window tables (_window_tables) and the window drivers that need nothing but their callbacks (sequential,
batched).  What the pieces compute together on the device is pinned by the tests/test_gpu_video_*.py files."""
import inspect

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, video

SHAPE = (12, 60, 108, 3)
MASKS = np.zeros((12, 60, 108), np.uint8)
DEFAULTS = {k: p.default for k, p in inspect.signature(video.inpaint_video).parameters.items()
            if p.default is not inspect.Parameter.empty and k != "device"}


class _Gen:
    """what the checks take for the generator: an object with engine()"""
    def engine(self):
        raise AssertionError("the engine was asked for")


def _call(shape=SHAPE, masks=MASKS, model=None, **kw):
    return video._check_call(shape, masks, model, **dict(DEFAULTS, **kw))


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_propagate_masks_device", touched)


# ------------------------------------------------------------------------------------------------ _check_call
def test_check_call_returns_the_normalised_record(no_device):
    c = _call()
    assert isinstance(c, video._Call) and c._fields == video._Call._fields
    assert c == video._Call(fmt=None, overlay=False, scenes=None, mask_keys=None, feather=0, region=None, box=None, max_regions=4,
                            size=None, restore=False, keep_float=False, reuse=False, batch_windows=1, in_flight=1, neighbor_stride=5,
                            ref_length=10, num_ref=-1, dilate=True, pad=True, context=0.5)
    with pytest.raises(AttributeError):
        c.feather = 3
    # an explicit box: checked integers, and the region says which kind it is
    c = _call(size=(54, 30), region=[np.int64(4), 2.0, 100, 50])
    assert (c.region, c.box) == ("box", (4, 2, 100, 50)) and all(type(v) is int for v in c.box) and c.size == (54, 30)
    for name in ("hole", "holes", "track"):
        c = _call(size=(54, 30), restore=True, region=name, max_regions=np.int64(2), feather=2.0)
        assert (c.region, c.box, c.restore) == (name, None, True)
        assert c.feather == 2 and type(c.feather) is int
        if name == "holes":
            assert c.max_regions == 2 and type(c.max_regions) is int
    assert _call(scenes=[np.int64(3)]).scenes == [3] and type(_call(scenes=(3, 7.0)).scenes[1]) is int
    assert _call(scenes="auto").scenes == "auto" and _call(scenes=[]).scenes == []
    # a layout string is that layout with yuv_format's defaults; the shape the other checks see is the decoded one
    c = _call(shape=(12, 90, 108), pixel_format="i420", size=(54, 30), region=(0, 0, 108, 60))
    assert c.fmt == video.yuv_format("i420") and isinstance(c.fmt, video.YuvFormat) and c.box == (0, 0, 108, 60)
    fmt = video.yuv_format("nv12", "bt601", True, "nearest")
    assert _call(shape=(12, 90, 108), pixel_format=fmt).fmt == fmt
    c = _call(masks="overlay", in_flight=2, keep_float=True, dilate=False, pad=False, context=0.25, num_ref=2, neighbor_stride=3,
              ref_length=4)
    assert c.overlay and (c.in_flight, c.keep_float, c.dilate, c.pad, c.context, c.num_ref, c.neighbor_stride, c.ref_length) == \
        (2, True, False, False, 0.25, 2, 3, 4)
    c = _call(masks=MASKS[:2], model=_Gen(), mask_keys=(np.int32(2), 9), scenes="auto", reuse=True)
    assert c.mask_keys == [2, 9] and all(type(v) is int for v in c.mask_keys) and c.scenes == "auto" and c.reuse
    assert _call(batch_windows=3).batch_windows == 3


RULES = [   # (what the raised message names, the exception, the call that breaks this rule alone)
    ("nv12", ValueError, dict(pixel_format="yv12")),
    ("keep_float", ValueError, dict(shape=(12, 90, 108), pixel_format="nv12", keep_float=True)),
    ("divisible by 3", ValueError, dict(shape=(12, 91, 108), pixel_format="nv12")),
    ("even", ValueError, dict(shape=(12, 90, 108), pixel_format="nv12", size=(53, 30))),
    ("overlay", ValueError, dict(masks="logo")),
    ('"auto"', ValueError, dict(scenes="cuts")),
    ("scenes", ValueError, dict(scenes=[12])),
    ("scenes", ValueError, dict(scenes=[5, 3])),
    ("overlay", ValueError, dict(masks="overlay", model=_Gen(), mask_keys=[2, 9])),
    ("mask_keys", ValueError, dict(masks=MASKS[:2], model=_Gen(), mask_keys=[9, 2])),
    ("mask_keys", ValueError, dict(masks=MASKS[:3], model=_Gen(), mask_keys=[2, 9])),
    ("InpaintGenerator", TypeError, dict(masks=MASKS[:2], model=None, mask_keys=[2, 9])),
    ("feather", ValueError, dict(size=(54, 30), restore=True, feather=video.FEATHER_MAX + 1)),
    ("feather", ValueError, dict(size=(54, 30), restore=True, feather=1.5)),
    ("feather", ValueError, dict(size=(54, 30), restore=True, feather=True)),
    ("no seam", ValueError, dict(size=(54, 30), feather=3)),
    ("without size", ValueError, dict(region="hole")),
    ("region must be", ValueError, dict(size=(54, 30), region="box")),
    ("box", ValueError, dict(size=(54, 30), region=(0, 0, 109, 60))),
    ("box", ValueError, dict(size=(54, 30), region=(0, 0, 10))),
    ("restore must be True", ValueError, dict(size=(54, 30), region="track")),
    ("reuse must be False", ValueError, dict(size=(54, 30), restore=True, region="track", reuse=True, model=_Gen())),
    ("batch_windows must be", ValueError, dict(size=(54, 30), restore=True, region="track", batch_windows=2)),
    ("in_flight must be", ValueError, dict(size=(54, 30), restore=True, region="track", in_flight=2)),
    ("max_regions", ValueError, dict(size=(54, 30), restore=True, region="holes", max_regions=0)),
    ("max_regions", ValueError, dict(size=(54, 30), restore=True, region="holes", max_regions=True)),
    ("restore must be True", ValueError, dict(size=(54, 30), region="holes")),
    ("nothing to restore", ValueError, dict(restore=True)),
    ("keep_float must be False", ValueError, dict(size=(54, 30), restore=True, keep_float=True)),
    ("batch_windows must be 1", ValueError, dict(reuse=True, model=_Gen(), batch_windows=2)),
    ("in_flight must be 1", ValueError, dict(reuse=True, model=_Gen(), in_flight=2)),
    ("InpaintGenerator", TypeError, dict(reuse=True, model=lambda x, n: (x, None))),
]


@pytest.mark.parametrize("k", range(len(RULES)))
def test_check_call_refuses_every_broken_rule(no_device, k):
    what, exc, kw = RULES[k]
    with pytest.raises(exc, match=what):
        _call(**kw)
    # and inpaint_video raises the same from the same call, before the device is looked at
    kw = dict(kw)
    frames = np.zeros(kw.pop("shape", SHAPE), np.uint8)
    with pytest.raises(exc, match=what):
        video.inpaint_video(kw.pop("model", None), frames, kw.pop("masks", MASKS), device="cpu", **kw)


def test_check_call_raises_the_first_of_two_broken_rules(no_device):
    """the order of the checks is part of the interface: a call that breaks two rules keeps raising the one it raised before"""
    with pytest.raises(ValueError, match="feather= ramps the paste-back .* there is no seam"):
        _call(feather=3, region="hole")                                     # not "region= ... without size"
    with pytest.raises(ValueError, match='region="track" gives every window a box of its own.* restore must be True'):
        _call(size=(54, 30), region="track", reuse=True, model=_Gen())      # not "reuse must be False"
    for kw, what in ((dict(feather=3, region="hole"), "no seam to feather"),
                     (dict(size=(54, 30), region="track", reuse=True), "restore must be True")):
        with pytest.raises(ValueError, match=what):
            video.inpaint_video(_Gen(), np.zeros(SHAPE, np.uint8), MASKS, device="cpu", **kw)


def test_a_good_call_reaches_the_device_only_after_the_checks(no_device):
    for kw in (dict(), dict(size=(54, 30), restore=True, region="track"), dict(scenes="auto", in_flight=2)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            video.inpaint_video(None, np.zeros(SHAPE, np.uint8), MASKS, device="cpu", **kw)


# ------------------------------------------------------------------------------------------------ _window_tables
PLANS = [(23, dict()), (12, dict(num_ref=2)), (11, dict(scenes=[4]))]


def _tables_restated(windows, length, run):
    """test.py:172-176's ``comp_frames[idx] is None`` over the windows that run"""
    seen, out = [None] * length, {}
    for k in run:
        nb, rf = windows[k]
        out[k] = (nb + rf, [1 if seen[j] is None else 0 for j in nb])
        for j in nb:
            seen[j] = k
    return out


@pytest.mark.parametrize("length,kw", PLANS)
def test_window_tables_are_the_seen_loop(length, kw):
    windows = video.plan_windows(length, **kw)
    ids, first = video._window_tables(windows, length, "cpu")
    want = _tables_restated(windows, length, range(len(windows)))
    assert len(ids) == len(first) == len(windows)
    for k in range(len(windows)):
        assert ids[k].dtype == torch.int32 and first[k].dtype == torch.uint8
        assert (ids[k].tolist(), first[k].tolist()) == want[k]
    flat = [f for k, (nb, _) in enumerate(windows) for f in first[k].tolist()]
    assert sum(flat) == length                           # every frame is some window's first exactly once


@pytest.mark.parametrize("length,kw", PLANS)
def test_window_tables_with_skipped_windows_never_saw_them(length, kw):
    windows = video.plan_windows(length, **kw)
    assert len(windows) >= 3
    for run in ([k for k in range(len(windows)) if k != 1], list(range(1, len(windows))), [len(windows) - 1], []):
        ids, first = video._window_tables(windows, length, "cpu", run)
        want = _tables_restated(windows, length, run)
        for k in range(len(windows)):
            if k in run:
                assert (ids[k].tolist(), first[k].tolist()) == want[k]
            else:
                assert ids[k] is None and first[k] is None
    # window 1 skipped: the frames only it and window 2 hold are window 2's first ones, which they are not when window 1 runs
    full = video._window_tables(windows, length, "cpu")[1]
    skip = video._window_tables(windows, length, "cpu", [0] + list(range(2, len(windows))))[1]
    assert skip[2].sum() > full[2].sum()


# ------------------------------------------------------------------------------------------------ the drivers
class _Pred:
    """a stand-in for a window's predictions: knows its window and whether it is the batch's output or a copy"""
    def __init__(self, window, copy=False):
        self.window, self.copy = window, copy

    def clone(self):
        return _Pred(self.window, True)


class _Recorder:
    def __init__(self):
        self.log, self.groups = [], []

    def predict(self, group):
        self.log.append(("predict", list(group)))
        self.groups.append(list(group))
        return [_Pred(i) for i in group]

    def composite(self, i, pred):
        assert pred.window == i
        self.log.append(("composite", i, pred.copy))


@pytest.mark.parametrize("batch_windows", [2, 3])
@pytest.mark.parametrize("plan", [(23,), (7, 3)])
def test_batched_driver_groups_by_shape_and_composites_in_window_order(plan, batch_windows):
    windows = video.plan_windows(*plan)
    rec = _Recorder()
    video._run_batched(windows, rec.predict, rec.composite, batch_windows)
    shape = lambda i: (len(windows[i][0]), len(windows[i][1]))
    assert sorted(i for g in rec.groups for i in g) == list(range(len(windows)))        # every window in exactly one forward
    for g in rec.groups:
        assert 1 <= len(g) <= batch_windows and len({shape(i) for i in g}) == 1 and g == sorted(g)
    counts = [[shape(i) for i in range(len(windows))].count(s) for s in {shape(i) for i in range(len(windows))}]
    assert len(rec.groups) == sum(-(-c // batch_windows) for c in counts)               # no more forwards than the shapes need
    done = [e[1] for e in rec.log if e[0] == "composite"]
    assert done == list(range(len(windows)))
    # a window is composited as soon as its forward and every earlier window's are done: straight from the batch's output when no
    # earlier window is still to come, else from a copy of its local frames (the batch's output is released)
    predicted = set()
    for n, e in enumerate(rec.log):
        if e[0] == "predict":
            predicted |= set(e[1])
            for i in e[1]:
                waits = any(j not in predicted for j in range(i))
                copies = [c[2] for c in rec.log if c[0] == "composite" and c[1] == i]
                assert copies == [waits], (e[1], i)
                if not waits:                           # composited before the next forward is issued
                    nxt = [m for m in range(n + 1, len(rec.log)) if rec.log[m][0] == "predict"]
                    assert rec.log.index(("composite", i, False)) < (nxt[0] if nxt else len(rec.log))


@pytest.mark.parametrize("n", [0, 1, 5])
def test_sequential_driver_interleaves_forward_and_compositing(n):
    rec = _Recorder()
    video._run_sequential(n, rec.predict, rec.composite)
    assert rec.log == [e for i in range(n) for e in (("predict", [i]), ("composite", i, False))]
