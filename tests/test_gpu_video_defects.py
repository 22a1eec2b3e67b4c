"""The dust-and-dirt detector on the device: ops.defect_candidates and ops.defect_clean (csrc/defects.hip) and video.detect_defects
against the numpy restatement of tests/defect_cases.py, every byte and every count equal, on every named case; ids without both
neighbours; reruns; size=, scenes= and the frame guard; the flows of the net's own SPyNet; and inpaint_video(masks_u8="defects")
against the two-step call, byte for byte."""
import importlib

import numpy as np
import pytest
import torch

from e2fgvi_amd import metrics, ops, video
from tests import defect_cases as D
from tests.test_gpu_video_restore import _stand_in_model
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

_CACHE = {}
DEFECT_SYMBOLS = ("e2fgvi_defect_candidates", "e2fgvi_defect_clean")


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.zeros(a.nbytes + shift, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _ids(ids, dev):
    return torch.tensor(ids, dtype=torch.int32).to(dev)


def _run(c, dev, ids, shift=0, fill=0):
    """(cand, masks, counts) of the two entries on a case, the byte buffers `shift` bytes off an allocation's start and pre-filled"""
    L, H, W = c["L"], c["H"], c["W"]
    fr, fwd, bwd = _up(c["frames"], dev, shift), _up(c["fwd"], dev), _up(c["bwd"], dev)
    cand = ops.defect_candidates(fr, fwd, bwd, _ids(ids, dev), c["threshold"], c["slack"],
                                 out=_up(np.full((L, H, W), fill, np.uint8), dev, shift))
    masks, counts = ops.defect_clean(cand, _ids(ids, dev), c["support"], c["radius"], out=_up(np.full((L, H, W), fill, np.uint8), dev, shift))
    return cand.cpu().numpy(), masks.cpu().numpy(), counts.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the two entries
@pytest.mark.parametrize("name", D.NAMES)
def test_entries_are_the_restatement(dev, name):
    c = D.case(name)
    ids = D.plan_np(c["L"], c["scenes"])
    want_cand, want_raw, _, _ = D.want(name)
    _, want_counts = D.clean_np(want_cand, ids, c["support"], c["radius"])
    for shift in (0, 1):
        cand, masks, counts = _run(c, dev, ids, shift)
        print(name, "shift", shift, "candidates", int(cand.sum()), "set", counts.tolist())
        assert cand.dtype == masks.dtype == np.uint8 and counts.dtype == np.int32 and counts.shape == (c["L"],)
        assert np.array_equal(cand, want_cand), int((cand != want_cand).sum())
        assert np.array_equal(masks, want_raw), int((masks != want_raw).sum())
        assert np.array_equal(counts, want_counts)
    # every byte of a listed frame is written, the zeros of a tile without a candidate included
    cand, masks, _ = _run(c, dev, ids, fill=77)
    assert all(np.array_equal(cand[t], want_cand[t]) and np.array_equal(masks[t], want_raw[t]) for t in ids)
    # without out= the buffers are zeros outside the listed frames; every listed frame in one launch or one launch each
    fr, fwd, bwd = _up(c["frames"], dev), _up(c["fwd"], dev), _up(c["bwd"], dev)
    cand = ops.defect_candidates(fr, fwd, bwd, _ids(ids, dev), c["threshold"], c["slack"])
    masks, counts = ops.defect_clean(cand, _ids(ids, dev), c["support"], c["radius"])
    assert np.array_equal(cand.cpu().numpy(), want_cand) and np.array_equal(masks.cpu().numpy(), want_raw)
    one = torch.zeros_like(cand)
    for t in ids:
        ops.defect_candidates(fr, fwd, bwd, _ids([t], dev), c["threshold"], c["slack"], out=one)
    assert torch.equal(one, cand)


def test_ids_without_both_neighbours_write_nothing(dev):
    c = D.case("cuts_L7")
    L = c["L"]
    want_cand, want_raw, _, _ = D.want("cuts_L7")
    cand, masks, counts = _run(c, dev, [0, L - 1, -5, L + 7, 2 ** 31 - 1, -2 ** 31], fill=77)
    assert (cand == 77).all() and (masks == 77).all() and not counts.any()
    # mixed with good ids: only those frames are written
    cand, masks, counts = _run(c, dev, [L - 1, 4, -1, 1, 0], fill=77)
    for t in range(L):
        if t in (1, 4):
            assert np.array_equal(cand[t], want_cand[t]) and np.array_equal(masks[t], want_raw[t]) and counts[t] == (want_raw[t] > 0).sum()
        else:
            assert (cand[t] == 77).all() and (masks[t] == 77).all() and counts[t] == 0
    # any non-zero byte of cand is a candidate
    ids = D.plan_np(L, c["scenes"])
    got, n = ops.defect_clean(_up(want_cand * 200, dev), _ids(ids, dev), c["support"], c["radius"])
    assert np.array_equal(got.cpu().numpy(), want_raw)


def test_runs_are_the_same_bits(dev):
    for name in ("wave_70x90", "nonfinite_33x64"):
        c = D.case(name)
        ids = D.plan_np(c["L"], c["scenes"])
        first = _run(c, dev, ids)
        for _ in range(5):
            again = _run(c, dev, ids)
            assert all(np.array_equal(a, b) for a, b in zip(first, again))


def test_arguments_are_checked(dev):
    c = D.case("half_9x13")
    fr, fwd, bwd, ids = _up(c["frames"], dev), _up(c["fwd"], dev), _up(c["bwd"], dev), _ids([1, 2], dev)
    # host inputs are uploaded
    got = ops.defect_candidates(np.array(c["frames"]), np.array(c["fwd"]), np.array(c["bwd"]), np.array([1, 2], np.int32), 4, 0)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), D.want("half_9x13")[0])
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(fwd=fwd.double()), "fwd"), (dict(bwd=bwd.half()), "bwd"),
                     (dict(ids=ids.long()), "ids"), (dict(frames=fr[..., :2]), "contiguous"), (dict(frames=fr[0]), "frames"),
                     (dict(fwd=fwd[1:]), "fwd"), (dict(bwd=bwd[:, :, :, :1].contiguous()), "bwd"), (dict(ids=ids[None]), "ids"),
                     (dict(fwd=fwd.transpose(1, 2)), "fwd"), (dict(threshold=255), "threshold"), (dict(threshold=True), "threshold"),
                     (dict(threshold=1.5), "threshold"), (dict(slack=3), "slack"), (dict(slack=-1), "slack"),
                     (dict(out=torch.zeros((4, 9, 12), dtype=torch.uint8, device=dev)), "out"),
                     (dict(bwd=bwd.cpu()), None)):
        a = dict(frames=fr, fwd=fwd, bwd=bwd, ids=ids, threshold=4, slack=0)
        a.update(kw)
        if what is None:                                 # a host tensor is simply uploaded
            ops.defect_candidates(**a)
            continue
        with pytest.raises(ValueError, match=what):
            ops.defect_candidates(**a)
    cand = D.want("half_9x13")[0]
    cd = _up(cand, dev)
    for kw, what in ((dict(cand=cd.int()), "cand"), (dict(cand=cd[0]), "cand"), (dict(ids=ids.float()), "ids"), (dict(support=0), "support"),
                     (dict(support=10), "support"), (dict(support=True), "support"), (dict(radius=17), "radius"),
                     (dict(radius=-1), "radius"), (dict(radius=2.0), "radius"), (dict(cand=cd[:, :, ::2]), "contiguous"),
                     (dict(out=torch.zeros((4, 9, 13), dtype=torch.int32, device=dev)), "out")):
        a = dict(cand=cd, ids=ids, support=1, radius=0)
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            ops.defect_clean(**a)


# ------------------------------------------------------------------------------------------------ detect_defects with given flows
def _detect(c, dev, **kw):
    flows = (np.array(c["fwd"]), np.array(c["bwd"]))    # writable copies: the cases are read-only
    return video.detect_defects(None, np.array(c["frames"]), flows=flows, device=dev, **dict(D.settings(c), **kw))


@pytest.mark.parametrize("name", D.NAMES)
def test_detect_defects_is_the_restatement(dev, name):
    c = D.case(name)
    _, _, want_masks, want_counts = D.want(name)
    with launch_trace() as trace:
        masks, counts = _detect(c, dev, return_counts=True)
    assert masks.dtype == np.uint8 and masks.shape == (c["L"], c["H"], c["W"]) and counts.shape == (c["L"],)
    assert np.array_equal(masks, want_masks) and np.array_equal(counts, want_counts)
    assert np.array_equal(_detect(c, dev), want_masks)
    n = [sum(r["symbol"] == s for r in trace) for s in DEFECT_SYMBOLS]
    assert n == ([0, 0] if c["L"] < 3 else [1, 1]) and (c["L"] >= 3 or not trace)       # L = 1, 2: nothing, no launch


def test_the_frame_guard_clears_the_frame_and_keeps_its_count(dev):
    c = D.case("wave_70x90")
    _, raw, want_masks, want_counts = D.want("wave_70x90")
    masks, counts = _detect(c, dev, return_counts=True)
    limit = int(c["max_fraction"] * c["H"] * c["W"])
    assert counts[4] == want_counts[4] > limit and not masks[4].any() and raw[4].any()
    assert all(0 < counts[t] <= limit and np.array_equal(masks[t], raw[t]) for t in (1, 2, 3))
    # with the guard open the flash comes back; with a cut in front of it, it is not judged at all
    loose, n = _detect(c, dev, return_counts=True, max_fraction=1.0)
    assert np.array_equal(loose, raw) and np.array_equal(n, want_counts)
    cut, n = _detect(c, dev, return_counts=True, scenes=[4])
    want, wn = D.detect_np(c["frames"], c["fwd"], c["bwd"], **dict(D.settings(c), scenes=[4]))
    assert np.array_equal(cut, want) and np.array_equal(n, wn) and not n[3:].any() and n[1] and n[2]


def test_size_is_the_manual_composition(dev):
    c = D.case("wave_70x90")
    rng = np.random.RandomState(3)
    base = np.repeat(np.repeat(rng.randint(60, 200, (c["L"], 10, 14, 3)), 10, axis=1), 10, axis=2).astype(np.uint8)
    base[2, 30:36, 40:47] = 255                          # a blotch that survives the resize
    base[3, 60:70, 100:108] = 0
    kw = dict(D.settings(c), flows=(np.array(c["fwd"]), np.array(c["bwd"])), device=dev, max_fraction=1.0, scenes=[5])
    got, n = video.detect_defects(None, base, size=(90, 70), return_counts=True, **kw)
    small = video.resize_frames(base, (90, 70), device=dev).cpu().numpy()
    want, wn = D.detect_np(small, c["fwd"], c["bwd"], **dict(D.settings(c), max_fraction=1.0, scenes=[5]))
    assert got.shape == (c["L"], 70, 90) and np.array_equal(got, want) and np.array_equal(n, wn) and got[2].any() and got[3].any()
    assert not got[4].any() and not got[5].any()         # the cut at 5 leaves frame 4 without its next neighbour
    assert np.array_equal(video.detect_defects(None, small, **kw), want)


# ------------------------------------------------------------------------------------------------ the net's own flows, the driver
def _net(dev, model="e2fgvi_hq"):
    """the generator with synthetic weights; e2fgvi_hq is the one that takes frames of any size"""
    if model not in _CACHE:
        from e2fgvi_amd.synth import synth_state_dict
        net = importlib.import_module("model." + model).InpaintGenerator()
        net.load_state_dict(synth_state_dict(model, "stress", 0))
        _CACHE[model] = net.to(dev).eval()
    return _CACHE[model]


def _dirty_clip(L, H, W, seed, cut=None):
    """a flat, slightly noisy scene (whatever flows synthetic weights produce, its neighbours' envelopes stay within a few levels)
    with white and black blotches on single frames; from frame ``cut`` on another scene, far darker"""
    rng = np.random.RandomState(seed)
    fr = rng.randint(118, 125, (L, H, W, 3)).astype(np.uint8)
    if cut is not None:
        fr[cut:] = rng.randint(20, 27, (L - cut, H, W, 3))
    for t in range(L):
        for k in range(3):
            h, w = rng.randint(3, 8, 2)
            y, x = rng.randint(H // 4, 3 * H // 4 - h), rng.randint(W // 4, 3 * W // 4 - w)
            fr[t, y:y + h, x:x + w] = 255 if (t + k) % 2 else 70 if cut is not None else 0
    return fr


def test_detect_defects_with_the_nets_flows(dev):
    net = _net(dev)
    frames = _dirty_clip(6, 60, 108, 4)
    with torch.no_grad():
        fwd, bwd = metrics.video_flows(net, frames)
        got, n = video.detect_defects(net, frames, return_counts=True)
        own = video.detect_defects(None, frames, flows=(fwd, bwd), device=dev)
    print("set pixels per frame", n.tolist(), "finite flows", bool(torch.isfinite(fwd).all() and torch.isfinite(bwd).all()))
    assert got.shape == (6, 60, 108) and np.array_equal(got, own)
    want, wn = D.detect_np(frames, fwd.cpu().numpy(), bwd.cpu().numpy())
    assert np.array_equal(got, want) and np.array_equal(n, wn)
    assert not got[0].any() and not got[5].any() and got[1:5].any()
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.detect_defects(lambda x, m: (x, None), frames, device=dev)


@pytest.mark.parametrize("form", ["plain", "restore", "auto", "nv12"])
def test_inpaint_video_defects_is_the_two_step_call(dev, form):
    net = _net(dev)
    with torch.no_grad():
        if form == "plain":
            frames, cuts, kw = _dirty_clip(6, 60, 108, 5), None, {}
        elif form == "restore":
            frames, cuts, kw = _dirty_clip(6, 120, 216, 6), None, dict(size=(108, 60), restore=True)
        elif form == "auto":
            frames, cuts, kw = _dirty_clip(12, 60, 108, 7, cut=6), [6], dict(scenes="auto")
            assert video.detect_cuts(frames, device=dev) == cuts
        else:
            frames, cuts, kw = _dirty_clip(6, 60, 108, 8), [3], dict(scenes=[3], pixel_format="nv12")
        rgb = frames
        if form == "nv12":
            frames = video.rgb_to_yuv420(rgb, "nv12", device=dev)
            rgb = video.yuv420_to_rgb(frames, "nv12", device=dev)
        masks = video.detect_defects(net, rgb, scenes=cuts)
        assert masks.shape == rgb.shape[:3] and masks.any()
        if cuts:
            assert not masks[cuts[0] - 1].any() and not masks[cuts[0]].any()
        want = video.inpaint_video(net, frames, masks, **kw)
        with launch_trace() as trace:
            got = video.inpaint_video(net, frames, "defects", **kw)
    assert got.shape == frames.shape and got.dtype == np.uint8 and np.array_equal(got, want), int((got != want).sum())
    assert (got != frames).any()
    assert [sum(r["symbol"] == s for r in trace) for s in DEFECT_SYMBOLS] == [1, 1]


def test_ordinary_masks_launch_what_they_launched(dev):
    """a call with masks runs no launch of the detector, and the same launches in every call"""
    f = _dirty_clip(6, 60, 108, 9)
    m = np.zeros((6, 60, 108), np.uint8)
    m[:, 20:40, 30:70] = 1
    stub = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    with launch_trace() as plain:
        a = video.inpaint_video(stub, f, m, device=dev)
    with launch_trace() as again:
        b = video.inpaint_video(stub, f, m, device=dev, scenes=[3])
    assert np.array_equal(a, video.inpaint_video(stub, f, m, device=dev)) and len(plain) > 0 and b.shape == a.shape
    for trace in (plain, again):
        assert not any(r["symbol"] in DEFECT_SYMBOLS for r in trace)
    # the launches of the masks path as they were before the detector existed: the masks, then clip and compositing per window
    # (two windows of six frames), then the bytes
    assert [r["symbol"] for r in plain] == ["e2fgvi_mask_prepare"] + ["e2fgvi_masked_clip", "e2fgvi_composite"] * 2 + ["e2fgvi_float_to_u8"]
