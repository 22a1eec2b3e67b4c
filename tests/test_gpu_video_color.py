"""The colour restoration on the device: ops.color_hist, ops.color_nodes, ops.color_lut and ops.color_apply (csrc/color.hip),
video.restore_color and video.apply_color against the numpy restatement of tests/color_cases.py, every word and every byte equal,
on every named case; buffers off their alignment; in place; reruns; and the faded 432 x 240 tennis video with a cut."""
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import color_cases as C
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLOR_SYMBOLS = ("e2fgvi_color_hist", "e2fgvi_color_nodes", "e2fgvi_color_lut", "e2fgvi_color_apply")
VIDEOS = tuple(n for n in C.NAMES if C.case(n)["kind"] == "video")
FRAMED = tuple(n for n in C.NAMES if C.case(n)["kind"] in ("video", "apply") and n != "slabs_65540")


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.zeros(a.nbytes + shift, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _run(name, dev, shift=0, fill=None, in_place=False):
    """the dict of C.keys(name) of the four entries on a case; the byte buffers -- frames, graded, lut and out -- `shift` bytes off
    an allocation's start, hist and out full of `fill` beforehand"""
    c, w = C.case(name), C.want(name)
    if c["kind"] == "nodes":
        return dict(Q=ops.color_nodes(_up(c["hist"], dev), _up(c["starts"], dev), _up(c["ids"], dev), c["clip"]).cpu().numpy())
    if c["kind"] == "lut":
        return dict(lut=ops.color_lut(_up(c["Q"], dev), _up(c["mode"], dev), _up(c["T"], dev), **C.lut_settings(c)).cpu().numpy())
    fr = _up(c["frames"], dev, shift)
    L = fr.shape[0]
    got = {}
    if c["kind"] == "video":
        full = None if fill is None else torch.full((L, 3, 256), fill, dtype=torch.int32, device=dev)
        got["hist"] = ops.color_hist(fr, out=full)
        got["Q"] = ops.color_nodes(got["hist"], _up(w["starts"], dev), _up(w["ids"], dev), c["clip"])
        if c["graded"] is not None:
            got["T"] = ops.color_nodes(ops.color_hist(_up(c["graded"], dev, shift)), _up(w["gstarts"], dev), _up(w["gids"], dev), c["clip"])
        got["lut"] = ops.color_lut(got["Q"], _up(w["mode"], dev), got.get("T"), **C.lut_settings(c))
        lut, group = got["lut"], _up(w["group"], dev)
        if shift:
            lut = _up(lut.cpu().numpy(), dev, shift)
    else:
        lut, group = _up(c["lut"], dev, shift), _up(c["group"], dev)
    if in_place:
        got["out"] = ops.color_apply(fr, lut, group, out=fr)
        assert got["out"].data_ptr() == fr.data_ptr()
    else:
        ob = _up(np.full(fr.shape, 0 if fill is None else fill, np.uint8), dev, shift) if shift or fill is not None else None
        got["out"] = ops.color_apply(fr, lut, group, out=ob)
        assert torch.equal(fr.cpu(), torch.from_numpy(np.array(c["frames"])))           # the input is only read
    return {k: v.cpu().numpy() for k, v in got.items()}


def _assert_equal(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


# ------------------------------------------------------------------------------------------------ the four entries
@pytest.mark.parametrize("name", C.NAMES)
def test_entries_are_the_restatement(dev, name):
    """hist, Q, T, lut and the output bytes on every named case -- among them W mod 4 = 1, 2 and 3, fewer pixels than a workgroup
    (5x7), several workgroups a frame (3x70x300), frames that start off a dword in an aligned buffer (w1_33x41), 67 600 pixels in
    one bin per channel (flat_260), pools past 2^31 pixels (big_N), ids and groups out of range, and 65 540 frames in two launches
    -- with the byte buffers on, one and three bytes off an allocation's start, and into hist and out buffers that were full of
    something else: every word and byte is written"""
    want = C.want(name)
    for shift, fill in ((0, None), (1, None), (0, 77), (3, 200)):
        got = _run(name, dev, shift, fill)
        print(name, "shift", shift, "fill", fill, {k: v.shape for k, v in got.items()})
        _assert_equal(got, want, C.keys(name), (name, shift, fill))
        if C.case(name)["kind"] in ("nodes", "lut") or name == "slabs_65540":
            break


@pytest.mark.parametrize("name", FRAMED)
def test_apply_in_place_gives_the_same_bytes(dev, name):
    want = C.want(name)
    for shift in (0, 1):
        _assert_equal(_run(name, dev, shift, in_place=True), want, C.keys(name), (name, shift))


def test_runs_are_the_same_bits(dev):
    for name in ("3x70x300", "keys_9", "flat_260"):
        first = _run(name, dev)
        for _ in range(5):
            again = _run(name, dev)
            assert all(np.array_equal(first[k], again[k]) for k in C.keys(name))


def test_arguments_are_checked(dev):
    c, want = C.case("keys_9"), C.want("keys_9")
    L, (H, W) = len(c["frames"]), c["frames"].shape[1:3]
    fr = _up(c["frames"], dev)
    # host inputs are uploaded
    hist = ops.color_hist(np.array(c["frames"]))
    assert hist.is_cuda and hist.dtype == torch.int32 and np.array_equal(hist.cpu().numpy(), want["hist"])
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(frames=fr[:, :, ::2]), "contiguous"), (dict(out=np.zeros((L, 3, 256), np.int32)), "out"),
                     (dict(out=torch.zeros((L, 256), dtype=torch.int32, device=dev)), "out"),
                     (dict(out=torch.zeros((L, 3, 256), dtype=torch.int64, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.color_hist(**dict(dict(frames=fr), **kw))
    starts, ids = _up(want["starts"], dev), _up(want["ids"], dev)
    good = dict(hist=hist, starts=starts, ids=ids, clip=(5, 5))
    for kw, what in ((dict(hist=hist.float()), "hist"), (dict(hist=hist[0]), "hist"), (dict(hist=hist[:, :, ::2]), "contiguous"),
                     (dict(hist=hist[:, :2].contiguous()), "hist"), (dict(starts=starts.long()), "starts"), (dict(starts=starts[:0]), "starts"),
                     (dict(starts=starts.view(2, 2)), "starts"), (dict(ids=ids.long()), "ids"), (dict(ids=ids.view(2, 3)), "ids"),
                     (dict(clip=(-1, 5)), "clip"), (dict(clip=(5, 251)), "clip"), (dict(clip=(True, 5)), "clip"), (dict(clip=5), "clip"),
                     (dict(clip=(1.5, 5)), "clip"), (dict(clip=(5, 5, 5)), "clip")):
        with pytest.raises(ValueError, match=what):
            ops.color_nodes(**dict(good, **kw))
    Q = ops.color_nodes(np.array(want["hist"]), np.array(want["starts"]), np.array(want["ids"]))
    assert Q.is_cuda and np.array_equal(Q.cpu().numpy(), want["Q"])
    mode, T = _up(want["mode"], dev), _up(want["T"], dev)
    good = dict(Q=Q, mode=mode, T=T)
    for kw, what in ((dict(Q=Q.float()), "Q"), (dict(Q=Q[0]), "Q"), (dict(Q=Q[..., :32].contiguous()), "Q"), (dict(Q=Q[:, :, ::2]), "contiguous"),
                     (dict(mode=mode[:-1]), "mode"), (dict(mode=mode.long()), "mode"), (dict(T=T[:-1]), "T"), (dict(T=T.long()), "T"),
                     (dict(target=(-1, -1)), "target"), (dict(target=(100, 100)), "target"), (dict(target=(0, 256)), "target"),
                     (dict(target=(True, 200)), "target"), (dict(target=16), "target"), (dict(min_range=0), "min_range"),
                     (dict(min_range=256), "min_range"), (dict(min_range=True), "min_range"), (dict(max_gain=255), "max_gain"),
                     (dict(max_gain=4097), "max_gain"), (dict(max_gain=2.5), "max_gain"), (dict(strength=-1), "strength"),
                     (dict(strength=257), "strength"), (dict(strength=None), "strength")):
        with pytest.raises(ValueError, match=what):
            ops.color_lut(**dict(good, **kw))
    lut = ops.color_lut(np.array(want["Q"]), np.array(want["mode"]), np.array(want["T"]))
    assert lut.is_cuda and lut.dtype == torch.uint8 and np.array_equal(lut.cpu().numpy(), want["lut"])
    # without T nothing is matched onto anything else: the nodes onto themselves
    same = ops.color_lut(Q, mode).cpu().numpy()
    assert np.array_equal(same, C.lut_np(want["Q"], want["mode"]))
    group = _up(want["group"], dev)
    good = dict(frames=fr, lut=lut, group=group)
    for kw, what in ((dict(frames=fr.int()), "frames"), (dict(frames=fr[0]), "frames"), (dict(lut=lut.int()), "lut"), (dict(lut=lut[0]), "lut"),
                     (dict(lut=lut[:, :, ::2]), "contiguous"), (dict(lut=lut[:, :2].contiguous()), "lut"), (dict(group=group[:-1]), "group"),
                     (dict(group=group.long()), "group"), (dict(out=np.zeros(fr.shape, np.uint8)), "out"),
                     (dict(out=torch.zeros((L, H, W + 1, 3), dtype=torch.uint8, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.color_apply(**dict(good, **kw))
    out = ops.color_apply(np.array(c["frames"]), np.array(want["lut"]), np.array(want["group"]))
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), want["out"])
    # an output that overlaps the frames without being them is refused by the entry, before any launch
    flat = torch.zeros(fr.numel() + 12, dtype=torch.uint8, device=dev)
    src, dst = flat[:fr.numel()].view(fr.shape).copy_(fr), flat[12:].view(fr.shape)
    with pytest.raises(lib.HipError, match="overlap"):
        ops.color_apply(src, lut, group, out=dst)
    assert np.array_equal(src.cpu().numpy(), c["frames"])
    # no frame, no pixel and no group: results of the right shapes, zeros where zeros are the answer
    for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
        e = torch.zeros(shape, dtype=torch.uint8, device=dev)
        h = ops.color_hist(e, out=torch.full((shape[0], 3, 256), 7, dtype=torch.int32, device=dev))
        q = ops.color_nodes(h, torch.tensor([0, shape[0]], dtype=torch.int32, device=dev),
                            torch.arange(shape[0], dtype=torch.int32, device=dev))
        o = ops.color_apply(e, lut, torch.zeros(shape[0], dtype=torch.int32, device=dev))
        assert h.shape == (shape[0], 3, 256) and not h.any() and q.shape == (1, 3, 34) and not q.any() and o.shape == shape
    none = torch.zeros((0, 3, 34), dtype=torch.int32, device=dev)
    q = ops.color_nodes(hist, torch.zeros(1, dtype=torch.int32, device=dev), ids)
    assert q.shape == (0, 3, 34) and ops.color_lut(none, torch.zeros(0, dtype=torch.int32, device=dev)).shape == (0, 3, 256)
    # no table at all: every frame's group is outside [0, 0) and every frame is copied
    o = ops.color_apply(fr, torch.zeros((0, 3, 256), dtype=torch.uint8, device=dev), group)
    assert np.array_equal(o.cpu().numpy(), c["frames"])


# ------------------------------------------------------------------------------------------------ restore_color, apply_color
@pytest.mark.parametrize("name", VIDEOS)
def test_restore_color_is_the_restatement(dev, name):
    """all three modes -- automatic levels, key frames, a reference alone -- among the cases"""
    c, want = C.case(name), C.want(name)
    host = np.array(c["frames"])                        # writable copies: the cases are read-only
    settings = dict(C.settings(c), graded=None if c["graded"] is None else np.array(c["graded"]))
    counts = [1, 1, 1, 1] if c["graded"] is None else [2, 2, 1, 1]
    with launch_trace() as trace:
        out, luts = video.restore_color(host, return_curves=True, device=dev, **settings)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and isinstance(luts, np.ndarray) and luts.dtype == np.uint8
    assert np.array_equal(out, want["out"]) and np.array_equal(luts, want["lut"]) and np.array_equal(host, c["frames"])
    assert [sum(r["symbol"] == s for r in trace) for s in COLOR_SYMBOLS] == counts
    # the curves that came back, applied: the same bytes, in one launch
    with launch_trace() as trace:
        again = video.apply_color(host, luts, scenes=c["scenes"], device=dev)
    assert isinstance(again, np.ndarray) and np.array_equal(again, want["out"])
    assert [sum(r["symbol"] == s for r in trace) for s in COLOR_SYMBOLS] == [0, 0, 0, 1]
    if name == "slabs_65540":
        return
    plain = video.restore_color(host, device=dev, **settings)
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, want["out"])
    # a device tensor is used where it is and a device tensor comes back
    x = _up(c["frames"], dev, 1)
    kw = dict(settings, graded=None if c["graded"] is None else _up(c["graded"], dev, 3))
    got, gl = video.restore_color(x, return_curves=True, **kw)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and gl.is_cuda and gl.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want["out"]) and np.array_equal(gl.cpu().numpy(), want["lut"])
    assert np.array_equal(x.cpu().numpy(), c["frames"])
    on = video.apply_color(x, gl, scenes=c["scenes"])
    assert on.is_cuda and np.array_equal(on.cpu().numpy(), want["out"]) and np.array_equal(x.cpu().numpy(), c["frames"])
    # strength == 0: no launch, the caller's bytes and identity tables
    with launch_trace() as trace:
        same, il = video.restore_color(host, return_curves=True, device=dev, **dict(settings, strength=0))
        on = video.restore_color(x, **dict(kw, strength=0))
    assert not any(r["symbol"].startswith("e2fgvi_color_") for r in trace)
    assert same.tobytes() == c["frames"].tobytes() and il.shape == want["lut"].shape and (il == np.arange(256, dtype=np.uint8)).all()
    assert on.is_cuda and np.array_equal(on.cpu().numpy(), c["frames"])


def test_no_frame_and_no_pixel_launch_nothing(dev):
    with launch_trace() as trace:
        for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
            scenes = [1] if shape[0] else None
            out, luts = video.restore_color(np.zeros(shape, np.uint8), scenes=scenes, return_curves=True, device=dev)
            assert out.shape == shape and out.dtype == np.uint8 and luts.shape == (2 if scenes else 1, 3, 256) and luts.dtype == np.uint8
            assert (luts == np.arange(256, dtype=np.uint8)).all()
            again = video.apply_color(np.zeros(shape, np.uint8), luts, scenes=scenes, device=dev)
            assert again.shape == shape and again.dtype == np.uint8
            g = video.restore_color(np.zeros(shape, np.uint8), graded=np.zeros((1, 2, 2, 3), np.uint8), device=dev)
            assert g.shape == shape
    assert not any(r["symbol"].startswith("e2fgvi_color_") for r in trace)


def test_faded_432x240_video_is_the_restatement(dev):
    """the 25 frames of tests/golden/tennis25.npz under color_cases.plant_fade (the affine fade) with a cut at frame 12: automatic
    levels, and frames 0 and 12 with their clean versions as keys, give the bytes of the restatement and the same bytes from a
    second call; without the cut, levels reach 31 dB against the clean video and frame 0 as the only key 42 dB over all frames"""
    clean = C.tennis25(ROOT)
    faded = C.plant_fade(clean, **C.FADES["affine"])
    for kw in (dict(scenes=[12]), dict(scenes=[12], graded=clean[[0, 12]], keys=[0, 12]), dict(), dict(graded=clean[:1], keys=[0])):
        want = C.restore_np(faded, **kw)
        out, luts = video.restore_color(faded, return_curves=True, device=dev, **kw)
        print(sorted(kw), "faded", C.psnr(faded, clean), "->", C.psnr(out, clean), "worst frame", min(C.psnr_frames(out, clean)))
        assert out.shape == (25, 240, 432, 3) and out.tobytes() == want["out"].tobytes() and np.array_equal(luts, want["lut"])
        assert (np.diff(luts.astype(np.int64), axis=-1) >= 0).all()
        assert video.restore_color(faded, device=dev, **kw).tobytes() == out.tobytes()
        if "scenes" not in kw:
            assert C.psnr(out, clean) >= (42 if kw else 31)
