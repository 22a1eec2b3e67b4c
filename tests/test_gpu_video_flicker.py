"""The deflicker on the device: ops.flicker_hist, ops.flicker_curves and ops.flicker_apply (csrc/flicker.hip) and video.deflicker
against the numpy restatement of tests/flicker_cases.py, every word and every byte equal, on every named case; buffers off their
alignment; in place; reruns; and the planted 432 x 240 tennis video with a cut."""
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import flicker_cases as C
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLICKER_SYMBOLS = ("e2fgvi_flicker_hist", "e2fgvi_flicker_curves", "e2fgvi_flicker_apply")
FRAMED = tuple(n for n in C.NAMES if C.case(n)["frames"] is not None)


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.zeros(a.nbytes + shift, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _run(c, dev, shift=0, fill=None, in_place=False):
    """the dict of C.KEYS of the three entries on a case; frames and out `shift` bytes off an allocation's start, hist and out
    full of `fill` beforehand"""
    L = c["L"]
    scene = torch.from_numpy(C.scene_of_np(L, c["scenes"])).to(dev)
    if c["frames"] is None:                             # curves alone
        Q, d = ops.flicker_curves(_up(c["hist"], dev), scene, c["N"], c["span"], c["max_shift"])
        return dict(Q=Q.cpu().numpy(), d=d.cpu().numpy())
    H, W = c["H"], c["W"]
    fr = _up(c["frames"], dev, shift)
    hist = ops.flicker_hist(fr, out=None if fill is None else torch.full((L, 256), fill, dtype=torch.int32, device=dev))
    Q, d = ops.flicker_curves(hist, scene, H * W, c["span"], c["max_shift"])
    if in_place:
        out = ops.flicker_apply(fr, d, out=fr)
        assert out.data_ptr() == fr.data_ptr()
    else:
        ob = _up(np.full((L, H, W, 3), 0 if fill is None else fill, np.uint8), dev, shift) if shift or fill is not None else None
        out = ops.flicker_apply(fr, d, out=ob)
        assert np.array_equal(fr.cpu().numpy(), c["frames"])           # the input is only read
    return {k: v.cpu().numpy() for k, v in dict(hist=hist, Q=Q, d=d, out=out).items()}


def _assert_equal(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


# ------------------------------------------------------------------------------------------------ the three entries
@pytest.mark.parametrize("name", C.NAMES)
def test_entries_are_the_restatement(dev, name):
    """hist, Q, d and the output bytes on every named case -- among them W mod 4 = 1, 2 and 3, fewer pixels than a workgroup (5x7),
    several workgroups a frame (3x70x300), frames that start off a dword in an aligned buffer (w1_33x41), 67 600 pixels in one bin
    (flat_260) and, for the curves alone, rows of 2^26 pixels (big_N) -- with the byte buffers on, one and three bytes off an
    allocation's start, and into hist and out buffers that were full of something else: every word and byte is written"""
    c, want = C.case(name), C.want(name)
    for shift, fill in ((0, None), (1, None), (0, 77), (3, 200)):
        got = _run(c, dev, shift, fill)
        print(name, "shift", shift, "fill", fill, "max |d|", int(np.abs(got["d"]).max()))
        _assert_equal(got, want, C.keys(name), (name, shift, fill))
        if c["frames"] is None:
            break


@pytest.mark.parametrize("name", FRAMED)
def test_apply_in_place_gives_the_same_bytes(dev, name):
    c, want = C.case(name), C.want(name)
    for shift in (0, 1):
        _assert_equal(_run(c, dev, shift, in_place=True), want, C.KEYS, (name, shift))


def test_runs_are_the_same_bits(dev):
    for name in ("3x70x300", "clip"):
        c = C.case(name)
        first = _run(c, dev)
        for _ in range(5):
            again = _run(c, dev)
            assert all(np.array_equal(first[k], again[k]) for k in C.KEYS)


def test_arguments_are_checked(dev):
    c, want = C.case("w2_30x42"), C.want("w2_30x42")
    L, N = c["L"], c["H"] * c["W"]
    fr = _up(c["frames"], dev)
    # host inputs are uploaded
    hist = ops.flicker_hist(np.array(c["frames"]))
    assert hist.is_cuda and hist.dtype == torch.int32 and np.array_equal(hist.cpu().numpy(), want["hist"])
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(frames=fr[:, :, ::2]), "contiguous"), (dict(out=np.zeros((L, 256), np.int32)), "out"),
                     (dict(out=torch.zeros((L, 255), dtype=torch.int32, device=dev)), "out"),
                     (dict(out=torch.zeros((L, 256), dtype=torch.int64, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.flicker_hist(**dict(dict(frames=fr), **kw))
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    good = dict(hist=hist, scene=scene, N=N, span=4, max_shift=32)
    for kw, what in ((dict(hist=hist.float()), "hist"), (dict(hist=hist[0]), "hist"), (dict(hist=hist[:, ::2]), "contiguous"),
                     (dict(hist=hist[:, :255].contiguous()), "hist"), (dict(scene=scene[:-1]), "scene"), (dict(scene=scene.long()), "scene"),
                     (dict(N=-1), "N"), (dict(N=(1 << 26) + 1), "N"), (dict(N=True), "N"), (dict(N=1.5), "N"), (dict(span=-1), "span"),
                     (dict(span=9), "span"), (dict(span=True), "span"), (dict(max_shift=0), "max_shift"), (dict(max_shift=65), "max_shift"),
                     (dict(max_shift=2.5), "max_shift")):
        with pytest.raises(ValueError, match=what):
            ops.flicker_curves(**dict(good, **kw))
    Q, d = ops.flicker_curves(np.array(want["hist"]), np.zeros(L, np.int32), N, 4, 32)
    assert Q.is_cuda and np.array_equal(Q.cpu().numpy(), want["Q"]) and np.array_equal(d.cpu().numpy(), want["d"])
    for kw, what in ((dict(frames=fr.int()), "frames"), (dict(frames=fr[0]), "frames"), (dict(d=d.int()), "d"), (dict(d=d[:-1]), "d"),
                     (dict(d=d[:, ::2]), "contiguous"), (dict(out=np.zeros(fr.shape, np.uint8)), "out"),
                     (dict(out=torch.zeros((L, c["H"], c["W"] + 1, 3), dtype=torch.uint8, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.flicker_apply(**dict(dict(frames=fr, d=d), **kw))
    # an output that overlaps the frames without being them is refused by the entry, before any launch
    flat = torch.zeros(fr.numel() + 12, dtype=torch.uint8, device=dev)
    src, dst = flat[:fr.numel()].view(fr.shape).copy_(fr), flat[12:].view(fr.shape)
    with pytest.raises(lib.HipError, match="overlap"):
        ops.flicker_apply(src, d, out=dst)
    assert np.array_equal(src.cpu().numpy(), c["frames"])
    # no frame and no pixel: no launch, results of the right shapes
    with launch_trace() as trace:
        for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
            e = torch.zeros(shape, dtype=torch.uint8, device=dev)
            h = ops.flicker_hist(e, out=torch.full((shape[0], 256), 7, dtype=torch.int32, device=dev))
            q, dd = ops.flicker_curves(h, torch.zeros(shape[0], dtype=torch.int32, device=dev), shape[1] * shape[2], 4, 32)
            o = ops.flicker_apply(e, dd)
            assert h.shape == (shape[0], 256) and not h.any() and not q.any() and not dd.any() and o.shape == shape


# ------------------------------------------------------------------------------------------------ deflicker
@pytest.mark.parametrize("name", FRAMED)
def test_deflicker_is_the_restatement(dev, name):
    c, want = C.case(name), C.want(name)
    host = np.array(c["frames"])
    with launch_trace() as trace:
        out, d = video.deflicker(host, return_curves=True, device=dev, **C.settings(c))
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and isinstance(d, np.ndarray) and d.dtype == np.int16
    assert np.array_equal(out, want["out"]) and np.array_equal(d, want["d"]) and np.array_equal(host, c["frames"])
    assert [sum(r["symbol"] == s for r in trace) for s in FLICKER_SYMBOLS] == [1, 1, 1]
    plain = video.deflicker(host, device=dev, **C.settings(c))
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, want["out"])
    # a device tensor is used where it is and a device tensor comes back
    x = _up(c["frames"], dev, 1)
    got, gd = video.deflicker(x, return_curves=True, **C.settings(c))
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and gd.is_cuda and gd.dtype == torch.int16
    assert np.array_equal(got.cpu().numpy(), want["out"]) and np.array_equal(gd.cpu().numpy(), want["d"])
    assert np.array_equal(x.cpu().numpy(), c["frames"])
    # span == 0: no launch, the caller's bytes
    with launch_trace() as trace:
        same, zd = video.deflicker(host, span=0, return_curves=True, device=dev)
        on = video.deflicker(x, span=0)
    assert not any(r["symbol"].startswith("e2fgvi_flicker_") for r in trace)
    assert same.tobytes() == c["frames"].tobytes() and zd.shape == (c["L"], 256) and not zd.any()
    assert on.is_cuda and np.array_equal(on.cpu().numpy(), c["frames"])


def test_no_frame_and_no_pixel_launch_nothing(dev):
    with launch_trace() as trace:
        for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
            out, d = video.deflicker(np.zeros(shape, np.uint8), return_curves=True, device=dev)
            assert out.shape == shape and out.dtype == np.uint8 and d.shape == (shape[0], 256) and d.dtype == np.int16
    assert not any(r["symbol"].startswith("e2fgvi_flicker_") for r in trace)


def test_planted_432x240_video_is_the_restatement(dev):
    """the 25 frames of tests/golden/tennis25.npz under flicker_cases.plant(seed 1) with a cut at frame 12 and the defaults: the
    bytes of the restatement, a roughness of at most 0.25 of the flickered video's, and the same bytes from a second call"""
    planted = C.plant(C.tennis25(ROOT), 1)
    want = C.deflicker_np(planted, scenes=[12], **C.DEFAULTS)
    out, d = video.deflicker(planted, scenes=[12], return_curves=True, device=dev)
    before, after = C.roughness(planted), C.roughness(out)
    print("roughness", before, "->", after, "ratio", after / before, "max |d|", int(np.abs(d).max()))
    assert out.shape == (25, 240, 432, 3) and out.tobytes() == want["out"].tobytes() and np.array_equal(d, want["d"])
    assert after <= 0.25 * before
    assert video.deflicker(planted, scenes=[12], device=dev).tobytes() == out.tobytes()
