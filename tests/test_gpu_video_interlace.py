"""The deinterlacer on the device: ops.deinterlace and ops.interlace_scores (csrc/interlace.hip), video.deinterlace and
video.detect_interlace against the numpy restatement of tests/interlace_cases.py, every byte and every word equal, on every named
case at every setting; buffers off their alignment; reruns; frames launched in slabs; and the planted 432 x 240 tennis clip."""
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import interlace_cases as C
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("e2fgvi_interlace_scores", "e2fgvi_deinterlace")


def _up(a, dev, shift=0, fill=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.full((a.nbytes + shift,), fill, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _scene(c, dev):
    return torch.from_numpy(C.scene_of_np(c["L"], c["scenes"])).to(dev)


def _fields(fr, scene, setting, shift=0, fill=None):
    """ops.deinterlace at a setting; with `fill` or `shift` into an out buffer `shift` bytes off an allocation's start and full of
    `fill` beforehand"""
    tff, mode, guard, edges = setting
    if fill is None and not shift:
        return ops.deinterlace(fr, scene, bool(tff), mode, bool(guard), edges)
    shape = ((2 if mode == 0 else 1) * fr.shape[0],) + tuple(fr.shape[1:])
    ob = _up(np.full(shape, fill or 0, np.uint8), fr.device, shift)
    out = ops.deinterlace(fr, scene, bool(tff), mode, bool(guard), edges, out=ob)
    assert out.data_ptr() == ob.data_ptr()
    return out


# ------------------------------------------------------------------------------------------------ the two entries
@pytest.mark.parametrize("name", C.NAMES)
def test_entries_are_the_restatement(dev, name):
    """the scores and the output bytes on every named case -- H in 1 .. 6 by W in 1 .. 7, sides that are no multiple of 4, rows of
    more than 1024 pixels, a tall narrow frame, one to four frames, a cut at every place, frames of 0 and 255 alone, flat frames
    -- at both orders, all three modes, guard on and off and edges 0, 1 and 2, with the byte buffers on, and one, two and three
    bytes off an allocation's start, and into out buffers that were full of something else: every byte is written"""
    c = C.case(name)
    scene = _scene(c, dev)
    for shift, fill in ((0, None), (1, None), (2, 77), (3, 200), (0, 255)):
        fr = _up(c["frames"], dev, shift)
        D = ops.interlace_scores(fr, scene)
        assert D.dtype == torch.int64 and np.array_equal(D.cpu().numpy(), C.want_scores(name)), (name, shift, D.tolist())
        for setting in C.SETTINGS:
            got = _fields(fr, scene, setting, shift, fill).cpu().numpy()
            want = C.want(name, setting)
            assert got.dtype == np.uint8 and got.shape == want.shape, (name, shift, setting, got.shape)
            assert np.array_equal(got, want), (name, shift, fill, setting, int((got != want).sum()))
        assert np.array_equal(fr.cpu().numpy(), c["frames"])           # the input is only read
    print(name, "D", C.want_scores(name).tolist()[:2])


def test_runs_are_the_same_bits(dev):
    for name in ("noise_37x53", "tall_300x20", "wide_9x1100"):
        c = C.case(name)
        fr, scene = _up(c["frames"], dev), _scene(c, dev)
        first = [ops.interlace_scores(fr, scene).cpu().numpy()] + [_fields(fr, scene, s).cpu().numpy() for s in ((1, 0, 1, 0), (0, 0, 1, 2))]
        for _ in range(5):
            again = [ops.interlace_scores(fr, scene).cpu().numpy()] + [_fields(fr, scene, s).cpu().numpy() for s in ((1, 0, 1, 0), (0, 0, 1, 2))]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_frame_rate_results_are_the_pictures_of_the_field_rate_result(dev):
    for name in ("noise_37x53", "cut2_40x52", "tiny_5x7"):
        c = C.case(name)
        fr, scene = _up(c["frames"], dev), _scene(c, dev)
        for tff, guard, edges in ((1, 1, 0), (0, 0, 2), (0, 1, 1)):
            full = _fields(fr, scene, (tff, 0, guard, edges))
            assert torch.equal(_fields(fr, scene, (tff, 1, guard, edges)), full[0::2])
            assert torch.equal(_fields(fr, scene, (tff, 2, guard, edges)), full[1::2])


def test_more_frames_than_a_launch_takes(dev):
    """65 540 frames of one pixel: both kernels carry the frames on the grid's y axis and launch them in slabs of 65 535; a cut in
    the second slab.  With one row the missing picture is the mean of the two frames around the field, and nothing is scored; the
    scores are exercised on frames of 4 x 1."""
    L, cut = 65540, 65537
    rng = np.random.RandomState(70)
    fr = rng.randint(0, 256, (L, 1, 1, 3)).astype(np.uint8)
    so = C.scene_of_np(L, [cut])
    nxt = np.concatenate([fr[1:], fr[-1:]]).astype(np.int64)
    nxt[cut - 1] = fr[cut - 1]
    want = np.zeros((2 * L, 1, 1, 3), np.uint8)
    want[0::2], want[1::2] = fr, (fr.astype(np.int64) + nxt) >> 1
    x, scene = _up(fr, dev), _up(so, dev)
    got = ops.deinterlace(x, scene, True, 0, True, 0).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(ops.deinterlace(x, scene, True, 2, False, 2).cpu().numpy(), want[1::2])
    assert not ops.interlace_scores(x, scene).any()
    tall = rng.randint(0, 256, (L, 4, 1, 3)).astype(np.uint8)
    Y = C.luma(tall)[:, :, 0]
    D = np.zeros((L, 2), np.int64)
    D[:-1, 1] = np.abs(2 * Y[1:, 1] - Y[:-1, 0] - Y[:-1, 2])
    D[:-1, 0] = np.abs(2 * Y[1:, 2] - Y[:-1, 1] - Y[:-1, 3])
    D[cut - 1] = 0
    assert np.array_equal(ops.interlace_scores(_up(tall, dev), scene).cpu().numpy(), D)


def test_arguments_are_checked(dev):
    c = C.case("noise_37x53")
    L, H, W = c["L"], c["H"], c["W"]
    fr, scene = _up(c["frames"], dev), _scene(c, dev)
    good = dict(frames=fr, scene=scene, tff=True, mode=0, guard=True, edges=0)
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(frames=fr[:, :, ::2]), "contiguous"), (dict(scene=scene[:-1]), "scene"), (dict(scene=scene.long()), "scene"),
                     (dict(tff=1), "tff"), (dict(tff=None), "tff"), (dict(guard=0), "guard"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
                     (dict(mode=True), "mode"), (dict(edges=3), "edges"), (dict(edges=1.5), "edges"), (dict(edges=False), "edges"),
                     (dict(out=np.zeros((2 * L, H, W, 3), np.uint8)), "out"),
                     (dict(out=torch.zeros((L, H, W, 3), dtype=torch.uint8, device=dev)), "out"),
                     (dict(mode=1, out=torch.zeros((2 * L, H, W, 3), dtype=torch.uint8, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.deinterlace(**dict(good, **kw))
    for kw, what in ((dict(frames=fr.int()), "frames"), (dict(frames=fr[0, 0]), "frames"), (dict(scene=scene[1:]), "scene"),
                     (dict(scene=scene.float()), "scene")):
        with pytest.raises(ValueError, match=what):
            ops.interlace_scores(**dict(dict(frames=fr, scene=scene), **kw))
    # host inputs are uploaded
    got = ops.deinterlace(np.array(c["frames"]), C.scene_of_np(L), True, 0, True, 0)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), C.want("noise_37x53", (1, 0, 1, 0)))
    # an output that overlaps the frames is refused by the entry, before any launch -- the frames themselves too
    n = fr.numel()
    flat = torch.zeros(3 * n + 12, dtype=torch.uint8, device=dev)
    src = flat[:n].view(fr.shape).copy_(fr)
    for mode, at in ((0, 12), (0, n - 1), (1, 12), (2, 0), (1, n - 1)):
        dst = flat[at:at + (2 if mode == 0 else 1) * n].view(((2 if mode == 0 else 1) * L, H, W, 3))
        with pytest.raises(lib.HipError, match="overlap"):
            ops.deinterlace(src, scene, True, mode, True, 0, out=dst)
    behind = flat[n:3 * n].view((2 * L, H, W, 3))                      # right behind the frames: no overlap
    assert np.array_equal(ops.deinterlace(src, scene, True, 0, True, 0, out=behind).cpu().numpy(), C.want("noise_37x53", (1, 0, 1, 0)))
    assert np.array_equal(src.cpu().numpy(), c["frames"])
    # no frame and no pixel: results of the right shapes
    for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
        e = torch.zeros(shape, dtype=torch.uint8, device=dev)
        sc = torch.zeros(shape[0], dtype=torch.int32, device=dev)
        D = ops.interlace_scores(e, sc)
        assert D.shape == (shape[0], 2) and not D.any()
        assert ops.deinterlace(e, sc, True, 0, True, 0).shape == (2 * shape[0],) + shape[1:]
        assert ops.deinterlace(e, sc, False, 2, True, 1).shape == shape


# ------------------------------------------------------------------------------------------------ video.deinterlace, video.detect_interlace
def _settings_kw(setting):
    tff, mode, guard, edges = setting
    return dict(order="tff" if tff else "bff", rate="field" if mode == 0 else "frame", keep="second" if mode == 2 else "first",
                guard=bool(guard), edges=edges)


@pytest.mark.parametrize("name", ("noise_37x53", "cut2_40x52", "tiny_1x1", "tiny_3x5", "single_6x7", "extremes_40x52", "wide_9x1100"))
def test_video_functions_are_the_restatement(dev, name):
    c = C.case(name)
    host = np.array(c["frames"])
    for setting in ((1, 0, 1, 0), (0, 0, 0, 2), (1, 1, 1, 1), (0, 2, 1, 0)):
        want = C.want(name, setting)
        with launch_trace() as trace:
            out = video.deinterlace(host, scenes=c["scenes"], device=dev, **_settings_kw(setting))
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and np.array_equal(out, want), (name, setting)
        assert [sum(r["symbol"] == s for r in trace) for s in SYMBOLS] == [0, 1]
        # a device tensor is used where it is -- on, and one, two and three bytes off a dword -- and a device tensor comes back
        for off in (0, 1, 2, 3):
            x = _up(c["frames"], dev, off)
            got = video.deinterlace(x, scenes=c["scenes"], **_settings_kw(setting))
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
            assert np.array_equal(x.cpu().numpy(), c["frames"])
    assert np.array_equal(host, c["frames"])
    assert np.array_equal(video.deinterlace(host, scenes=c["scenes"], device=dev), C.want(name, (1, 0, 1, 0)))      # the defaults
    with launch_trace() as trace:
        verdict, D, votes = video.detect_interlace(host, scenes=c["scenes"], return_scores=True, device=dev)
    assert [sum(r["symbol"] == s for r in trace) for s in SYMBOLS] == [1, 0]
    assert isinstance(D, np.ndarray) and D.dtype == np.int64 and np.array_equal(D, C.want_scores(name))
    assert (verdict, votes.tolist()) == (C.field_order_np(D, c["scenes"])[0], C.field_order_np(D, c["scenes"])[1].tolist())
    on = video.detect_interlace(_up(c["frames"], dev, 1), scenes=c["scenes"], return_scores=True, margin=20)
    assert on[0] == C.field_order_np(D, c["scenes"], 20)[0] and isinstance(on[1], np.ndarray) and np.array_equal(on[1], D)
    assert video.detect_interlace(host, scenes=c["scenes"], device=dev) == verdict


def test_scene_by_scene_is_the_call_with_scenes(dev):
    c = C.case("cut2_40x52")
    x = _up(c["frames"], dev)
    for kw in (dict(), dict(order="bff", guard=False, edges=2), dict(rate="frame", keep="second", edges=1)):
        whole = video.deinterlace(x, scenes=[2], **kw)
        parts = torch.cat([video.deinterlace(x[:2].contiguous(), **kw), video.deinterlace(x[2:].contiguous(), **kw)])
        assert torch.equal(whole, parts)
        assert not torch.equal(whole, video.deinterlace(x, **kw))       # and the cut is seen


def test_no_frame_and_no_pixel_launch_nothing(dev):
    with launch_trace() as trace:
        for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
            out = video.deinterlace(np.zeros(shape, np.uint8), device=dev)
            assert isinstance(out, np.ndarray) and out.shape == (2 * shape[0],) + shape[1:] and out.dtype == np.uint8
            assert video.deinterlace(np.zeros(shape, np.uint8), rate="frame", device=dev).shape == shape
            on = video.deinterlace(torch.zeros(shape, dtype=torch.uint8, device=dev), rate="frame", keep="second")
            assert on.is_cuda and tuple(on.shape) == shape
            verdict, D, votes = video.detect_interlace(np.zeros(shape, np.uint8), return_scores=True, device=dev)
            assert verdict == "progressive" and D.shape == (shape[0], 2) and not D.any() and votes.shape == (shape[0],)
    assert not any(r["symbol"] in SYMBOLS for r in trace)


def test_planted_432x240_clips_are_the_restatement(dev):
    """the panning clip of tests/golden/tennis25.npz interlaced in either order: the verdict, the scores and the field-rate bytes of
    the restatement; order="auto" finds the order with one more launch, and refuses the progressive frames"""
    f = C.tennis25(ROOT)
    for tff in (True, False):
        clip, src = C.pan_clip(f, tff)
        with launch_trace() as trace:
            verdict, D, votes = video.detect_interlace(clip, return_scores=True, device=dev)
        assert verdict == ("tff" if tff else "bff") and np.array_equal(D, C.scores_np(clip)) and len(trace) == 1
        print("tff" if tff else "bff", "D0 / D1", (D[:-1, 0] / D[:-1, 1]).round(3).tolist(), votes.tolist())
        with launch_trace() as trace:
            out = video.deinterlace(clip, order="auto", device=dev)
        assert [sum(r["symbol"] == s for r in trace) for s in SYMBOLS] == [1, 1]
        assert out.shape == src.shape and out.tobytes() == video.deinterlace(clip, order=verdict, device=dev).tobytes()
        if tff:
            assert out.tobytes() == C.deinterlace_np(clip, None, 1, 0, 1, 0).tobytes()
            print("PSNR over the missing rows", C.psnr_missing(out, src), "line averaging", C.psnr_missing(C.line_average(clip), src))
    with pytest.raises(ValueError, match="order"):
        video.deinterlace(f[:12], order="auto", device=dev)
