"""The temporal denoiser on the device: ops.denoise (csrc/denoise.hip) and video.denoise against the numpy restatement of
tests/denoise_cases.py, every byte equal, on every named case at every setting; buffers off their alignment; reruns; frames
launched in slabs; what the definition guarantees; the net's own flows."""
import importlib
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, metrics, ops, video
from tests import denoise_cases as C
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "e2fgvi_denoise"
_CACHE = {}


def _up(a, dev, shift=0, fill=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.full((a.nbytes + shift,), fill, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _inputs(c, dev, shift=0):
    """(frames, fwd, bwd, scene) of a case on the device; the frames `shift` bytes off an allocation's start"""
    return (_up(c["frames"], dev, shift), _up(c["fwd"], dev), _up(c["bwd"], dev),
            torch.from_numpy(C.scene_of_np(c["L"], c["scenes"])).to(dev))


# ------------------------------------------------------------------------------------------------ the entry
@pytest.mark.parametrize("name", C.NAMES)
def test_entry_is_the_restatement(dev, name):
    """the output bytes on every named case -- frames of 1 x 1 to 64 x 128, sides that are no multiple of 4 or 64, frames smaller
    than a patch and than the search window, more than one tile on either axis, one to five frames, a cut at every place, flows on
    exact halves, on the last row and column and just outside, on - 0.5, non-finite ones, flows into the corners, random ones of
    +- 6 px, bytes of 0 and 255 alone, flat frames -- at strength 1, 8 and 64, search 0, 1 and 2 and max_change 0, 3 and 255, with
    the frames on, and one, two and three bytes off an allocation's start, and into out buffers that were full of something else:
    every byte is written"""
    c = C.case(name)
    for shift, fill in ((0, None), (1, 77), (2, None), (3, 255)):
        fr, fwd, bwd, scene = _inputs(c, dev, shift)
        for setting in C.SETTINGS:
            want = C.want(name, setting)
            if fill is None:
                got = ops.denoise(fr, fwd, bwd, scene, *setting)
            else:
                ob = _up(np.full(want.shape, fill, np.uint8), dev, shift)
                got = ops.denoise(fr, fwd, bwd, scene, *setting, out=ob)
                assert got.data_ptr() == ob.data_ptr()
            got = got.cpu().numpy()
            assert got.dtype == np.uint8 and got.shape == want.shape, (name, shift, setting, got.shape)
            assert np.array_equal(got, want), (name, shift, fill, setting, int((got != want).sum()))
        assert np.array_equal(fr.cpu().numpy(), c["frames"])           # the input is only read


def test_runs_are_the_same_bits(dev):
    for name in ("soft_64x128", "random_33x70", "nonfinite_17x23"):
        fr, fwd, bwd, scene = _inputs(C.case(name), dev)
        first = [ops.denoise(fr, fwd, bwd, scene, *s).cpu().numpy() for s in ((8, 1, 255), (64, 2, 3))]
        for _ in range(5):
            again = [ops.denoise(fr, fwd, bwd, scene, *s).cpu().numpy() for s in ((8, 1, 255), (64, 2, 3))]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_more_frames_than_a_launch_takes(dev):
    """65 537 frames of 2 x 2: the frames ride on the grid's y axis and are launched in slabs of 65 535; frame 65 535, the first of
    the second slab, takes from frame 65 534 of the first, and a cut lies in the second slab"""
    L, cut = 65537, 65536
    rng = np.random.RandomState(70)
    base = rng.randint(60, 200, (1, 2, 2, 3))
    fr = np.clip(base + rng.randint(-6, 7, (L, 2, 2, 3)), 0, 255).astype(np.uint8)
    fwd = rng.randint(-2, 3, (L - 1, 2, 2, 2)).astype(np.float32) * 0.5
    bwd = rng.randint(-2, 3, (L - 1, 2, 2, 2)).astype(np.float32) * 0.5
    scene = C.scene_of_np(L, [cut])
    want = C.reference(fr, fwd, bwd, scene, 64, 1, 255)
    assert not np.array_equal(want[65530:], fr[65530:]) and np.array_equal(want[cut], fr[cut])
    got = ops.denoise(_up(fr, dev), _up(fwd, dev), _up(bwd, dev), _up(scene, dev), 64, 1, 255).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())


def test_guarantees_hold_on_the_device(dev):
    for name in ("soft_33x70", "cut2_17x23", "extremes_64x128"):
        c = C.case(name)
        fr, fwd, bwd, scene = _inputs(c, dev)
        alone = torch.arange(c["L"], dtype=torch.int32, device=dev)
        for h, s in ((8, 1), (64, 2), (1, 0)):
            assert torch.equal(ops.denoise(fr, fwd, bwd, scene, h, s, 0), fr)
            assert torch.equal(ops.denoise(fr, fwd, bwd, alone, h, s, 255), fr)
            for limit in (1, 3):
                d = ops.denoise(fr, fwd, bwd, scene, h, s, limit).int() - fr.int()
                assert int(d.abs().max()) <= limit
    # a video denoised scene by scene and joined is the call with the scene table
    c = C.case("cut2_17x23")
    fr, fwd, bwd, scene = _inputs(c, dev)
    zeros = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    for setting in ((8, 1, 255), (64, 2, 3)):
        whole = ops.denoise(fr, fwd, bwd, scene, *setting)
        parts = torch.cat([ops.denoise(fr[a:b].contiguous(), fwd[a:b - 1].contiguous(), bwd[a:b - 1].contiguous(), zeros(b - a), *setting)
                           for a, b in ((0, 2), (2, 5))])
        assert torch.equal(whole, parts)
        assert not torch.equal(whole, ops.denoise(fr, fwd, bwd, zeros(5), *setting))    # and the cut is seen
    # a still video, with and without a blotch on one frame: byte for byte at search 0; a flat one at every search
    f = C.tennis25(ROOT)
    zero = torch.zeros((4, 40, 60, 2), dtype=torch.float32, device=dev)
    for blotch in (False, True):
        clip = _up(C.still_clip(f, blotch), dev)
        assert torch.equal(ops.denoise(clip, zero, zero, zeros(5), 8, 0, 255), clip)
    flat = np.full((5, 40, 60, 3), 120, np.uint8)
    flat[2, 17:22, 30:35] += 80
    flat = _up(flat, dev)
    for s in (0, 1, 2):
        assert torch.equal(ops.denoise(flat, zero, zero, zeros(5), 8, s, 255), flat)


def test_arguments_are_checked(dev):
    c = C.case("soft_17x23")
    L, H, W = c["L"], c["H"], c["W"]
    fr, fwd, bwd, scene = _inputs(c, dev)
    good = dict(frames=fr, fwd=fwd, bwd=bwd, scene=scene, strength=8, search=1, max_change=255)
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(fwd=fwd[:1]), "fwd"), (dict(bwd=bwd[:, :5]), "bwd"), (dict(fwd=fwd.double()), "fwd"),
                     (dict(scene=scene[:-1]), "scene"), (dict(scene=scene.long()), "scene"),
                     (dict(strength=0), "strength"), (dict(strength=65), "strength"), (dict(strength=True), "strength"),
                     (dict(search=3), "search"), (dict(search=-1), "search"), (dict(search=1.5), "search"), (dict(search=False), "search"),
                     (dict(max_change=256), "max_change"), (dict(max_change=-1), "max_change"), (dict(max_change=True), "max_change"),
                     (dict(out=np.zeros((L, H, W, 3), np.uint8)), "out"),
                     (dict(out=torch.zeros((L, H, W), dtype=torch.uint8, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.denoise(**dict(good, **kw))
    # host inputs are uploaded
    got = ops.denoise(np.array(c["frames"]), np.array(c["fwd"]), np.array(c["bwd"]), C.scene_of_np(L), 8, 1, 255)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), C.want("soft_17x23", (8, 1, 255)))
    # an output that overlaps the frames is refused by the entry, before any launch -- the frames themselves too
    n = fr.numel()
    flat = torch.zeros(2 * n + 12, dtype=torch.uint8, device=dev)
    src = flat[:n].view(fr.shape).copy_(fr)
    for at in (0, 12, n - 1):
        with pytest.raises(lib.HipError, match="overlap"):
            ops.denoise(src, fwd, bwd, scene, 8, 1, 255, out=flat[at:at + n].view(fr.shape))
    behind = flat[n:2 * n].view(fr.shape)                              # right behind the frames: no overlap
    assert np.array_equal(ops.denoise(src, fwd, bwd, scene, 8, 1, 255, out=behind).cpu().numpy(), C.want("soft_17x23", (8, 1, 255)))
    assert np.array_equal(src.cpu().numpy(), c["frames"])
    # flows off an 8-byte boundary are refused by the entry, from the address alone
    odd = torch.zeros(fwd.numel() + 1, dtype=torch.float32, device=dev)[1:].view(fwd.shape).copy_(fwd)
    with pytest.raises(lib.HipError, match="aligned"):
        ops.denoise(fr, odd, bwd, scene, 8, 1, 255)
    # no frame and no pixel: results of the right shapes, nothing launched
    for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
        e = torch.zeros(shape, dtype=torch.uint8, device=dev)
        g = torch.zeros((max(shape[0] - 1, 0),) + shape[1:3] + (2,), dtype=torch.float32, device=dev)
        assert ops.denoise(e, g, g, torch.zeros(shape[0], dtype=torch.int32, device=dev), 8, 1, 255).shape == shape


# ------------------------------------------------------------------------------------------------ video.denoise
@pytest.mark.parametrize("name", ("soft_33x70", "cut2_17x23", "random_1x1", "soft_3x5", "edges_17x23", "nonfinite_17x23", "extremes_64x128"))
def test_video_denoise_is_the_entry(dev, name):
    c = C.case(name)
    host, flows = np.array(c["frames"]), (c["fwd"], c["bwd"])
    fr, fwd, bwd, scene = _inputs(c, dev)
    for setting in ((8, 1, 255), (64, 2, 3), (1, 0, 255)):
        kw = dict(zip(("strength", "search", "max_change"), setting))
        want = C.want(name, setting)
        assert np.array_equal(ops.denoise(fr, fwd, bwd, scene, *setting).cpu().numpy(), want)
        with launch_trace() as trace:
            out = video.denoise(None, host, flows=flows, scenes=c["scenes"], device=dev, **kw)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and np.array_equal(out, want), (name, setting)
        assert [r["symbol"] for r in trace] == [SYMBOL]
        # a device tensor is used where it is -- on, and one byte off a dword -- and a device tensor comes back; flows on the device
        for off in (0, 1):
            x = _up(c["frames"], dev, off)
            got = video.denoise(None, x, flows=(fwd, bwd), scenes=c["scenes"], **kw)
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
            assert np.array_equal(x.cpu().numpy(), c["frames"])
    assert np.array_equal(host, c["frames"])
    assert np.array_equal(video.denoise(None, host, flows=flows, scenes=c["scenes"], device=dev), C.want(name, (8, 1, 255)))    # the defaults


def test_no_work_launches_nothing(dev):
    c = C.case("soft_17x23")
    flows = (c["fwd"], c["bwd"])
    with launch_trace() as trace:
        for kw in (dict(max_change=0), dict(scenes=[1, 2])):
            out = video.denoise(None, np.array(c["frames"]), flows=flows, device=dev, **kw)
            assert isinstance(out, np.ndarray) and np.array_equal(out, c["frames"])
            x = _up(c["frames"], dev)
            on = video.denoise(None, x, flows=flows, **kw)
            assert on.is_cuda and on.data_ptr() != x.data_ptr() and torch.equal(on, x)
        for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
            g = np.zeros((max(shape[0] - 1, 0),) + shape[1:3] + (2,), np.float32)
            assert video.denoise(None, np.zeros(shape, np.uint8), flows=(g, g), device=dev).shape == shape
            on = video.denoise(None, torch.zeros(shape, dtype=torch.uint8, device=dev), flows=(g, g))
            assert on.is_cuda and tuple(on.shape) == shape
    assert not trace


def _net(dev, model="e2fgvi_hq"):
    """the generator with synthetic weights; e2fgvi_hq is the one that takes frames of any size"""
    if model not in _CACHE:
        from e2fgvi_amd.synth import synth_state_dict
        net = importlib.import_module("model." + model).InpaintGenerator()
        net.load_state_dict(synth_state_dict(model, "stress", 0))
        _CACHE[model] = net.to(dev).eval()
    return _CACHE[model]


def test_denoise_with_the_nets_flows(dev):
    """without flows= the call computes the net's own and is the call that is given them; with every frame alone it computes none"""
    net = _net(dev)
    frames = C.soft(5, 60, 108, 40)
    with torch.no_grad():
        fwd, bwd = metrics.video_flows(net, frames)
        got = video.denoise(net, frames, scenes=[3], strength=16)
        own = video.denoise(None, frames, flows=(fwd, bwd), scenes=[3], strength=16, device=dev)
    assert isinstance(got, np.ndarray) and got.shape == frames.shape and np.array_equal(got, own)
    want = C.reference(frames, fwd.cpu().numpy(), bwd.cpu().numpy(), C.scene_of_np(5, [3]), 16, 1, 255)
    print("bytes changed", int((got != frames).sum()), "finite flows", bool(torch.isfinite(fwd).all() and torch.isfinite(bwd).all()))
    assert np.array_equal(got, want)
    with launch_trace() as trace:
        assert np.array_equal(video.denoise(net, frames, scenes=[1, 2, 3, 4]), frames)
    assert not trace
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.denoise(lambda x, m: (x, None), frames, device=dev)
