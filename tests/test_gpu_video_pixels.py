"""Real pixels for restored holes on the device: ops.pixel_track_step and ops.pixel_fill (csrc/pixel_track.hip) and
video.propagate_pixels against the float64 numpy restatement of tests/pixel_track_cases.py -- ages and filled bytes equal, origins
bit for bit -- on every named case; the lockstep launches against one job per launch; paste_mask against what restore_frames
pastes; the flows of the net's own SPyNet; and the video without a hole, which launches nothing."""
import importlib

import numpy as np
import pytest
import torch

from e2fgvi_amd import metrics, ops, video
from tests import pixel_track_cases as P
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

_CACHE = {}


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.zeros(a.nbytes + shift, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _inputs(c, dev, shift=0):
    """(hole, age, origin, fwd, bwd) of a case on the device: hole and age `shift` bytes off an allocation's start, the origins
    filled with NaN as the restatement's"""
    hole = _up(c["hole"], dev, shift)
    age = _up(np.stack([c["hole"] * 255] * 2).astype(np.uint8), dev, shift)
    origin = torch.full((2, c["L"], c["H"], c["W"], 2), float("nan"), dtype=torch.float32, device=dev)
    return hole, age, origin, _up(c["fwd"], dev), _up(c["bwd"], dev)


def _jobs(jobs, dev):
    return torch.tensor(jobs, dtype=torch.int32).reshape(-1, 2).to(dev)


def _run(c, dev, tables, check=True, shift=0):
    hole, age, origin, fwd, bwd = _inputs(c, dev, shift)
    tables = [_jobs(t, dev) for t in tables]            # every table is on the device before the first launch
    for tb in tables:
        ops.pixel_track_step(hole, age, origin, fwd, bwd, tb, c.get("reach") or 254, check)
    return hole, age, origin


def _one_by_one(c, dev, check=True, shift=0):
    """the chains of the restatement's walk, one job per launch"""
    return _run(c, dev, [[j] for ch in P.chains_np(c["L"], c.get("scenes")) for j in ch], check, shift)


def _lockstep(c, dev, check=True, shift=0):
    return _run(c, dev, video.plan_pixel_chains(c["L"], c.get("scenes")), check, shift)


def _same_planes(age, origin, want_age, want_origin):
    got_age, got_origin = age.cpu().numpy(), origin.cpu().numpy()
    assert np.array_equal(got_age, want_age), int((got_age != want_age).sum())
    m = (want_age >= 1) & (want_age <= 254)
    a, b = got_origin[m].view(np.uint32), np.array(want_origin)[m].view(np.uint32)
    assert np.array_equal(a, b), int((a != b).sum())
    return int(m.sum())


def _propagate(c, dev, check=True, tensors=False, **kw):
    up = (lambda a: torch.from_numpy(np.array(a)).to(dev)) if tensors else np.array
    return video.propagate_pixels(None, up(c["src"]), up(P.masks_of(c)), up(c["filled"]), flows=(up(c["fwd"]), up(c["bwd"])),
                                  dilate=False, scenes=c.get("scenes"), reach=c.get("reach"), check=check, device=dev, **kw)


# ------------------------------------------------------------------------------------------------ the kernels and the driver
@pytest.mark.parametrize("name", P.NAMES)
def test_steps_fill_and_driver_are_the_reference(dev, name):
    c = P.case(name)
    want_out, want_source, want_age, want_origin = P.reference(name)
    for shift in (0, 1, 2):                             # hole and age 0, 1 and 2 bytes off a dword: whole words and single bytes
        hole, age, origin = _one_by_one(c, dev, True, shift)
        n = _same_planes(age, origin, want_age, want_origin)
        out = _up(c["filled"], dev, shift)
        got, source = ops.pixel_fill(_up(c["src"], dev), hole, age, origin, out, return_source=True)
        assert got is out and np.array_equal(got.cpu().numpy(), want_out), (shift, int((got.cpu().numpy() != want_out).sum()))
        assert np.array_equal(source.cpu().numpy(), want_source)
        plain = ops.pixel_fill(_up(c["src"], dev), hole, age, origin, _up(c["filled"], dev))
        assert torch.equal(plain, got)
    print("%s: %d reached (pixel, plane)s, sources %s" % (name, n, np.bincount(want_source.ravel(), minlength=4).tolist()))
    for tensors in (False, True):
        got, source = _propagate(c, dev, tensors=tensors, return_source=True)
        if tensors:
            assert isinstance(got, torch.Tensor) and got.is_cuda and source.is_cuda
            got, source = got.cpu().numpy(), source.cpu().numpy()
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want_out.shape
        assert np.array_equal(got, want_out) and np.array_equal(source, want_source)
        assert np.array_equal(_propagate(c, dev, tensors=False), want_out)


@pytest.mark.parametrize("name", ["smooth_70x90", "nonfinite_33x64", "ragged_9x13"])
def test_without_the_consistency_test(dev, name):
    c = P.case(name)
    want_out, want_source, want_age, want_origin = P.reference(name, False)
    hole, age, origin = _lockstep(c, dev, False)
    _same_planes(age, origin, want_age, want_origin)
    got, source = _propagate(c, dev, check=False, return_source=True)
    assert np.array_equal(got, want_out) and np.array_equal(source, want_source)


@pytest.mark.parametrize("name", P.NAMES)
def test_lockstep_launches_are_the_single_jobs(dev, name):
    c = P.case(name)
    _, a_age, a_origin = _lockstep(c, dev, shift=3)
    _, b_age, b_origin = _one_by_one(c, dev)
    assert torch.equal(a_age, b_age)
    assert torch.equal(a_origin.view(torch.int32), b_origin.view(torch.int32))     # NaN where nothing was stored, in both
    with launch_trace() as trace:
        _propagate(c, dev)
    steps = [r for r in trace if r["symbol"] == "e2fgvi_pixel_track_step"]
    scenes = np.diff([0] + list(c.get("scenes") or []) + [c["L"]])
    assert len(steps) == len(video.plan_pixel_chains(c["L"], c.get("scenes"))) == scenes.max() - 1
    assert len([r for r in trace if r["symbol"] == "e2fgvi_pixel_fill"]) == 1


def test_runs_are_the_same_bits(dev):
    c = P.case("smooth_70x90")
    _, a_age, a_origin = _lockstep(c, dev)
    _, b_age, b_origin = _lockstep(c, dev)
    a, sa = _propagate(c, dev, return_source=True)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _, s_age, s_origin = _lockstep(c, dev)
        b, sb = _propagate(c, dev, return_source=True)
    side.synchronize()
    for x, y in ((a_age, b_age), (a_age, s_age), (a_origin.view(torch.int32), b_origin.view(torch.int32)),
                 (a_origin.view(torch.int32), s_origin.view(torch.int32))):
        assert torch.equal(x, y)
    assert np.array_equal(a, b) and np.array_equal(sa, sb) and np.array_equal(a, P.reference("smooth_70x90")[0])


def test_jobs_outside_the_video_write_nothing_and_arguments_are_checked(dev):
    c = P.case("ragged_9x13")
    hole, age, origin, fwd, bwd = _inputs(c, dev)
    before = (age.clone(), origin.clone())
    assert ops.pixel_track_step(hole, age, origin, fwd, bwd, _jobs([(2, 0), (-1, 1), (0, 2), (1 << 20, 0)], dev))[0] is age
    ops.pixel_track_step(hole, age, origin, fwd, bwd, _jobs([], dev))              # no job: no launch
    assert torch.equal(age, before[0]) and torch.equal(origin.view(torch.int32), before[1].view(torch.int32))
    job = _jobs([(0, 0)], dev)
    # host arrays for what is only read
    ops.pixel_track_step(np.array(c["hole"]), age, origin, np.array(c["fwd"]), np.array(c["bwd"]), np.array([(0, 0)], np.int32))
    want = np.stack([c["hole"] * 255] * 2).astype(np.uint8)
    worg = np.full(origin.shape, np.nan, np.float32)
    P.step_np(c["hole"][1], want[0, 0], worg[0, 0], want[0, 1], worg[0, 1], c["bwd"][0], c["fwd"][0])
    _same_planes(age, origin, want, worg)
    for bad in (age.cpu(), age.cpu().numpy()):
        with pytest.raises(ValueError, match="age"):
            ops.pixel_track_step(hole, bad, origin, fwd, bwd, job)
    for bad in (age.int(), age[0], age[:, :1], age[..., ::2]):
        with pytest.raises(ValueError, match="age"):
            ops.pixel_track_step(hole, bad, origin, fwd, bwd, job)
    for bad in (hole.int(), hole[:2], hole[..., ::2]):
        with pytest.raises(ValueError, match="hole"):
            ops.pixel_track_step(bad, age, origin, fwd, bwd, job)
    for bad in (origin.double(), origin[0], origin[..., :1], origin.cpu()):
        with pytest.raises(ValueError, match="origin"):
            ops.pixel_track_step(hole, age, bad, fwd, bwd, job)
    for bad in (fwd.double(), fwd[:1], fwd[..., :1], fwd.transpose(1, 2)):
        with pytest.raises(ValueError, match="fwd"):
            ops.pixel_track_step(hole, age, origin, bad, bwd, job)
        with pytest.raises(ValueError, match="bwd"):
            ops.pixel_track_step(hole, age, origin, fwd, bad, job)
    for bad in (job.long(), job[0], _jobs([(0, 0)], dev).reshape(1, 2, 1)):
        with pytest.raises(ValueError, match="jobs"):
            ops.pixel_track_step(hole, age, origin, fwd, bwd, bad)
    for bad in (0, 255, True, 1.5, None):
        with pytest.raises(ValueError, match="reach"):
            ops.pixel_track_step(hole, age, origin, fwd, bwd, job, reach=bad)
    for bad in (2, -1, None, "on"):
        with pytest.raises(ValueError, match="check"):
            ops.pixel_track_step(hole, age, origin, fwd, bwd, job, check=bad)
    src, out = _up(c["src"], dev), _up(c["filled"], dev)
    with pytest.raises(ValueError, match="out"):
        ops.pixel_fill(src, hole, age, origin, out.cpu())
    with pytest.raises(ValueError, match="src"):
        ops.pixel_fill(out, hole, age, origin, out)
    for bad in (src[:2], src[..., :2], src.int()):
        with pytest.raises(ValueError, match="src"):
            ops.pixel_fill(bad, hole, age, origin, out)
    with pytest.raises(ValueError, match="age"):
        ops.pixel_fill(src, hole, age[0], origin, out)
    with pytest.raises(ValueError, match="origin"):
        ops.pixel_fill(src, hole, age, origin[0], out)


def test_a_candidate_outside_the_video_or_the_image_is_none(dev):
    """planes that no chain wrote: an age that points past the last frame or before the first, an origin outside the image or not
    finite, and an age of 0 at a hole pixel -- each is just no candidate, and the pixel keeps its bytes"""
    c = P.case("ragged_9x13")
    L, H, W = c["L"], c["H"], c["W"]
    hole = np.zeros((L, H, W), np.uint8)
    hole[1, 2:6, 3:9] = 1
    age = np.zeros((2, L, H, W), np.uint8)
    origin = np.zeros((2, L, H, W, 2), np.float32)
    age[0, 1, 2:6, 3:9], age[1, 1, 2:6, 3:9] = 2, 2                                # frames -1 and 3
    age[0, 1, 3, 3:9] = 1
    origin[0, 1, 3, 3:9] = [(-0.25, 1.0), (3.0, float(H)), (np.nan, 1.0), (1.0, np.inf), (1e30, 1.0), (float(W - 1), float(H - 1))]
    age[1, 1, 4, 3:9] = 0                                                           # its own origin: a hole pixel
    cc = dict(c, hole=hole)
    want_out, want_source = P.fill_np(cc, age, origin)
    got, source = ops.pixel_fill(_up(c["src"], dev), _up(hole, dev), _up(age, dev), _up(origin, dev), _up(c["filled"], dev), True)
    assert np.array_equal(got.cpu().numpy(), want_out) and np.array_equal(source.cpu().numpy(), want_source)
    assert (want_source[hole == 1] == 3).sum() == 23 and want_source[1, 3, 8] == 1


# ------------------------------------------------------------------------------------------------ paste_mask
def test_paste_mask_is_what_restore_frames_pastes(dev):
    L, H, W, size = 3, 70, 101, (36, 22)                # neither 101 / 36 nor 70 / 22 is whole
    rng = np.random.RandomState(5)
    masks = np.zeros((L, 50, 61), np.uint8)             # masks of a third size
    masks[0, 8:30, 10:33], masks[1, 20:44, 25:50], masks[2, 3:20, 30:58] = 1, 77, 255
    masks[2][rng.rand(50, 61) < 0.02] = 9
    for dilate in (True, False):
        pm = video.paste_mask(masks, (H, W), size, dilate, device=dev)
        assert pm.is_cuda and pm.dtype == torch.uint8 and tuple(pm.shape) == (L, H, W) and pm.is_contiguous()
        m01 = video.prepare_masks(masks, (size[1], size[0]), dev, dilate)
        lo = torch.full((L, size[1], size[0], 3), 7, dtype=torch.uint8, device=dev)
        src = torch.full((L, H, W, 3), 200, dtype=torch.uint8, device=dev)
        pasted = video.restore_frames(lo, m01, src)
        assert set(np.unique(pasted.cpu().numpy()).tolist()) == {7, 200}
        assert torch.equal(pm, (pasted[..., 0] == 7).to(torch.uint8)) and torch.equal(pm, (pasted[..., 2] != 200).to(torch.uint8))
        assert 0 < int(pm.sum()) < pm.numel()
        same = video.paste_mask(torch.from_numpy(masks).to(dev), (H, W), None, dilate)
        assert torch.equal(same, video.prepare_masks(masks, (H, W), dev, dilate))


def test_the_two_line_composition_after_inpaint_video(dev):
    """out = inpaint_video(..., size=, restore=True); out = propagate_pixels(..., out, size=): an object that moves over a still
    background.  What the restore left alone is paste_mask's complement, and what is fetched is the background to the byte."""
    from tests.test_gpu_video_restore import _stand_in_model
    L, H, W, size = 6, 120, 216, (108, 60)
    rng = np.random.RandomState(216)
    background = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    frames = np.repeat(background[None], L, 0)
    masks = np.zeros((L, H, W), np.uint8)
    for t in range(L):
        masks[t, 40:60, 30 + 24 * t:60 + 24 * t] = 255
    frames[masks != 0] = 0                              # the object
    stub = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    filled = video.inpaint_video(stub, frames, masks, size=size, restore=True, device=dev)
    flows = (np.zeros((L - 1, H, W, 2), np.float32),) * 2               # the completed frames stand still
    out, source = video.propagate_pixels(None, frames, masks, filled, flows=flows, size=size, return_source=True, device=dev)
    hole = video.paste_mask(masks, (H, W), size, device=dev).cpu().numpy() == 1
    assert hole[masks != 0].all() and hole.sum() > (masks != 0).sum()             # the object and the dilation around it
    assert np.array_equal(filled[~hole], frames[~hole]) and (filled[hole] != frames[hole]).any()
    assert np.array_equal(out[~hole], frames[~hole]) and np.array_equal(source != 0, hole)
    got = (source == 1) | (source == 2)
    truth = np.repeat(background[None], L, 0)
    assert got[hole].mean() > 0.9 and np.array_equal(out[got], truth[got]) and (filled[got] != truth[got]).any()
    assert np.array_equal(out[source == 3], filled[source == 3])


# ------------------------------------------------------------------------------------------------ the net's own flows
def _net(dev, model="e2fgvi"):
    if model not in _CACHE:
        from e2fgvi_amd.synth import synth_state_dict
        net = importlib.import_module("model." + model).InpaintGenerator()
        net.load_state_dict(synth_state_dict(model, "stress", 0))
        _CACHE[model] = net.to(dev).eval()
    return _CACHE[model]


def test_the_nets_flows_are_those_of_the_completed_frames(dev):
    from e2fgvi_amd.synth import synth_clip
    net = _net(dev)
    L, H, W = 5, 64, 96
    x, _ = synth_clip(1, L, H, W, seed=4, moving=True)
    filled = ((x[0] * 0.5 + 0.5) * 255).round().clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()
    masks = np.zeros((L, 32, 48), np.uint8)
    for t in range(L):
        masks[t, 8 + t:18 + t, 10 + 2 * t:24 + 2 * t] = 255
    frames = filled.copy()
    frames[np.repeat(np.repeat(masks, 2, 1), 2, 2) != 0] = 0                       # the unwanted object, in the caller's frames only
    kw = dict(size=(48, 32))
    with torch.no_grad():
        flows = metrics.video_flows(net, filled)
        got, source = video.propagate_pixels(net, frames, masks, filled, return_source=True, **kw)
        want, wsource = video.propagate_pixels(None, frames, masks, filled, flows=flows, return_source=True, **kw)
    assert np.array_equal(got, want) and np.array_equal(source, wsource)
    hole = video.paste_mask(masks, (H, W), (48, 32), device=dev).cpu().numpy() == 1
    assert hole.any() and np.array_equal(source != 0, hole)
    keep = ~hole | (source == 3)
    assert np.array_equal(got[keep], filled[keep])
    print("sources", np.bincount(source.ravel(), minlength=4).tolist())
    with torch.no_grad():                               # and without the consistency test, which these flows rarely pass
        got, source = video.propagate_pixels(net, frames, masks, filled, check=False, return_source=True, **kw)
        want, wsource = video.propagate_pixels(None, frames, masks, filled, flows=flows, check=False, return_source=True, **kw)
    assert np.array_equal(got, want) and np.array_equal(source, wsource)
    keep = ~hole | (source == 3)
    assert np.array_equal(got[keep], filled[keep])
    print("sources without the test", np.bincount(source.ravel(), minlength=4).tolist())
    assert ((source == 1) | (source == 2)).any()
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.propagate_pixels(lambda x, n: (x, None), frames, masks, filled, device=dev, **kw)


def test_a_video_without_a_hole_launches_nothing(dev, monkeypatch):
    def launched(*a, **k):
        raise AssertionError("a launch for a video without a hole")
    monkeypatch.setattr(ops, "pixel_track_step", launched)
    monkeypatch.setattr(ops, "pixel_fill", launched)
    c = P.case("smooth_70x90")
    flows = (np.array(c["fwd"]), np.array(c["bwd"]))
    none = np.zeros_like(c["hole"])
    got, source = video.propagate_pixels(None, np.array(c["src"]), none, np.array(c["filled"]), flows=flows, dilate=False,
                                         return_source=True, device=dev)
    assert np.array_equal(got, c["filled"]) and not source.any() and source.shape == none.shape
    filled_d = torch.from_numpy(np.array(c["filled"])).to(dev)
    got = video.propagate_pixels(None, np.array(c["src"]), none, filled_d, flows=flows)
    assert isinstance(got, torch.Tensor) and got.is_cuda and torch.equal(got, filled_d) and got.data_ptr() != filled_d.data_ptr()
    # a single frame: nothing to fetch from, hole or not
    got, source = video.propagate_pixels(None, np.array(c["src"][:1]), P.masks_of(c)[:1], np.array(c["filled"][:1]),
                                         flows=(flows[0][:0], flows[1][:0]), dilate=False, return_source=True, device=dev)
    assert np.array_equal(got, c["filled"][:1]) and np.array_equal(source, 3 * c["hole"][:1]) and source.any()
