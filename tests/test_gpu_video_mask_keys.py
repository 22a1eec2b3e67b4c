"""Masks from keyframes on the device: ops.mask_track_step (csrc/mask_track.hip) and video.propagate_masks against the float64 numpy
restatement of tests/mask_key_cases.py, every byte equal, on every named case with the consistency test on and off; the lockstep
launches against one job per launch; the flows of the net's own SPyNet; size=; and inpaint_video(mask_keys=) against the two-step
call, byte for byte."""
import importlib

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, metrics, ops, video
from tests import mask_key_cases as K
from tests.test_gpu_video_restore import _stand_in_model
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

_CACHE = {}


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.zeros(a.nbytes + shift, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _planes(c, dev, shift=0):
    p = np.zeros((2, c["L"], c["H"], c["W"]), np.uint8)
    p[:, list(c["keys"])] = K.binarise(c["key_masks"])
    return _up(p, dev, shift)


def _flows(c, dev):
    return _up(c["fwd"], dev), _up(c["bwd"], dev)


def _jobs(jobs, dev):
    return torch.tensor(jobs, dtype=torch.int32).to(dev)


def _one_by_one(c, dev, check=True, shift=0, flows=None):
    """the chains of the restatement's walk, one job per launch -> the planes"""
    planes = _planes(c, dev, shift)
    fwd, bwd = flows if flows is not None else _flows(c, dev)
    tables = [_jobs([j], dev) for ch in K.chains_np(c["L"], c["keys"], c.get("scenes"), c.get("reach")) for j in ch]
    for tb in tables:
        ops.mask_track_step(planes, fwd, bwd, tb, check)
    return planes, len(tables)


def _lockstep(c, dev, check=True, shift=0):
    planes = _planes(c, dev, shift)
    fwd, bwd = _flows(c, dev)
    steps = video.plan_mask_chains(c["L"], c["keys"], c.get("scenes"), c.get("reach"))
    for tb in [_jobs(s, dev) for s in steps]:
        ops.mask_track_step(planes, fwd, bwd, tb, check)
    return planes, len(steps)


def _propagate(c, dev, check=True, **kw):
    flows = (np.array(c["fwd"]), np.array(c["bwd"]))    # writable copies: the cases are read-only
    return video.propagate_masks(None, K.frames_of(c), np.array(c["key_masks"]), c["keys"], flows=flows, scenes=c.get("scenes"),
                                 reach=c.get("reach"), check=check, device=dev, **kw)


# ------------------------------------------------------------------------------------------------ the step and the chains
@pytest.mark.parametrize("check", [True, False], ids=["check", "nocheck"])
@pytest.mark.parametrize("name", K.NAMES)
def test_step_and_propagation_are_the_reference(dev, name, check):
    c = K.case(name)
    want_planes, records = K.planes_np(c, check)
    want = K.reference(name, check)[0]
    assert np.array_equal(want, want_planes[0] | want_planes[1])
    for shift in (0, 1, 2):                             # the planes 0, 1 and 2 bytes off a dword: whole words and single bytes
        planes, n = _one_by_one(c, dev, check, shift)
        got = planes.cpu().numpy()
        assert n == len(records) and np.array_equal(got, want_planes), (shift, int((got != want_planes).sum()))
    got = _propagate(c, dev, check)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), int((got != want).sum())
    assert set(np.unique(got).tolist()) <= {0, 1}
    for k, m in zip(c["keys"], K.binarise(c["key_masks"])):
        assert np.array_equal(got[k], m)


@pytest.mark.parametrize("name", K.NAMES)
def test_lockstep_launches_are_the_single_jobs(dev, name):
    c = K.case(name)
    for check in (True, False):
        a, launches = _lockstep(c, dev, check, shift=3)
        b, jobs = _one_by_one(c, dev, check)
        assert torch.equal(a, b)
        assert launches == max(len(ch) for ch in K.chains_np(c["L"], c["keys"], c.get("scenes"), c.get("reach"))) <= jobs
    if name == "smooth_70x90":
        assert (launches, jobs) == (2, 4)               # 0 -> 1 -> 2 and 4 -> 3 -> 2; nothing leaves key 5 across the cut


def test_runs_are_the_same_bits(dev):
    c = K.case("smooth_70x90")
    a, _ = _lockstep(c, dev)
    b, _ = _lockstep(c, dev)
    ma = _propagate(c, dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s, _ = _lockstep(c, dev)
        ms = _propagate(c, dev)
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, s) and np.array_equal(ma, ms)
    assert np.array_equal(ma, K.reference("smooth_70x90")[0]) and np.array_equal(ma, (a[0] | a[1]).cpu().numpy())


def test_non_finite_flows_give_zeros(dev):
    """a pull flow that is nan, inf or 1e30 excludes its pixel whatever the source mask holds; a check flow that is not finite
    excludes every pixel that samples it -- and a source mask of ones changes nothing under excluded pixels"""
    L, H, W = 2, 19, 23
    job = _jobs([(0, 0)], dev)
    for value in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        bad = np.full((L - 1, H, W, 2), value, np.float32)
        zero = np.zeros_like(bad)
        for g, cflow, check in ((bad, zero, True), (bad, zero, False), (zero, bad, True)):
            planes = torch.ones((2, L, H, W), dtype=torch.uint8, device=dev)
            ops.mask_track_step(planes, _up(cflow, dev), _up(g, dev), job, check)
            # (1e30 as the check flow is finite: inconsistent, which gives zero as well)
            assert not planes[0, 1].any() and planes[0, 0].all() and planes[1].all(), (value, check)
    c = K.case("nonfinite_33x64")
    g = c["bwd"][0].astype(np.float64)                  # the pull flow of the job (0, 0)
    excluded = ~np.isfinite(g).all(-1)
    assert 20 < excluded.sum() < excluded.size // 4
    fwd, bwd = _flows(c, dev)
    outs = []
    for fill in (0, 1):
        planes = _planes(c, dev)
        planes[0, 0] = fill
        ops.mask_track_step(planes, fwd, bwd, _jobs([(0, 0)], dev), True)
        outs.append(planes[0, 1].cpu().numpy())
        assert not outs[-1][excluded].any()
    assert not outs[0].any() and outs[1].any()


def test_host_inputs_are_uploaded_and_arguments_checked(dev):
    c = K.case("tie_9x13")
    p = np.zeros((2, c["L"], c["H"], c["W"]), np.uint8)
    p[:, c["keys"]] = K.binarise(c["key_masks"])
    want, _ = K.planes_np(c)
    got = ops.mask_track_step(p, np.array(c["fwd"]), np.array(c["bwd"]), np.array([(1, 0)], np.int32))
    assert isinstance(got, torch.Tensor) and got.is_cuda and np.array_equal(got[0, 2].cpu().numpy(), want[0, 2])
    planes, (fwd, bwd), job = _planes(c, dev), _flows(c, dev), _jobs([(1, 0)], dev)
    assert ops.mask_track_step(planes, fwd, bwd, job) is planes and np.array_equal(planes.cpu().numpy()[0, 2], want[0, 2])
    assert ops.mask_track_step(planes, fwd, bwd, job[:0]) is planes                       # no job: no launch
    # jobs outside the video write nothing
    before = planes.clone()
    ops.mask_track_step(planes, fwd, bwd, _jobs([(2, 0), (-1, 1), (0, 2), (1 << 20, 0)], dev))
    assert torch.equal(planes, before)
    for bad in (planes.int(), planes[0], planes[:, :1], planes[:, :, :, ::2], planes.float()):
        with pytest.raises(ValueError, match="planes"):
            ops.mask_track_step(bad, fwd, bwd, job)
    for bad in (fwd.double(), fwd[:1], fwd[..., :1], fwd.transpose(1, 2)):
        with pytest.raises(ValueError, match="fwd"):
            ops.mask_track_step(planes, bad, bwd, job)
        with pytest.raises(ValueError, match="bwd"):
            ops.mask_track_step(planes, fwd, bad, job)
    for bad in (job.long(), job[0], job.float(), _jobs([(0, 0, 0)], dev)):
        with pytest.raises(ValueError, match="jobs"):
            ops.mask_track_step(planes, fwd, bwd, bad)
    for bad in (2, -1, None, "on", 0.5):
        with pytest.raises(ValueError, match="check"):
            ops.mask_track_step(planes, fwd, bwd, job, bad)
    # device tensors for frames, masks and flows
    got = video.propagate_masks(None, torch.from_numpy(K.frames_of(c)).to(dev), torch.from_numpy(np.array(c["key_masks"])).to(dev),
                                c["keys"], flows=(fwd, bwd))
    assert np.array_equal(got, K.reference("tie_9x13")[0])
    one = video.propagate_masks(None, K.frames_of(c)[:1], np.array(c["key_masks"][:1]), [0], flows=(fwd[:0], bwd[:0]), device=dev)
    assert np.array_equal(one, K.binarise(c["key_masks"])[:1])                            # a single frame: its key mask, no launch


# ------------------------------------------------------------------------------------------------ the net's own flows
def _net(dev, model="e2fgvi"):
    """the generator with synthetic weights; e2fgvi_hq is the one that takes frames of any size"""
    if model not in _CACHE:
        from e2fgvi_amd.synth import synth_state_dict
        net = importlib.import_module("model." + model).InpaintGenerator()
        net.load_state_dict(synth_state_dict(model, "stress", 0))
        _CACHE[model] = net.to(dev).eval()
    return _CACHE[model]


def _clip(L, H, W, seed):
    from e2fgvi_amd.synth import synth_clip
    x, _ = synth_clip(1, L, H, W, seed=seed, moving=True)
    return ((x[0] * 0.5 + 0.5) * 255).round().clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()


def _key_masks(K_, H, W):
    m = np.zeros((K_, H, W), np.uint8)
    for k in range(K_):
        y, x = H // 5 + 3 * k, W // 6 + 7 * k
        m[k, y:y + H // 3, x:x + W // 4] = 255
    return m


NET_SEED = 4                   # of the clip; a seed whose flows leave too little to compare is changed, the cap below stays


def test_propagate_masks_with_the_nets_flows(dev):
    """L = 6 at 40 x 72 on the synthetic-weights generator: propagate_masks(net, ...) is, bit for bit, the test's own chain over
    metrics.video_flows(net, frames); the numpy restatement on the downloaded flows agrees with each chain up to the first step whose
    margin is below 1e-9 (from there a last-bit difference may flip a pixel that later steps carry on), and that rule may leave out
    at most a quarter of all steps"""
    net = _net(dev)
    frames = _clip(6, 40, 72, NET_SEED)
    keys, km = [0, 3], _key_masks(2, 40, 72)
    with torch.no_grad():
        fwd, bwd = metrics.video_flows(net, frames)
        got = video.propagate_masks(net, frames, km, keys)
    c = dict(L=6, H=40, W=72, fwd=fwd.cpu().numpy(), bwd=bwd.cpu().numpy(), keys=keys, key_masks=km)
    planes, n = _one_by_one(c, dev, flows=(fwd, bwd))
    own = planes.cpu().numpy()
    assert got.shape == (6, 40, 72) and got.dtype == np.uint8 and np.array_equal(got, own[0] | own[1])
    assert np.array_equal(got[0], km[0] // 255) and np.array_equal(got[3], km[1] // 255)
    want, records = K.planes_np(c)
    assert n == len(records) == 6
    compared, broken = 0, set()
    for t, d, i, margin, cand in records:
        chain = (d, [k for k in keys if (k <= t if d == 0 else k > t)][-1 if d == 0 else 0])
        print("pair %d dir %d step %d of its chain: margin %.3e over %d candidates" % (t, d, i, margin, cand))
        if margin < 1e-9:
            broken.add(chain)
        if chain in broken:
            continue
        f = t + 1 if d == 0 else t
        assert np.array_equal(own[d, f], want[d, f]), (t, d, int((own[d, f] != want[d, f]).sum()))
        compared += 1
    print("compared %d of %d steps" % (compared, len(records)))
    assert 4 * (len(records) - compared) <= len(records)
    # without the test nothing hangs on a comparison of rounded sums: s is a sum of exact products, every step is compared
    with torch.no_grad():
        loose = video.propagate_masks(net, frames, km, keys, check=False)
    want, _ = K.propagate_np(c, check=False)
    print("pixels per frame with the test %s, without %s" % (got.reshape(6, -1).sum(1).tolist(), loose.reshape(6, -1).sum(1).tolist()))
    assert np.array_equal(loose, want) and all(loose[t].any() for t in (0, 3))
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.propagate_masks(lambda x, n: (x, None), frames, km, keys, device=dev)


def test_size_is_the_manual_composition(dev):
    c = K.case("smooth_70x90")
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, (c["L"], 100, 140, 3)).astype(np.uint8)
    km = np.zeros((3, 50, 61), np.uint8)                # masks of a third size
    km[0, 8:30, 10:33], km[1, 20:44, 25:50], km[2, 3:20, 30:58] = 1, 77, 255
    kw = dict(flows=(np.array(c["fwd"]), np.array(c["bwd"])), scenes=c["scenes"], reach=c["reach"], device=dev)
    got = video.propagate_masks(None, frames, km, c["keys"], size=(90, 70), **kw)
    small = video.resize_frames(frames, (90, 70), device=dev)
    masks = video.prepare_masks(km, (70, 90), dev, dilate=False)
    want = video.propagate_masks(None, small, masks, c["keys"], **kw)
    assert got.shape == (c["L"], 70, 90) and np.array_equal(got, want) and got[1].any() and got[2].any()
    ref, _ = K.propagate_np(dict(c, key_masks=masks.cpu().numpy()))
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------------ the driver
def test_inpaint_video_mask_keys_is_the_two_step_call(dev):
    net = _net(dev, "e2fgvi_hq")
    frames = _clip(6, 120, 216, 5)
    keys, km = [1, 4], _key_masks(2, 120, 216)
    kw = dict(size=(108, 60), restore=True)
    with torch.no_grad():
        masks = video.propagate_masks(net, frames, km, keys, size=(108, 60))
        assert masks.shape == (6, 60, 108) and all(masks[t].any() for t in (1, 4))
        want = video.inpaint_video(net, frames, masks, **kw)
        got = video.inpaint_video(net, frames, km, mask_keys=keys, **kw)
        assert got.shape == frames.shape and got.dtype == np.uint8 and np.array_equal(got, want), int((got != want).sum())
        assert (got != frames).any()
        # a cut and 4:2:0 frames: the masks are made on the decoded frames with the cut respected
        yuv = video.rgb_to_yuv420(frames, "nv12", device=dev)
        rgb = video.yuv420_to_rgb(yuv, "nv12", device=dev)
        kw = dict(kw, scenes=[3], pixel_format="nv12")
        masks = video.propagate_masks(net, rgb, km, keys, size=(108, 60), scenes=[3])
        want = video.inpaint_video(net, yuv, masks, **kw)
        got = video.inpaint_video(net, yuv, km, mask_keys=keys, **kw)
        assert got.shape == yuv.shape and np.array_equal(got, want), int((got != want).sum())
        # without size the masks are made at the frames' own size
        small = _clip(6, 60, 108, 6)
        km = _key_masks(2, 60, 108)
        masks = video.propagate_masks(net, small, km, keys)
        assert np.array_equal(video.inpaint_video(net, small, km, mask_keys=keys), video.inpaint_video(net, small, masks))


def test_without_mask_keys_no_launch_is_added(dev):
    """mask_keys=None: the launches and the bytes of a call without the argument; with keys, one launch per step of the plan"""
    f = _clip(6, 60, 108, 7)
    m = np.zeros((6, 60, 108), np.uint8)
    m[:, 20:40, 30:70] = 1
    stub = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    with launch_trace() as plain:
        a = video.inpaint_video(stub, f, m, device=dev)
    with launch_trace() as none:
        b = video.inpaint_video(stub, f, m, device=dev, mask_keys=None)
    assert np.array_equal(a, b) and [r["symbol"] for r in plain] == [r["symbol"] for r in none] and len(plain) > 0
    assert not any(r["symbol"] == "e2fgvi_mask_track_step" for r in none)
    c = K.case("smooth_70x90")
    with launch_trace() as trace:
        _propagate(c, dev)
    steps = [r for r in trace if r["symbol"] == "e2fgvi_mask_track_step"]
    assert len(steps) == len(video.plan_mask_chains(c["L"], c["keys"], c["scenes"], c["reach"])) == 2
