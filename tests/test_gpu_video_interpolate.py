"""Frame interpolation on the device: ops.interpolate (csrc/interpolate.hip), video.retime and video.replace_frames against the
numpy restatement of tests/interpolate_cases.py, every byte of the frames and of the source codes equal, on every named case at
every setting; buffers off their alignment; reruns; jobs launched in slabs; a frames buffer past 2^32 bytes; jobs outside their
ranges; the net's own flows."""
import importlib

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, metrics, ops, video
from tests import big_video as B
from tests import interpolate_cases as C
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

SYMBOL = "e2fgvi_interpolate"
_CACHE = {}


def _up(a, dev, shift=0, fill=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.full((a.nbytes + shift,), fill, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _inputs(c, dev, shift=0):
    """(frames, fwd, bwd, jobs) of a case on the device; the frames `shift` bytes off an allocation's start"""
    return _up(c["frames"], dev, shift), _up(c["fwd"], dev), _up(c["bwd"], dev), _up(c["jobs"], dev)


def _same(got, want, what):
    for g, w, part in zip(got, want, ("out", "source")):
        g = g.cpu().numpy()
        assert g.dtype == np.uint8 and g.shape == w.shape, (what, part, g.shape, w.shape)
        assert np.array_equal(g, w), (what, part, int((g != w).sum()))


# ------------------------------------------------------------------------------------------------ the entry
@pytest.mark.parametrize("name", C.NAMES)
def test_entry_is_the_restatement(dev, name):
    """the frames and the source codes on every named case -- frames of 1 x 1 to 64 x 128, rows that are no multiple of four pixels,
    more than one workgroup, two to five frames, jobs over adjacent and non-adjacent frames and over a frame with itself, the
    fractions 0/1, 1/1, 1/2, 1/3, 2/3, 1/64, 63/64 and 32/64, flows that are zero, on exact halves and sixteenths, ending on the
    last row and column and just outside, of -0.5, random ones of +-6 px, a step edge, non-finite ones and 1e30, bytes of 0 and 255
    alone -- at iterations 0, 1, 3 and 8, tolerance 0, 8 and 255 and match 0, 96 and 765, with the frames on, and one, two and
    three bytes off an allocation's start, and into out and source buffers that were full of something else: every byte is
    written"""
    c = C.case(name)
    for shift, fill in ((0, None), (1, 77), (2, None), (3, 255)):
        fr, fwd, bwd, jobs = _inputs(c, dev, shift)
        for setting in C.SETTINGS:
            want = C.want(name, setting)
            if fill is None:
                got = ops.interpolate(fr, fwd, bwd, jobs, *setting, source=True)
            else:
                ob, sb = _up(np.full(want[0].shape, fill, np.uint8), dev, shift), _up(np.full(want[1].shape, fill, np.uint8), dev, shift)
                got = ops.interpolate(fr, fwd, bwd, jobs, *setting, out=ob, source=sb)
                assert got[0].data_ptr() == ob.data_ptr() and got[1].data_ptr() == sb.data_ptr()
            _same(got, want, (name, shift, fill, setting))
            alone = ops.interpolate(fr, fwd, bwd, jobs, *setting)               # without source: the frames alone
            assert isinstance(alone, torch.Tensor) and np.array_equal(alone.cpu().numpy(), want[0])
        for t, key in ((fr, "frames"), (fwd, "fwd"), (bwd, "bwd"), (jobs, "jobs")):     # the inputs are only read
            assert np.array_equal(t.cpu().numpy(), c[key], equal_nan=key in ("fwd", "bwd")), key


def test_runs_are_the_same_bits(dev):
    for name in ("smooth_33x70", "random_64x128", "nonfinite_17x23", "occlusion_64x128"):
        fr, fwd, bwd, jobs = _inputs(C.case(name), dev)
        run = lambda: [t.cpu().numpy().tobytes() for s in ((3, 8, 96), (8, 255, 765)) for t in ops.interpolate(fr, fwd, bwd, jobs, *s, source=True)]
        first = run()
        for _ in range(5):
            assert run() == first


def test_more_jobs_than_a_launch_takes(dev):
    """65 537 jobs on frames of 2 x 2: the jobs ride on the grid's y axis and are launched in slabs of 65 535.  The table repeats
    with a period of 7, which does not divide the slab, so the second slab starts in the middle of a period."""
    rng = np.random.RandomState(80)
    fr = rng.randint(0, 256, (3, 2, 2, 3)).astype(np.uint8)
    fwd = (rng.randint(-8, 9, (2, 2, 2, 2)) / 16.0).astype(np.float32)
    period = [(0, 1, 0, 1, 2), (1, 2, 1, 1, 3), (2, 0, 0, 0, 5), (0, 2, 1, 63, 64), (1, 1, 0, 2, 3), (2, 1, 1, 7, 7), (0, 1, 1, 32, 64)]
    n = 65537
    jobs = np.asarray([period[j % 7] for j in range(n)], np.int32)
    wo, ws = C.reference(fr, fwd, -fwd, period, 3, 8, 765)
    assert len({wo[j].tobytes() for j in range(7)}) == 7                # a job run in another's place would show
    got = ops.interpolate(_up(fr, dev), _up(fwd, dev), _up(-fwd, dev), _up(jobs, dev), 3, 8, 765, source=True)
    B.assert_tiled(got[0], wo, "out")
    B.assert_tiled(got[1], ws, "source")


def test_frames_past_4gib(dev):
    """a frames buffer of more than 2^32 bytes: the clip of pan_64x128 repeated, every tile's jobs on its own frames; the frames a
    32-bit offset would fetch are others (big_video.wrap_is_visible), and every tile of the result is the restatement's"""
    c = C.case("pan_64x128")
    rows = np.asarray([(0, 1, 0, 0, 1), (1, 2, 1, 1, 2), (2, 3, 2, 1, 3), (0, 3, 0, 4, 4)], np.int64)   # two copies, a half and a third
    want = C.reference(c["frames"], c["fwd"], c["bwd"], rows, *C.DEFAULT)
    assert len({want[0][j].tobytes() for j in range(4)}) == 4
    with B.measured("interpolate", dev):
        k, tile = c["L"], B.nbytes(c["frames"])
        n = B.tiles_past(tile)
        fr = B.tiled(c["frames"], n, dev)
        B.wrap_is_visible(fr, tile, "interpolate frames")
        assert B.WRAP % B.nbytes(c["frames"][:1]) != 0
        jobs = np.tile(rows, (n, 1))
        jobs[:, :2] += k * np.repeat(np.arange(n), len(rows))[:, None]
        assert jobs[:, :2].max() == fr.shape[0] - 1 and int(jobs[-1, 0]) * (tile // k) > B.WRAP
        print("interpolate L", fr.shape[0], "jobs", len(jobs), "bytes", fr.numel())
        out, src = ops.interpolate(fr, _up(c["fwd"], dev), _up(c["bwd"], dev), torch.from_numpy(jobs.astype(np.int32)).to(dev),
                                   *C.DEFAULT, source=True)
        B.assert_tiled(out, want[0], "interpolate out")
        B.assert_tiled(src, want[1], "interpolate source")
        B.assert_tiled(fr, c["frames"], "interpolate frames")


def test_jobs_outside_their_ranges_write_nothing(dev):
    c = C.case("pan_17x23")
    L, P = c["L"], c["P"]
    fr, fwd, bwd, _ = _inputs(c, dev)
    good = [(0, 1, 0, 1, 2), (1, 1, 0, 0, 1), (2, 3, P - 1, 2, 3)]
    bad = [(-1, 1, 0, 1, 2), (0, L, 0, 1, 2), (L, 0, 0, 0, 1), (0, -1, 0, 1, 1), (0, 1, -1, 1, 2), (0, 1, P, 1, 2), (0, 1, P, 0, 1),
           (0, 1, 0, 1, 0), (0, 1, 0, 0, 0), (0, 1, 0, 1, 65), (0, 1, 0, 65, 65), (0, 1, 0, 0, -1), (0, 1, 0, -1, 2), (0, 1, 0, 3, 2),
           (2 ** 31 - 1, 0, 0, 1, 2), (0, 1, -2 ** 31, 1, 2), (0, 1, 0, 2 ** 31 - 1, 2 ** 31 - 1)]
    rows = np.asarray([good[0]] + bad[:9] + [good[1]] + bad[9:] + [good[2]], np.int32)
    pre_o = np.random.RandomState(81).randint(0, 256, (len(rows), c["H"], c["W"], 3)).astype(np.uint8)
    pre_s = np.random.RandomState(82).randint(6, 256, (len(rows), c["H"], c["W"])).astype(np.uint8)
    want = C.reference(c["frames"], c["fwd"], c["bwd"], rows, *C.DEFAULT, out=pre_o, source=pre_s)
    kept = [j for j, r in enumerate(rows.tolist()) if tuple(r) in bad]
    assert len(kept) == len(bad) and all(np.array_equal(want[0][j], pre_o[j]) and np.array_equal(want[1][j], pre_s[j]) for j in kept)
    got = ops.interpolate(fr, fwd, bwd, _up(rows, dev), *C.DEFAULT, out=_up(pre_o, dev), source=_up(pre_s, dev))
    _same(got, want, "ranges")
    # the same table on the host is refused before any launch
    with launch_trace() as trace:
        for r in bad:
            with pytest.raises(ValueError, match="jobs"):
                ops.interpolate(fr, fwd, bwd, np.asarray([good[0], r], np.int32), *C.DEFAULT)
    assert not trace


def test_arguments_are_checked(dev):
    c = C.case("pan_17x23")
    H, W, n = c["H"], c["W"], len(c["jobs"])
    fr, fwd, bwd, jobs = _inputs(c, dev)
    good = dict(frames=fr, fwd=fwd, bwd=bwd, jobs=jobs, iterations=3, tolerance=8, match=96)
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(fwd=fwd[:, :5]), "fwd"), (dict(bwd=bwd[:1]), "bwd"), (dict(fwd=fwd.double()), "fwd"), (dict(bwd=bwd[0]), "bwd"),
                     (dict(jobs=jobs[:, :4]), "contiguous"), (dict(jobs=jobs[:, :4].contiguous()), "jobs"), (dict(jobs=jobs.long()), "jobs"),
                     (dict(iterations=9), "iterations"), (dict(iterations=-1), "iterations"), (dict(iterations=True), "iterations"),
                     (dict(tolerance=256), "tolerance"), (dict(tolerance=-1), "tolerance"), (dict(tolerance=1.5), "tolerance"),
                     (dict(match=766), "match"), (dict(match=-1), "match"), (dict(match=False), "match"),
                     (dict(out=np.zeros((n, H, W, 3), np.uint8)), "out"), (dict(out=torch.zeros((n, H, W), dtype=torch.uint8, device=dev)), "out"),
                     (dict(source=torch.zeros((n, H, W, 3), dtype=torch.uint8, device=dev)), "source"),
                     (dict(source=np.zeros((n, H, W), np.uint8)), "source")):
        with pytest.raises(ValueError, match=what):
            ops.interpolate(**dict(good, **kw))
    # host inputs are uploaded
    got = ops.interpolate(np.array(c["frames"]), np.array(c["fwd"]), np.array(c["bwd"]), np.array(c["jobs"]), 3, 8, 96, source=True)
    assert got[0].is_cuda
    _same(got, C.want("pan_17x23"), "host inputs")
    # an output that overlaps the frames is refused by the entry, before any launch
    nb = fr.numel()
    flat = torch.zeros(nb + n * H * W * 3 + 12, dtype=torch.uint8, device=dev)
    src = flat[:nb].view(fr.shape).copy_(fr)
    for at in (0, 12, nb - 1):
        with pytest.raises(lib.HipError, match="overlap"):
            ops.interpolate(src, fwd, bwd, jobs, 3, 8, 96, out=flat[at:at + n * H * W * 3].view(n, H, W, 3))
    behind = flat[nb:nb + n * H * W * 3].view(n, H, W, 3)               # right behind the frames: no overlap
    assert np.array_equal(ops.interpolate(src, fwd, bwd, jobs, 3, 8, 96, out=behind).cpu().numpy(), C.want("pan_17x23")[0])
    # and so is a source that lies on the frames or on out
    for bad in (src.view(-1)[:n * H * W].view(n, H, W), behind.view(-1)[5:5 + n * H * W].view(n, H, W)):
        with pytest.raises(lib.HipError, match="source must not overlap"):
            ops.interpolate(src, fwd, bwd, jobs, 3, 8, 96, out=behind, source=bad)
    assert np.array_equal(src.cpu().numpy(), c["frames"])
    # flows off an 8-byte boundary are refused by the entry, from the address alone
    odd = torch.zeros(fwd.numel() + 1, dtype=torch.float32, device=dev)[1:].view(fwd.shape).copy_(fwd)
    with pytest.raises(lib.HipError, match="aligned"):
        ops.interpolate(fr, odd, bwd, jobs, 3, 8, 96)
    # no job and no pixel: results of the right shapes
    none = torch.zeros((0, 5), dtype=torch.int32, device=dev)
    o, s = ops.interpolate(fr, fwd, bwd, none, 3, 8, 96, source=True)
    assert tuple(o.shape) == (0, H, W, 3) and tuple(s.shape) == (0, H, W)
    e, g = torch.zeros((2, 0, 7, 3), dtype=torch.uint8, device=dev), torch.zeros((1, 0, 7, 2), dtype=torch.float32, device=dev)
    assert tuple(ops.interpolate(e, g, g, [(0, 1, 0, 1, 2)], 3, 8, 96).shape) == (1, 0, 7, 3)


# ------------------------------------------------------------------------------------------------ video.retime, video.replace_frames
RETIME = (("pan_64x128", 2, None), ("pan_33x70", (3, 2), None), ("five_33x70", 3, [2]), ("five_33x70", (1, 2), None),
          ("nonfinite_17x23", (64, 63), None), ("pan_17x23", (5, 3), [1, 3]), ("pan_1x9", 4, None), ("five_33x70", 2, [1, 2, 3, 4]))


def _adjacent_flows(c):
    """flows for every adjacent pair of a case's frames, [L-1,H,W,2]: the case's own pairs, repeated when they are fewer"""
    at = np.arange(c["L"] - 1) % c["P"]
    return np.ascontiguousarray(c["fwd"][at]), np.ascontiguousarray(c["bwd"][at])


@pytest.mark.parametrize("name, rate, scenes", RETIME)
def test_retime_is_the_planner_and_the_restatement(dev, name, rate, scenes):
    c = C.case(name)
    host, (fwd, bwd) = np.array(c["frames"]), _adjacent_flows(c)
    rows, pairs = video.plan_retime(c["L"], rate, scenes)
    P = max(len(pairs), 1)
    for setting in ((3, 8, 96), (0, 255, 765)):
        kw = dict(zip(("iterations", "tolerance", "match"), setting))
        want = C.reference(host, fwd[pairs] if pairs else np.zeros((P,) + fwd.shape[1:], np.float32),
                           bwd[pairs] if pairs else np.zeros((P,) + fwd.shape[1:], np.float32), rows, *setting)
        with launch_trace() as trace:
            out, src = video.retime(None, host, rate, flows=(fwd, bwd), scenes=scenes, return_source=True, device=dev, **kw)
        assert [r["symbol"] for r in trace] == [SYMBOL]
        assert isinstance(out, np.ndarray) and isinstance(src, np.ndarray)
        assert np.array_equal(out, want[0]) and np.array_equal(src, want[1]), (name, rate, setting)
        for j, (ia, ib, fi, k, d) in enumerate(rows):                   # a frame that falls on a source frame is the caller's bytes
            if k == 0:
                assert np.array_equal(out[j], host[ia]) and (src[j] == 5).all()
        # a device tensor is used where it is -- on, and one byte off a dword -- and device tensors come back; flows on the device
        for off in (0, 1):
            x = _up(host, dev, off)
            got = video.retime(None, x, rate, flows=(_up(fwd, dev), _up(bwd, dev)), scenes=scenes, **kw)
            assert isinstance(got, torch.Tensor) and got.is_cuda and np.array_equal(got.cpu().numpy(), want[0])
            assert np.array_equal(x.cpu().numpy(), host)
    assert np.array_equal(host, c["frames"])


REPLACE = (("five_33x70", [2], None), ("five_33x70", [1, 2, 3], None), ("five_33x70", [0, 2, 4], None), ("five_33x70", [1, 3], [2]),
           ("pan_64x128", [1, 2], None), ("nonfinite_17x23", [1], None), ("five_33x70", [0, 1], [3]))


@pytest.mark.parametrize("name, bad, scenes", REPLACE)
def test_replace_frames_is_the_planner_and_the_restatement(dev, name, bad, scenes):
    c = C.case(name)
    host, L = np.array(c["frames"]), c["L"]
    runs = video.plan_replace(L, bad, scenes)
    bridged = [(a, b) for a, b, _ in runs if a is not None and b is not None]
    flows = [(np.ascontiguousarray(c["fwd"][i % c["P"]]), np.ascontiguousarray(c["bwd"][i % c["P"]])) for i in range(len(bridged))]
    rows = video._replace_jobs(L, runs)
    zero = np.zeros((1, c["H"], c["W"], 2), np.float32)
    fw, bw = (np.stack([f[i] for f in flows]) if flows else zero for i in (0, 1))
    for setting in ((3, 8, 96), (8, 0, 0)):
        kw = dict(zip(("iterations", "tolerance", "match"), setting))
        want = C.reference(host, fw, bw, rows, *setting)
        with launch_trace() as trace:
            out, src = video.replace_frames(None, host, bad, flows=flows, scenes=scenes, return_source=True, device=dev, **kw)
        assert [r["symbol"] for r in trace] == [SYMBOL]
        assert out.shape == host.shape and np.array_equal(out, want[0]) and np.array_equal(src, want[1]), (name, bad, setting)
        for i in range(L):                                              # every frame not in bad is the caller's bytes
            if i not in bad:
                assert np.array_equal(out[i], host[i]) and (src[i] == 5).all()
        x = _up(host, dev, 1)
        got = video.replace_frames(None, x, bad, flows=[(_up(f, dev), _up(b, dev)) for f, b in flows], scenes=scenes, **kw)
        assert isinstance(got, torch.Tensor) and got.is_cuda and np.array_equal(got.cpu().numpy(), want[0])
        assert np.array_equal(x.cpu().numpy(), host)
    assert any(not np.array_equal(out[i], host[i]) for i in bad)


def test_no_work_launches_nothing(dev):
    c = C.case("pan_17x23")
    host, flows = np.array(c["frames"]), _adjacent_flows(c)
    with launch_trace() as trace:
        for call in (lambda x, **kw: video.retime(None, x, 1, flows=flows, **kw), lambda x, **kw: video.retime(None, x, (7, 7), **kw),
                     lambda x, **kw: video.replace_frames(None, x, [], **kw),
                     lambda x, **kw: video.retime(None, x[:1], 5, **kw), lambda x, **kw: video.retime(None, x[:0], (3, 2), **kw)):
            out, src = call(host, return_source=True, device=dev)
            assert isinstance(out, np.ndarray) and out.shape[1:] == host.shape[1:] and np.array_equal(out, host[:len(out)])
            assert src.shape == out.shape[:3] and (src == 5).all()
            x = _up(host, dev)
            on = call(x)
            assert on.is_cuda and on.data_ptr() != x.data_ptr() and torch.equal(on, x[:len(on)])
    assert not trace


def _net(dev, model="e2fgvi_hq"):
    """the generator with synthetic weights; e2fgvi_hq is the one that takes frames of any size"""
    if model not in _CACHE:
        from e2fgvi_amd.synth import synth_state_dict
        net = importlib.import_module("model." + model).InpaintGenerator()
        net.load_state_dict(synth_state_dict(model, "stress", 0))
        _CACHE[model] = net.to(dev).eval()
    return _CACHE[model]


def test_with_the_nets_flows(dev):
    """without flows= the calls compute the net's own, for the pairs that need them alone, and are ops.interpolate fed
    metrics.video_flows' output byte for byte"""
    net = _net(dev)
    frames = C.soft(5, 64, 128, 41, sigma=1.0)
    frames[1:] = np.roll(frames[1:], 1, axis=2)
    x = torch.from_numpy(frames).to(dev)
    with torch.no_grad():
        fwd, bwd = metrics.video_flows(net, frames)
        # retime: a cut at 2, so the pairs 0, 2 and 3 are interpolated and pair 1 is not
        rows, pairs = video.plan_retime(5, 2, [2])
        assert pairs == [0, 2, 3]
        at = torch.tensor(pairs, device=dev)
        want = ops.interpolate(x, fwd[at].contiguous(), bwd[at].contiguous(), rows, 3, 8, 96, source=True)
        with launch_trace() as trace:
            got = video.retime(net, frames, 2, scenes=[2], return_source=True)
        assert [r["symbol"] for r in trace].count(SYMBOL) == 1
        assert isinstance(got[0], np.ndarray) and got[0].shape == (9, 64, 128, 3)
        _same(want, got, "retime")
        print("retime source codes", np.bincount(got[1].ravel(), minlength=6))
        # replace_frames: the run 1, 2 between 0 and 3; its flows are those of the two-frame video (0, 3)
        f2, b2 = metrics.video_flows(net, frames[[0, 3]])
        want = ops.interpolate(x, f2, b2, video._replace_jobs(5, video.plan_replace(5, [1, 2])), 3, 8, 96, source=True)
        with launch_trace() as trace:
            got = video.replace_frames(net, frames, [1, 2], return_source=True)
        assert [r["symbol"] for r in trace].count(SYMBOL) == 1
        _same(want, got, "replace_frames")
        for i in (0, 3, 4):
            assert np.array_equal(got[0][i], frames[i])
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.retime(lambda x, m: (x, None), frames, device=dev)
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.replace_frames(None, frames, [2], device=dev)
