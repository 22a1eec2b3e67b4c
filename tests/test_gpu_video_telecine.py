"""The inverse telecine on the device: ops.telecine_scores and ops.field_weave (csrc/telecine.hip), video.telecine_scores,
video.detect_telecine and video.inverse_telecine against the restatement of tests/telecine_cases.py, every word and every byte
equal, on every named case; buffers off their alignment; reruns; frames launched in slabs; results inside sentinel-filled arenas;
and the planted 432 x 240 tennis clips."""
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import telecine_cases as C
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("e2fgvi_telecine_scores", "e2fgvi_field_weave")


def _up(a, dev, shift=0, fill=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.full((a.nbytes + shift,), fill, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _scene(c, dev):
    return torch.from_numpy(C.scene_of_np(c["L"], c["scenes"])).to(dev)


def _count(trace):
    return [sum(r["symbol"] == s for r in trace) for s in SYMBOLS]


# ------------------------------------------------------------------------------------------------ the two entries
@pytest.mark.parametrize("name", C.NAMES)
def test_entries_are_the_restatement(dev, name):
    """the scores and the woven bytes on every named case -- H in 1 .. 6 by W in 1 .. 7, sides that are no multiple of 4 or 16, rows
    of more than 1024 pixels, a tall narrow frame, one to four frames, a cut at every place, frames of 0 and 255 alone, flat
    frames -- with the byte buffers on, and one, two and three bytes off an allocation's start, either field kept, into out
    buffers that were full of something else: every byte is written; the inputs are only read"""
    c = C.case(name)
    scene, jobs = _scene(c, dev), C.case_jobs(name)
    for shift, fill in ((0, None), (1, 77), (2, 200), (3, 255)):
        fr = _up(c["frames"], dev, shift)
        M = ops.telecine_scores(fr, scene)
        assert M.dtype == torch.int64 and tuple(M.shape) == (c["L"], 2, 3, 16)
        assert np.array_equal(M.cpu().numpy(), C.want_scores(name)), (name, shift, int((M.cpu().numpy() != C.want_scores(name)).sum()))
        for keep in (0, 1):
            want = C.want_weave(name, keep)
            if fill is None:
                got = ops.field_weave(fr, jobs, keep)
            else:
                ob = _up(np.full(want.shape, fill, np.uint8), dev, (shift + keep) % 4)
                got = ops.field_weave(fr, np.array(jobs), keep, out=ob)
                assert got.data_ptr() == ob.data_ptr()
            assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy(), want), (name, shift, fill, keep, int((got.cpu().numpy() != want).sum()))
        assert np.array_equal(fr.cpu().numpy(), c["frames"])           # the input is only read
    print(name, "M[0][1]", C.want_scores(name)[0, 1].sum(axis=1).tolist())


@pytest.mark.parametrize("name", ("noise_37x53", "cut2_40x52", "tiny_4x1", "tiny_6x7", "tall_300x20", "wide_9x1100", "noise_70x150"))
def test_cells_of_the_next_frame_sum_to_the_interlace_scores(dev, name):
    """wherever t has a successor in its scene the sum over the cells of M[t][q][2] is D[t][q] of ops.interlace_scores; where a
    candidate was replaced by t, M[t][q][j] == M[t][q][1]"""
    c = C.case(name)
    fr, scene = _up(c["frames"], dev), _scene(c, dev)
    M, D = ops.telecine_scores(fr, scene).cpu().numpy(), ops.interlace_scores(fr, scene).cpu().numpy()
    so = C.scene_of_np(c["L"], c["scenes"])
    for t in range(c["L"]):
        if t + 1 < c["L"] and so[t + 1] == so[t]:
            assert np.array_equal(M[t, :, 2].sum(axis=1), D[t]), (name, t)
        else:
            assert np.array_equal(M[t, :, 2], M[t, :, 1]), (name, t)
        if not (t > 0 and so[t - 1] == so[t]):
            assert np.array_equal(M[t, :, 0], M[t, :, 1]), (name, t)


def test_runs_are_the_same_bits(dev):
    for name in ("noise_37x53", "tall_300x20", "wide_9x1100", "noise_70x150"):
        c = C.case(name)
        fr, scene, jobs = _up(c["frames"], dev, 1), _scene(c, dev), C.case_jobs(name)
        first = [ops.telecine_scores(fr, scene).cpu().numpy(), ops.field_weave(fr, jobs, 0).cpu().numpy()]
        for _ in range(5):
            again = [ops.telecine_scores(fr, scene).cpu().numpy(), ops.field_weave(fr, jobs, 0).cpu().numpy()]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 4 x 1 and of 1 x 1: the scores carry the frames on the grid's y axis and launch them in slabs of 65 535, the
    weave carries its jobs on the y and z axes of one launch; a cut in the second slab.  With four rows and one column, row 1
    (q = 1) falls into cell 4 and row 2 (q = 0) into cell 8; with one row nothing is scored."""
    L, cut = 65540, 65537
    rng = np.random.RandomState(71)
    so = C.scene_of_np(L, [cut])
    scene = _up(so, dev)
    jobs = np.stack([np.arange(L), np.clip(np.arange(L) + rng.randint(-1, 2, L), 0, L - 1)], axis=1)
    tall = rng.randint(0, 256, (L, 4, 1, 3)).astype(np.uint8)
    Y = C.luma(tall)[:, :, 0]
    nxt, prv = np.concatenate([Y[1:], Y[-1:]]), np.concatenate([Y[:1], Y[:-1]])
    nxt[cut - 1], prv[cut] = Y[cut - 1], Y[cut]
    want = np.zeros((L, 2, 3, 16), np.int64)
    for j, S in enumerate((prv, Y, nxt)):
        want[:, 1, j, 4] = np.abs(2 * S[:, 1] - Y[:, 0] - Y[:, 2])
        want[:, 0, j, 8] = np.abs(2 * S[:, 2] - Y[:, 1] - Y[:, 3])
    x = _up(tall, dev)
    got = ops.telecine_scores(x, scene).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(ops.field_weave(x, jobs, 1).cpu().numpy(), C.weave_np(tall, jobs, 1))
    one = rng.randint(0, 256, (L, 1, 1, 3)).astype(np.uint8)
    x = _up(one, dev, 3)
    assert not ops.telecine_scores(x, scene).any()
    assert np.array_equal(ops.field_weave(x, jobs, 0).cpu().numpy(), one) and np.array_equal(ops.field_weave(x, jobs, 1).cpu().numpy(), one[jobs[:, 1]])


def test_nothing_is_written_outside_the_results(dev):
    """M and out inside larger arenas full of a sentinel: not a byte changes outside the slice, and the slice is the restatement's"""
    so = lib.load()
    for name in ("noise_37x53", "tall_300x20", "tiny_4x3", "wide_9x1100"):
        c = C.case(name)
        fr, scene, jobs = _up(c["frames"], dev, 2), _scene(c, dev), C.case_jobs(name)
        words, guard = c["L"] * 96, 1024
        arena = torch.full((words + 2 * guard,), -0x0123456789ABCDEF, dtype=torch.int64, device=dev)
        M = arena[guard:guard + words]
        lib.check(so.e2fgvi_telecine_scores(ops._ptr(fr), ops._ptr(scene), ops._ptr(M), c["L"], c["H"], c["W"], ops._stream()), "telecine_scores")
        got = arena.cpu().numpy()
        assert (got[:guard] == -0x0123456789ABCDEF).all() and (got[guard + words:] == -0x0123456789ABCDEF).all()
        assert np.array_equal(got[guard:guard + words].reshape(c["L"], 2, 3, 16), C.want_scores(name))
        want = C.want_weave(name, 1)
        for off in (0, 1, 7, 16):
            bytes_ = torch.full((want.size + 2 * guard + off,), 0xA5, dtype=torch.uint8, device=dev)
            out = bytes_[guard + off:guard + off + want.size].view(want.shape)
            assert ops.field_weave(fr, jobs, 1, out=out).data_ptr() == out.data_ptr()
            got = bytes_.cpu().numpy()
            assert (got[:guard + off] == 0xA5).all() and (got[guard + off + want.size:] == 0xA5).all(), (name, off)
            assert np.array_equal(got[guard + off:guard + off + want.size].reshape(want.shape), want), (name, off)


def test_arguments_are_checked(dev):
    c = C.case("noise_37x53")
    L, H, W = c["L"], c["H"], c["W"]
    fr, scene, jobs = _up(c["frames"], dev), _scene(c, dev), C.case_jobs("noise_37x53")
    for kw, what in ((dict(frames=fr.int()), "frames"), (dict(frames=fr[0, 0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(scene=scene[1:]), "scene"), (dict(scene=scene.float()), "scene")):
        with pytest.raises(ValueError, match=what):
            ops.telecine_scores(**dict(dict(frames=fr, scene=scene), **kw))
    n = len(jobs)
    good = dict(frames=fr, jobs=jobs, keep=0)
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[:, :, ::2]), "contiguous"),
                     (dict(keep=2), "keep"), (dict(keep=-1), "keep"), (dict(keep=True), "keep"), (dict(keep="top"), "keep"),
                     (dict(jobs=[(0, L)]), "jobs"), (dict(jobs=[(-1, 0)]), "jobs"), (dict(jobs=[(0, 1, 2)]), "jobs"), (dict(jobs=[0, 1]), "jobs"),
                     (dict(jobs=[(0.0, 1.0)]), "jobs"), (dict(jobs=torch.tensor(jobs, device=dev)), "jobs"),
                     (dict(out=np.zeros((n, H, W, 3), np.uint8)), "out"),
                     (dict(out=torch.zeros((n + 1, H, W, 3), dtype=torch.uint8, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.field_weave(**dict(good, **kw))
    # host inputs are uploaded
    got = ops.field_weave(np.array(c["frames"]), torch.tensor(jobs), 0)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), C.want_weave("noise_37x53", 0))
    got = ops.telecine_scores(np.array(c["frames"]), C.scene_of_np(L))
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), C.scores_np(c["frames"]))
    # an output that overlaps the frames is refused by the entry, before any launch -- the frames themselves too
    size = fr.numel()
    flat = torch.zeros(2 * size + 12, dtype=torch.uint8, device=dev)
    src = flat[:size].view(fr.shape).copy_(fr)
    same = [(t, t) for t in range(L)]
    for at in (0, 12, size - 1):
        with pytest.raises(lib.HipError, match="overlap"):
            ops.field_weave(src, same, 0, out=flat[at:at + size].view(fr.shape))
    behind = flat[size:2 * size].view(fr.shape)                         # right behind the frames: no overlap
    assert np.array_equal(ops.field_weave(src, same, 0, out=behind).cpu().numpy(), c["frames"])
    assert np.array_equal(src.cpu().numpy(), c["frames"])
    # no frame, no pixel and no job: results of the right shapes
    for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
        e = torch.zeros(shape, dtype=torch.uint8, device=dev)
        M = ops.telecine_scores(e, torch.zeros(shape[0], dtype=torch.int32, device=dev))
        assert tuple(M.shape) == (shape[0], 2, 3, 16) and not M.any()
        assert tuple(ops.field_weave(e, [], 0).shape) == (0,) + shape[1:]
        if shape[0]:
            assert tuple(ops.field_weave(e, [(0, 1), (2, 2)], 1).shape) == (2,) + shape[1:]
    assert tuple(ops.field_weave(fr, [], 1).shape) == (0, H, W, 3) and tuple(ops.field_weave(fr, np.zeros((0, 2), np.int32), 1).shape) == (0, H, W, 3)


def test_entries_refuse_bad_arguments_with_device_pointers(dev):
    """E2FGVI_EINVAL for each refused argument, from the arguments alone: nothing is launched and the out buffers keep what they held"""
    so = lib.load()
    c = C.case("noise_37x53")
    L, H, W = c["L"], c["H"], c["W"]
    fr, scene = _up(c["frames"], dev), _scene(c, dev)
    jobs = torch.tensor(C.case_jobs("noise_37x53"), dtype=torch.int32, device=dev)
    n = int(jobs.shape[0])
    out = torch.full((n, H, W, 3), 0x5A, dtype=torch.uint8, device=dev)
    M = torch.full((L, 2, 3, 16), 0x5A5A, dtype=torch.int64, device=dev)
    ptr = lambda t: t.data_ptr()                                        # plain integers: an address can be moved off its alignment

    def weave(**kw):
        a = dict(dict(frames=ptr(fr), jobs=ptr(jobs), out=ptr(out), L=L, n=n, H=H, W=W, keep=0), **kw)
        return so.e2fgvi_field_weave(*[a[k] for k in ("frames", "jobs", "out", "L", "n", "H", "W", "keep")], ops._stream())

    def scores(**kw):
        a = dict(dict(frames=ptr(fr), scene=ptr(scene), M=ptr(M), L=L, H=H, W=W), **kw)
        return so.e2fgvi_telecine_scores(*[a[k] for k in ("frames", "scene", "M", "L", "H", "W")], ops._stream())

    for kw, word in ((dict(keep=2), b"keep"), (dict(keep=-1), b"keep"), (dict(n=-1), b"negative"), (dict(L=-1), b"negative"), (dict(H=-1), b"negative"),
                     (dict(W=-1), b"negative"), (dict(H=8193, W=8192), b"2^26"), (dict(jobs=ptr(jobs) + 2), b"aligned"), (dict(frames=None), b"null"),
                     (dict(jobs=None), b"null"), (dict(out=None), b"null"), (dict(L=0), b"no frame"), (dict(out=ptr(fr)), b"overlap"),
                     (dict(out=ptr(fr) + fr.numel() - 1), b"overlap")):
        assert weave(**kw) == -1 and word in so.e2fgvi_last_error() and b"field_weave" in so.e2fgvi_last_error(), kw
    for kw, word in ((dict(L=-1), b"negative"), (dict(H=-1), b"negative"), (dict(W=-1), b"negative"), (dict(H=8193, W=8192), b"2^26"),
                     (dict(scene=ptr(scene) + 2), b"aligned"), (dict(M=ptr(M) + 4), b"aligned"), (dict(frames=None), b"null"), (dict(scene=None), b"null"),
                     (dict(M=None), b"null")):
        assert scores(**kw) == -1 and word in so.e2fgvi_last_error() and b"telecine_scores" in so.e2fgvi_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((M == 0x5A5A).all()) and np.array_equal(fr.cpu().numpy(), c["frames"])
    # and the same pointers with good arguments are taken
    assert weave() == 0 and scores() == 0
    assert np.array_equal(out.cpu().numpy(), C.want_weave("noise_37x53", 0)) and np.array_equal(M.cpu().numpy(), C.want_scores("noise_37x53"))


# ------------------------------------------------------------------------------------------------ the three video functions
@pytest.mark.parametrize("name", ("noise_37x53", "cut2_40x52", "cuts_6x7", "tiny_1x1", "tiny_3x5", "single_6x7", "extremes_40x52", "wide_9x1100"))
def test_video_functions_are_the_restatement(dev, name):
    c = C.case(name)
    host = np.array(c["frames"])
    M = C.want_scores(name)
    with launch_trace() as trace:
        got = video.telecine_scores(host, scenes=c["scenes"], device=dev)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, M) and _count(trace) == [1, 0]
    for keep, margin, cadence in (("top", 10, "3:2"), ("bottom", 10, "3:2"), ("top", 50, None), ("bottom", 1, None)):
        want, plan = C.inverse_telecine_np(host, c["scenes"], keep, margin, cadence, M=M)
        with launch_trace() as trace:
            out, got_plan = video.inverse_telecine(host, scenes=c["scenes"], keep=keep, margin=margin, cadence=cadence, return_plan=True, device=dev)
        assert _count(trace) == [1, 1] and len(trace) == 2
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == want.shape and np.array_equal(out, want), (name, keep, margin)
        assert sorted(got_plan) == ["cuts", "locks", "matches", "orphan", "source"]
        assert got_plan["matches"].dtype == np.int8 and got_plan["orphan"].dtype == np.bool_ and got_plan["source"].dtype == np.int32
        for key in ("matches", "orphan", "source"):
            assert np.array_equal(got_plan[key], plan[key]), (name, key)
        assert (got_plan["cuts"], got_plan["locks"]) == (plan["cuts"], plan["locks"])
        # a device tensor is used where it is -- on, and one, two and three bytes off a dword -- and a device tensor comes back
        for off in (0, 1, 2, 3):
            x = _up(c["frames"], dev, off)
            on = video.inverse_telecine(x, scenes=c["scenes"], keep=keep, margin=margin, cadence=cadence)
            assert isinstance(on, torch.Tensor) and on.is_cuda and on.dtype == torch.uint8 and np.array_equal(on.cpu().numpy(), want)
            assert np.array_equal(x.cpu().numpy(), c["frames"])
        k, _, locks = C.matches_np(M, keep, c["scenes"], margin)
        with launch_trace() as trace:
            verdict, gM, gk, glocks = video.detect_telecine(host, scenes=c["scenes"], keep=keep, margin=margin, return_scores=True, device=dev)
        assert _count(trace) == [1, 0]
        assert verdict == C.verdict_np(k, locks, c["scenes"]) and np.array_equal(gM, M) and gk.tolist() == k.tolist() and glocks == locks
        assert video.detect_telecine(_up(c["frames"], dev, 1), scenes=c["scenes"], keep=keep, margin=margin) == verdict
    assert np.array_equal(host, c["frames"])
    assert np.array_equal(video.inverse_telecine(host, scenes=c["scenes"], device=dev), C.inverse_telecine_np(host, c["scenes"], M=M)[0])      # the defaults


def test_planted_432x240_clips_recover_their_source_bytes(dev):
    """the panning clip of tests/golden/tennis25.npz under 3:2 pulldown in both field orders and phases, either field kept, and the
    locked-off clip: the scores of the restatement, the verdict "3:2", and the film's frames back byte for byte; the progressive
    frames read "none" and come back as they were"""
    f = C.tennis25(ROOT)
    for film, arms in ((C.pan_film(f), C.ARMS), (C.locked_off_film(f), C.ARMS[:2])):
        for tff, phase, keep in arms:
            clip, origin = C.telecine(film, tff, phase)
            with launch_trace() as trace:
                out, plan = video.inverse_telecine(clip, keep=keep, return_plan=True, device=dev)
            assert _count(trace) == [1, 1]
            assert out.shape == film.shape and out.tobytes() == film.tobytes(), (tff, phase, keep)
            assert plan["locks"][0] is not None and not plan["orphan"].any()
            assert C.film_of(plan, origin, keep)[:, 0].tolist() == list(range(len(film)))
            if keep == "top":
                verdict, M, k, locks = video.detect_telecine(clip, return_scores=True, device=dev)
                assert verdict == "3:2" and np.array_equal(M, C.scores_np(clip)) and k.tolist() == plan["matches"].tolist()
                print(len(film), tff, phase, "".join("-0+"[v + 1] for v in k), locks)
    x = _up(f[:12], dev)
    assert video.detect_telecine(x) == "none" and torch.equal(video.inverse_telecine(x), x)
    still = np.repeat(f[:1], 6, axis=0)
    assert video.detect_telecine(still, device=dev) == "none" and np.array_equal(video.inverse_telecine(still, device=dev), still)


def _joined(f, start=2):
    """two telecined clips joined at a cut, the first started `start` frames into the cadence and the second ended three frames
    early: with the top field kept the first frame is an orphan, with the bottom field kept the last one"""
    first = C.telecine(f[:12], True, 0)[0][start:]
    return np.concatenate([first, C.telecine(f[12:25], True, 1)[0][:-3]]), len(first)


def test_scene_by_scene_is_the_call_with_scenes(dev):
    clip, cut = _joined(C.tennis25(ROOT))
    x = _up(clip, dev)
    for kw in (dict(), dict(keep="bottom"), dict(cadence=None, margin=20)):
        whole, plan = video.inverse_telecine(x, scenes=[cut], return_plan=True, **kw)
        a, pa = video.inverse_telecine(x[:cut].contiguous(), return_plan=True, **kw)
        b, pb = video.inverse_telecine(x[cut:].contiguous(), return_plan=True, **kw)
        assert torch.equal(whole, torch.cat([a, b])) and plan["cuts"] == [len(a)]
        assert plan["matches"].tolist() == pa["matches"].tolist() + pb["matches"].tolist()
        assert plan["orphan"].tolist() == pa["orphan"].tolist() + pb["orphan"].tolist() and plan["locks"] == pa["locks"] + pb["locks"]
        assert np.array_equal(video.telecine_scores(x, scenes=[cut]), np.concatenate([video.telecine_scores(x[:cut].contiguous()), video.telecine_scores(x[cut:].contiguous())]))
    assert not np.array_equal(video.telecine_scores(x), video.telecine_scores(x, scenes=[cut]))        # and the cut is seen


def test_deinterlaced_orphans_are_the_deinterlacer_s_pictures(dev):
    """orphans="deinterlace": an orphan's output is deinterlace(frames, order, rate="frame", keep=<the kept field>, scenes=scenes)[t],
    every other frame is the one orphans="keep" gives"""
    clip, cut = _joined(C.tennis25(ROOT))
    x = _up(clip, dev)
    seen = 0
    for keep, order, field in (("top", "tff", "first"), ("top", "bff", "second"), ("bottom", "tff", "second"), ("bottom", "bff", "first")):
        kept, plan = video.inverse_telecine(x, scenes=[cut], keep=keep, return_plan=True)
        out, plan2 = video.inverse_telecine(x, scenes=[cut], keep=keep, orphans="deinterlace", order=order, return_plan=True)
        assert np.array_equal(plan["source"], plan2["source"]) and plan["orphan"].tolist() == plan2["orphan"].tolist()
        pictures = video.deinterlace(x, order, rate="frame", keep=field, scenes=[cut])
        for i, (t, _) in enumerate(plan["source"].tolist()):
            if plan["orphan"][t]:
                seen += 1
                assert torch.equal(out[i], pictures[t]) and not torch.equal(out[i], kept[i]), (keep, order, t)
            else:
                assert torch.equal(out[i], kept[i]), (keep, order, t)
    assert seen == 4                                                    # one orphan in each of the four arms
    assert np.array_equal(video.inverse_telecine(clip, scenes=[cut], orphans="deinterlace", order="tff", device=dev),
                          video.inverse_telecine(x, scenes=[cut], orphans="deinterlace", order="tff").cpu().numpy())


def test_no_frame_and_no_pixel_launch_nothing(dev):
    with launch_trace() as trace:
        for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
            out, plan = video.inverse_telecine(np.zeros(shape, np.uint8), return_plan=True, device=dev)
            assert isinstance(out, np.ndarray) and out.shape == shape and out.dtype == np.uint8
            assert plan["source"].shape == (shape[0], 2) and plan["matches"].shape == (shape[0],) and not plan["orphan"].any()
            on = video.inverse_telecine(torch.zeros(shape, dtype=torch.uint8, device=dev), orphans="deinterlace", order="bff")
            assert on.is_cuda and tuple(on.shape) == shape
            verdict, M, k, locks = video.detect_telecine(np.zeros(shape, np.uint8), return_scores=True, device=dev)
            assert verdict == "none" and M.shape == (shape[0], 2, 3, 16) and not M.any() and k.shape == (shape[0],)
            assert video.telecine_scores(np.zeros(shape, np.uint8), device=dev).shape == (shape[0], 2, 3, 16)
    assert not any(r["symbol"] in SYMBOLS + ("e2fgvi_deinterlace",) for r in trace)
