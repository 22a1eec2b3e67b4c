"""The weave stabiliser on the device: ops.weave_profiles, ops.weave_match, ops.weave_path and ops.weave_apply (csrc/weave.hip),
video.stabilize and video.apply_shifts against the numpy restatement of tests/weave_cases.py, every word and every byte equal, on
every named case; buffers off their alignment; a tensor used in place; reruns; frames launched in slabs; and the planted 432 x 240
tennis video."""
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import weave_cases as C
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEAVE_SYMBOLS = ("e2fgvi_weave_profiles", "e2fgvi_weave_match", "e2fgvi_weave_path", "e2fgvi_weave_apply")


def _up(a, dev, shift=0, fill=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.full((a.nbytes + shift,), fill, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _run(c, dev, shift=0, fill=None):
    """the dict of C.KEYS of the four entries on a case; frames, out and mask `shift` bytes off an allocation's start, out and mask
    full of `fill` beforehand"""
    L, H, W = c["L"], c["H"], c["W"]
    scene = torch.from_numpy(C.scene_of_np(L, c["scenes"])).to(dev)
    fr = _up(c["frames"], dev, shift)
    col, row = ops.weave_profiles(fr)
    motion = ops.weave_match(col, row, scene, c["radius"], c["tex"])
    sh = ops.weave_path(motion, scene, c["span"], c["max_shift"], c["subpixel"])
    if fill is None and not shift:
        out, mask = ops.weave_apply(fr, sh, return_mask=True)
    else:
        ob = _up(np.full((L, H, W, 3), fill or 0, np.uint8), dev, shift)
        mb = _up(np.full((L, H, W), fill or 0, np.uint8), dev, shift)
        out, mask = ops.weave_apply(fr, sh, out=ob, mask=mb)
        assert out.data_ptr() == ob.data_ptr() and mask.data_ptr() == mb.data_ptr()
    assert np.array_equal(fr.cpu().numpy(), c["frames"])               # the input is only read
    return {k: v.cpu().numpy() for k, v in dict(col=col, row=row, motion=motion, shift=sh, out=out, mask=mask).items()}


def _assert_equal(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


# ------------------------------------------------------------------------------------------------ the four entries
@pytest.mark.parametrize("name", C.NAMES)
def test_entries_are_the_restatement(dev, name):
    """col, row, motion, shift and the output and mask bytes on every named case -- among them sides that are no multiple of 4 or
    8, an empty band (rows_7x64), one pixel, windows too short to measure, two workgroups a band (tall_300x20), rows of more than
    1024 pixels (wide_9x1100), radius 1 and 32, span 0, 1 and 16 -- with the byte buffers on, and one, two and three bytes off an
    allocation's start, and into out and mask buffers that were full of something else: every byte is written"""
    c, want = C.case(name), C.want(name)
    for shift, fill in ((0, None), (1, None), (2, 77), (3, 200), (0, 255)):
        got = _run(c, dev, shift, fill)
        print(name, "shift", shift, "fill", fill, "motion", got["motion"].tolist()[:3])
        _assert_equal(got, want, C.KEYS, (name, shift, fill))


@pytest.mark.parametrize("planes", [3, 1])
def test_apply_alone_on_shift_tables(dev, planes):
    """shifts beyond the frame and beyond the clamp, fractions of either sign, one axis at a time: three bytes a pixel and one"""
    for name in ("sub_37x53", "weave_40x52", "wide_9x1100", "one_1x1"):
        fr = C.case(name)["frames"]
        fr = np.ascontiguousarray(np.resize(fr, (len(C.APPLY_SHIFTS),) + fr.shape[1:]) if planes == 3 else
                                  np.resize(fr[..., 1], (len(C.APPLY_SHIFTS),) + fr.shape[1:3]))
        want_out, want_mask = C.apply_np(fr, C.APPLY_SHIFTS)
        for shift in (0, 1, 2, 3):
            out, mask = ops.weave_apply(_up(fr, dev, shift), _up(C.APPLY_SHIFTS, dev), out=_up(0 * fr + 9, dev, shift),
                                        mask=_up(0 * fr[:, :, :, 0] + 9 if planes == 3 else 0 * fr + 9, dev, shift))
            assert np.array_equal(out.cpu().numpy(), want_out), (name, shift, int((out.cpu().numpy() != want_out).sum()))
            assert np.array_equal(mask.cpu().numpy(), want_mask), (name, shift)
        plain = ops.weave_apply(fr, C.APPLY_SHIFTS)                    # host inputs are uploaded; no mask asked for, none made
        assert isinstance(plain, torch.Tensor) and plain.is_cuda and np.array_equal(plain.cpu().numpy(), want_out)
        moved = video.apply_shifts(fr, C.APPLY_SHIFTS, device=dev)
        assert isinstance(moved, np.ndarray) and moved.dtype == np.uint8 and np.array_equal(moved, want_out)
        on = video.apply_shifts(_up(fr, dev, 1), _up(C.APPLY_SHIFTS, dev))
        assert isinstance(on, torch.Tensor) and on.is_cuda and np.array_equal(on.cpu().numpy(), want_out)


def test_runs_are_the_same_bits(dev):
    for name in ("sub_37x53", "tall_300x20"):
        c = C.case(name)
        first = _run(c, dev)
        for _ in range(5):
            again = _run(c, dev)
            assert all(np.array_equal(first[k], again[k]) for k in C.KEYS)


def test_more_frames_than_a_launch_takes(dev):
    """65 540 frames of one pixel: the profiles and the apply kernel carry the frames on the grid's y axis and launch them in slabs
    of 65 535"""
    L = 65540
    rng = np.random.RandomState(60)
    fr = rng.randint(0, 256, (L, 1, 1, 3)).astype(np.uint8)
    sh = rng.randint(-40, 41, (L, 2)).astype(np.int32)
    col, row = ops.weave_profiles(_up(fr, dev))
    y = C.luma(fr).reshape(L)
    for prof in (col, row):
        got = prof.cpu().numpy()
        assert got.shape == (L, 8, 1) and np.array_equal(got[:, 7, 0], y) and not got[:, :7].any()
    out, mask = ops.weave_apply(_up(fr, dev), _up(sh, dev), return_mask=True)
    assert np.array_equal(out.cpu().numpy(), fr) and np.array_equal(mask.cpu().numpy().reshape(L) == 255, sh.any(axis=1))
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    motion = ops.weave_match(col, row, scene, 16, 2)
    assert motion.shape == (L, 4) and not motion.any() and not ops.weave_path(motion, scene, 4, 16).any()


def test_path_alone_on_motion_tables(dev):
    """the path entry on tables that no video here gives: long segments, every span, breaks next to each other, both roundings"""
    rng = np.random.RandomState(61)
    L = 700
    motion = np.concatenate([rng.randint(-500, 501, (L, 2)), rng.choice([8, 8, 8, 8, 8, 4, 3, 0], (L, 2))], axis=1).astype(np.int32)
    scenes = [1, 2, 300, 301, 650]
    so = C.scene_of_np(L, scenes)
    for span in (0, 1, 2, 7, 16):
        for max_shift, subpixel in ((64, True), (3, True), (16, False)):
            got = ops.weave_path(_up(motion, dev), _up(so, dev), span, max_shift, subpixel).cpu().numpy()
            assert got.dtype == np.int32 and np.array_equal(got, C.path_np(motion, so, span, max_shift, subpixel)), (span, max_shift)


def test_arguments_are_checked(dev):
    c, want = C.case("sub_37x53"), C.want("sub_37x53")
    L, H, W = c["L"], c["H"], c["W"]
    fr = _up(c["frames"], dev)
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(frames=fr[:, :, ::2]), "contiguous"), (dict(frames=torch.zeros((1, 4097, 2, 3), dtype=torch.uint8, device=dev)), "4096")):
        with pytest.raises(ValueError, match=what):
            ops.weave_profiles(**kw)
    col, row = ops.weave_profiles(np.array(c["frames"]))                # host inputs are uploaded
    assert col.is_cuda and np.array_equal(col.cpu().numpy(), want["col"]) and np.array_equal(row.cpu().numpy(), want["row"])
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    good = dict(col=col, row=row, scene=scene, radius=4, tex=2)
    for kw, what in ((dict(col=col.float()), "col"), (dict(col=col[0]), "col"), (dict(col=col[:, :7].contiguous()), "col"),
                     (dict(col=col[:, :, ::2]), "contiguous"), (dict(row=row[1:]), "row"), (dict(row=row.long()), "row"),
                     (dict(scene=scene[:-1]), "scene"), (dict(scene=scene.long()), "scene"), (dict(radius=0), "radius"),
                     (dict(radius=33), "radius"), (dict(radius=True), "radius"), (dict(radius=2.5), "radius"), (dict(tex=-1), "tex"),
                     (dict(tex=65536), "tex"), (dict(tex=True), "tex")):
        with pytest.raises(ValueError, match=what):
            ops.weave_match(**dict(good, **kw))
    motion = ops.weave_match(**good)
    assert np.array_equal(motion.cpu().numpy(), want["motion"])
    good = dict(motion=motion, scene=scene, span=4, max_shift=16)
    for kw, what in ((dict(motion=motion.float()), "motion"), (dict(motion=motion[:, :3].contiguous()), "motion"),
                     (dict(motion=motion[0]), "motion"), (dict(scene=scene[:-1]), "scene"), (dict(span=-1), "span"), (dict(span=17), "span"),
                     (dict(span=True), "span"), (dict(max_shift=0), "max_shift"), (dict(max_shift=65), "max_shift"),
                     (dict(max_shift=1.5), "max_shift"), (dict(subpixel=1), "subpixel"), (dict(subpixel=None), "subpixel")):
        with pytest.raises(ValueError, match=what):
            ops.weave_path(**dict(good, **kw))
    sh = ops.weave_path(**good)
    assert np.array_equal(sh.cpu().numpy(), want["shift"])
    for kw, what in ((dict(frames=fr.int()), "frames"), (dict(frames=fr[0, 0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(shift=sh.float()), "shift"), (dict(shift=sh[:-1]), "shift"), (dict(shift=sh[:, :1]), "contiguous"),
                     (dict(out=np.zeros(fr.shape, np.uint8)), "out"), (dict(mask=np.zeros(fr.shape[:3], np.uint8)), "mask"),
                     (dict(out=torch.zeros((L, H, W + 1, 3), dtype=torch.uint8, device=dev)), "out"),
                     (dict(mask=torch.zeros((L, H, W, 3), dtype=torch.uint8, device=dev)), "mask")):
        with pytest.raises(ValueError, match=what):
            ops.weave_apply(**dict(dict(frames=fr, shift=sh), **kw))
    # an output or a mask that overlaps the frames is refused by the entry, before any launch -- the frames themselves too
    flat = torch.zeros(fr.numel() + 12, dtype=torch.uint8, device=dev)
    src, dst = flat[:fr.numel()].view(fr.shape).copy_(fr), flat[12:].view(fr.shape)
    for kw in (dict(out=dst), dict(out=src), dict(mask=flat[5:5 + L * H * W].view(L, H, W))):
        with pytest.raises(lib.HipError, match="overlap"):
            ops.weave_apply(src, sh, **kw)
    assert np.array_equal(src.cpu().numpy(), c["frames"])
    # no frame and no pixel: no launch, results of the right shapes
    with launch_trace() as trace:
        for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
            e = torch.zeros(shape, dtype=torch.uint8, device=dev)
            cl, rw = ops.weave_profiles(e)
            sc = torch.zeros(shape[0], dtype=torch.int32, device=dev)
            mo = ops.weave_match(cl, rw, sc, 16, 2)
            s2 = ops.weave_path(mo, sc, 4, 16)
            o, m = ops.weave_apply(e, s2, return_mask=True)
            assert cl.shape == (shape[0], 8, shape[2]) and rw.shape == (shape[0], 8, shape[1]) and mo.shape == (shape[0], 4)
            assert not mo.any() and not s2.any() and o.shape == shape and m.shape == shape[:3]


# ------------------------------------------------------------------------------------------------ stabilize
@pytest.mark.parametrize("name", C.NAMES)
def test_stabilize_is_the_restatement(dev, name):
    c, want = C.case(name), C.want(name)
    host = np.array(c["frames"])
    with launch_trace() as trace:
        out, shifts, motion, mask = video.stabilize(host, return_shifts=True, return_mask=True, device=dev, **C.settings(c))
    # span == 0 measures nothing: no launch, the motion table is zeros
    want = dict(want, motion=0 * want["motion"]) if c["span"] == 0 else want
    for a, k in ((out, "out"), (shifts, "shift"), (motion, "motion"), (mask, "mask")):
        assert isinstance(a, np.ndarray) and a.dtype == want[k].dtype and np.array_equal(a, want[k]), k
    assert np.array_equal(host, c["frames"])
    assert [sum(r["symbol"] == s for r in trace) for s in WEAVE_SYMBOLS] == ([0] * 4 if c["span"] == 0 else [1] * 4)
    plain = video.stabilize(host, device=dev, **C.settings(c))
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, want["out"])
    only_mask = video.stabilize(host, return_mask=True, device=dev, **C.settings(c))
    assert len(only_mask) == 2 and np.array_equal(only_mask[1], want["mask"])
    # a device tensor is used where it is -- on, and one, two and three bytes off a dword -- and device tensors come back
    for off in (0, 1, 2, 3):
        x = _up(c["frames"], dev, off)
        got, gs, gm = video.stabilize(x, return_shifts=True, **C.settings(c))
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in (got, gs, gm)) and got.dtype == torch.uint8 and gs.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), want["out"]) and np.array_equal(gs.cpu().numpy(), want["shift"])
        assert np.array_equal(gm.cpu().numpy(), want["motion"]) and np.array_equal(x.cpu().numpy(), c["frames"])
    # the masks painted on the source video move with the frames
    painted = np.ascontiguousarray(c["frames"][..., 0])
    assert np.array_equal(video.apply_shifts(painted, shifts, device=dev), C.apply_np(painted, want["shift"])[0])
    # span == 0: no launch, the caller's bytes
    with launch_trace() as trace:
        same, zs, zm, zk = video.stabilize(host, span=0, return_shifts=True, return_mask=True, device=dev)
        on = video.stabilize(x, span=0)
    assert not any(r["symbol"].startswith("e2fgvi_weave_") for r in trace)
    assert same.tobytes() == c["frames"].tobytes() and zs.shape == (c["L"], 2) and zm.shape == (c["L"], 4) and not zs.any() and not zm.any()
    assert zk.shape == c["frames"].shape[:3] and not zk.any() and on.is_cuda and on.data_ptr() == x.data_ptr()


def test_no_frame_and_no_pixel_launch_nothing(dev):
    with launch_trace() as trace:
        for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
            out, s, m, k = video.stabilize(np.zeros(shape, np.uint8), return_shifts=True, return_mask=True, device=dev)
            assert out.shape == shape and out.dtype == np.uint8 and s.shape == (shape[0], 2) and s.dtype == np.int32
            assert m.shape == (shape[0], 4) and k.shape == shape[:3] and k.dtype == np.uint8
    assert not any(r["symbol"].startswith("e2fgvi_weave_") for r in trace)


def test_planted_432x240_video_is_the_restatement(dev):
    """the 25 frames of tests/golden/tennis25.npz under weave_cases.plant(seed 1) with a cut at frame 12, radius 24: the words and
    bytes of the restatement, the same from a second call, and corrections of whole pixels keep every byte that stays inside"""
    planted, d = C.plant(C.tennis25(ROOT), 1)
    want = C.stabilize_np(planted, scenes=[12], radius=24)
    out, shifts, motion, mask = video.stabilize(planted, scenes=[12], radius=24, return_shifts=True, return_mask=True, device=dev)
    print("motion", motion.tolist(), "shifts", shifts.tolist(), "exposed", int((mask > 0).sum()))
    assert out.shape == (25, 240, 432, 3) and np.array_equal(motion, want["motion"]) and np.array_equal(shifts, want["shift"])
    assert out.tobytes() == want["out"].tobytes() and mask.tobytes() == want["mask"].tobytes()
    assert video.stabilize(planted, scenes=[12], radius=24, device=dev).tobytes() == out.tobytes()
    whole, ws = video.stabilize(planted, scenes=[12], radius=24, subpixel=False, return_shifts=True, device=dev)[:2]
    assert not (ws & 15).any() and np.array_equal(whole, C.apply_np(planted, ws)[0])
    assert set(np.unique(whole).tolist()) <= set(np.unique(planted).tolist())
