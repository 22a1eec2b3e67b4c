"""The line-scratch detector on the device: ops.line_sums, ops.line_columns and ops.line_paint (csrc/line_scratch.hip) and
video.detect_line_scratches against the numpy restatement of tests/line_scratch_cases.py, every entry and every byte equal, on
every named case; buffers off their alignment; reruns; a planted 432 x 240 video; and inpaint_video with the detected masks."""
import importlib

import numpy as np
import pytest
import torch

from e2fgvi_amd import ops, video
from tests import line_scratch_cases as C
from tests.test_gpu_video_restore import _stand_in_model
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

LINE_SYMBOLS = ("e2fgvi_line_sums", "e2fgvi_line_columns", "e2fgvi_line_paint")
_CACHE = {}


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.zeros(a.nbytes + shift, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


def _run(c, dev, shift=0, fill=None):
    """the dict of C.KEYS of the three entries on a case; frames and masks `shift` bytes off an allocation's start"""
    L, H, W = c["L"], c["H"], c["W"]
    S = ops.line_sums(_up(c["frames"], dev, shift), c["rows"])
    cand, cnt, col, b0, b1 = ops.line_columns(S, c["rows"], c["tau"], c["gap"], c["side"], c["drift"], c["coverage"])
    scene = torch.from_numpy(C.scene_of_np(L, c["scenes"])).to(dev)
    out = _up(np.full((L, H, W), 0 if fill is None else fill, np.uint8), dev, shift) if shift or fill is not None else None
    keep, counts, masks = ops.line_paint(col, b0, b1, scene, H, c["rows"], c["drift"], c["span"], c["persist"], c["radius"], out=out)
    got = dict(S=S, cand=cand, cnt=cnt, col=col, b0=b0, b1=b1, keep=keep, counts=counts, masks=masks)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _assert_equal(got, want, what):
    for k in C.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


# ------------------------------------------------------------------------------------------------ the three entries
@pytest.mark.parametrize("name", C.NAMES)
def test_entries_are_the_restatement(dev, name):
    """S, the candidate bits, cnt, col, b0, b1, keep, counts and the mask bytes, on every named case -- among them W mod 4 = 1 and
    2 (small_9x13, nondefault_12x75x110: every parameter off its default), less than a workgroup of pixels (small_9x13) and more
    than one tile of columns (wide_20x300) -- with the byte buffers on and one byte off an allocation's start, and into a mask
    buffer that was full of something else: every byte is written, the zeros of a tile without a kept column included"""
    c, want = C.case(name), C.want(name)
    for shift, fill in ((0, None), (1, None), (0, 77), (3, 200)):
        got = _run(c, dev, shift, fill)
        print(name, "shift", shift, "fill", fill, "candidates", int((got["cand"] > 0).sum()), "kept", got["counts"].tolist())
        _assert_equal(got, want, (name, shift, fill))


def test_runs_are_the_same_bits(dev):
    for name in ("nondefault_12x75x110", "wide_20x300"):
        c = C.case(name)
        first = _run(c, dev)
        for _ in range(5):
            again = _run(c, dev)
            assert all(np.array_equal(first[k], again[k]) for k in C.KEYS)
    fr = np.array(C.case("nondefault_12x75x110")["frames"])
    kw = C.settings(C.case("nondefault_12x75x110"))
    a = video.detect_line_scratches(fr, device=dev, **kw)
    b = video.detect_line_scratches(fr, device=dev, **kw)
    assert a.tobytes() == b.tobytes() and a.any()


def test_arguments_are_checked(dev):
    c, want = C.case("bright_w1"), C.want("bright_w1")
    fr = _up(c["frames"], dev)
    # host inputs are uploaded
    S = ops.line_sums(np.array(c["frames"]), 16)
    assert S.is_cuda and S.dtype == torch.int32 and np.array_equal(S.cpu().numpy(), want["S"])
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(frames=fr[:, :, ::2]), "contiguous"), (dict(rows=3), "rows"), (dict(rows=65), "rows"), (dict(rows=True), "rows"),
                     (dict(rows=16.5), "rows")):
        with pytest.raises(ValueError, match=what):
            ops.line_sums(**dict(dict(frames=fr, rows=16), **kw))
    good = dict(S=S, rows=16, tau=6, gap=2, side=3, drift=1, coverage=50)
    for kw, what in ((dict(S=S.float()), "S"), (dict(S=S[0]), "S"), (dict(S=S[:, :, ::2]), "contiguous"), (dict(tau=255), "tau"),
                     (dict(tau=-1), "tau"), (dict(gap=5), "gap"), (dict(side=0), "side"), (dict(side=9), "side"), (dict(drift=3), "drift"),
                     (dict(coverage=0), "coverage"), (dict(coverage=101), "coverage"), (dict(coverage=True), "coverage"),
                     (dict(rows=2), "rows")):
        with pytest.raises(ValueError, match=what):
            ops.line_columns(**dict(good, **kw))
    col, b0, b1 = (_up(want[k], dev) for k in ("col", "b0", "b1"))
    scene = torch.zeros(c["L"], dtype=torch.int32, device=dev)
    good = dict(col=col, b0=b0, b1=b1, scene=scene, H=c["H"], rows=16, drift=1, span=2, persist=3, radius=2)
    for kw, what in ((dict(col=col.int()), "col"), (dict(col=col[:, 0]), "col"), (dict(b0=b0.long()), "b0"), (dict(b1=b1[:, :1]), "b1"),
                     (dict(scene=scene[:-1]), "scene"), (dict(scene=scene.long()), "scene"), (dict(H=-1), "H"), (dict(H=True), "H"),
                     (dict(span=5), "span"), (dict(persist=6), "persist"), (dict(persist=0), "persist"), (dict(radius=17), "radius"),
                     (dict(drift=-1), "drift"), (dict(out=np.zeros((c["L"], c["H"], c["W"]), np.uint8)), "out"),
                     (dict(out=torch.zeros((c["L"], c["H"], c["W"] + 1), dtype=torch.uint8, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.line_paint(**dict(good, **kw))
    # any non-zero byte of col is a column
    keep, counts, masks = ops.line_paint(col * 200, b0, b1, scene, c["H"], 16, 1, 2, 3, 2)
    assert np.array_equal(keep.cpu().numpy(), want["keep"]) and np.array_equal(masks.cpu().numpy(), want["masks"])


# ------------------------------------------------------------------------------------------------ detect_line_scratches
@pytest.mark.parametrize("name", C.NAMES)
def test_detect_line_scratches_is_the_restatement(dev, name):
    c, want = C.case(name), C.want(name)
    with launch_trace() as trace:
        masks, counts = video.detect_line_scratches(np.array(c["frames"]), return_counts=True, device=dev, **C.settings(c))
    assert masks.dtype == np.uint8 and counts.dtype == np.int32
    assert np.array_equal(masks, want["masks"]) and np.array_equal(counts, want["counts"])
    assert [sum(r["symbol"] == s for r in trace) for s in LINE_SYMBOLS] == [1, 1, 1]
    got = video.detect_line_scratches(_up(c["frames"], dev), **C.settings(c))            # a device tensor is used where it is
    assert isinstance(got, np.ndarray) and np.array_equal(got, want["masks"])


def test_planted_432x240_video_is_the_restatement(dev):
    """twelve frames of noise around mid grey with three wandering scratches (line_scratch_cases.plant), a cut, the defaults"""
    base = np.repeat(np.random.RandomState(21).randint(100, 140, (12, 240, 432, 1)), 3, axis=-1).astype(np.uint8)
    frames, marks = C.plant(base, seed=2)
    want = C.detect_np(frames, scenes=[7])
    masks, counts = video.detect_line_scratches(frames, scenes=[7], return_counts=True, device=dev)
    recall, strays = C.recall_and_strays(masks, marks)
    print("kept per frame", counts.tolist(), "recall %.4f" % recall, "strays", strays)
    assert masks.shape == (12, 240, 432) and masks.tobytes() == want["masks"].tobytes() and np.array_equal(counts, want["counts"])
    assert counts.all() and recall >= 0.95 and strays == 0
    assert video.detect_line_scratches(frames, scenes=[7], device=dev).tobytes() == masks.tobytes()


# ------------------------------------------------------------------------------------------------ with the driver
def _net(dev, model="e2fgvi_hq"):
    """the generator with synthetic weights; e2fgvi_hq is the one that takes frames of any size"""
    if model not in _CACHE:
        from e2fgvi_amd.synth import synth_state_dict
        net = importlib.import_module("model." + model).InpaintGenerator()
        net.load_state_dict(synth_state_dict(model, "stress", 0))
        _CACHE[model] = net.to(dev).eval()
    return _CACHE[model]


def _scratched_clip(L, H, W, seed):
    rng = np.random.RandomState(seed)
    g = rng.randint(110, 131, (L, H, W)).astype(np.int64)
    g[:, :, 30] += 60
    g[:, :, 61:63] -= 55
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=-1).astype(np.uint8))


def test_inpaint_video_with_the_detected_masks(dev):
    """the masks go into inpaint_video(size=(108, 60), restore=True) as any others do: what it returns differs from the caller's
    frames only where restore pastes -- the painted mask at the model's size, dilated there, NEAREST back (video.paste_mask)"""
    net = _net(dev)
    frames = _scratched_clip(6, 64, 96, 22)
    masks = video.detect_line_scratches(frames, device=dev)
    assert masks[:, :, 28:33].all() and masks[:, :, 59:65].all() and not masks[:, :, :27].any() and not masks[:, :, 66:].any()
    with torch.no_grad():
        out = video.inpaint_video(net, frames, masks, size=(108, 60), restore=True)
    pasted = video.paste_mask(masks, (64, 96), (108, 60), device=dev).cpu().numpy() != 0
    changed = (out != frames).any(axis=-1)
    print("painted", int((masks > 0).sum()), "pasted", int(pasted.sum()), "changed", int(changed.sum()))
    assert out.shape == frames.shape and out.dtype == np.uint8
    assert not (changed & ~pasted).any() and changed.any() and pasted[masks > 0].all()
    assert np.array_equal(out[~pasted], frames[~pasted])


def test_ordinary_masks_launch_no_line_kernel(dev):
    f = _scratched_clip(6, 60, 108, 23)
    m = np.zeros((6, 60, 108), np.uint8)
    m[:, 20:40, 30:70] = 1
    stub = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    with launch_trace() as trace:
        video.inpaint_video(stub, f, m, device=dev)
        video.inpaint_video(stub, f, m, device=dev, size=(108, 60), restore=True, scenes=[3])
    assert len(trace) > 0 and not any(r["symbol"].startswith("e2fgvi_line_") for r in trace)
