"""The local deflicker on the device: ops.flicker_local_hist, ops.flicker_local_curves and ops.flicker_local_apply
(csrc/flicker_local.hip) and video.deflicker_local against the numpy restatement of tests/flicker_local_cases.py, every word and
every byte equal, on every named case; buffers off their alignment inside sentinel bytes; in place; reruns; one cell against
video.deflicker; and the planted 432 x 240 tennis video, with a cut and under the conditions the grids are judged on."""
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import flicker_cases as C
from tests import flicker_local_cases as LC
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCAL_SYMBOLS = ("e2fgvi_flicker_local_hist", "e2fgvi_flicker_local_curves", "e2fgvi_flicker_local_apply")
FRAMED = tuple(n for n in LC.NAMES if LC.case(n)["frames"] is not None)
GUARD, SENTINEL = 256, 0xA5


class _Embedded:
    """an array on the device inside a larger buffer of sentinel bytes, its first byte `shift` bytes off a 256-byte boundary"""

    def __init__(self, a, dev, shift=0):
        a = np.array(a)                                 # a writable copy: the cases are read-only
        self.buf = torch.full((a.nbytes + 2 * GUARD + shift,), SENTINEL, dtype=torch.uint8, device=dev)
        self.lo, self.hi = GUARD + shift, GUARD + shift + a.nbytes
        self.t = self.buf[self.lo:self.hi].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))

    def intact(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.hi:] == SENTINEL).all())


def _up(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _run(c, dev, shift=0, fill=0, in_place=False):
    """the dict of LC.KEYS of the three entries on a case; frames, hist and out inside sentinel bytes, frames and out `shift` bytes
    off a dword, hist and out full of `fill` beforehand"""
    L, (gy, gx) = c["L"], c["grid"]
    scene = torch.from_numpy(C.scene_of_np(L, c["scenes"])).to(dev)
    if c["frames"] is None:                             # curves alone
        Q, d16 = ops.flicker_local_curves(_up(c["hist"], dev), scene, c["H"], c["W"], c["span"], c["max_shift"])
        return dict(Q=Q.cpu().numpy(), d16=d16.cpu().numpy())
    H, W = c["H"], c["W"]
    fr = _Embedded(c["frames"], dev, shift)
    hb = _Embedded(np.full((L, gy, gx, 256), fill, np.int32), dev)
    hist = ops.flicker_local_hist(fr.t, c["grid"], out=hb.t)
    assert hist.data_ptr() == hb.t.data_ptr()
    Q, d16 = ops.flicker_local_curves(hist, scene, H, W, c["span"], c["max_shift"])
    if in_place:
        out = ops.flicker_local_apply(fr.t, d16, out=fr.t)
        assert out.data_ptr() == fr.t.data_ptr()
        ob = fr
    else:
        ob = _Embedded(np.full((L, H, W, 3), fill, np.uint8), dev, shift)
        out = ops.flicker_local_apply(fr.t, d16, out=ob.t)
        assert np.array_equal(fr.t.cpu().numpy(), c["frames"])             # the input is only read
    assert fr.intact() and hb.intact() and ob.intact()                    # nothing beside the buffers was written
    return {k: v.cpu().numpy() for k, v in dict(hist=hist, Q=Q, d16=d16, out=out).items()}


def _assert_equal(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


# ------------------------------------------------------------------------------------------------ the three entries
@pytest.mark.parametrize("name", LC.NAMES)
def test_entries_are_the_restatement(dev, name):
    """hist, Q, d16 and the output bytes on every named case with the byte buffers on, one and three bytes off a dword, inside
    sentinel bytes that must be intact afterwards, and into hist and out buffers that were full of something else: every word and
    byte is written, and none beside them"""
    c, want = LC.case(name), LC.want(name)
    for shift, fill in ((0, 0), (1, 77), (3, 200)):
        got = _run(c, dev, shift, fill)
        print(name, "shift", shift, "fill", fill, "max |d16|", int(np.abs(got["d16"]).max()))
        _assert_equal(got, want, LC.keys(name), (name, shift, fill))
        if c["frames"] is None:
            break


@pytest.mark.parametrize("name", FRAMED)
def test_apply_in_place_gives_the_same_bytes(dev, name):
    c, want = LC.case(name), LC.want(name)
    for shift in (0, 1):
        _assert_equal(_run(c, dev, shift, in_place=True), want, LC.KEYS, (name, shift))


def test_runs_are_the_same_bits(dev):
    for name in ("3x70x300_g34", "clip_g22"):
        c = LC.case(name)
        first = _run(c, dev)
        for _ in range(5):
            again = _run(c, dev)
            assert all(np.array_equal(first[k], again[k]) for k in LC.KEYS)


def test_cell_histograms_sum_to_the_frame_histogram(dev):
    for name in FRAMED:
        c = LC.case(name)
        fr = _up(c["frames"], dev)
        cells = ops.flicker_local_hist(fr, c["grid"])
        assert torch.equal(cells.sum(dim=(1, 2)).to(torch.int32), ops.flicker_hist(fr)), name


def test_arguments_are_checked(dev):
    c, want = LC.case("w2_30x42_g34"), LC.want("w2_30x42_g34")
    L, H, W, grid = c["L"], c["H"], c["W"], c["grid"]
    fr = _up(c["frames"], dev)
    # host inputs are uploaded
    hist = ops.flicker_local_hist(np.array(c["frames"]), grid)
    assert hist.is_cuda and hist.dtype == torch.int32 and np.array_equal(hist.cpu().numpy(), want["hist"])
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(grid=(0, 2)), "grid"), (dict(grid=(3, 9)), "grid"), (dict(grid=3), "grid"), (dict(grid=(True, 2)), "grid"),
                     (dict(grid=(2, 2, 2)), "grid"), (dict(grid=(2.0, 2)), "grid"), (dict(frames=fr[:, :2], grid=(3, 4)), "contiguous"),
                     (dict(frames=fr[:, :2].contiguous(), grid=(3, 4)), "grid"),
                     (dict(out=np.zeros((L, 3, 4, 256), np.int32)), "out"),
                     (dict(out=torch.zeros((L, 4, 3, 256), dtype=torch.int32, device=dev)), "out"),
                     (dict(out=torch.zeros((L, 3, 4, 256), dtype=torch.int64, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.flicker_local_hist(**dict(dict(frames=fr, grid=grid), **kw))
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    good = dict(hist=hist, scene=scene, H=H, W=W, span=4, max_shift=32)
    for kw, what in ((dict(hist=hist.float()), "hist"), (dict(hist=hist[0]), "hist"), (dict(hist=hist[..., ::2]), "contiguous"),
                     (dict(hist=hist[..., :255].contiguous()), "hist"), (dict(hist=hist.repeat(1, 3, 1, 1)), "hist"),
                     (dict(scene=scene[:-1]), "scene"), (dict(scene=scene.long()), "scene"), (dict(H=-1), "H"), (dict(W=True), "W"),
                     (dict(H=1.5), "H"), (dict(H=1 << 14, W=1 << 13), "H W"), (dict(H=2), "grid"), (dict(W=3), "grid"),
                     (dict(span=-1), "span"), (dict(span=9), "span"), (dict(span=True), "span"), (dict(max_shift=0), "max_shift"),
                     (dict(max_shift=65), "max_shift"), (dict(max_shift=2.5), "max_shift")):
        with pytest.raises(ValueError, match=what):
            ops.flicker_local_curves(**dict(good, **kw))
    Q, d16 = ops.flicker_local_curves(np.array(want["hist"]), np.zeros(L, np.int32), H, W, 4, 32)
    assert Q.is_cuda and np.array_equal(Q.cpu().numpy(), want["Q"]) and np.array_equal(d16.cpu().numpy(), want["d16"])
    for kw, what in ((dict(frames=fr.int()), "frames"), (dict(frames=fr[0]), "frames"), (dict(d16=d16.int()), "d16"),
                     (dict(d16=d16[:-1]), "d16"), (dict(d16=d16[..., ::2]), "contiguous"), (dict(d16=d16[:, 0]), "d16"),
                     (dict(d16=d16.repeat(1, 3, 1, 1)), "d16"), (dict(frames=fr[:, :2].contiguous()), "grid"),
                     (dict(out=np.zeros(fr.shape, np.uint8)), "out"),
                     (dict(out=torch.zeros((L, H, W + 1, 3), dtype=torch.uint8, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.flicker_local_apply(**dict(dict(frames=fr, d16=d16), **kw))
    # an output that overlaps the frames without being them is refused by the entry, before any launch
    flat = torch.zeros(fr.numel() + 12, dtype=torch.uint8, device=dev)
    src, dst = flat[:fr.numel()].view(fr.shape).copy_(fr), flat[12:].view(fr.shape)
    with pytest.raises(lib.HipError, match="overlap"):
        ops.flicker_local_apply(src, d16, out=dst)
    assert np.array_equal(src.cpu().numpy(), c["frames"])
    # no frame and no pixel: results of the right shapes, zeros
    for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
        e = torch.zeros(shape, dtype=torch.uint8, device=dev)
        h = ops.flicker_local_hist(e, (2, 3), out=torch.full((shape[0], 2, 3, 256), 7, dtype=torch.int32, device=dev))
        q, dd = ops.flicker_local_curves(h, torch.zeros(shape[0], dtype=torch.int32, device=dev), shape[1], shape[2], 4, 32)
        o = ops.flicker_local_apply(e, dd)
        assert h.shape == (shape[0], 2, 3, 256) and not h.any() and not q.any() and not dd.any() and o.shape == shape


# ------------------------------------------------------------------------------------------------ deflicker_local
@pytest.mark.parametrize("name", FRAMED)
def test_deflicker_local_is_the_restatement(dev, name):
    c, want = LC.case(name), LC.want(name)
    host = np.array(c["frames"])
    with launch_trace() as trace:
        out, d16 = video.deflicker_local(host, return_curves=True, device=dev, **LC.settings(c))
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and isinstance(d16, np.ndarray) and d16.dtype == np.int16
    assert np.array_equal(out, want["out"]) and np.array_equal(d16, want["d16"]) and np.array_equal(host, c["frames"])
    assert [sum(r["symbol"] == s for r in trace) for s in LOCAL_SYMBOLS] == [1, 1, 1]
    assert not any(r["symbol"] in ("e2fgvi_flicker_hist", "e2fgvi_flicker_curves", "e2fgvi_flicker_apply") for r in trace)
    plain = video.deflicker_local(host, device=dev, **LC.settings(c))
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, want["out"])
    # a device tensor is used where it is and a device tensor comes back
    x = _Embedded(c["frames"], dev, 1)
    got, gd = video.deflicker_local(x.t, return_curves=True, **LC.settings(c))
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and gd.is_cuda and gd.dtype == torch.int16
    assert np.array_equal(got.cpu().numpy(), want["out"]) and np.array_equal(gd.cpu().numpy(), want["d16"])
    assert np.array_equal(x.t.cpu().numpy(), c["frames"]) and x.intact()
    # span == 0: no launch, the caller's bytes
    with launch_trace() as trace:
        same, zd = video.deflicker_local(host, grid=c["grid"], span=0, return_curves=True, device=dev)
        on = video.deflicker_local(x.t, grid=c["grid"], span=0)
    assert not any(r["symbol"].startswith("e2fgvi_flicker_") for r in trace)
    assert same.tobytes() == c["frames"].tobytes() and zd.shape == (c["L"],) + c["grid"] + (256,) and not zd.any()
    assert on.is_cuda and np.array_equal(on.cpu().numpy(), c["frames"])


def test_no_frame_and_no_pixel_launch_nothing(dev):
    with launch_trace() as trace:
        for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
            out, d16 = video.deflicker_local(np.zeros(shape, np.uint8), grid=(2, 3), return_curves=True, device=dev)
            assert out.shape == shape and out.dtype == np.uint8 and d16.shape == (shape[0], 2, 3, 256) and d16.dtype == np.int16
    assert not any(r["symbol"].startswith("e2fgvi_flicker_") for r in trace)


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.case(n)["frames"] is not None])
def test_one_cell_is_deflicker_on_the_device(dev, name):
    """grid=(1,1) on flicker_cases' own cases: the bytes of video.deflicker on the device, and d16 rounds to its d"""
    c = C.case(name)
    x = _up(c["frames"], dev)
    want, d = video.deflicker(x, return_curves=True, **C.settings(c))
    got, d16 = video.deflicker_local(x, grid=(1, 1), return_curves=True, **C.settings(c))
    assert got.data_ptr() != x.data_ptr() and torch.equal(got, want)
    assert d16.shape == (c["L"], 1, 1, 256) and torch.equal((d16[:, 0, 0].to(torch.int32) + 8) >> 4, d.to(torch.int32))
    assert np.array_equal(got.cpu().numpy(), C.want(name)["out"])


def test_planted_432x240_video_with_a_cut_is_the_restatement(dev):
    """the 25 frames of tests/golden/tennis25.npz under flicker_local_cases.plant_tilted(seed 1) with a cut at frame 12 and the
    defaults: the bytes of the restatement, and the same bytes from a second call"""
    planted = LC.tennis(ROOT, 1)
    want = LC.deflicker_local_np(planted, scenes=[12], **LC.DEFAULTS)
    out, d16 = video.deflicker_local(np.array(planted), scenes=[12], return_curves=True, device=dev)
    print("max |d16|", int(np.abs(d16).max()))
    assert out.shape == (25, 240, 432, 3) and out.tobytes() == want["out"].tobytes() and np.array_equal(d16, want["d16"])
    assert video.deflicker_local(np.array(planted), scenes=[12], device=dev).tobytes() == out.tobytes()


@pytest.mark.parametrize("seed", [1, 2])
def test_planted_tilted_flicker_on_tennis25_on_the_device(dev, seed):
    """the conditions of tests/test_video_flicker_local.py on the device's output, which is the restatement's bytes: block_roughness
    at (2,2) at most 0.5 of the global video.deflicker's on the same planted video, at (3,4) at most 0.4"""
    planted = np.array(LC.tennis(ROOT, seed))
    glob = video.deflicker(planted, device=dev)
    assert glob.tobytes() == LC.tennis(ROOT, (seed, "global")).tobytes()
    rough = LC.block_roughness(glob)
    for grid, bound in (((2, 2), 0.5), ((3, 4), 0.4)):
        out = video.deflicker_local(planted, grid=grid, device=dev)
        after = LC.block_roughness(out)
        print("seed", seed, "grid", grid, "block_roughness", LC.block_roughness(planted), "global", rough, "local", after, "ratio",
              after / rough)
        assert out.tobytes() == LC.tennis(ROOT, (seed, grid)).tobytes()
        assert after <= bound * rough


def test_clean_tennis25_at_the_default_grid_on_the_device(dev):
    clean = np.array(LC.tennis(ROOT, None))
    out = video.deflicker_local(clean, device=dev)
    diff = np.abs(out.astype(np.int64) - clean).max(axis=-1)
    print("changed by more than 3 levels", float((diff > 3).mean()), "largest change", int(diff.max()))
    assert out.tobytes() == LC.tennis(ROOT, (None, (2, 2))).tobytes()
    assert (diff > 3).mean() <= 0.03 and diff.max() <= LC.DEFAULTS["max_shift"]
