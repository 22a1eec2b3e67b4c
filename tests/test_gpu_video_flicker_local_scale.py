"""The local deflicker past the sizes of the other tests, as tests/test_gpu_video_scale.py does for the global passes (the helpers
are those of tests/big_video.py).

Part A: the three entries on the 3 x 70 x 300 case at (3,4) tiled along L until the frames pass 2^32 bytes, every tile a scene of
its own; hist, Q, d16 and the output against the restatement's result for one tile, every word and byte, on the device; in place
too.  A kernel that forms a byte offset in 32 bits reads or writes another phase of the tile: the buffer is asserted to show that
(big_video.wrap_is_visible), and the restatement on the bytes such a kernel would fetch gives another result.

Part B: 65 540 frames of 2 x 2 at (2,2), every cell one pixel: the histogram and the apply pass launch the frames in slabs of
65 535 (the grid's y axis), the curves pass is one launch of 4 L workgroups; a cut lies inside the second slab."""
import numpy as np
import pytest
import torch

from e2fgvi_amd import ops
from tests import big_video as B
from tests import flicker_cases as C
from tests import flicker_local_cases as LC

pytestmark = pytest.mark.gpu

SLAB = 65535
FRAMES_CASE = "3x70x300_g34"
L_B, CUT_B = 65540, 65537


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                       # a writable copy: the cases are read-only


def test_flicker_local_past_4gib(dev):
    with B.measured("flicker_local_hist / flicker_local_curves / flicker_local_apply", dev):
        c, want = LC.case(FRAMES_CASE), LC.want(FRAMES_CASE)
        k, base = c["L"], c["frames"]
        assert c["scenes"] is None and not np.array_equal(want["out"], base)
        fr = B.tiled(base, B.tiles_past(B.nbytes(base)), dev)
        B.wrap_is_visible(fr, B.nbytes(base), "flicker_local")
        assert B.WRAP % B.nbytes(base[:1]) != 0                        # a frame does not divide 2^32 either
        print("L", fr.shape[0], "bytes", fr.numel())
        scene = B.scene_of(fr.shape[0], k, dev)
        hist = ops.flicker_local_hist(fr, c["grid"])
        B.assert_tiled(hist, want["hist"], "flicker_local_hist")
        Q, d16 = ops.flicker_local_curves(hist, scene, c["H"], c["W"], c["span"], c["max_shift"])
        B.assert_tiled(Q, want["Q"], "flicker_local_curves Q")
        B.assert_tiled(d16, want["d16"], "flicker_local_curves d16")
        out = ops.flicker_local_apply(fr, d16)
        B.assert_tiled(out, want["out"], "flicker_local_apply")
        B.assert_tiled(fr, base, "flicker_local frames")               # the input is only read
        B.assert_tiled(ops.flicker_local_apply(out, d16, out=out), LC.apply_np(want["out"], want["d16"]), "flicker_local_apply in place")


def test_a_wrapped_offset_would_be_seen():
    """on the host: the restatement on the bytes a kernel with one 32-bit offset would fetch for the first tile past 2^32 gives other
    histograms and another output than the expected ones"""
    c, want = LC.case(FRAMES_CASE), LC.want(FRAMES_CASE)
    wrong = B.wrapped_tile(c["frames"])
    assert not np.array_equal(wrong, c["frames"])
    assert not np.array_equal(LC.hist_np(wrong, c["grid"]), want["hist"])
    assert not np.array_equal(LC.apply_np(wrong, want["d16"]), want["out"])


def test_flicker_local_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 2 x 2 at (2,2).  Frame 65 535, the first of the second slab, is averaged over frames 65 531 .. 65 536 (the cut
    lies at 65 537).  The histograms and the output against the restatement on the whole video; the curves, whose nodes the
    restatement walks level by level in Python, on its first 80 and its last 100 frames."""
    with B.measured("flicker_local slabs", dev):
        span, max_shift, grid = 4, 32, (2, 2)
        rng = np.random.RandomState(81)
        fr = np.clip(rng.randint(40, 216, (L_B, 1, 1, 1)) + rng.randint(-30, 31, (L_B, 2, 2, 3)), 0, 255).astype(np.uint8)
        so = C.scene_of_np(L_B, [CUT_B])
        x = _dev(fr, dev)
        hist = ops.flicker_local_hist(x, grid)
        # every cell is one pixel: its histogram is one count at the pixel's luma
        want_hist = (C.luma(fr)[..., None] == np.arange(256)).astype(np.int32)
        assert np.array_equal(want_hist[:50], LC.hist_np(fr[:50], grid)) and np.array_equal(hist.cpu().numpy(), want_hist)
        Q, d16 = ops.flicker_local_curves(hist, _dev(so, dev), 2, 2, span, max_shift)
        Q, d16 = Q.cpu().numpy(), d16.cpu().numpy()
        for a, b in ((0, 80), (L_B - 100, L_B)):
            wq, wd = LC.curves_np(want_hist[a:b], so[a:b], 2, 2, span, max_shift)
            lo, hi = (a, b - span) if a == 0 else (a + span, b)        # the frames whose whole window lies in [a, b)
            assert np.array_equal(Q[a:b], wq) and np.array_equal(d16[lo:hi], wd[lo - a:hi - a]), (a, b)
        assert d16[SLAB].any() and d16[CUT_B].any()
        want = LC.apply_np(fr, d16)
        assert not np.array_equal(want[SLAB:], fr[SLAB:])
        got = ops.flicker_local_apply(x, _dev(d16, dev)).cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())
