"""Static overlays, host side: the numpy restatement of video.overlay_mask (tests/overlay_cases.py) on hand-counted frames and on the
tennis fixture with a drawn overlay, and the argument checks of overlay_mask and inpaint_video that need no device.  The kernels
and the driver are compared with the restatement in tests/test_gpu_video_overlay.py."""
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import overlay_cases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_on_hand_counted_frames():
    """a 1 x 4 row of lumas 10 10 50 50 held for three frames, then the same with the last frame mirrored"""
    grey = lambda row: np.repeat(np.asarray(row, np.uint8)[None, :, None], 3, -1)
    assert O.luma_np(grey([10, 50, 255])).tolist() == [[10, 50, 255]]               # 77 + 150 + 29 = 256: greys keep their value
    assert O.luma_np(np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)).tolist() == [77, 149, 29]
    f = np.stack([grey([10, 10, 50, 50])] * 3)
    sx, sy, m = O.stats_np(f)
    assert sx.tolist() == [[0, 120, 120, 0]] and sy.tolist() == [[0, 0, 0, 0]] and m.tolist() == [[0, 120, 120, 0]]
    assert O.edges_np((sx, sy, m), 3, 40, 256).tolist() == [[False, True, True, False]]        # M = g_min L and |S| = M: both at equality
    assert not O.edges_np((sx, sy, m), 3, 41, 256).any()
    f[2] = f[2, :, ::-1]
    sx, sy, m = O.stats_np(f)
    assert sx.tolist() == [[0, 40, 40, 0]] and m.tolist() == [[0, 120, 120, 0]]
    assert not O.edges_np((sx, sy, m), 3, 32, 86).any() and O.edges_np((sx, sy, m), 3, 32, 85).sum() == 2   # 256 * 40 / 120 = 85.3
    # a column: the same along y; a single pixel has no gradient at all
    sx, sy, m = O.stats_np(np.stack([grey([10, 10, 50, 50])] * 3).transpose(0, 2, 1, 3))
    assert sy.ravel().tolist() == [0, 120, 120, 0] and not sx.any()
    assert not O.stats_np(np.full((4, 1, 1, 3), 200, np.uint8)).any()


def test_restatement_kinds_are_what_they_are_for():
    L, H, W = 6, 9, 14
    sx, sy, m = O.stats_np(O.content("vstep", L, H, W))
    assert not sy.any() and np.array_equal(np.abs(sx), m) and m.max() == 120 * L
    assert O.edges_np((sx, sy, m), L, 32, 256).sum() == 2 * H and not O.edges_np((sx, sy, m), L, 121, 256).any()
    sx, sy, m = O.stats_np(O.content("checker", L, H, W))
    assert not sx.any() and not sy.any() and m[1:-1, 1:-1].min() == m.max() == 510 * L
    assert not O.edges_np((sx, sy, m), L, 32, 1).any()
    sx, sy, m = O.stats_np(O.content("step255", L, H, W))
    assert np.abs(sy).max() == 255 * L == np.abs(sx).max()
    assert not O.stats_np(O.content("zeros", L, H, W)).any()


def test_dilation_is_clipped_at_the_frame():
    E = np.zeros((5, 7), bool)
    E[0, 0] = E[4, 6] = True
    D = O.dilate_np(E, 1)
    assert D.sum() == 8 and D[:2, :2].all() and D[3:, 5:].all()
    assert np.array_equal(O.dilate_np(E, 0), E) and O.dilate_np(E, 16).all()


def test_fill_and_filter():
    """a ring's inside is filled, a C's is not (its complement reaches the frame), a small blob goes"""
    D = np.zeros((20, 30), bool)
    D[2:9, 2:9] = True
    D[4:7, 4:7] = False                                 # a ring: 40 pixels, 9 inside
    D[11:18, 2:9] = True
    D[13:16, 4:9] = False                               # a C, open to the right: 34 pixels
    D[0:3, 26:30] = True                                # 12 pixels in the corner
    D[1, 27] = False                                    # enclosed by them: filled although the component touches the frame's edge
    m = O.fill_and_filter_np(D, 13)
    assert set(np.unique(m).tolist()) == {0, 255} and m.dtype == np.uint8
    want = D.copy()
    want[4:7, 4:7] = True
    want[0:3, 26:30] = False
    assert np.array_equal(m > 0, want)
    assert (O.fill_and_filter_np(D, 12) > 0).sum() == want.sum() + 12
    assert not O.fill_and_filter_np(D, 50).any() and not O.fill_and_filter_np(np.zeros((4, 4), bool), 1).any()
    # the complement is 8-connected too: a diamond around (1, 1) leaks through its corners, to (0, 0) on the frame's edge for one
    D = np.zeros((6, 6), bool)
    D[0, 1] = D[1, 0] = D[1, 2] = D[2, 1] = True
    assert not O.fill_and_filter_np(D, 1)[1, 1] and (O.fill_and_filter_np(D, 1) > 0).sum() == 4


def test_tennis_plain_has_no_overlay():
    assert not O.clip_mask("plain").any()
    assert O.clip("plain").shape == (25, 240, 432, 3)


@pytest.mark.parametrize("name", ["alpha1.0", "alpha0.5"])
def test_tennis_with_a_drawn_overlay(name):
    """a ring and a row of bars drawn into the 25 frames of the slow pan, opaque and half transparent: every overlay pixel is found,
    next to nothing farther than 8 pixels from it, and the disc inside the ring is part of the mask"""
    truth, inside = O.overlay_truth()
    assert truth[120:].sum() == 8 * 8 * 18 and truth[:120].sum() > 1300 and inside.sum() > 400 and not (truth & inside).any()
    m = O.clip_mask(name)
    assert m.dtype == np.uint8 and m.shape == (240, 432) and set(np.unique(m).tolist()) == {0, 255}
    M = m > 0
    recall = (M & truth).sum() / truth.sum()
    stray = int((M & ~O.dilate_np(truth, 8)).sum())
    print("%s: %d mask pixels, recall %.4f, %d farther than 8 px from the overlay" % (name, M.sum(), recall, stray))
    assert recall >= 0.99
    assert stray <= 16
    assert M[inside].all()


def test_a_still_clip_exceeds_max_fraction():
    f = O.clip("still")
    _, n = O.dilated_np(O.stats_np(f), 25, 32, 224, 3)
    assert n > 0.25 * 240 * 432
    with pytest.raises(ValueError, match="static"):
        O.mask_np(f)
    # and the unmoved scenery is what the mask would be: most of the frame with a threshold that lets it through
    assert (O.mask_np(f, max_fraction=1.0) > 0).sum() > 0.25 * 240 * 432


def test_overlay_mask_checks_its_arguments_before_the_library(monkeypatch):
    """every refusal comes from the arguments and the shapes alone: the library is never loaded, nothing is uploaded"""
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(lib, "load", no_library)
    monkeypatch.setattr(video, "_upload", lambda *a, **k: no_library())
    f = np.zeros((4, 6, 8, 3), np.uint8)
    bad = dict(g_min=(0, -1, 1.5, True, None, "3"), coherence=(0, 257, 1.5, True), radius=(-1, 17, 0.5, False, True),
               min_area=(0, 2.5, True), max_fraction=(0, 0.0, 1.01, -0.5, True, None))
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=key):
                video.overlay_mask(f, **{key: v})
    with pytest.raises(ValueError, match="frames"):
        video.overlay_mask(f[..., :2])
    with pytest.raises(ValueError, match="frames"):
        video.overlay_mask(f[0])
    with pytest.raises(ValueError, match="at least one frame"):
        video.overlay_mask(f[:0])
    # no pixels: an empty mask, and no launch
    for shape in ((3, 0, 8, 3), (3, 6, 0, 3)):
        m = video.overlay_mask(np.zeros(shape, np.uint8))
        assert m.shape == shape[1:3] and m.dtype == np.uint8
    assert (video.OVERLAY_G_MIN, video.OVERLAY_COHERENCE, video.OVERLAY_RADIUS, video.OVERLAY_MIN_AREA,
            video.OVERLAY_MAX_FRACTION) == tuple(O.DEFAULTS[k] for k in ("g_min", "coherence", "radius", "min_area", "max_fraction"))


def test_inpaint_video_refuses_other_strings_for_masks():
    f = np.zeros((12, 8, 8, 3), np.uint8)

    def model(x, n):
        raise AssertionError("no forward")

    for bad in ("bogus", "", "Overlay", "auto"):
        with pytest.raises(ValueError, match="overlay"):
            video.inpaint_video(model, f, bad, device="cpu")
    # the string passes the checks: on a host without a device the call gets as far as the refusal of the CPU device
    with pytest.raises(RuntimeError, match="no CPU path"):
        video.inpaint_video(model, f, "overlay", device="cpu")
    # the planners keep asking for masks
    for fn in (video.hole_regions, video.track_regions):
        with pytest.raises((ValueError, TypeError, AttributeError)):
            fn("overlay", (8, 8), (108, 60), device="cpu")


def test_header_and_binding_declare_the_entries():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    stats = re.search(r"int e2fgvi_overlay_stats\(([^;]*)\);", header)
    edges = re.search(r"int e2fgvi_overlay_edges\(([^;]*)\);", header)
    assert stats and edges
    names = lambda m: [a.split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]
    assert names(stats) == ["frames", "L", "H", "W", "stats", "stream"]
    assert names(edges) == ["stats", "L", "H", "W", "g_min", "coherence", "radius", "out", "count", "stream"]
    for name, n in (("e2fgvi_overlay_stats", 6), ("e2fgvi_overlay_edges", 10)):
        res, args = lib.SYMBOLS[name]
        assert len(args) == n and args[-1] is lib._fp
    assert lib.ABI_VERSION == 9                          # symbols were only added
    assert (ops.OVERLAY_TILE_W, ops.OVERLAY_TILE_H, ops.OVERLAY_CHUNK, ops.OVERLAY_RADIUS_MAX, ops.OVERLAY_FRAMES_MAX) == (64, 32, 8, 16, 1 << 22)
