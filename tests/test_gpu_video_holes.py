"""inpaint_video(region="holes") on the device: the component labelling of the masks' footprint (csrc/video.hip
hole_footprint_kernel, label_*_kernel) against the flood-fill restatement of tests/hole_label_cases.py, every integer equal, and
the driver against its definition -- one explicit-box call per planned region, pasted into the caller's frames -- byte for byte."""
import ctypes
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import hole_label_cases as C
from tests.test_gpu_video_restore import _stand_in_model, _toy_video
from tests.test_video_restore import frames

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tennis25.npz")
TW, TH = ops.LABEL_TILE_W, ops.LABEL_TILE_H
SIZES = [(1, 1), (1, 200), (130, 1), (5, 7), (33, 130), (2 * TH + 3, 2 * TW + 5)]


@functools.lru_cache(maxsize=None)
def _cases(Hm, Wm):
    """name -> (footprint, labels, boxes): the restatement runs once per size"""
    return {name: (U,) + C.components_np(U) for name, U in C.footprints(Hm, Wm, TH, TW).items()}


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    buf = torch.zeros(a.size + shift, dtype=torch.uint8, device=dev)
    out = buf[shift:].view(a.shape).copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert out.is_contiguous() and out.data_ptr() % 16 == shift
    return out


def _check(got, labels, boxes, what):
    gl, gb = got
    assert gl.is_cuda and gl.dtype == torch.int32 and tuple(gl.shape) == labels.shape, what
    assert gb.is_cuda and gb.dtype == torch.int32 and tuple(gb.shape) == boxes.shape, (what, tuple(gb.shape), boxes.shape)
    gl, gb = gl.cpu().numpy(), gb.cpu().numpy()
    assert np.array_equal(gl, labels), (what, int((gl != labels).sum()))
    assert np.array_equal(gb, boxes), what


@pytest.mark.parametrize("Hm,Wm", SIZES, ids=str)
def test_hole_components_is_the_restatement(dev, Hm, Wm):
    """one pixel, one row, one column, rows shorter than a 16-byte word, more than one tile along x at a pitch that is no multiple
    of 16, and three tiles along both axes with the last ones partial; per size every footprint of hole_label_cases.footprints,
    spread over L = 3 frames with the values 1 and 255, at a base as allocated and one byte further.  (33,130): a frame is 4290
    bytes, so frames 1 and 2 start 2 and 4 bytes off a 16-byte boundary either way."""
    for k, (name, (U, labels, boxes)) in enumerate(_cases(Hm, Wm).items()):
        v = C.video_of(U, name, L=3, seed=k)
        for shift in (0, 1):
            _check(ops.hole_components(_up(v, dev, shift)), labels, boxes, (name, shift))
    full = _cases(Hm, Wm)["full"]
    assert full[1].max() == 1 and full[2].tolist() == [[0, 0, Wm, Hm, Hm * Wm]]
    iso = _cases(Hm, Wm)["isolated"]
    assert len(iso[2]) == ((Hm + 1) // 2) * ((Wm + 1) // 2) and (iso[2][:, 4] == 1).all()
    if (Hm, Wm) == SIZES[-1]:
        count = lambda name: len(_cases(Hm, Wm)[name][2])
        assert [count(n) for n in ("checkerboard", "spiral", "comb_bottom", "comb_top", "two_combs")] == [1, 1, 1, 1, 2]
        assert [count(n) for n in ("corner_diag", "corner_anti", "corner_apart")] == [1, 1, 2]
        assert count("isolated") > 2 * 1024                                          # dense numbers from three scan blocks and more


def test_hole_components_beyond_one_round_of_the_scan(dev):
    """520 x 520 pixels are 265 blocks of 1024, more than the 256 the scan takes per round: small rectangles scattered over the image
    (the flood fill only walks hole pixels), the last two components in the last rows"""
    Hm = Wm = 520
    assert (Hm * Wm + 1023) // 1024 > 256
    rng = np.random.RandomState(5)
    U = np.zeros((Hm, Wm), bool)
    for _ in range(60):
        y, x = int(rng.randint(0, Hm - 12)), int(rng.randint(0, Wm - 12))
        U[y:y + int(rng.randint(1, 12)), x:x + int(rng.randint(1, 12))] = True
    U[Hm - 2:, Wm - 3:] = True
    U[Hm - 1, 0] = True
    labels, boxes = C.components_np(U)
    assert len(boxes) > 30 and labels[Hm - 1, 0] == len(boxes) == labels[Hm - 1, Wm - 1] + 1
    _check(ops.hole_components(_up(C.video_of(U, seed=1), dev, 1)), labels, boxes, "blobs")


def test_hole_components_without_frames_or_pixels(dev):
    labels, boxes = ops.hole_components(torch.zeros((0, 5, 7), dtype=torch.uint8, device=dev))
    assert tuple(labels.shape) == (5, 7) and not labels.any() and tuple(boxes.shape) == (0, 5)
    labels, boxes = ops.hole_components(torch.zeros((2, 0, 7), dtype=torch.uint8, device=dev))                # no launch
    assert tuple(labels.shape) == (0, 7) and tuple(boxes.shape) == (0, 5) and boxes.dtype == torch.int32


def test_hole_components_twice_is_the_same_bits(dev):
    Hm, Wm = SIZES[-1]
    for name in ("noise0.41", "spiral", "isolated"):
        U, labels, boxes = _cases(Hm, Wm)[name]
        md = _up(C.video_of(U, name, seed=2), dev)
        a, b = ops.hole_components(md), ops.hole_components(md)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        _check(a, labels, boxes, name)


def test_hole_label_does_not_depend_on_the_workspace(dev):
    """the C entries on a workspace full of 0xFF bytes, then again on the same workspace (which now holds the first call's ranks,
    footprint and offsets), with labels, count and boxes filled with other values in front of every call"""
    so = lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for Hm, Wm in ((5, 7), (33, 130), SIZES[-1]):
        U, labels, boxes = _cases(Hm, Wm)["noise0.41"]
        md = _up(C.video_of(U, seed=3), dev, 5)
        nbytes = so.e2fgvi_hole_label_workspace(Hm, Wm)
        assert nbytes >= 5 * Hm * Wm
        work = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for fill in (-7, 0x7F7F7F7F):
            gl = torch.full((Hm, Wm), fill, dtype=torch.int32, device=dev)
            gk = torch.full((1,), fill, dtype=torch.int32, device=dev)
            assert so.e2fgvi_hole_label(p(md), 3, Hm, Wm, p(work), p(gl), p(gk), st) == 0
            K = int(gk.item())
            assert K == len(boxes)
            gb = torch.full((K, 5), fill, dtype=torch.int32, device=dev)
            assert so.e2fgvi_label_boxes(p(gl), Hm, Wm, K, p(gb), st) == 0
            _check((gl, gb), labels, boxes, (Hm, Wm, fill))
        # the footprint is the second part of the workspace, behind the ranks
        off = (4 * Hm * Wm + 15) // 16 * 16
        assert np.array_equal(work[off:off + Hm * Wm].cpu().numpy().reshape(Hm, Wm), U.astype(np.uint8))


def test_label_boxes_skips_labels_out_of_range(dev):
    """K smaller than the labels hold: the components beyond it are left out, nothing is written past the table"""
    so = lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    U, labels, boxes = _cases(33, 130)["noise0.3"]
    gl = torch.from_numpy(labels).to(dev)
    y, x = np.argwhere(labels == 0)[0]
    gl[int(y), int(x)] = -5                                                            # a background pixel with a negative label
    want = boxes
    assert len(boxes) > 41
    K = 40
    gb = torch.full((K + 1, 5), -3, dtype=torch.int32, device=dev)
    assert so.e2fgvi_label_boxes(p(gl), 33, 130, K, p(gb), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    gb = gb.cpu().numpy()
    assert np.array_equal(gb[:K], want[:K]) and (gb[K] == -3).all()


def test_hole_components_checks_its_arguments(dev):
    m = torch.zeros((3, 5, 7), dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError):
        ops.hole_components(m.int())
    with pytest.raises(TypeError):
        ops.hole_components(m.cpu())
    with pytest.raises(TypeError):
        ops.hole_components(m.cpu().numpy())
    with pytest.raises(ValueError):
        ops.hole_components(m[0])
    with pytest.raises(ValueError):
        ops.hole_components(m.unsqueeze(-1))
    with pytest.raises(ValueError):
        ops.hole_components(m.permute(0, 2, 1))
    labels, boxes = ops.hole_components(m)
    assert not labels.any() and tuple(boxes.shape) == (0, 5)


# ------------------------------------------------------------------------------------------------ the driver
L, SIZE, FRAME = 7, (108, 60), (250, 131)
A, B, C3 = (8, 10, 40, 30), (200, 95, 240, 120), (60, 12, 75, 25)            # tests/test_video_holes.py plans these by hand
REGIONS2 = [(0, 0, 108, 60), (142, 71, 250, 131)]
REGIONS3 = [(0, 0, 134, 75), (142, 71, 250, 131)]


def _rect_masks(boxes, drift=True):
    """every box holds a rectangle six pixels narrower that drifts by a pixel per frame from its left to its right end: the
    component's box over the L = 7 frames is the box itself"""
    m = np.zeros((L, FRAME[1], FRAME[0]), np.uint8)
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        for i in range(L):
            m[i, y0:y1, x0 + i:x1 - 6 + i] = (1, 255, 77)[(i + k) % 3]
    return m


def _video(boxes=(A, B)):
    return _toy_video(L, FRAME[1], FRAME[0], seed=4)[0], _rect_masks(boxes)


def _net(dev, calls=None):
    def net(x, n):
        if calls is not None:
            calls.append(tuple(x.shape))
        return _stand_in_model(x.cpu(), n)[0].to(dev), None
    return net


def _by_definition(net, f, m, regions, dev, **kw):
    """the caller's frames with the bytes inside every region replaced by those of the explicit-box call; returns the passes too"""
    out, passes = f.copy(), []
    for (left, upper, right, lower) in regions:
        r = video.inpaint_video(net, f, m, device=dev, size=SIZE, region=(left, upper, right, lower), restore=True, **kw)
        out[:, upper:lower, left:right] = r[:, upper:lower, left:right]
        passes.append(r)
    return out, passes


def test_hole_regions_are_the_hand_computed_boxes(dev):
    f, m = _video()
    assert np.array_equal(frames(L, FRAME[0], FRAME[1], 4), f)                       # the toy video's frames are test_video_restore's
    labels, table = ops.hole_components(torch.from_numpy(m).to(dev))
    assert table.cpu().tolist() == [list(A) + [32 * 20], list(B) + [40 * 25]]
    assert video.hole_regions(m, FRAME, SIZE, device=dev) == REGIONS2
    assert video.hole_regions(torch.from_numpy(m).to(dev), FRAME, SIZE) == REGIONS2
    assert video.hole_regions(m, FRAME, SIZE, max_regions=1, device=dev) == [video.hole_region(m, FRAME, SIZE, device=dev)]
    assert video.hole_regions(_rect_masks((A, B, C3)), FRAME, SIZE, device=dev) == REGIONS3
    assert video.hole_regions(m * 0, FRAME, SIZE, device=dev) == []
    # more components than the planner takes: the box of region="hole"
    many = np.zeros((2, 131, 250), np.uint8)
    many[0, ::2, ::2] = 1
    assert int(ops.hole_components(torch.from_numpy(many).to(dev))[1].shape[0]) == 66 * 125 > video.HOLE_COMPONENTS_MAX
    assert video.hole_regions(many, FRAME, SIZE, device=dev) == [video.hole_region(many, FRAME, SIZE, device=dev)]


@pytest.mark.parametrize("kw", [{}, {"in_flight": 2}, {"batch_windows": 2}, {"feather": 3}, {"scenes": [3]}, {"dilate": False}], ids=str)
def test_inpaint_video_holes_is_its_definition(dev, kw):
    f, m = _video()
    net = _net(dev)
    want, passes = _by_definition(net, f, m, REGIONS2, dev, **kw)
    fd = torch.from_numpy(f).to(dev)
    got = video.inpaint_video(net, fd, m, device=dev, size=SIZE, region="holes", restore=True, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == f.shape
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(fd.cpu().numpy(), f)                                      # a device tensor of frames is left as it was
    outside = np.ones(f.shape[1:3], bool)
    for left, upper, right, lower in REGIONS2:
        outside[upper:lower, left:right] = False
        assert (got[:, upper:lower, left:right] != f[:, upper:lower, left:right]).any()
    assert np.array_equal(got[:, outside], f[:, outside])
    # every pass left the other region alone, so pasting the boxes is pasting the differences
    assert all(np.array_equal(p[:, outside], f[:, outside]) for p in passes)
    hole = video.inpaint_video(net, f, m, device=dev, size=SIZE, region="hole", restore=True, **kw)
    assert not np.array_equal(got, hole)


def test_inpaint_video_holes_merges_overlapping_regions(dev):
    f, m = _video((A, B, C3))
    net = _net(dev)
    want, _ = _by_definition(net, f, m, REGIONS3, dev)
    got = video.inpaint_video(net, f, m, device=dev, size=SIZE, region="holes", restore=True)
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(got, _by_definition(net, f, m, REGIONS2, dev)[0])


def test_inpaint_video_holes_with_one_region_is_region_hole(dev):
    net = _net(dev)
    f, m = _video()
    hole = video.inpaint_video(net, f, m, device=dev, size=SIZE, region="hole", restore=True)
    assert np.array_equal(video.inpaint_video(net, f, m, device=dev, size=SIZE, region="holes", restore=True, max_regions=1), hole)
    assert (hole != f).any()
    f, m = _video((C3,))                                                            # one component
    calls = []
    got = video.inpaint_video(_net(dev, calls), f, m, device=dev, size=SIZE, region="holes", restore=True, feather=2)
    n = len(calls)
    assert n == len(video.plan_windows(L)) and np.array_equal(got, video.inpaint_video(net, f, m, device=dev, size=SIZE, region="hole",
                                                                                       restore=True, feather=2))


def test_inpaint_video_holes_without_a_hole_returns_the_source(dev):
    f, m = _video()
    calls = []
    got = video.inpaint_video(_net(dev, calls), f, m * 0, device=dev, size=SIZE, region="holes", restore=True)
    assert np.array_equal(got, f) and calls == []
    video.inpaint_video(_net(dev, calls), f, m, device=dev, size=SIZE, region="holes", restore=True)
    assert len(calls) == 2 * len(video.plan_windows(L))                             # G passes over the video


def test_inpaint_video_holes_with_masks_of_another_size(dev):
    f, m = _video()
    small = np.ascontiguousarray(m[:, ::2, ::3])                                    # 66 x 84
    mask_wh = (84, 66)
    boxes = []
    for b in (A, B):
        ys, xs = np.nonzero(_rect_masks((b,))[:, ::2, ::3].any(0))
        boxes.append(video._scale_box((xs.min(), ys.min(), xs.max() + 1, ys.max() + 1), mask_wh, FRAME))
    assert boxes[0] == (8, 9, 42, 30)                                               # columns 3 .. 13 and rows 5 .. 14 of the small mask
    regions = [r for r, _ in video.plan_holes(boxes, FRAME, SIZE)]
    assert len(regions) == 2 and video.hole_regions(small, FRAME, SIZE, device=dev) == regions
    net = _net(dev)
    want, _ = _by_definition(net, f, small, regions, dev)
    got = video.inpaint_video(net, f, small, device=dev, size=SIZE, region="holes", restore=True)
    assert np.array_equal(got, want) and (got != f).any()


def test_inpaint_video_holes_checks_its_arguments(dev):
    f, m = _video()
    net = _net(dev)
    with pytest.raises(ValueError, match="size"):
        video.inpaint_video(net, f, m, device=dev, region="holes", restore=True)
    with pytest.raises(ValueError, match="restore"):
        video.inpaint_video(net, f, m, device=dev, size=SIZE, region="holes")
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError, match="max_regions"):
            video.inpaint_video(net, f, m, device=dev, size=SIZE, region="holes", restore=True, max_regions=bad)
        with pytest.raises(ValueError, match="max_regions"):
            video.hole_regions(m, FRAME, SIZE, max_regions=bad, device=dev)


def test_e2fgvi_inpaints_two_holes_at_source_resolution(dev):
    """the fixed-size e2fgvi model on six 864x480 frames (the tennis clip, PIL-upscaled) with two small holes far apart: both
    regions are exactly 432x240, so both resizes are the identity and inside each box the result is inpaint_video on the numpy slice
    of the frames and masks (the same kernels on the same bytes), with and without reuse; outside the dilated masks it is the source"""
    from PIL import Image
    from e2fgvi_amd.synth import synth_state_dict
    z = np.load(GOLD)
    big = np.stack([np.asarray(Image.fromarray(f).resize((864, 480))) for f in z["frames"][:6]])
    m = np.zeros((6, 480, 864), np.uint8)
    for i in range(6):
        m[i, 60 + i:100 + i, 100 + 2 * i:160 + 2 * i] = 255
        m[i, 330 - i:380 - i, 650 + 2 * i:710 + 2 * i] = 1
    regions = video.hole_regions(m, (864, 480), (432, 240), device=dev)
    assert regions == [(0, 0, 432, 240), (432, 232, 864, 472)]
    assert regions == [video.plan_region(b, (864, 480), (432, 240)) for b in ((100, 60, 170, 105), (650, 325, 720, 380))]
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
    net = net.to(dev).eval()
    M = np.zeros(m.shape, bool)
    for left, upper, right, lower in regions:
        M[:, upper:lower, left:right] = video.prepare_masks(m[:, upper:lower, left:right], (240, 432), dev).cpu().numpy() != 0
    assert M[m != 0].all() and 0 < M.mean() < 0.1
    for kw in ({}, {"reuse": True}):
        out = video.inpaint_video(net, big, m, size=(432, 240), region="holes", restore=True, **kw)
        assert out.shape == big.shape and out.dtype == np.uint8
        for left, upper, right, lower in regions:
            ref = video.inpaint_video(net, big[:, upper:lower, left:right], m[:, upper:lower, left:right], **kw)
            assert np.array_equal(out[:, upper:lower, left:right], ref), (kw, left)
            assert (out[:, upper:lower, left:right][M[:, upper:lower, left:right]] != big[:, upper:lower, left:right][M[:, upper:lower, left:right]]).any()
        assert np.array_equal(out[~M], big[~M])
