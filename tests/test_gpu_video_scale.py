"""The video tools at the two edges a film reel reaches and the pinned clips do not.

Part A: buffers of more than 2^32 bytes.  A named case of a tool's cases module is repeated along L on the device
(tests/big_video.py) until the frames pass 2^32 bytes, every tile a scene of its own; the device result is compared with the numpy
restatement's result for one tile, every byte of it, on the device.  A kernel that forms one offset in 32 bits reads or writes at
`offset mod 2^32`, which lies at another phase of the tile: every case asserts of its own inputs that those bytes differ
(big_video.wrap_is_visible), and for flicker_apply, denoise and mask_track_step the restatement is run on the bytes such a kernel
would fetch and must give another result (test_a_wrapped_offset_would_be_seen, on the host).

Part B: more frames, or jobs, than one launch takes (65 535 on the grid's y axis).  65 540 frames or jobs of a few pixels against
the restatement, a scene cut inside the second slab.  Where the restatement walks the frames one by one in Python (20 s and more for
65 540 of them), the content repeats with a period that 65 535 is no multiple of, and the restatement is run on the stretches that
differ -- both ends, the slab boundary, the cut -- and on one period: a launch that drops `t0` shows as a shifted phase.

Every test prints its wall time and the peak of device memory.  Measured on an MI355X (wall time of the test's body, restatement
included; peak of torch's allocator), Part A -- L frames of H x W, k frames a tile, bytes of the buffer that passes 2^32:
  flicker hist / curves / apply   68 184 of 70 x 300, k 3, frames 4 295 592 000          0.43 s    9.1 GiB
  denoise (search 1)             174 774 of 64 x 128, k 3, frames 4 295 245 824,
                                 flows 11 453 923 328 each                               0.24 s   31.0 GiB
  mask_track_step                 85 236 of 70 x 90, k 6, 85 236 jobs, flows 4 295 844 000 each  0.46 s    9.5 GiB
  scene_diff / overlay_stats / weave / interlace   the flicker frames             0.13 / 0.55 / 0.15 / 0.22 s   4.3 / 6.0 / 10.3 / 13.0 GiB
  line_sums / columns / paint    173 580 of 75 x 110, k 12, frames 4 296 105 000         0.32 s    7.6 GiB
  yuv420_to_rgb / rgb_to_yuv420  159 510 of 66 x 136, k 3, RGB 4 295 285 280             0.16 s    9.0 GiB
  u8_to_float / float_to_u8 / pred_to_u8   4 295 592 000 elements, 17 182 368 000 bytes  0.22 s   25.7 GiB
  gather_slabs / scatter_slabs    68 184 slots of 63 000 bytes                           0.14 s    4.3 GiB
  grain_blocks / grain_apply     309 894 of 66 x 70, k 3, frames 4 295 130 840           0.50 s   12.7 GiB
  defect_candidates / clean      227 268 of 70 x 90, k 6, frames 4 295 365 200,
                                 flows 11 454 256 800 each, 151 512 ids                  0.30 s   29.0 GiB
  hole_bbox / _frames / label    500 589 masks of 66 x 130, k 3, 4 295 053 620           0.78 s    5.3 GiB
  warp_error uint8 / float        65 535 of 131 x 171, k 3, frames 4 404 148 605 / 17 616 594 420,
                                 flows 11 744 217 072 each                        0.22 / 0.22 s   26.1 / 38.4 GiB
  mask_prepare / masked_clip / composite   the masks of the holes, the flicker frames,
                                 an accumulator of 17 182 368 000                        0.29 s   22.3 GiB
  pixel_track_step                85 236 of 70 x 90, k 6, origins 8 591 788 800          0.20 s   17.5 GiB
  pixel_fill                     227 268 of 70 x 90, k 6, frames 4 295 365 200, origins 22 908 614 400   0.20 s   34.7 GiB
Part B: 0.1 to 0.6 s a test, peaks of 0.4 GiB at the most."""
import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, metrics, ops, video
from oracle import metrics_ref
from tests import big_video as B
from tests import color_cases as CL
from tests import defect_cases as DF
from tests import denoise_cases as DN
from tests import flicker_cases as FL
from tests import flicker_local_cases as FLL
from tests import grain_cases as GR
from tests import interlace_cases as IL
from tests import line_scratch_cases as LN
from tests import mask_key_cases as MK
from tests import pixel_track_cases as PT
from tests import scene_diff_cases as SD
from tests import telecine_cases as TC
from tests import warp_error_cases as WE
from tests import weave_cases as WV
from tests import yuv_cases as YV

pytestmark = pytest.mark.gpu

SLAB = 65535                      # frames or jobs per launch: the grid's y axis
FRAMES_CASE = "3x70x300"          # flicker_cases: three frames of 70 x 300, 63 000 bytes a frame -- no divisor of 2^32


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                       # a writable copy: the cases are read-only


def _frames_tile():
    return FL.case(FRAMES_CASE)["frames"]


def _big_frames(base, dev, what):
    """(frames on the device, the number of tiles): base [k,H,W,3] repeated past 2^32 bytes; the conditions of a pass asserted"""
    n = B.tiles_past(B.nbytes(base))
    fr = B.tiled(base, n, dev)
    B.wrap_is_visible(fr, B.nbytes(base), what)
    assert B.WRAP % B.nbytes(base[:1]) != 0, what                     # a frame does not divide 2^32 either
    print(what, "L", fr.shape[0], "H", fr.shape[1], "W", fr.shape[2], "k", len(base), "bytes", fr.numel() * fr.element_size())
    return fr, n


def _scene_table(L, k, dev, inner=None):
    """int32 [L]: every tile a scene of its own; `inner` int [k]: the scenes inside a tile"""
    s = B.scene_of(L, k, dev)
    if inner is None:
        return s
    inner = torch.from_numpy(np.asarray(inner, np.int32)).to(dev)
    return s * int(inner.max() + 1) + inner[torch.arange(L, device=dev) % k]


# ================================================================================================ Part A: past 2^32 bytes
def _flicker(dev):
    c, want = FL.case(FRAMES_CASE), FL.want(FRAMES_CASE)
    k, N = c["L"], c["H"] * c["W"]
    assert c["scenes"] is None and not np.array_equal(want["out"], c["frames"])
    fr, n = _big_frames(c["frames"], dev, "flicker")
    scene = _scene_table(fr.shape[0], k, dev)
    hist = ops.flicker_hist(fr)
    B.assert_tiled(hist, want["hist"], "flicker_hist")
    Q, d = ops.flicker_curves(hist, scene, N, c["span"], c["max_shift"])
    B.assert_tiled(Q, want["Q"], "flicker_curves Q")
    B.assert_tiled(d, want["d"], "flicker_curves d")
    out = ops.flicker_apply(fr, d)
    B.assert_tiled(out, want["out"], "flicker_apply")
    B.assert_tiled(fr, c["frames"], "flicker frames")                  # the input is only read
    B.assert_tiled(ops.flicker_apply(out, d, out=out), FL.apply_np(want["out"], want["d"]), "flicker_apply in place")


def test_flicker_past_4gib(dev):
    with B.measured("flicker_hist / flicker_curves / flicker_apply", dev):
        _flicker(dev)


DENOISE_CASE, DENOISE_SETTING = "soft_64x128", (8, 1, 255)


def _flow_tiles(c, n, dev):
    """(fwd, bwd) on the device, [n k - 1, H, W, 2] each: the tile's flows, the pair between two tiles filled with a flow of its own"""
    fwd, bwd = B.padded_flows(c["fwd"], 1), B.padded_flows(c["bwd"], 2)
    return (B.tiled(fwd, n, dev, drop=1), B.tiled(bwd, n, dev, drop=1)), (fwd, bwd)


def _denoise(dev):
    c, want = DN.case(DENOISE_CASE), DN.want(DENOISE_CASE, DENOISE_SETTING)
    assert not c["scenes"] and not np.array_equal(want, c["frames"])
    fr, n = _big_frames(c["frames"], dev, "denoise")
    (fwd, bwd), (fwd_tile, _) = _flow_tiles(c, n, dev)
    B.wrap_is_visible(fwd, B.nbytes(fwd_tile), "denoise fwd")
    B.wrap_is_visible(bwd, B.nbytes(fwd_tile), "denoise bwd")
    out = ops.denoise(fr, fwd, bwd, _scene_table(fr.shape[0], c["L"], dev), *DENOISE_SETTING)
    B.assert_tiled(out, want, "denoise")
    B.assert_tiled(fr, c["frames"], "denoise frames")


def test_denoise_past_4gib(dev):
    with B.measured("denoise", dev):
        _denoise(dev)


MASK_CASE = "smooth_70x90"
MASK_JOBS = ((0, 0), (2, 0), (4, 0), (0, 1), (2, 1), (4, 1))          # of a tile of six frames: no job reads what another writes


def _mask_tile(fwd=None, bwd=None):
    """(planes before, planes after the six jobs of a tile, the case): a mask in every frame of both planes"""
    c = MK.case(MASK_CASE)
    L, H, W = c["L"], c["H"], c["W"]
    assert L == 6
    keys = MK.binarise(c["key_masks"])
    before = np.stack([np.stack([np.roll(keys[(t + d) % len(keys)], (3 * t, 5 * d + t), axis=(0, 1)) for t in range(L)]) for d in (0, 1)])
    after = before.copy()
    for t, d in MASK_JOBS:
        MK.run_job(after, c["fwd"] if fwd is None else fwd, c["bwd"] if bwd is None else bwd, t, d, True)
    return before, after, c


def _jobs_of_tiles(jobs, k, n, dev, seed):
    """int32 [n len(jobs), 2] on the device: the jobs (pair, dir) of a tile for every tile, shuffled"""
    t = torch.tensor([j[0] for j in jobs], dtype=torch.int64, device=dev)
    d = torch.tensor([j[1] for j in jobs], dtype=torch.int64, device=dev)
    at = torch.arange(n, device=dev).view(n, 1) * k + t.view(1, -1)
    table = torch.stack([at, d.view(1, -1).expand_as(at)], dim=-1).view(-1, 2)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return table[torch.randperm(table.shape[0], generator=g).to(dev)].to(torch.int32).contiguous()


def _mask_track(dev):
    before, after, c = _mask_tile()
    assert not np.array_equal(before, after)
    k = c["L"]
    fwd_tile, bwd_tile = B.padded_flows(c["fwd"], 3), B.padded_flows(c["bwd"], 4)
    n = B.tiles_past(B.nbytes(fwd_tile))
    fwd, bwd = B.tiled(fwd_tile, n, dev, drop=1), B.tiled(bwd_tile, n, dev, drop=1)
    B.wrap_is_visible(fwd, B.nbytes(fwd_tile), "mask_track fwd")
    B.wrap_is_visible(bwd, B.nbytes(bwd_tile), "mask_track bwd")
    planes = B.tiled_planes(before, n, dev)
    jobs = _jobs_of_tiles(MASK_JOBS, k, n, dev, 5)
    assert jobs.shape[0] > SLAB
    print("mask_track_step L", n * k, "H", c["H"], "W", c["W"], "k", k, "jobs", jobs.shape[0], "flow bytes", fwd.numel() * 4,
          "plane bytes", planes.numel())
    got = ops.mask_track_step(planes, fwd, bwd, jobs, True)
    assert got.data_ptr() == planes.data_ptr()
    for d in (0, 1):
        B.assert_tiled(planes[d], after[d], "mask_track_step plane %d" % d)


def test_mask_track_step_past_4gib(dev):
    with B.measured("mask_track_step", dev):
        _mask_track(dev)


def test_a_wrapped_offset_would_be_seen():
    """on the host: the restatement on the bytes a kernel with one 32-bit offset would fetch for the first tile past 2^32 -- frames
    for flicker_apply, frames and flows for denoise, flows for mask_track_step -- gives another result than the expected one"""
    c, want = FL.case(FRAMES_CASE), FL.want(FRAMES_CASE)
    wrong = B.wrapped_tile(c["frames"])
    assert not np.array_equal(wrong, c["frames"])
    assert not np.array_equal(FL.apply_np(wrong, want["d"]), want["out"])
    assert not np.array_equal(FL.hist_np(wrong), want["hist"])
    c, want = DN.case(DENOISE_CASE), DN.want(DENOISE_CASE, DENOISE_SETTING)
    scene = DN.scene_of_np(c["L"])
    assert not np.array_equal(DN.reference(B.wrapped_tile(c["frames"]), c["fwd"], c["bwd"], scene, *DENOISE_SETTING), want)
    fwd_wrong = B.wrapped_tile(B.padded_flows(c["fwd"], 1))[:-1]
    assert not np.array_equal(DN.reference(c["frames"], fwd_wrong, c["bwd"], scene, *DENOISE_SETTING), want)
    _, after, c = _mask_tile()
    for which in ("fwd", "bwd"):
        wrong = B.wrapped_tile(B.padded_flows(c[which], 3 if which == "fwd" else 4))[:-1]
        assert not np.array_equal(_mask_tile(**{which: wrong})[1], after), which


def _scene_diff(dev):
    base = _frames_tile()
    want = SD.scene_diff_np(np.concatenate([base, base[:1]]))         # the pair between two tiles is one pair more
    assert want.all()
    fr, n = _big_frames(base, dev, "scene_diff")
    B.assert_tiled(ops.scene_diff(fr), want, "scene_diff")


def test_scene_diff_past_4gib(dev):
    with B.measured("scene_diff", dev):
        _scene_diff(dev)


def _luma_t(x):
    x = x.to(torch.int64)
    return (77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8


def _overlay_stats(dev):
    from tests import overlay_cases as OV
    base = _frames_tile()
    fr, n = _big_frames(base, dev, "overlay_stats")
    got = ops.overlay_stats(fr)
    # the sums again, int64 torch on the device, a stretch of frames at a time
    L, H, W = fr.shape[:3]
    want = torch.zeros((3, H, W), dtype=torch.int64, device=dev)
    xs, ys = torch.arange(W, device=dev), torch.arange(H, device=dev)
    per = max(1, (B.CHUNK // 8) // (H * W * 3))
    for a in range(0, L, per):
        Y = _luma_t(fr[a:a + per])
        gx = Y[:, :, (xs + 1).clamp(max=W - 1)] - Y[:, :, (xs - 1).clamp(min=0)]
        gy = Y[:, (ys + 1).clamp(max=H - 1)] - Y[:, (ys - 1).clamp(min=0)]
        want += torch.stack([gx.sum(0), gy.sum(0), (gx.abs() + gy.abs()).sum(0)])
        del Y, gx, gy
    assert int(want.abs().max()) < 2 ** 31
    assert torch.equal(got.to(torch.int64), want)
    tile = OV.stats_np(base).astype(np.int64)
    assert tile[2].any() and np.array_equal(want.cpu().numpy(), n * tile)        # and the torch sums are the restatement's


def test_overlay_stats_past_4gib(dev):
    with B.measured("overlay_stats", dev):
        _overlay_stats(dev)


def _weave(dev):
    base = _frames_tile()
    shifts = np.array([[-37, 43], [16, 0], [15, -150]], np.int32)
    col, row = WV.profiles_np(base)
    out_t, mask_t = WV.apply_np(base, shifts)
    assert not np.array_equal(out_t, base) and mask_t.any()
    fr, n = _big_frames(base, dev, "weave")
    c, r = ops.weave_profiles(fr)
    B.assert_tiled(c, col, "weave_profiles col")
    B.assert_tiled(r, row, "weave_profiles row")
    del c, r
    out, mask = ops.weave_apply(fr, B.tiled(shifts, n, dev), return_mask=True)
    B.assert_tiled(out, out_t, "weave_apply")
    B.assert_tiled(mask, mask_t, "weave_apply mask")


def test_weave_past_4gib(dev):
    with B.measured("weave_profiles / weave_apply", dev):
        _weave(dev)


INTERLACE_SETTING = (1, 0, 1, 2)                                        # tff, field rate, guard, edges 2


def _interlace(dev):
    base = _frames_tile()
    tff, mode, guard, edges = INTERLACE_SETTING
    D = IL.scores_np(base)
    want = IL.deinterlace_np(base, None, tff, mode, guard, edges)
    assert D[:-1].all() and not D[-1].any() and not np.array_equal(want[1::2], base)
    fr, n = _big_frames(base, dev, "interlace")
    scene = _scene_table(fr.shape[0], len(base), dev)
    B.assert_tiled(ops.interlace_scores(fr, scene), D, "interlace_scores")
    out = ops.deinterlace(fr, scene, bool(tff), mode, bool(guard), edges)
    assert out.shape[0] == 2 * fr.shape[0]
    B.assert_tiled(out, want, "deinterlace")


def test_interlace_past_4gib(dev):
    with B.measured("interlace_scores / deinterlace", dev):
        _interlace(dev)


LINE_CASE = "nondefault_12x75x110"


def _line(dev):
    c, want = LN.case(LINE_CASE), LN.want(LINE_CASE)
    assert want["keep"].any() and want["masks"].any() and not want["masks"].all()
    fr, n = _big_frames(c["frames"], dev, "line_scratch")
    scene = _scene_table(fr.shape[0], c["L"], dev, LN.scene_of_np(c["L"], c["scenes"]))
    S = ops.line_sums(fr, c["rows"])
    B.assert_tiled(S, want["S"], "line_sums")
    cand, cnt, col, b0, b1 = ops.line_columns(S, c["rows"], c["tau"], c["gap"], c["side"], c["drift"], c["coverage"])
    for got, key in ((cand, "cand"), (cnt, "cnt"), (col, "col"), (b0, "b0"), (b1, "b1")):
        B.assert_tiled(got, want[key], "line_columns " + key)
    keep, counts, masks = ops.line_paint(col, b0, b1, scene, c["H"], c["rows"], c["drift"], c["span"], c["persist"], c["radius"])
    for got, key in ((keep, "keep"), (counts, "counts"), (masks, "masks")):
        B.assert_tiled(got, want[key].astype(np.int32) if key == "counts" else want[key], "line_paint " + key)


def test_line_scratch_past_4gib(dev):
    with B.measured("line_sums / line_columns / line_paint", dev):
        _line(dev)


YUV_SHAPE = (3, 66, 136)                                                # H even, W a multiple of 8: the wide loads


def _yuv(dev):
    L, H, W = YUV_SHAPE
    dec, enc = video.yuv_coefficients("bt709", False)
    yo = 16
    for layout, chroma in (("nv12", "left"), ("i420", "nearest")):
        x = YV.frames("random", L, H, W, layout)
        want = YV.decode_np(x, layout, chroma, dec, yo)
        n = B.tiles_past(B.nbytes(want))                                # the RGB side is the larger one
        big = B.tiled(x, n, dev)
        rgb = ops.yuv420_to_rgb(big, layout, chroma, tuple(dec) + (yo,))
        B.wrap_is_visible(rgb, B.nbytes(want), "yuv rgb")
        assert B.WRAP % B.nbytes(x) != 0 and big.numel() > B.WRAP // 2
        print("yuv", layout, "L", big.shape[0], "H", H, "W", W, "k", L, "rgb bytes", rgb.numel(), "yuv bytes", big.numel())
        B.assert_tiled(rgb, want, "yuv420_to_rgb " + layout)
        back = ops.rgb_to_yuv420(rgb, layout, tuple(enc) + (yo,))
        B.assert_tiled(back, YV.encode_np(want, layout, enc, yo), "rgb_to_yuv420 " + layout)
        del big, rgb, back
        torch.cuda.empty_cache()


def test_yuv_past_4gib(dev):
    with B.measured("yuv420_to_rgb / rgb_to_yuv420", dev):
        _yuv(dev)


def _conversions(dev):
    base = _frames_tile()
    fr, n = _big_frames(base, dev, "u8_to_float")
    assert fr.numel() > B.WRAP                                          # more than 2^32 ELEMENTS: 17 GB of floats, and more than 2^32
    # threads for float_to_u8 and pred_to_u8 -- of which the runtime launched `threads mod 2^32` before their grids were capped
    f = ops.u8_to_float(fr)
    B.assert_tiled(f, base.astype(np.float32), "u8_to_float")
    f += 0.75                                                           # float_to_u8 truncates
    B.assert_tiled(ops.float_to_u8(f), base, "float_to_u8")
    del f
    torch.cuda.empty_cache()
    # pred_to_u8: [N,3,Hp,Wp] in (-1, 1) -> [N,H,W,3], cropped
    k, H, W = base.shape[:3]
    Hp, Wp = H + 2, W + 4
    rng = np.random.RandomState(9)
    pred = (2 * rng.random_sample((k, 3, Hp, Wp)) - 1).astype(np.float32)
    want = ((pred.astype(np.float32) + np.float32(1)) / np.float32(2) * np.float32(255)).astype(np.int32).astype(np.uint8)
    want = np.ascontiguousarray(want[:, :, :H, :W].transpose(0, 2, 3, 1))
    big = B.tiled(pred, n, dev)
    got = ops.pred_to_u8(big, H, W)
    assert got.numel() > B.WRAP and big.numel() > B.WRAP
    B.assert_tiled(got, want, "pred_to_u8")


def test_conversions_past_4gib(dev):
    with B.measured("u8_to_float / float_to_u8 / pred_to_u8", dev):
        _conversions(dev)


def _slabs(dev):
    """a cache of slots whose byte offsets slot * slab_bytes pass 2^32: rows gathered from the far end and scattered back"""
    base = np.ascontiguousarray(_frames_tile()).reshape(3, -1).view(np.int32)          # three slabs of 63 000 bytes
    slab = base.shape[1] * 4
    n = B.tiles_past(3 * slab)
    cache = B.tiled(base.view(np.float32), n, dev)                      # [slots, words]: bit patterns, copied as they are
    slots = cache.shape[0]
    assert (slots - 1) * slab > B.WRAP and B.WRAP % slab != 0
    ids_np = np.array([slots - 1, 0, B.WRAP // slab, B.WRAP // slab + 1, B.WRAP // 2 // slab + 1, slots - 2, -1, slots], np.int32)
    rows = ops.gather_slabs(cache, _dev(ids_np, dev))
    want = np.stack([base[i % 3] if 0 <= i < slots else np.zeros_like(base[0]) for i in ids_np])
    assert np.array_equal(rows.cpu().numpy().view(np.int32), want)
    print("slabs: slots", slots, "slab bytes", slab, "cache bytes", cache.numel() * 4)
    # scatter: distinct rows into slots on both sides of 2^31 and 2^32; every other slot stays
    put = np.array([slots - 1, 1, B.WRAP // slab + 1, B.WRAP // 2 // slab + 1, slots + 5, -3], np.int32)
    new = np.arange(len(put) * base.shape[1], dtype=np.int32).reshape(len(put), -1) * 7 + 1
    ops.scatter_slabs(_dev(new.view(np.float32), dev), _dev(put, dev), cache)
    view = cache.view(torch.int32)
    for i, s in enumerate(put):
        if 0 <= s < slots:
            assert torch.equal(view[int(s)], _dev(new[i], dev)), int(s)
            view[int(s)] = _dev(base[int(s) % 3], dev)                  # put back: the rest is compared as tiles
    B.assert_tiled(view, base, "scatter_slabs left the other slots alone")


def test_slabs_past_4gib(dev):
    with B.measured("gather_slabs / scatter_slabs", dev):
        _slabs(dev)


# ================================================================================================ Part B: more than one launch
L_B, CUT_B = 65540, 65537          # frames (or jobs): two slabs of 65 535; a scene cut inside the second


def _periodic(base, L):
    """base [P, ...] repeated along the first axis to L entries"""
    base = np.ascontiguousarray(base)
    return np.resize(base, (L,) + base.shape[1:])


def test_flicker_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 2 x 2: flicker_hist and flicker_apply launch the frames in slabs; flicker_curves is one launch of L
    workgroups.  Frame 65 535, the first of the second slab, is averaged over frames 65 531 .. 65 536 (the cut lies at 65 537).  The
    histograms and the output against the restatement on the whole video; the curves, which the restatement walks level by level in
    Python (280 s for the video), on its first 80 and its last 100 frames."""
    with B.measured("flicker slabs", dev):
        span, max_shift = 4, 32
        rng = np.random.RandomState(80)
        fr = np.clip(rng.randint(40, 216, (L_B, 1, 1, 1)) + rng.randint(-30, 31, (L_B, 2, 2, 3)), 0, 255).astype(np.uint8)
        so = FL.scene_of_np(L_B, [CUT_B])
        x = _dev(fr, dev)
        hist = ops.flicker_hist(x)
        want_hist = FL.hist_np(fr)
        assert np.array_equal(hist.cpu().numpy(), want_hist)
        Q, d = ops.flicker_curves(hist, _dev(so, dev), 4, span, max_shift)
        Q, d = Q.cpu().numpy(), d.cpu().numpy()
        for a, b in ((0, 80), (L_B - 100, L_B)):
            wq, wd = FL.curves_np(want_hist[a:b], so[a:b], span, max_shift)
            lo, hi = (a + span if a else a), (b - span if b < L_B else b)
            assert np.array_equal(Q[lo:hi], wq[lo - a:hi - a]) and np.array_equal(d[lo:hi], wd[lo - a:hi - a]), (a, b)
            assert wd[lo - a:hi - a].any()
        assert d[SLAB].any() and d[CUT_B].any()
        want = FL.apply_np(fr, d)
        assert not np.array_equal(want[SLAB:], fr[SLAB:])
        got = ops.flicker_apply(x, _dev(d, dev)).cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())


def _grain_apply_np(filled, where, lut, scene_of, seed):
    """grain_cases.apply_np for all frames at once (its noise is a hash of the frame number: grain_cases.mix takes arrays)"""
    L, H, W = filled.shape[:3]
    t = np.arange(L, dtype=np.uint64).reshape(L, 1, 1, 1)
    key = GR.mix((np.uint64(seed) + np.uint64(0x9E3779B9) * t) & GR.M32)
    ys, xs, cs = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), np.arange(3, dtype=np.uint64), indexing="ij")
    h = GR.mix(key ^ (((ys * np.uint64(W) + xs) * np.uint64(3) + cs) & GR.M32)[None])
    n = ((h & 255) + ((h >> 8) & 255) + ((h >> 16) & 255) + ((h >> 24) & 255)).astype(np.int64) - 510
    S = lut.shape[0]
    ok = (scene_of >= 0) & (scene_of < S)
    g = np.clip(lut.astype(np.int64), 0, GR.SCALE_MAX)[np.where(ok, scene_of, 0)[:, None, None], GR.luma(filled)]
    v = np.clip(filled.astype(np.int64) + ((n * g + 32768) >> 16), 0, 255).astype(np.uint8)
    on = (where != 0) & ok[:, None, None]
    return np.where(on[..., None], v, filled)


def test_grain_more_frames_than_a_launch_takes(dev):
    """65 540 frames: grain_blocks on frames of 10 x 10 (one block a frame, a hole pixel in some footprints) against the restatement
    on the whole video; grain_apply on frames of 2 x 2 against the restatement with the frame numbers as an array, which is the
    restatement itself on the first frames and across the slab boundary.  A frame's noise depends on its number: a slab that
    forgets where it starts gives other bytes."""
    with B.measured("grain slabs", dev):
        rng = np.random.RandomState(81)
        fr = rng.randint(1, 255, (L_B, 10, 10, 3)).astype(np.uint8)
        fr[::7, 4, 5, 1] = 255
        hole = (rng.rand(L_B, 10, 10) < 0.004).astype(np.uint8) * 9
        energy, band = ops.grain_blocks(_dev(fr, dev), _dev(hole, dev))
        we, wb = GR.blocks_np(fr, hole)
        assert len(np.unique(wb)) > 2 and (wb[SLAB:] != 255).any() and np.array_equal(energy.cpu().numpy(), we) and np.array_equal(band.cpu().numpy(), wb)
        filled = rng.randint(0, 256, (L_B, 2, 2, 3)).astype(np.uint8)
        where = rng.choice([0, 1, 255], (L_B, 2, 2)).astype(np.uint8)
        so = GR.scene_table(L_B, [CUT_B])[0]
        so[5], so[SLAB + 1] = 7, -1                                     # frames in no scene are copied
        lut = rng.randint(0, 400000, (2, 256, 3)).astype(np.int32)
        seed = 0xC0FFEE11
        want = _grain_apply_np(filled, where, lut, so, seed)
        for a, b in ((0, 40), (SLAB - 20, L_B)):
            sub = GR.apply_np(filled[a:b], where[a:b], lut, so[a:b], (seed + 0x9E3779B9 * a) & 0xFFFFFFFF)
            assert np.array_equal(want[a:b], sub), (a, b)
        assert not np.array_equal(want[SLAB:], filled[SLAB:])
        got = ops.grain_apply(_dev(filled, dev), _dev(where, dev), _dev(lut, dev), _dev(so, dev), seed).cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())


def test_line_scratch_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 4 x 3 (one band, one column that has both its sides): line_sums, line_columns and both launches of line_paint
    carry the frames on the grid's y axis.  A column is kept by the votes of the two frames on either side of its own: frame 65 535
    counts frame 65 534, and the cut at 65 537 stops the votes."""
    with B.measured("line scratch slabs", dev):
        kw = dict(rows=4, tau=0, gap=0, side=1, drift=0, coverage=50, span=2, persist=2, radius=0)
        rng = np.random.RandomState(82)
        fr = rng.randint(0, 256, (L_B, 4, 3, 3)).astype(np.uint8)
        want = LN.detect_np(fr, scenes=[CUT_B], **kw)
        assert want["keep"][SLAB:].any() and want["masks"][SLAB:].any() and not want["masks"][SLAB:].all()
        S = ops.line_sums(_dev(fr, dev), kw["rows"])
        cand, cnt, col, b0, b1 = ops.line_columns(S, kw["rows"], kw["tau"], kw["gap"], kw["side"], kw["drift"], kw["coverage"])
        keep, counts, masks = ops.line_paint(col, b0, b1, _dev(LN.scene_of_np(L_B, [CUT_B]), dev), 4, kw["rows"], kw["drift"],
                                             kw["span"], kw["persist"], kw["radius"])
        got = dict(S=S, cand=cand, cnt=cnt, col=col, b0=b0, b1=b1, keep=keep, counts=counts, masks=masks)
        for key in LN.KEYS:
            g = got[key].cpu().numpy()
            assert g.shape == want[key].shape and np.array_equal(g, want[key]), (key, int((g != want[key]).sum()))


PAIRS_B = 5                         # pairs of frames a period: ten frames, and 65 535 is no multiple of ten


def _pair_jobs(L, dev, seed):
    """int32 [L, 2]: the jobs (t, dir) of every even pair t in both directions, shuffled -- no job reads a frame another writes, and
    the two directions of a pair, in whichever slab they land, read the same two flows"""
    t = np.arange(0, L - 1, 2)
    jobs = np.concatenate([np.stack([t, np.zeros_like(t)], 1), np.stack([t, np.ones_like(t)], 1)]).astype(np.int32)
    return jobs[np.random.RandomState(seed).permutation(len(jobs))]


def _pair_flows(rng, P, H, W):
    """fwd, bwd [2 P, H, W, 2]: flows on halves, mostly consistent with each other, some non-finite"""
    fwd = (rng.randint(-2, 3, (2 * P, H, W, 2)) * 0.5).astype(np.float32)
    bwd = (-fwd + (rng.rand(2 * P, H, W, 2) < 0.2) * 1.5).astype(np.float32)
    fwd[1, 0, 0, 0], bwd[3, 1, 1, 1] = np.nan, np.inf
    return fwd, bwd


def test_mask_track_more_jobs_than_a_launch_takes(dev):
    """65 542 jobs on 65 542 frames of 2 x 2: every even pair in both directions, shuffled over the two slabs.  The content repeats
    every ten frames, so the restatement runs ten jobs; a job that is not run leaves its frame as it was, which is not what is
    expected of it."""
    with B.measured("mask_track slabs", dev):
        L, P = L_B + 2, PAIRS_B
        rng = np.random.RandomState(83)
        base = (rng.rand(2, 2 * P, 2, 2) < 0.6).astype(np.uint8)
        fwd, bwd = _pair_flows(rng, P, 2, 2)
        after = base.copy()
        for t in range(0, 2 * P, 2):
            for d in (0, 1):
                MK.run_job(after, fwd, bwd, t, d, True)
        assert all(not np.array_equal(after[d, t + 1 - d], base[d, t + 1 - d]) for d in (0, 1) for t in (0, 2)), "the jobs change their frames"
        planes = _dev(np.stack([_periodic(base[0], L), _periodic(base[1], L)]), dev)
        jobs = _pair_jobs(L, dev, 7)
        assert len(jobs) > SLAB + 1
        ops.mask_track_step(planes, _dev(_periodic(fwd, L - 1), dev), _dev(_periodic(bwd, L - 1), dev), _dev(jobs, dev), True)
        want = np.stack([_periodic(after[0], L), _periodic(after[1], L)])
        got = planes.cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())


def test_pixel_track_more_jobs_than_a_launch_takes(dev):
    """the same jobs for pixel_track_step: ages and origins of both planes"""
    with B.measured("pixel_track_step slabs", dev):
        L, P = L_B + 2, PAIRS_B
        rng = np.random.RandomState(84)
        hole = (rng.rand(2 * P, 2, 2) < 0.5).astype(np.uint8)
        fwd, bwd = _pair_flows(rng, P, 2, 2)
        age0 = np.stack([hole * 255, hole * 255]).astype(np.uint8)
        org0 = rng.rand(2, 2 * P, 2, 2, 2).astype(np.float32)          # what the buffers hold before: kept where nothing is reached
        age, org = age0.copy(), org0.copy()
        for t in range(0, 2 * P, 2):
            for d in (0, 1):
                s, dst = (t, t + 1) if d == 0 else (t + 1, t)
                g, c = (bwd[t], fwd[t]) if d == 0 else (fwd[t], bwd[t])
                PT.step_np(hole[dst], age[d, s], org[d, s], age[d, dst], org[d, dst], g, c, 254, True)
        assert not np.array_equal(age, age0) and not np.array_equal(org, org0)
        tile2 = lambda a: np.stack([_periodic(a[0], L), _periodic(a[1], L)])
        d_age, d_org = _dev(tile2(age0), dev), _dev(tile2(org0), dev)
        jobs = _pair_jobs(L, dev, 8)
        assert len(jobs) > SLAB + 1
        ops.pixel_track_step(_dev(_periodic(hole, L), dev), d_age, d_org, _dev(_periodic(fwd, L - 1), dev),
                             _dev(_periodic(bwd, L - 1), dev), _dev(jobs, dev), 254, True)
        assert np.array_equal(d_age.cpu().numpy(), tile2(age))
        assert np.array_equal(d_org.cpu().numpy().view(np.uint32), tile2(org).view(np.uint32))


def test_pixel_fill_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 2 x 2 with ages of 0, 1, 2 and 255 and origins all over the frame: a hole pixel of frame 65 535 takes its
    colour from frame 65 534 or 65 533 (plane 0) or from 65 536 or 65 537 (plane 1).  The content repeats every seven frames: the
    restatement runs on one period inside a stretch of five, and on the first and the last 28 frames, where the video ends."""
    with B.measured("pixel_fill slabs", dev):
        L, P = L_B, 7
        rng = np.random.RandomState(85)
        hole_p = (rng.rand(P, 2, 2) < 0.45).astype(np.uint8)
        age_p = np.where(hole_p[None] == 1, rng.choice([1, 2, 255, 1], (2, P, 2, 2)), 0).astype(np.uint8)
        # origins on pixels (one corner has all the weight), on halves between two, and a few anywhere
        org_p = rng.choice([0.0, 1.0, 0.0, 1.0, 0.5, 0.3], (2, P, 2, 2, 2)).astype(np.float32)
        org_p[0, 2, 0, 0], org_p[1, 4, 1, 1] = (np.nan, 0.5), (1.0, 1.0)
        src_p = rng.randint(0, 256, (P, 2, 2, 3)).astype(np.uint8)
        filled_p = rng.randint(0, 256, (P, 2, 2, 3)).astype(np.uint8)

        def video(n):
            two = lambda a: np.stack([_periodic(a[0], n), _periodic(a[1], n)])
            return dict(L=n, H=2, W=2, hole=_periodic(hole_p, n), src=_periodic(src_p, n), filled=_periodic(filled_p, n)), two(age_p), two(org_p)

        def restate(a, b, full):
            """the restatement on frames [a, b) of the video"""
            c, age, org = full
            sub = dict(L=b - a, H=2, W=2, hole=c["hole"][a:b], src=c["src"][a:b], filled=c["filled"][a:b])
            return PT.fill_np(sub, age[:, a:b], org[:, a:b])

        full = video(L)
        out_p, source_p = restate(0, 5 * P, video(5 * P))
        want, source = _periodic(out_p[2 * P:3 * P], L), _periodic(source_p[2 * P:3 * P], L)
        for a, b, lo, hi in ((0, 4 * P, 0, 4 * P - 2), (L - 4 * P, L, L - 4 * P + 2, L)):
            o, s = restate(a, b, full)
            want[lo:hi], source[lo:hi] = o[lo - a:hi - a], s[lo - a:hi - a]
        print("pixel_fill sources", np.unique(source, return_counts=True), "changed behind the slab", int((want[SLAB:] != full[0]["filled"][SLAB:]).sum()))
        assert not np.array_equal(want[SLAB:], full[0]["filled"][SLAB:]) and set(np.unique(source)) == {0, 1, 2, 3}
        c, age, org = full
        out = _dev(c["filled"], dev)
        got, src_of = ops.pixel_fill(_dev(c["src"], dev), _dev(c["hole"], dev), _dev(age, dev), _dev(org, dev), out, return_source=True)
        assert got.data_ptr() == out.data_ptr()
        got, src_of = got.cpu().numpy(), src_of.cpu().numpy()
        assert np.array_equal(src_of, source), int((src_of != source).sum())
        assert np.array_equal(got, want), int((got != want).sum())


def test_defects_more_ids_than_a_launch_takes(dev):
    """65 540 ids, every frame of 65 540 of 2 x 2 once and shuffled: the centre frames ride on the grid's y axis.  Neighbouring
    centres, in whichever slab, read each other's frames; the ids 0 and L - 1 have no two neighbours and write nothing.  The
    content repeats every seven frames: the restatement runs on one period inside a stretch of three."""
    with B.measured("defect slabs", dev):
        L, P, tau, slack, support, radius = L_B, 7, 12, 0, 1, 1
        rng = np.random.RandomState(86)
        fr_p = np.clip(rng.randint(90, 140, (P, 2, 2, 1)) + rng.randint(-60, 61, (P, 2, 2, 3)) * (rng.rand(P, 2, 2, 1) < 0.3), 0, 255).astype(np.uint8)
        fwd_p = (rng.randint(-1, 2, (P, 2, 2, 2)) * 0.5).astype(np.float32)
        bwd_p = (rng.randint(-1, 2, (P, 2, 2, 2)) * 0.5).astype(np.float32)
        mid = list(range(P, 2 * P))
        cand_p = DF.candidates_np(_periodic(fr_p, 3 * P), _periodic(fwd_p, 3 * P - 1), _periodic(bwd_p, 3 * P - 1), mid, tau, slack)
        masks_p, counts_p = DF.clean_np(cand_p, mid, support, radius)
        assert cand_p[mid].any() and not cand_p[mid].all()
        want = {k: _periodic(v[P:2 * P], L) for k, v in dict(cand=cand_p, masks=masks_p, counts=counts_p.astype(np.int32)).items()}
        for v in want.values():
            v[0], v[L - 1] = 0, 0
        ids = _dev(np.random.RandomState(87).permutation(L).astype(np.int32), dev)
        assert len(ids) > SLAB
        cand = ops.defect_candidates(_dev(_periodic(fr_p, L), dev), _dev(_periodic(fwd_p, L - 1), dev), _dev(_periodic(bwd_p, L - 1), dev),
                                     ids, tau, slack)
        masks, counts = ops.defect_clean(cand, ids, support, radius)
        for key, got in (("cand", cand), ("masks", masks), ("counts", counts)):
            g = got.cpu().numpy()
            assert g.dtype == want[key].dtype and np.array_equal(g, want[key]), (key, int((g != want[key]).sum()))


def test_hole_bbox_frames_more_frames_than_a_launch_takes(dev):
    """65 540 masks of 2 x 3: a box per frame, the frames on the grid's y axis, the table of boxes offset per slab"""
    with B.measured("hole_bbox_frames slabs", dev):
        rng = np.random.RandomState(88)
        m = ((rng.rand(L_B, 2, 3) < 0.3) * rng.randint(1, 256, (L_B, 2, 3))).astype(np.uint8)
        on = m != 0
        xs, ys = on.any(1), on.any(2)
        empty = ~on.any((1, 2))
        want = np.stack([np.where(empty, 0x7f7f7f7f, xs.argmax(1)), np.where(empty, 0x7f7f7f7f, ys.argmax(1)),
                         np.where(empty, 0, 3 - xs[:, ::-1].argmax(1)), np.where(empty, 0, 2 - ys[:, ::-1].argmax(1))], 1).astype(np.int32)
        assert empty[SLAB:].any() and not empty[SLAB:].all()
        got = ops.hole_bbox_frames(_dev(m, dev)).cpu().numpy()
        assert np.array_equal(got, want), int((got != want).any(1).sum())
        whole = ops.hole_bbox(_dev(m[SLAB:], dev)).cpu().numpy()
        assert whole.tolist() == [0, 0, 3, 2]


def test_scene_diff_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 2 x 2: the histogram pass carries the frames on the grid's y axis; pair 65 534 sets the last frame of the first
    slab against the first of the second"""
    with B.measured("scene_diff slabs", dev):
        fr = np.random.RandomState(89).randint(0, 256, (L_B, 2, 2, 3)).astype(np.uint8)
        want = SD.scene_diff_np(fr)
        assert want[SLAB - 1:].any()
        got = ops.scene_diff(_dev(fr, dev)).cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, want), int((got != want).sum())


def _stretches(margin):
    """(a, b, cuts, lo, hi): where the restatement walks the frames in Python it runs on frames [a, b) alone -- the start of the video,
    and its last 30 frames with the slab boundary and the cut among them; `cuts` is the cut as that stretch numbers it.  Frames
    [lo, hi) of a stretch read no frame outside it when a frame reads `margin` frames either side."""
    for a, b in ((0, 24), (L_B - 30, L_B)):
        yield a, b, ([CUT_B - a] if a < CUT_B < b else None), (a + margin if a else a), (b - margin if b < L_B else b)


def _tiny_frames(seed, spread=None):
    """uint8 [L_B,4,4,3]: noise, or with `spread` a level per frame and noise of that spread around it"""
    rng = np.random.RandomState(seed)
    if spread is None:
        return rng.randint(0, 256, (L_B, 4, 4, 3)).astype(np.uint8)
    return np.clip(rng.randint(40, 216, (L_B, 1, 1, 1)) + rng.randint(-spread, spread + 1, (L_B, 4, 4, 3)), 0, 255).astype(np.uint8)


def test_flicker_local_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 4 x 4 on a grid of 2 x 2: flicker_local_hist and flicker_local_apply launch the frames in slabs;
    flicker_local_curves is one launch.  Histograms and curves against the restatement on the stretches, the output on the whole
    video (the restatement's blend is one fancy index) with the device's curves."""
    with B.measured("flicker_local slabs", dev):
        grid, span, max_shift = (2, 2), 4, 32
        fr = _tiny_frames(93, spread=30)
        so = FL.scene_of_np(L_B, [CUT_B])
        x = _dev(fr, dev)
        hist = ops.flicker_local_hist(x, grid)
        Q, d16 = ops.flicker_local_curves(hist, _dev(so, dev), 4, 4, span, max_shift)
        hist, Q, d16 = hist.cpu().numpy(), Q.cpu().numpy(), d16.cpu().numpy()
        for a, b, _, lo, hi in _stretches(span):
            wh = FLL.hist_np(fr[a:b], grid)
            assert np.array_equal(hist[a:b], wh), (a, b)
            wq, wd = FLL.curves_np(wh, so[a:b], 4, 4, span, max_shift)
            assert np.array_equal(Q[lo:hi], wq[lo - a:hi - a]) and np.array_equal(d16[lo:hi], wd[lo - a:hi - a]), (a, b)
            assert wd[lo - a:hi - a].any()
        assert (hist.sum(axis=(1, 2, 3)) == 16).all() and d16[SLAB].any() and d16[CUT_B].any()
        want = FLL.apply_np(fr, d16)
        assert not np.array_equal(want[SLAB:], fr[SLAB:])
        got = ops.flicker_local_apply(x, _dev(d16, dev)).cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())


def test_color_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 4 x 4: color_hist and color_apply launch the frames in slabs.  Both against the restatement on the whole
    video; the tables are the caller's own, one either side of the cut, and two frames are in no group and copied."""
    with B.measured("color slabs", dev):
        fr = _tiny_frames(94)
        x = _dev(fr, dev)
        got = ops.color_hist(x).cpu().numpy()
        want = CL.hist_np(fr)
        assert np.array_equal(got, want), int((got != want).sum())
        lut = np.random.RandomState(95).randint(0, 256, (2, 3, 256)).astype(np.uint8)
        group = FL.scene_of_np(L_B, [CUT_B]).astype(np.int32)
        group[5], group[SLAB + 1] = -1, 2
        want = CL.apply_np(fr, lut, group)
        assert np.array_equal(want[SLAB + 1], fr[SLAB + 1]) and not np.array_equal(want[SLAB], fr[SLAB])
        got = ops.color_apply(x, _dev(lut, dev), _dev(group, dev)).cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())


def test_weave_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 4 x 4: weave_profiles and weave_apply launch the frames in slabs.  The profiles against the restatement on
    the whole video, the moved frames and their masks, a shift of its own per frame, on the stretches."""
    with B.measured("weave slabs", dev):
        fr = _tiny_frames(96)
        x = _dev(fr, dev)
        col, row = ops.weave_profiles(x)
        wc, wr = WV.profiles_np(fr)
        assert wc[SLAB:].any() and np.array_equal(col.cpu().numpy(), wc) and np.array_equal(row.cpu().numpy(), wr)
        shifts = np.random.RandomState(97).randint(-40, 41, (L_B, 2)).astype(np.int32)
        out, mask = ops.weave_apply(x, _dev(shifts, dev), return_mask=True)
        out, mask = out.cpu().numpy(), mask.cpu().numpy()
        for a, b, _, lo, hi in _stretches(0):
            wo, wm = WV.apply_np(fr[a:b], shifts[a:b])
            assert not np.array_equal(wo, fr[a:b]) and wm.any() and not wm.all()
            assert np.array_equal(out[a:b], wo) and np.array_equal(mask[a:b], wm), (a, b)


def test_interlace_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 4 x 4: interlace_scores launches the 65 539 pairs in slabs and deinterlace the frames; pair 65 534 sets the
    last frame of the first slab against the first of the second, and a picture of frame 65 535 reads frames 65 534 and 65 536."""
    with B.measured("interlace slabs", dev):
        tff, mode, guard, edges = INTERLACE_SETTING
        fr = _tiny_frames(98)
        x, scene = _dev(fr, dev), _dev(IL.scene_of_np(L_B, [CUT_B]), dev)
        D = ops.interlace_scores(x, scene).cpu().numpy()
        out = ops.deinterlace(x, scene, bool(tff), mode, bool(guard), edges).cpu().numpy()
        assert out.shape[0] == 2 * L_B
        for a, b, cuts, lo, hi in _stretches(1):
            wd = IL.scores_np(fr[a:b], cuts)
            assert wd[:-1].any() and np.array_equal(D[a:hi], wd[:hi - a]), (a, b)     # the last pair of a stretch reads the frame behind it
            want = IL.deinterlace_np(fr[a:b], cuts, tff, mode, guard, edges)
            assert not np.array_equal(want[1::2], fr[a:b])
            assert np.array_equal(out[2 * lo:2 * hi], want[2 * (lo - a):2 * (hi - a)]), (a, b)
        assert not D[CUT_B - 1].any() and not D[L_B - 1].any() and D[SLAB - 1].any() and D[SLAB].any()


def test_telecine_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 4 x 4: telecine_scores launches the frames in slabs; field_weave carries 65 540 jobs over 16 frames on the
    grid's y and z axes, against the restatement on all of them."""
    with B.measured("telecine slabs", dev):
        fr = _tiny_frames(99)
        M = ops.telecine_scores(_dev(fr, dev), _dev(IL.scene_of_np(L_B, [CUT_B]), dev)).cpu().numpy()
        for a, b, cuts, lo, hi in _stretches(1):
            wm = TC.scores_np(fr[a:b], cuts)
            assert wm[lo - a:hi - a].any() and np.array_equal(M[lo:hi], wm[lo - a:hi - a]), (a, b)
        jobs = np.random.RandomState(100).randint(0, 16, (L_B, 2))
        want = TC.weave_np(fr[:16], jobs, 1)
        assert not np.array_equal(want[SLAB:], fr[:16][jobs[SLAB:, 0]])
        got = ops.field_weave(_dev(fr[:16], dev), jobs, 1).cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())


def test_denoise_more_frames_than_a_launch_takes(dev):
    """65 540 frames of 4 x 4 with flows on halves: the luma pass and the filter pass launch the frames in slabs; frame 65 535
    averages over frames 65 534 and 65 536, frame 65 537 begins a scene."""
    with B.measured("denoise slabs", dev):
        rng = np.random.RandomState(101)
        fr = np.clip(rng.randint(60, 200, (1, 4, 4, 3)) + rng.randint(-6, 7, (L_B, 4, 4, 3)), 0, 255).astype(np.uint8)
        fwd = (rng.randint(-2, 3, (L_B - 1, 4, 4, 2)) * 0.5).astype(np.float32)
        bwd = (rng.randint(-2, 3, (L_B - 1, 4, 4, 2)) * 0.5).astype(np.float32)
        so = DN.scene_of_np(L_B, [CUT_B])
        got = ops.denoise(_dev(fr, dev), _dev(fwd, dev), _dev(bwd, dev), _dev(so, dev), *DENOISE_SETTING).cpu().numpy()
        for a, b, _, lo, hi in _stretches(1):
            want = DN.reference(fr[a:b], fwd[a:b - 1], bwd[a:b - 1], so[a:b], *DENOISE_SETTING)
            assert not np.array_equal(want[lo - a:hi - a], fr[lo:hi])
            assert np.array_equal(got[lo:hi], want[lo - a:hi - a]), (a, b)


# ------------------------------------------------------------------------------------------------ limits that are refusals
def test_warp_error_takes_65536_frames_and_refuses_more(dev):
    """65 536 frames of one pixel are 65 535 pairs, all the grid's y axis holds; one more is refused by name.  With one pixel a sample
    stays inside only for a flow of exactly zero; the pairs repeat every seven frames and the float64 reference runs on seven."""
    with B.measured("warp_error limit", dev):
        L, P = 65536, 7
        rng = np.random.RandomState(90)
        fr_p = rng.randint(0, 256, (P, 1, 1, 3)).astype(np.float32)
        fwd_p = np.zeros((P, 1, 1, 2), np.float32)
        bwd_p = (rng.randint(-1, 2, (P, 1, 1, 2)) * 0.5).astype(np.float32)
        fwd_p[2, 0, 0, 0], fwd_p[5, 0, 0, 1], bwd_p[3, 0, 0, 0] = 0.25, np.nan, 4.0      # outside, not finite, occluded
        ref = WE.rows(WE.reference(np.concatenate([fr_p, fr_p[:1]]), fwd_p, bwd_p))
        assert set(ref[:, 1]) == {0.0, 1.0} and (ref[:, 0] > 0).sum() >= 3
        want = _periodic(ref, L - 1)
        for u8 in (False, True):
            frames = _periodic(fr_p, L)
            got = metrics.warp_error(_dev(frames.astype(np.uint8) if u8 else frames, dev), _dev(_periodic(fwd_p, L - 1), dev),
                                     _dev(_periodic(bwd_p, L - 1), dev)).cpu().numpy()
            assert got.shape == (L - 1, 2) and np.array_equal(got[:, 1], want[:, 1])
            assert (np.abs(got[:, 0] - want[:, 0]) <= 1e-9 * np.maximum(want[:, 0], 1e-12)).all()      # test_gpu_warp_error's bound
        z = torch.zeros((L, 1, 1, 2), dtype=torch.float32, device=dev)
        with pytest.raises(lib.HipError, match="65536"):
            metrics.warp_error(torch.zeros((L + 1, 1, 1, 3), dtype=torch.uint8, device=dev), z, z)


def test_slab_copies_take_65535_rows_and_refuse_more(dev):
    with B.measured("gather / scatter limit", dev):
        n = SLAB
        g = torch.Generator(device="cpu").manual_seed(91)
        cache = torch.randn((9, 4), generator=g).to(dev)
        ids = torch.randint(-1, 10, (n,), generator=g).to(torch.int32).to(dev)          # -1 and 9: no slot, a row of zeros
        want = torch.where(((ids >= 0) & (ids < 9)).view(n, 1), cache[ids.long().clamp(0, 8)], torch.zeros((), device=dev))
        assert torch.equal(ops.gather_slabs(cache, ids), want)
        rows = torch.randn((n, 4), generator=g).to(dev)
        perm = torch.randperm(n + 3, generator=g)[:n].to(torch.int32).to(dev)
        big = torch.full((n + 3, 4), 5.0, device=dev)
        expect = big.clone()
        expect[perm.long()] = rows
        assert torch.equal(ops.scatter_slabs(rows, perm, big), expect)
        more = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        with pytest.raises(lib.HipError, match="gather_slabs"):
            ops.gather_slabs(cache, more)
        with pytest.raises(lib.HipError, match="scatter_slabs"):
            ops.scatter_slabs(torch.zeros((n + 1, 4), device=dev), more, big)
        assert torch.equal(big, expect)                                                 # the refused call wrote nothing


def test_psnr_ssim_takes_65535_pairs_and_refuses_more(dev):
    """the pairs ride on the grid's y axis: 65 535 pairs of 3 x 3 with a window of 3 -- one window a channel -- against
    oracle/metrics_ref on 300 of them, the last ones among them, and against its formulas on arrays for all; one pair more is
    refused with a message that names the limit (it used to come back as whatever the failed launch said)"""
    with B.measured("psnr_ssim limit", dev):
        N = SLAB
        rng = np.random.RandomState(92)
        a = rng.randint(0, 256, (N, 3, 3, 3)).astype(np.float32)
        b = np.clip(a + rng.randint(-40, 41, a.shape), 0, 255).astype(np.float32)
        b[7] = a[7]                                                     # identical: PSNR is inf
        got = metrics.psnr_ssim(_dev(a, dev), _dev(b, dev), 3).cpu().numpy()
        assert got.shape == (N, 2)
        A, Bb = a.astype(np.float64), b.astype(np.float64)
        mse = ((A - Bb) ** 2).mean(axis=(1, 2, 3))
        with np.errstate(divide="ignore"):
            psnr = np.where(mse == 0, np.inf, 20.0 * np.log10(255.0 / np.sqrt(np.where(mse == 0, 1.0, mse))))
        ux, uy = A.mean(axis=(1, 2)), Bb.mean(axis=(1, 2))              # per channel: the one window is the image
        cn = 9.0 / 8.0
        vx, vy, vxy = cn * ((A * A).mean((1, 2)) - ux * ux), cn * ((Bb * Bb).mean((1, 2)) - uy * uy), cn * ((A * Bb).mean((1, 2)) - ux * uy)
        C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        ssim = (((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))).mean(1)
        pick = np.unique(np.concatenate([np.arange(100), np.arange(N - 100, N), rng.randint(0, N, 100)]))
        ref = np.array([metrics_ref.calc_psnr_and_ssim(a[i], b[i], 3) for i in pick])
        fin = np.isfinite(ref[:, 0])
        assert np.isinf(ref[:, 0][~fin]).all() and (~fin).sum() == 1
        # 1e-9: the bound test_gpu_warp_error holds evaluate_video's metrics to against the same oracle
        assert np.abs(psnr[pick][fin] - ref[fin, 0]).max() <= 1e-9 * ref[fin, 0].max() and np.abs(ssim[pick] - ref[:, 1]).max() <= 1e-9
        assert np.array_equal(np.isinf(got[:, 0]), mse == 0) and np.isinf(got[7, 0])
        ok = mse != 0
        assert np.abs(got[ok, 0] - psnr[ok]).max() <= 1e-9 * psnr[ok].max() and np.abs(got[:, 1] - ssim).max() <= 1e-9
        z = torch.zeros((N + 1, 3, 3, 3), dtype=torch.float32, device=dev)
        with pytest.raises(lib.HipError, match="65535"):
            metrics.psnr_ssim(z, z, 3)


# ================================================================================================ Part A, continued
GRAIN_CASE = "bands_66x70"


def _grain(dev):
    c, want = GR.case(GRAIN_CASE), GR.want(GRAIN_CASE)
    k = c["L"]
    assert c["hole"] is None and len(np.unique(want["band"])) > 2
    fr, n = _big_frames(c["frames"], dev, "grain_blocks")
    energy, band = ops.grain_blocks(fr)
    B.assert_tiled(energy, want["energy"], "grain_blocks energy")
    B.assert_tiled(band, want["band"], "grain_blocks band")
    del fr, energy, band
    torch.cuda.empty_cache()
    # grain_apply: the noise depends on the frame number, so whole tiles are compared at both ends and where the buffers pass 2^31
    # and 2^32 bytes, with the inputs read back and the true frame numbers; everywhere else the bytes outside `where` are the input's
    filled = B.tiled(c["filled"], n, dev)
    where = B.tiled(c["where"], n, dev)
    B.wrap_is_visible(filled, B.nbytes(c["filled"]), "grain_apply filled")
    lut = np.stack([want["lut"][0], c["alt_lut"][0]])
    scene = (B.scene_of(n * k, k, dev) % 3 - 1).to(torch.int32)        # scene -1: a tile that is copied
    seed = c["seed"]
    out = ops.grain_apply(filled, where, _dev(lut, dev), scene, seed)
    tiles = B.tile_windows(n, B.nbytes(c["filled"]), (B.nbytes(c["where"]),))
    assert len(tiles) >= 4
    changed = 0
    for i in tiles + [t + 1 for t in tiles[:-1]]:
        a, b = i * k, (i + 1) * k
        sub = GR.apply_np(filled[a:b].cpu().numpy(), where[a:b].cpu().numpy(), lut, scene[a:b].cpu().numpy(), (seed + 0x9E3779B9 * a) & 0xFFFFFFFF)
        got = out[a:b].cpu().numpy()
        assert np.array_equal(got, sub), (i, int((got != sub).sum()))
        changed += int((sub != c["filled"]).sum())
    assert changed
    per = max(1, B.CHUNK // B.nbytes(c["filled"][:1]))
    for a in range(0, n * k, per):
        keep = (where[a:a + per] == 0).unsqueeze(-1)
        assert torch.equal(torch.where(keep, out[a:a + per], 0), torch.where(keep, filled[a:a + per], 0)), a
    B.assert_tiled(filled, c["filled"], "grain_apply filled")


def test_grain_past_4gib(dev):
    with B.measured("grain_blocks / grain_apply", dev):
        _grain(dev)


DEFECT_CASE = "wave_70x90"


def _defects(dev):
    c = DF.case(DEFECT_CASE)
    k = c["L"]
    inner = DF.plan_np(k, c["scenes"])
    cand_t = DF.candidates_np(c["frames"], c["fwd"], c["bwd"], inner, c["threshold"], c["slack"])
    masks_t, counts_t = DF.clean_np(cand_t, inner, c["support"], c["radius"])
    assert cand_t.any() and masks_t.any() and not np.array_equal(masks_t, 255 * cand_t)
    fr, n = _big_frames(c["frames"], dev, "defects")
    (fwd, bwd), (fwd_tile, _) = _flow_tiles(c, n, dev)
    B.wrap_is_visible(fwd, B.nbytes(fwd_tile), "defects fwd")
    B.wrap_is_visible(bwd, B.nbytes(fwd_tile), "defects bwd")
    ids = (torch.arange(n, device=dev).view(n, 1) * k + _dev(np.asarray(inner, np.int64), dev).view(1, -1)).view(-1)
    g = torch.Generator(device="cpu").manual_seed(11)
    ids = ids[torch.randperm(ids.numel(), generator=g).to(dev)].to(torch.int32).contiguous()
    assert ids.numel() > SLAB
    cand = ops.defect_candidates(fr, fwd, bwd, ids, c["threshold"], c["slack"])
    B.assert_tiled(cand, cand_t, "defect_candidates")
    masks, counts = ops.defect_clean(cand, ids, c["support"], c["radius"])
    B.assert_tiled(masks, masks_t, "defect_clean masks")
    B.assert_tiled(counts, counts_t.astype(np.int32), "defect_clean counts")
    B.assert_tiled(fr, c["frames"], "defects frames")


def test_defects_past_4gib(dev):
    with B.measured("defect_candidates / defect_clean", dev):
        _defects(dev)


def _holes(dev):
    from tests import hole_label_cases as HL
    Hm, Wm, k = 66, 130, 3
    U = HL.footprints(Hm, Wm, ops.LABEL_TILE_H, ops.LABEL_TILE_W)["two_combs"]
    U = U & (np.random.RandomState(12).rand(Hm, Wm) < 0.9)
    U[:3], U[:, :2], U[-2:], U[:, -5:] = False, False, False, False    # the box is not the frame
    base = HL.video_of(U, L=k, seed=13).astype(np.uint8)
    base[1, :20], base[2, :, 100:] = 0, 0                               # a box of its own for every frame
    labels_t, boxes_t = HL.components_np(HL.footprint_np(base))
    assert len(boxes_t) > 1
    n = B.tiles_past(B.nbytes(base))
    masks = B.tiled(base, n, dev)
    B.wrap_is_visible(masks, B.nbytes(base), "hole masks")
    L = masks.shape[0]
    print("holes L", L, "H", Hm, "W", Wm, "k", k, "bytes", masks.numel())
    # the footprint and the box again: torch reductions on the device, a stretch of frames at a time
    foot = torch.zeros((Hm, Wm), dtype=torch.bool, device=dev)
    per = max(1, B.CHUNK // (Hm * Wm))
    for a in range(0, L, per):
        foot |= (masks[a:a + per] != 0).any(0)
    assert np.array_equal(foot.cpu().numpy(), HL.footprint_np(base))
    xs, ys = foot.any(0).nonzero().view(-1), foot.any(1).nonzero().view(-1)
    box = [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]
    assert box != [0, 0, Wm, Hm] and ops.hole_bbox(masks).tolist() == box
    per_frame = []
    for m in base:
        y, x = np.nonzero(m)
        per_frame.append([x.min(), y.min(), x.max() + 1, y.max() + 1])
    assert len({tuple(b) for b in per_frame}) > 1
    B.assert_tiled(ops.hole_bbox_frames(masks), np.asarray(per_frame, np.int32), "hole_bbox_frames")
    labels, boxes = ops.hole_components(masks)
    assert torch.equal(labels != 0, foot)
    assert np.array_equal(labels.cpu().numpy(), labels_t) and np.array_equal(boxes.cpu().numpy(), boxes_t)


def test_holes_past_4gib(dev):
    with B.measured("hole_bbox / hole_bbox_frames / hole_label", dev):
        _holes(dev)


def _warp_error(dev, u8):
    """warp_error takes 65 536 frames at the most, so the frames are large enough for 65 535 of them to pass 2^32 bytes"""
    k, H, W = 3, 131, 171
    c = WE.smooth(H, W, k + 1, 14)
    frames = np.rint(c["frames"][:k]).astype(np.uint8) if u8 else np.ascontiguousarray(c["frames"][:k])
    fwd, bwd = np.ascontiguousarray(c["fwd"]), np.ascontiguousarray(c["bwd"])        # k flows: the last is the pair between two tiles
    ref = WE.reference(np.concatenate([frames, frames[:1]]).astype(np.float32), fwd, bwd)
    want = WE.rows(ref)
    assert (want[:, 1] > 0).all() and (want[:, 1] < H * W).all() and (want[:, 0] > 0).all() and min(r["margin"] for r in ref) >= 1e-9
    n = 65535 // k
    assert n * k <= 65536
    fr = B.tiled(frames, n, dev)
    big_fwd, big_bwd = B.tiled(fwd, n, dev, drop=1), B.tiled(bwd, n, dev, drop=1)
    for t, nb, what in ((fr, B.nbytes(frames), "frames"), (big_fwd, B.nbytes(fwd), "fwd"), (big_bwd, B.nbytes(bwd), "bwd")):
        B.wrap_is_visible(t, nb, "warp_error " + what)
    print("warp_error", "u8" if u8 else "f32", "L", fr.shape[0], "H", H, "W", W, "k", k, "frame bytes", fr.numel() * fr.element_size(),
          "flow bytes", big_fwd.numel() * 4)
    got = metrics.warp_error(fr, big_fwd, big_bwd).cpu().numpy()
    rows = _periodic(want, n * k - 1)
    assert got.shape == rows.shape and np.array_equal(got[:, 1], rows[:, 1])
    assert (np.abs(got[:, 0] - rows[:, 0]) <= 1e-9 * np.maximum(rows[:, 0], 1e-12)).all()          # test_gpu_warp_error's bound


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "float"])
def test_warp_error_past_4gib(dev, u8):
    with B.measured("warp_error %s" % ("u8" if u8 else "f32"), dev):
        _warp_error(dev, u8)


def _far_frames(L, frame_bytes):
    """frame numbers at both ends and on either side of byte offsets 2^31 and 2^32 of a buffer with `frame_bytes` a frame"""
    at31, at32 = B.WRAP // 2 // frame_bytes, B.WRAP // frame_bytes
    assert at32 + 2 < L
    return [L - 1, at32 + 1, 0, at32, at31 + 1, at32 + 2, at31, L - 2]


def _window_kernels(dev):
    """mask_prepare with ids, masked_clip and composite: a window's frames picked by number out of a video of more than 2^32 bytes"""
    from PIL import Image
    from oracle import video_ref
    # mask_prepare: source masks of one byte a pixel, 2^32 bytes of them
    Hin, Win, H, W, k = 66, 130, 50, 70, 3
    rng = np.random.RandomState(15)
    base = ((rng.rand(k, Hin, Win) > 0.97) * rng.randint(1, 256, (k, Hin, Win))).astype(np.uint8)
    n = B.tiles_past(B.nbytes(base))
    masks = B.tiled(base, n, dev)
    B.wrap_is_visible(masks, B.nbytes(base), "mask_prepare masks")
    L = masks.shape[0]
    far = _far_frames(L, Hin * Win)
    assert len({f % k for f in far}) == k
    ids = far + [-1, L]                                                # outside the video: an empty mask
    ytab, xtab = (_dev(video.nearest_table(a, b), dev) for a, b in ((Hin, H), (Win, W)))
    got = ops.mask_prepare(masks, ytab, xtab, H, W, 4, ids=_dev(np.asarray(ids, np.int32), dev)).cpu().numpy()
    for i, f in enumerate(ids):
        want = np.zeros((H, W), np.uint8)
        if 0 <= f < L:
            r = np.array(Image.fromarray(base[f % k]).resize((W, H), Image.NEAREST).convert("L"))
            want = video_ref.dilate_cross_np(r > 0, 4).astype(np.uint8)
            assert want.any() and not want.all()
        assert np.array_equal(got[i], want), (i, f)
    print("mask_prepare L", L, "H", Hin, "W", Win, "k", k, "bytes", masks.numel())
    # every mask of the video at its own size: more than 2^32 threads' worth of output pixels.  The runtime launches
    # `threads mod 2^32` of a grid that holds more, so the entry strides a smaller grid over them.
    same_y, same_x = (_dev(video.nearest_table(a, a), dev) for a in (Hin, Win))
    whole = np.stack([video_ref.dilate_cross_np(m > 0, 2) for m in base]).astype(np.uint8)
    assert L * Hin * Win > B.WRAP and not np.array_equal(whole, (base > 0).astype(np.uint8))
    B.assert_tiled(ops.mask_prepare(masks, same_y, same_x, Hin, Win, 2), whole, "mask_prepare of every frame")
    del masks
    torch.cuda.empty_cache()
    # masked_clip and composite: frames of 2^32 bytes, their masks, and an fp32 accumulator of four times that
    fbase = _frames_tile()
    k, H, W = fbase.shape[:3]
    mbase = (rng.rand(k, H, W) < 0.3).astype(np.uint8)
    fr, n = _big_frames(fbase, dev, "masked_clip / composite")
    m01 = B.tiled(mbase, n, dev)
    L = fr.shape[0]
    far = _far_frames(L, H * W * 3)
    assert len({f % k for f in far}) == k
    ids_t = _dev(np.asarray(far, np.int32), dev)
    Hp, Wp = H + 2, W + 4
    clip = ops.masked_clip(fr, m01, ids_t, Hp, Wp).cpu().numpy()
    sy = np.where(np.arange(Hp) < H, np.arange(Hp), 2 * H - 1 - np.arange(Hp))
    sx = np.where(np.arange(Wp) < W, np.arange(Wp), 2 * W - 1 - np.arange(Wp))
    for i, f in enumerate(far):
        v = (fbase[f % k].astype(np.float32) / np.float32(255)) * np.float32(2) - np.float32(1)
        v = v * (np.float32(1) - mbase[f % k].astype(np.float32))[..., None]
        want = v[sy][:, sx].transpose(2, 0, 1)
        assert np.array_equal(clip[0, i], want), (i, f)
    comp_base = (fbase.astype(np.float32) * np.float32(0.5) + np.float32(3.25))
    comp = B.tiled(comp_base, n, dev)
    assert comp.numel() * 4 > 4 * B.WRAP
    pred = (2 * rng.random_sample((len(far), 3, Hp, Wp)) - 1).astype(np.float32)
    first = np.array([1, 0, 0, 1, 0, 1, 0, 0], np.uint8)
    ops.composite(_dev(pred, dev), ids_t, _dev(first, dev), fr, m01, comp)
    for i, f in enumerate(far):
        p = ((pred[i, :, :H, :W].transpose(1, 2, 0) + np.float32(1)) / np.float32(2) * np.float32(255)).astype(np.int32).astype(np.uint8)
        img = np.where(mbase[f % k][..., None] != 0, p, fbase[f % k]).astype(np.float32)
        want = img if first[i] else comp_base[f % k] * np.float32(0.5) + img * np.float32(0.5)
        assert not np.array_equal(want, comp_base[f % k])
        assert np.array_equal(comp[f].cpu().numpy(), want), (i, f)
        comp[f] = _dev(comp_base[f % k], dev)                           # put back: every other frame is compared as tiles
    B.assert_tiled(comp, comp_base, "composite left the other frames alone")
    B.assert_tiled(fr, fbase, "composite frames")


def test_window_kernels_past_4gib(dev):
    with B.measured("mask_prepare ids / masked_clip / composite", dev):
        _window_kernels(dev)


PIXEL_CASE = "smooth_70x90"


def _bits(a):
    """fp32 as its bit patterns: origins that were never stored are NaN on both sides"""
    return a.view(torch.int32) if isinstance(a, torch.Tensor) else np.ascontiguousarray(a).view(np.int32)


def _pixel_track(dev):
    """one launch of the six jobs of every tile from the planes' first state: ages 255 in the hole, origins that hold something else"""
    c = PT.case(PIXEL_CASE)
    k, H, W = c["L"], c["H"], c["W"]
    assert k == 6
    hole = c["hole"]
    age0 = np.stack([hole * 255, hole * 255]).astype(np.uint8)
    org0 = np.random.RandomState(16).rand(2, k, H, W, 2).astype(np.float32)
    age, org = age0.copy(), org0.copy()
    for t, d in MASK_JOBS:
        s, dst = (t, t + 1) if d == 0 else (t + 1, t)
        g, f = (c["bwd"][t], c["fwd"][t]) if d == 0 else (c["fwd"][t], c["bwd"][t])
        PT.step_np(hole[dst], age[d, s], org[d, s], age[d, dst], org[d, dst], g, f, 254, True)
    assert not np.array_equal(age, age0) and not np.array_equal(org, org0) and (age == 255).any() and (age == 1).any()
    fwd_tile, bwd_tile = B.padded_flows(c["fwd"], 5), B.padded_flows(c["bwd"], 6)
    n = B.tiles_past(B.nbytes(fwd_tile))
    fwd, bwd = B.tiled(fwd_tile, n, dev, drop=1), B.tiled(bwd_tile, n, dev, drop=1)
    B.wrap_is_visible(fwd, B.nbytes(fwd_tile), "pixel_track fwd")
    B.wrap_is_visible(bwd, B.nbytes(bwd_tile), "pixel_track bwd")
    d_age = B.tiled_planes(age0, n, dev)
    d_org = B.tiled_planes(org0, n, dev)
    B.wrap_is_visible(d_org, B.nbytes(org0[0]), "pixel_track origin")
    jobs = _jobs_of_tiles(MASK_JOBS, k, n, dev, 17)
    assert jobs.shape[0] > SLAB
    print("pixel_track_step L", n * k, "H", H, "W", W, "k", k, "jobs", jobs.shape[0], "flow bytes", fwd.numel() * 4, "origin bytes",
          d_org.numel() * 4, "age bytes", d_age.numel())
    ops.pixel_track_step(B.tiled(hole, n, dev), d_age, d_org, fwd, bwd, jobs, 254, True)
    for d in (0, 1):
        B.assert_tiled(d_age[d], age[d], "pixel_track_step age %d" % d)
        B.assert_tiled(_bits(d_org[d]), _bits(org[d]), "pixel_track_step origin %d" % d)


def test_pixel_track_step_past_4gib(dev):
    with B.measured("pixel_track_step", dev):
        _pixel_track(dev)


def _pixel_fill(dev):
    """the fill over the planes the case's chains leave: the frame a colour comes from lies in the pixel's own tile"""
    c = PT.case(PIXEL_CASE)
    out_t, source_t, age_t, org_t = PT.reference(PIXEL_CASE)
    k = c["L"]
    assert not np.array_equal(out_t, c["filled"]) and set(np.unique(source_t)) == {0, 1, 2, 3}
    src, n = _big_frames(c["src"], dev, "pixel_fill")
    age = B.tiled_planes(age_t, n, dev)
    org = B.tiled_planes(org_t, n, dev)
    B.wrap_is_visible(org, B.nbytes(org_t[0]), "pixel_fill origin")
    out = B.tiled(c["filled"], n, dev)
    got, source = ops.pixel_fill(src, B.tiled(c["hole"], n, dev), age, org, out, return_source=True)
    assert got.data_ptr() == out.data_ptr()
    print("pixel_fill origin bytes", org.numel() * 4, "age bytes", age.numel())
    B.assert_tiled(out, out_t, "pixel_fill")
    B.assert_tiled(source, source_t, "pixel_fill source")
    B.assert_tiled(src, c["src"], "pixel_fill src")


def test_pixel_fill_past_4gib(dev):
    with B.measured("pixel_fill", dev):
        _pixel_fill(dev)


def _restore(dev):
    """the paste-back into source frames of more than 2^32 bytes: restore_u8 over the whole frame with the hard edge and in a box
    with a feathered one, and restore_blend of a window whose frames lie at the far end of the source and of its fp32 accumulator;
    lo and its masks stay small"""
    from tests.test_video_feather import feather_np
    from tests.test_video_restore import frames as rframes, masks as rmasks, restore_np
    (w, h), (W, H), k = (36, 20), (400, 30), 3
    box, touch, r = (129, 9, 260, 29), (100, 3, 300, 30), 3
    lo_t, src_t, m_t = rframes(k, w, h, 21), rframes(k, W, H, 22), rmasks(h, w, 23)[[4, 5, 1]]        # 30 % noise, a diagonal, full
    src, n = _big_frames(src_t, dev, "restore")
    L = src.shape[0]
    lo, m = B.tiled(lo_t, n, dev), B.tiled(m_t, n, dev)
    want = restore_np(lo_t, m_t, src_t)
    assert not np.array_equal(want, src_t)
    out = ops.restore_u8(lo, m, src, *video._restore_tables((h, w), (H, W), dev))
    B.assert_tiled(out, want, "restore_u8")
    tabs = video._restore_tables((h, w), (box[3] - box[1], box[2] - box[0]), dev)
    want = feather_np(lo_t, m_t, src_t, r, box)
    assert not np.array_equal(want, src_t) and not np.array_equal(want, restore_np(lo_t, m_t, src_t))
    assert ops.restore_u8(lo, m, src, *tabs, out=out, box=box, feather=r) is out
    B.assert_tiled(out, want, "restore_u8 in a box, feathered")
    B.assert_tiled(src, src_t, "restore_u8 src")
    del out, lo, m
    torch.cuda.empty_cache()
    acc_t = src_t.astype(np.float32) * np.float32(0.5) + np.float32(0.25)
    acc = B.tiled(acc_t, n, dev)
    B.wrap_is_visible(acc, B.nbytes(acc_t), "restore_blend acc")
    far = _far_frames(L, H * W * 3)
    ids = far + [-1, L]                                                # outside the video: skipped
    lo_w, m_w = rframes(len(ids), w, h, 24), rmasks(h, w, 25)[[4, 5, 1, 4, 5, 2, 3, 4, 1, 1]]
    first = np.array([1, 0, 0, 1, 0, 1, 0, 0, 1, 0], np.uint8)
    print("restore_blend L", L, "H", H, "W", W, "k", k, "acc bytes", acc.numel() * 4, "src bytes", src.numel())
    for feather, tch in ((0, None), (r, touch)):
        tl, tu, tr, tb = tch or box
        got = ops.restore_blend(_dev(lo_w, dev), _dev(m_w, dev), src, _dev(np.asarray(ids, np.int32), dev), _dev(first, dev), acc, *tabs,
                                box=box, touch=tch, feather=feather)
        assert got is acc
        for i, f in enumerate(far):
            one = src_t[f % k][None]
            img = (feather_np(lo_w[i:i + 1], m_w[i:i + 1], one, feather, box) if feather else
                   _restore_box_np(lo_w[i:i + 1], m_w[i:i + 1], one, box, restore_np))[0].astype(np.float32)
            want = acc_t[f % k].copy()
            want[tu:tb, tl:tr] = img[tu:tb, tl:tr] if first[i] else acc_t[f % k][tu:tb, tl:tr] * np.float32(0.5) + img[tu:tb, tl:tr] * np.float32(0.5)
            assert not np.array_equal(want, acc_t[f % k])
            assert np.array_equal(_bits(acc[f].cpu().numpy()), _bits(want)), (feather, i, f)
            acc[f] = _dev(acc_t[f % k], dev)                            # put back: every other frame is compared as tiles
        B.assert_tiled(_bits(acc), _bits(acc_t), "restore_blend left the other frames alone")


def _restore_box_np(lo, m, src, box, restore_np):
    """the hard paste confined to a box: restore_np of the box's pixels, the source outside"""
    left, upper, right, lower = box
    out = src.copy()
    out[:, upper:lower, left:right] = restore_np(lo, m, src[:, upper:lower, left:right])
    return out


def test_restore_past_4gib(dev):
    with B.measured("restore_u8 / restore_blend", dev):
        _restore(dev)
