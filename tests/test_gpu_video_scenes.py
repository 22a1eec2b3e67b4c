"""Scene cuts on the device: the block-histogram kernels (csrc/video.hip scene_hist_kernel / scene_diff_kernel) against the numpy
restatement of tests/scene_diff_cases.py, every integer equal, and inpaint_video(scenes=) in every driver against the calls on
each scene's frames alone, byte for byte."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, metrics, ops, video
from tests import scene_diff_cases as S

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 1), (3, 3, 5), (4, 7, 5), (5, 37, 53), (3, 64, 256), (25, 240, 432)]


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    buf = torch.zeros(a.size + shift, dtype=torch.uint8, device=dev)
    return buf[shift:].view(a.shape).copy_(torch.from_numpy(np.ascontiguousarray(a)))


@pytest.mark.parametrize("L,H,W", SHAPES, ids=str)
def test_scene_diff_is_the_restatement(dev, L, H, W):
    """random bytes, constant frames of 0, 255 and a mid value (every pixel of a cell in one bin: all adds of a wave meet on one
    counter), a smooth gradient; at 25 x 240 x 432 the tennis fixture as well.  (4,7,5): a frame is 105 bytes, so every frame
    after the first starts misaligned; the other bases are moved by hand."""
    videos = [(k, S.content(k, L, H, W)) for k in S.CONTENTS]
    if (L, H, W) == (25, 240, 432):
        videos.append(("tennis", S.tennis()))
    for i, (kind, f) in enumerate(videos):
        want = S.scene_diff_np(f)
        for shift in ((0, 1 + i) if H * W <= 37 * 53 or kind == "tennis" else (i % 2 * 3,)):
            got = ops.scene_diff(_up(f, dev, shift))
            assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (L - 1,)
            assert got.cpu().tolist() == want.tolist(), (kind, shift)
        if kind in ("zeros", "full"):
            assert want.tolist() == [0] * (L - 2) + [2 * H * W]
        if kind == "mid":
            assert want.tolist() == [2 * H * W] * (L - 1)


def test_scene_diff_does_not_depend_on_the_workspace(dev):
    """the C entry on a workspace full of 0xFF bytes, then again on the same workspace (which now holds the first call's tables):
    the integers of ops.scene_diff, three times"""
    so = lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for L, H, W in ((4, 7, 5), (5, 37, 53), (3, 64, 256)):
        f = S.content("random", L, H, W, seed=3)
        fd = _up(f, dev, 5)
        want = S.scene_diff_np(f).tolist()
        assert ops.scene_diff(fd).cpu().tolist() == want
        nbytes = so.e2fgvi_scene_diff_workspace(L, H, W)
        assert nbytes == L * 4096
        work = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            out = torch.full((L - 1,), -7, dtype=torch.int64, device=dev)
            assert so.e2fgvi_scene_diff(p(fd), L, H, W, p(work), p(out), st) == 0
            assert out.cpu().tolist() == want
        # the workspace holds the frames' tables afterwards
        assert np.array_equal(work.view(torch.int32).cpu().numpy().reshape(L, 16, 64), S.hist_np(f))


def test_scene_diff_checks_its_arguments(dev):
    f = torch.zeros((3, 7, 5, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError):
        ops.scene_diff(f.int())
    with pytest.raises(TypeError):
        ops.scene_diff(f.cpu())
    with pytest.raises(ValueError):
        ops.scene_diff(f[..., :2].contiguous())
    with pytest.raises(ValueError):
        ops.scene_diff(f.permute(0, 2, 1, 3))
    with pytest.raises(ValueError):
        ops.scene_diff(f[:1])
    assert ops.scene_diff(f).cpu().tolist() == [0, 0]


def test_detect_cuts_on_the_tennis_join(dev):
    f = S.tennis_join()
    s = video.scene_scores(f, device=dev)
    assert s.dtype == np.float64 and np.array_equal(s, S.scores_np(f))
    assert video.detect_cuts(f, device=dev) == [S.TENNIS_CUT] == [12]
    assert video.detect_cuts(torch.from_numpy(f).to(dev)) == [12]
    assert video.detect_cuts(S.tennis(), device=dev) == []
    assert video.detect_cuts(f, threshold=0.5, device=dev) == [] and video.detect_cuts(f, min_scene=13, device=dev) == []


# ------------------------------------------------------------------------------------------------ the drivers
def _fake_model(x, n_local):
    # tests/test_video_driver.py's stand-in: every output depends on the whole clip through its mean
    b, t, c, H, W = x.shape
    y = torch.tanh(x.reshape(b * t, c, H, W) * 0.7 + 0.1 * x.mean(dim=(1, 2, 3, 4)).view(1, 1, 1, 1))
    return y, None


def _fake_model_batch(x, n_local):
    # per-clip (batch independent) stand-in
    b, t, c, H, W = x.shape
    y = torch.tanh(x * 0.7 + 0.1 * x.mean(dim=(1, 2, 3, 4), keepdim=True)).reshape(b * t, c, H, W)
    return y, None


def _per_scene(run, f, m, cuts):
    bounds = list(zip([0] + cuts, cuts + [len(f)]))
    return np.concatenate([run(f[s:e], m[s:e]) for s, e in bounds])


@pytest.mark.parametrize("kw", [{}, {"batch_windows": 3}, {"in_flight": 2}], ids=str)
def test_scenes_are_independent(dev, kw):
    """L = 23, a cut at 9, stride 5: the bytes of the two calls on frames[:9] and frames[9:]; other content behind the cut leaves
    the frames in front of it as they were -- which is not so without scenes="""
    L, c = 23, 9
    f, m = S.toy_video(L, 50, 70)
    fm = _fake_model_batch if "batch_windows" in kw else _fake_model
    net = lambda x, n: (fm(x.cpu(), n)[0].to(dev), None)
    run = lambda ff, mm, **k: video.inpaint_video(net, ff, mm, 5, 10, -1, device=dev, **kw, **k)
    out = run(f, m, scenes=[c])
    assert out.shape == f.shape and out.dtype == np.uint8
    want = _per_scene(run, f, m, [c])
    assert np.array_equal(out, want), int((out != want).sum())
    other = f.copy()
    other[c:] = f[c:] // 4                              # darker: the stand-in sees a clip through its mean
    assert np.array_equal(run(other, m, scenes=[c])[:c], out[:c])
    plain = run(f, m)
    assert not np.array_equal(run(other, m)[:c], plain[:c])
    assert not np.array_equal(run(other, m), run(other, m, scenes=[c]))
    assert np.array_equal(run(f, m, scenes=[]), plain) and np.array_equal(run(f, m, scenes=None), plain)


@pytest.mark.parametrize("kw", [{}, {"reuse": True}], ids=str)
def test_scenes_with_the_real_network(dev, kw):
    """e2fgvi_hq, fp32, 60 x 100 frames (padded to 60 x 108), L = 17 with a cut at 7: the windows of a scene have the shapes they
    have in a call on the scene alone, hence the same kernels on the same bytes"""
    from e2fgvi_amd.synth import synth_state_dict
    f, m = S.toy_video(17, 60, 100, seed=3)
    net = importlib.import_module("model.e2fgvi_hq").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi_hq", "stress", 0))
    net = net.to(dev).eval()
    net.precision = "fp32"
    run = lambda ff, mm, **k: video.inpaint_video(net, ff, mm, 5, 10, -1, **kw, **k)
    out = run(f, m, scenes=[7])
    want = _per_scene(run, f, m, [7])
    print("scenes=[7] %s against the per-scene calls: %d bytes differ, max %d"
          % (kw, int((out != want).sum()), int(np.abs(out.astype(int) - want.astype(int)).max())))
    assert np.array_equal(out, want), int((out != want).sum())
    assert not np.array_equal(out, run(f, m))


def test_track_with_scenes(dev):
    """region="track" on the track tests' moving hole, stride 2 and a cut at 5: the per-scene calls' bytes, and their boxes"""
    from tests.test_gpu_video_restore import _stand_in_model
    from tests.test_video_track import moving_hole_video
    size, c = (108, 60), 5
    f, m = moving_hole_video()
    net = lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None)
    run = lambda ff, mm, **k: video.inpaint_video(net, ff, mm, neighbor_stride=2, device=dev, size=size, region="track", restore=True, **k)
    out = run(f, m, scenes=[c])
    want = _per_scene(run, f, m, [c])
    assert np.array_equal(out, want), int((out != want).sum())
    assert (out != f).any()
    boxes = video.track_regions(m, (250, 131), size, neighbor_stride=2, device=dev, scenes=[c])
    alone = [video.track_regions(mm, (250, 131), size, neighbor_stride=2, device=dev) for mm in (m[:c], m[c:])]
    assert boxes == alone[0] + alone[1] and boxes != video.track_regions(m, (250, 131), size, neighbor_stride=2, device=dev)
    assert len(boxes) == len(video.plan_windows(12, 2, scenes=[c]))


def test_scenes_auto(dev):
    """two toy shots, the random texture and a smooth gradient: "auto" finds the cut and returns the bytes of scenes=[cut]"""
    c = 9
    toy, m = S.toy_video(23, 50, 70)
    f = np.concatenate([toy[:c], S.gradient_video(14, 50, 70)])
    assert video.detect_cuts(f, device=dev) == [c]
    net = lambda x, n: (_fake_model(x.cpu(), n)[0].to(dev), None)
    auto = video.inpaint_video(net, f, m, 5, 10, -1, device=dev, scenes="auto")
    assert np.array_equal(auto, video.inpaint_video(net, f, m, 5, 10, -1, device=dev, scenes=[c]))
    # with size= the cuts are looked for in the caller's frames, before the resize
    a = video.inpaint_video(net, f, m, 5, 10, -1, device=dev, scenes="auto", size=(54, 40))
    assert np.array_equal(a, video.inpaint_video(net, f, m, 5, 10, -1, device=dev, scenes=[c], size=(54, 40)))
    # one shot: no cut, today's bytes
    assert np.array_equal(video.inpaint_video(net, toy, m, 5, 10, -1, device=dev, scenes="auto"),
                          video.inpaint_video(net, toy, m, 5, 10, -1, device=dev))


def test_evaluate_video_with_scenes(dev):
    """test_evaluate_video_with_warp's video, stand-in model and flows with a cut at 6: the row of pair (5, 6) is (0, 0), the
    others are warp_error's rows of the per-scene completion"""
    from tests import warp_error_cases as C
    rng = np.random.RandomState(5)
    L, h, w, c = 13, 70, 90, 6
    frames = np.stack([np.clip(rng.randint(0, 256, (h, w, 3)) * 0.3 + 90 + 20 * i, 0, 255).astype(np.uint8) for i in range(L)])
    masks = np.zeros((L, h, w), np.uint8)
    for i in range(L):
        masks[i, 20 + i:45 + i, 30:60] = 1
    model = lambda x, n: (torch.tanh(x.cpu().reshape(-1, 3, h, w) * 0.6 + 0.1 * x.cpu().mean()).to(dev), None)
    case = C.case("eval_70x90")
    flows = (torch.from_numpy(case["fwd"].copy()).to(dev), torch.from_numpy(case["bwd"].copy()).to(dev))
    psnr, ssim, warp = metrics.evaluate_video(model, frames, masks, warp=True, flows=flows, scenes=[c])
    comp = video.inpaint_video(model, frames, masks, 5, 10, -1, dilate=False, pad=False, keep_float=True, scenes=[c], device=dev)
    want = metrics.warp_error(comp, *flows).cpu().numpy()
    assert warp.shape == (L - 1, 2) and want[c - 1, 1] > 0 and warp[c - 1].tolist() == [0.0, 0.0]
    keep = np.arange(L - 1) != c - 1
    assert np.array_equal(warp[keep], want[keep])
    assert metrics.warp_score(warp) == float(want[keep][want[keep][:, 1] > 0, 0].mean())
    one = metrics.evaluate_video(model, frames, masks, warp=True, flows=flows)
    assert not np.array_equal(one[0], psnr) and one[2][c - 1, 1] > 0
    two = metrics.evaluate_video(model, frames, masks, scenes=[c])
    assert len(two) == 2 and np.array_equal(two[0], psnr) and np.array_equal(two[1], ssim)
