"""The frame resize of test.py:97-104,127 and core/dataset.py:115 -- PIL's ``Image.resize(size)``, BICUBIC for RGB -- on the
device (video.resize_frames, csrc/video.hip resample_u8), and inpaint_video(size=...) built on it.  Pillow is the oracle;
``_resample_np`` below restates its two-pass integer resample around video.bicubic_tables (test infrastructure, not a CPU
path of the package)."""
import importlib
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd import video
from oracle import video_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tennis25.npz")


def _pass_np(a, n_out, axis):
    """one separable pass of Pillow's 8-bit resample along `axis` of uint8 [..., H, W, 3] (axis -3: rows, -2: columns)"""
    n_in = a.shape[axis]
    bounds, coeffs = video.bicubic_tables(n_in, n_out)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    acc = np.full((n_out,) + a.shape[1:], 1 << 21, np.int64)
    bshape = (n_out,) + (1,) * (a.ndim - 1)
    for j in range(coeffs.shape[1]):
        # coefficients past a row's tap count are zero; the clipped index only keeps the gather in range
        idx = np.minimum(bounds[:, 0] + j, n_in - 1)
        acc += a[idx] * coeffs[:, j].reshape(bshape)
    assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31          # Pillow's int32 accumulator never overflows here
    return np.moveaxis(np.clip(acc >> 22, 0, 255).astype(np.uint8), 0, axis)


def _resample_np(a, size):
    """uint8 [..., H, W, 3] -> [..., h, w, 3] for size = (w, h): horizontal pass first (its uint8 result clamped), then vertical,
    each only if that dimension changes"""
    w, h = size
    if a.shape[-2] != w:
        a = _pass_np(a, w, -2)
    if a.shape[-3] != h:
        a = _pass_np(a, h, -3)
    return a.copy()


def _pil(frame, size):
    from PIL import Image
    return np.asarray(Image.fromarray(frame).resize(size))


# (W, H) -> (w, h), PIL order: test.py's and evaluate.py's sizes, the inverse upscale, one-axis changes, extreme aspect ratios,
# one-pixel edges, then random pairs from a fixed seed
_FIXED = [((854, 480), (432, 240)), ((1920, 1080), (1296, 720)), ((432, 240), (864, 480)), ((432, 240), (432, 240)),
          ((640, 240), (432, 240)), ((432, 360), (432, 240)), ((7, 300), (300, 7)), ((1, 1), (5, 3)), ((1, 37), (9, 12)),
          ((37, 1), (12, 9)), ((64, 48), (1, 48)), ((64, 48), (64, 1)), ((5, 3), (1, 1)), ((1280, 720), (432, 240)),
          ((432, 240), (1296, 720))]
_rng = np.random.RandomState(11)
SIZES = _FIXED + [(tuple(int(v) for v in _rng.randint(1, 400, 2)), tuple(int(v) for v in _rng.randint(1, 400, 2)))
                  for _ in range(10)]


def _frames(L, W, H, seed):
    """smooth gradients (no clamping) plus noise patches (large negative taps: the uint8 clamps of both passes)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.empty((L, H, W, 3), np.uint8)
    for i in range(L):
        for c in range(3):
            f[i, :, :, c] = (xx * (3 + c) + yy * (5 - c) + 40 * i) % 256
        f[i, : H // 2, W // 3:] = rng.randint(0, 256, f[i, : H // 2, W // 3:].shape)
    return f


def test_bicubic_tables_restate_pillow():
    """bicubic_tables + the two-pass integer resample == PIL.Image.resize(size) (BICUBIC), bit-exact"""
    for (W, H), size in SIZES:
        f = _frames(1, W, H, seed=W * 7 + H)[0]
        got = _resample_np(f, size)
        ref = _pil(f, size)
        assert got.shape == ref.shape == (size[1], size[0], 3), ((W, H), size)
        assert np.array_equal(got, ref), ((W, H), size, int((got != ref).sum()))


def test_bicubic_tables_shapes():
    bounds, coeffs = video.bicubic_tables(854, 432)
    assert bounds.dtype == coeffs.dtype == np.int32 and bounds.shape == (432, 2)
    assert coeffs.shape == (432, 2 * int(np.ceil(2 * 854 / 432)) + 1)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 854).all() and (bounds[:, 1] <= coeffs.shape[1]).all()
    # the fixed-point weights of every output sum to 1.0 up to their rounding
    assert np.abs(coeffs.astype(np.int64).sum(1) - (1 << 22)).max() <= coeffs.shape[1]
    bounds, coeffs = video.bicubic_tables(240, 480)                     # upscale: support 2, five taps
    assert coeffs.shape == (480, 5) and (bounds[:, 1] <= 4).all()


# ------------------------------------------------------------------------------------------------------------------ device
@pytest.mark.gpu
def test_resize_frames_kernel_is_pillow(dev):
    """video.resize_frames (two resample_u8 passes) == PIL bicubic, bit-exact, on every size pair; no pass when nothing changes"""
    for (W, H), size in SIZES:
        f = _frames(3, W, H, seed=W + 13 * H)
        got = video.resize_frames(f, size, dev)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, size[1], size[0], 3)
        got = got.cpu().numpy()
        for i in range(3):
            assert np.array_equal(got[i], _pil(f[i], size)), ((W, H), size, i)
        if size == (W, H):
            assert np.array_equal(got, f)


@pytest.mark.gpu
def test_resample_u8_checks_its_arguments(dev):
    from e2fgvi_amd import ops
    f = torch.zeros((2, 30, 10, 3), dtype=torch.uint8, device=dev)
    b, c = (torch.from_numpy(t).to(dev) for t in video.bicubic_tables(10, 5))
    assert tuple(ops.resample_u8(f, 5, 2, b, c).shape) == (2, 30, 5, 3)
    with pytest.raises(ValueError):
        ops.resample_u8(f, 5, 1, b, c)                                  # the taps of 10 -> 5, not of 30 rows -> 5
    with pytest.raises(ValueError):
        ops.resample_u8(f, 4, 2, b, c)                                  # table rows != n_out
    with pytest.raises(ValueError):
        ops.resample_u8(f, 5, 3, b, c)                                  # axis must be 1 (H) or 2 (W)
    with pytest.raises(TypeError):
        ops.resample_u8(f.float(), 5, 2, b, c)
    with pytest.raises(TypeError):
        ops.resample_u8(f, 5, 2, b.cpu(), c)


@pytest.mark.gpu
def test_resize_frames_beyond_2gib(dev):
    """a source of more than 2**32 bytes (700 frames of 1920x1080): 64-bit indexing; the first frame, the frames that hold byte
    offsets 2**31 and 2**32 of the source, their neighbours and the last frame == PIL"""
    L, H, W, size = 700, 1080, 1920, (1296, 720)
    g = torch.Generator(device=dev).manual_seed(5)
    src = torch.randint(0, 256, (L, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    frame = H * W * 3
    at31, at32 = 2 ** 31 // frame, 2 ** 32 // frame
    assert src.numel() > 2 ** 32 + 2 * frame and 2 ** 32 % frame != 0 and at32 < L - 2
    src[:, : H // 2, : W // 2] = 128                                  # a flat quadrant next to the noise
    out = video.resize_frames(src, size)
    assert tuple(out.shape) == (L, 720, 1296, 3)
    for i in (0, at31, at31 + 1, L // 2, at32 - 1, at32, at32 + 1, L - 1):
        assert np.array_equal(out[i].cpu().numpy(), _pil(src[i].cpu().numpy(), size)), i
    # the frame a 32-bit offset would read in the place of the one at 2**32 is another picture
    assert not torch.equal(src[at32 + 1], src[0]) and not torch.equal(out[at32 + 1], out[0])
    del src, out
    torch.cuda.empty_cache()


def _toy_video(L, h, w, seed):
    rng = np.random.RandomState(seed)
    frames = _frames(L, w, h, seed)
    masks = np.zeros((L, h, w), np.uint8)
    for i in range(L):
        masks[i, h // 4 + i % 3:h // 2 + i % 3, w // 4 + i:w // 2 + i] = rng.randint(1, 256)
    return frames, masks


def _stand_in_model(x, n_local):
    # deterministic, batch-free stand-in with the InpaintGenerator output convention, evaluated on the CPU in both loops so that
    # the comparison isolates the byte kernels
    b, t, c, H, W = x.shape
    y = torch.tanh(x.reshape(b * t, c, H, W) * 0.7 + 0.1 * x.mean(dim=(1, 2, 3, 4)).view(1, 1, 1, 1))
    return y, None


@pytest.mark.gpu
@pytest.mark.parametrize("hw_in,size", [((100, 141), (70, 50)), ((33, 47), (108, 60)), ((50, 70), (70, 50))])
def test_inpaint_video_with_size_matches_reference_loop(dev, hw_in, size):
    """inpaint_video(size=S) == the reference loop fed PIL-bicubic frames of size S and PIL-NEAREST + dilated masks (test.py:56-69,
    97-104,127), bit-exact: downscale, upscale, S equal to the frame size"""
    from PIL import Image
    L = 12
    frames, masks = _toy_video(L, hw_in[0], hw_in[1], seed=4)
    rs = [_pil(f, size) for f in frames]
    dil = [video_ref.dilate_cross_np(np.asarray(Image.fromarray(m).resize(size, Image.NEAREST)) > 0, 4) for m in masks]
    ref = video_ref.run(lambda x, n: _stand_in_model(x, n)[0], rs, dil, 5, 10, -1)
    out = video.inpaint_video(lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None), frames, masks, device=dev, size=size)
    assert out.shape == ref.shape == (L, size[1], size[0], 3) and out.dtype == np.uint8
    assert np.array_equal(out, ref), int((out != ref).sum())


@pytest.mark.gpu
def test_e2fgvi_on_a_larger_video_with_size(dev):
    """the fixed-size e2fgvi model on 864x480 frames (the tennis clip, PIL-upscaled): size=(432, 240) returns the bytes of
    inpaint_video on the PIL-downscaled frames, with one window at a time, batch_windows=2 and in_flight=2; without size the
    864x480 frames are refused as before"""
    from e2fgvi_amd.synth import synth_state_dict
    z = np.load(GOLD)
    small = z["frames"]
    masks = z["masks_raw"]
    big = np.stack([_pil(f, (864, 480)) for f in small])
    down = np.stack([_pil(f, (432, 240)) for f in big])
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
    net = net.to(dev).eval()
    for kw in ({}, {"batch_windows": 2}, {"in_flight": 2}):
        ref = video.inpaint_video(net, down, masks, **kw)
        out = video.inpaint_video(net, big, masks, size=(432, 240), **kw)
        assert out.shape == (len(small), 240, 432, 3)
        assert np.array_equal(out, ref), (kw, int((out != ref).sum()))
    with pytest.raises(ValueError):
        video.inpaint_video(net, big, masks)


@pytest.mark.gpu
def test_evaluate_recipe_on_raw_frames(dev):
    """README's evaluate.py recipe: resize_frames gives the ground truth; inpaint_video(size, pad=False, keep_float=True) leaves it
    untouched outside the NEAREST-resized, dilated holes (core/dataset.py:115-127); calc_psnr_and_ssim takes the pair"""
    from e2fgvi_amd import metrics
    frames, masks = _toy_video(7, 96, 130, seed=6)
    size = (140, 80)                                                    # SSIM's 65-pixel window needs 65 rows
    gt = video.resize_frames(frames, size)
    comp = video.inpaint_video(lambda x, n: (_stand_in_model(x.cpu(), n)[0].to(dev), None), frames, masks, device=dev, size=size,
                               pad=False, keep_float=True)
    assert comp.dtype == torch.float32 and comp.shape == gt.shape
    holes = video.prepare_masks(masks, (80, 140), dev).bool()
    assert torch.equal(comp[~holes], gt.float()[~holes]) and bool((comp[holes] != gt.float()[holes]).any())
    psnr, ssim = metrics.calc_psnr_and_ssim(gt[0], comp[0])
    assert 0 < psnr < float("inf") and 0 < ssim < 1
