"""evaluate.py's image metrics on the device (reference: core/metrics.py:13-56).

``calc_psnr_and_ssim(img1, img2)`` keeps the reference's name and meaning -- PSNR and
``skimage.measure.compare_ssim(data_range=255, multichannel=True, win_size=65)`` of two [H,W,3] frames in [0,255] -- but
takes device tensors (or anything ``torch.as_tensor`` accepts, uploaded first) and also whole batches [N,H,W,3]; the
arithmetic runs in fp64 HIP kernels (csrc/metrics.hip).  VFID (I3D network + checkpoint) is out of scope.

``warp_error`` adds the table's fourth column, the flow-warping temporal error E_warp (evaluate.py:142-151 only saves the frames
"for evaluating warping errors"): a fused gather / test / reduce kernel in the same fp64 style, fed with flows at the frames' own
size from the model's SPyNet (``video_flows``) or from the caller; ``evaluate_video(warp=True)`` returns it beside PSNR / SSIM.
"""
import ctypes as C

import numpy as np
import torch

from . import lib as _L
from .ops import _chk, _ptr, _stream


def psnr_ssim(img1, img2, win_size=65):
    """fp32 device tensors [N,H,W,3] (or [H,W,3]) in [0,255] -> float64 tensor [N,2] of (psnr, ssim) on the device."""
    lib = _L.load()
    a = _chk(img1 if img1.dim() == 4 else img1[None], "img1")
    b = _chk(img2 if img2.dim() == 4 else img2[None], "img2")
    if a.shape != b.shape or a.shape[-1] != 3:
        raise ValueError("image shapes differ or are not [N,H,W,3]: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    N, H, W, _ = a.shape
    nbytes = lib.e2fgvi_psnr_ssim_workspace(N, H, W)
    if nbytes < 0:
        _L.check(int(nbytes), "psnr_ssim_workspace")
    work = torch.empty(int(nbytes) // 8, dtype=torch.float64, device=a.device)
    out = torch.empty((N, 2), dtype=torch.float64, device=a.device)
    _L.check(lib.e2fgvi_psnr_ssim(_ptr(a), _ptr(b), N, H, W, win_size, _ptr(work), _ptr(out), _stream()), "psnr_ssim")
    return out


def calc_psnr_and_ssim(img1, img2, device="cuda"):
    """core/metrics.py:39-56: img1, img2 ndarray / tensor [H,W,3] in [0,255] -> (psnr, ssim) python floats."""
    a = torch.as_tensor(np.asarray(img1, dtype=np.float32) if not isinstance(img1, torch.Tensor) else img1).float().to(device)
    b = torch.as_tensor(np.asarray(img2, dtype=np.float32) if not isinstance(img2, torch.Tensor) else img2).float().to(device)
    r = psnr_ssim(a.contiguous(), b.contiguous()).cpu()
    return float(r[0, 0]), float(r[0, 1])


def calculate_epe(flow1, flow2):
    """core/metrics.py:13-18 (end point error of two flow fields [N,2,H,W]); a reduction torch already does on device."""
    return torch.sum((flow1 - flow2) ** 2, dim=1).sqrt().view(-1).mean().item()


def _device_tensor(x, device):
    """a device tensor as it is, anything else through torch.as_tensor and uploaded (no cast, no copy into another layout: the
    checks of the caller see the dtype and the strides that were passed)"""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x
    return torch.as_tensor(x).to(device)


def warp_error(frames, flow_fwd, flow_bwd, valid=None):
    """E_warp, the flow-warping temporal error of the paper's result table, after Lai et al. (ECCV 2018) with the occlusion test
    of Ruder et al. (2016), in fp64 on the device (csrc/metrics.hip).

    frames [L,H,W,3], L >= 2, uint8 or finite fp32 in [0,255]; flow_fwd [L-1,H,W,2] fp32: flow_fwd[t] is the flow from frame t to
    t+1 on frame t's grid, in pixels, channel 0 = x (the NHWC layout Engine.pair_flows returns); flow_bwd [L-1,H,W,2]: flow_bwd[t]
    is the flow from frame t+1 to t on frame t+1's grid; valid (optional) [L,H,W] uint8.  Device tensors, or anything
    torch.as_tensor accepts (uploaded first); wrong dtypes, shapes that do not fit, non-contiguous inputs and L < 2 raise
    ValueError.

    For pair t write A = frames[t], B = frames[t+1], f = flow_fwd[t], g = flow_bwd[t]; all arithmetic is fp64 on the fp32 / uint8
    inputs.  For pixel p = (x, y):
      sample position  q = (x + f_x(p), y + f_y(p)); inside = 0 <= q_x <= W-1 and 0 <= q_y <= H-1 (decided in floating point
                       before any conversion to an integer: a flow of 1e30 is simply outside);
      sampler          bil(T, q) = the 4-corner bilinear sample, corners outside the image contribute 0: flow_warp(padding_mode=
                       'zeros') of flow_comp.py:345-383, i.e. grid_sample(align_corners=True);
      warped           g_w = bil(g, q), B_w = bil(B, q);
      occlusion        |f + g_w|^2 > 0.01 (|f|^2 + |g_w|^2) + 0.5;
      motion boundary  |dx f|^2 + |dy f|^2 > 0.01 |f|^2 + 0.002 with forward differences dx f = f(x+1,y) - f(x,y),
                       dy f = f(x,y+1) - f(x,y), a difference being 0 on the last column / row;
      kept             M(p) = inside, not occluded, not on a motion boundary and (with valid) valid[t](p) != 0;
      non-finite       a pixel is excluded when f(p), f at the right / lower neighbour used above or g_w is not finite --
                       by select, never by a multiplication with 0;
      per pair         n_t = sum M, e_t = sum_p M(p) sum_c ((A_c - B_w,c) / 255)^2 / n_t, e_t = 0 when n_t = 0.

    Returns the float64 device tensor [L-1, 2] of rows (e_t, n_t); the video's score is the mean of e_t over the pairs with
    n_t > 0 (warp_score).  The same inputs give the same bits in every run.

    The paper's absolute values were computed with FlowNet2 flows.  Numbers from SPyNet flows (video_flows) are comparable with
    each other -- one method or setting against another under the same flows -- not with that table."""
    lib = _L.load()
    device = next((t.device for t in (frames, flow_fwd, flow_bwd, valid) if isinstance(t, torch.Tensor) and t.is_cuda), "cuda")
    fr, fw, bw = (_device_tensor(t, device) for t in (frames, flow_fwd, flow_bwd))
    va = None if valid is None else _device_tensor(valid, device)
    if fr.dtype not in (torch.uint8, torch.float32):
        raise ValueError("frames must be uint8 or float32, got %s" % fr.dtype)
    for t, nm in ((fw, "flow_fwd"), (bw, "flow_bwd")):
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (nm, t.dtype))
    if va is not None and va.dtype != torch.uint8:
        raise ValueError("valid must be uint8, got %s" % va.dtype)
    if fr.dim() != 4 or fr.shape[3] != 3:
        raise ValueError("frames must be [L,H,W,3], got %s" % (tuple(fr.shape),))
    L, H, W, _ = fr.shape
    if L < 2:
        raise ValueError("warp_error needs at least two frames, got %d" % L)
    for t, nm in ((fw, "flow_fwd"), (bw, "flow_bwd")):
        if tuple(t.shape) != (L - 1, H, W, 2):
            raise ValueError("%s must be [%d,%d,%d,2] for frames %s, got %s" % (nm, L - 1, H, W, tuple(fr.shape), tuple(t.shape)))
    if va is not None and tuple(va.shape) != (L, H, W):
        raise ValueError("valid must be [%d,%d,%d], got %s" % (L, H, W, tuple(va.shape)))
    for t, nm in ((fr, "frames"), (fw, "flow_fwd"), (bw, "flow_bwd"), (va, "valid")):
        if t is not None and not t.is_contiguous():
            raise ValueError("%s must be contiguous" % nm)
        if t is not None and t.device != fr.device:
            raise ValueError("%s is on %s, the frames on %s" % (nm, t.device, fr.device))
    nbytes = lib.e2fgvi_warp_error_workspace(L, H, W)
    if nbytes < 0:
        _L.check(int(nbytes), "warp_error_workspace")
    with torch.cuda.device(fr.device):
        work = torch.empty(int(nbytes) // 8, dtype=torch.float64, device=fr.device)
        out = torch.empty((L - 1, 2), dtype=torch.float64, device=fr.device)
        _L.check(lib.e2fgvi_warp_error(_ptr(fr), _L.DT_U8 if fr.dtype == torch.uint8 else _L.DT_F32, _ptr(fw), _ptr(bw), _ptr(va),
                                       L, H, W, _ptr(work), _ptr(out), _stream()), "warp_error")
    return out


def warp_score(rows):
    """the video's E_warp from warp_error's [L-1, 2] rows (tensor or array): the mean of e_t over the pairs with n_t > 0 (nan
    when no pair keeps a pixel)"""
    r = rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    keep = r[:, 1] > 0
    return float(r[keep, 0].mean()) if keep.any() else float("nan")


def video_flows(model, frames_u8, chunk=4):
    """Forward and backward flows of a video's adjacent frames at the frames' own size, from the model's own SPyNet
    (Engine.pair_flows(downscale=1)): frames_u8 [L,H,W,3] uint8, L >= 2 -> (fwd, bwd) fp32 device tensors [L-1,H,W,2] in
    warp_error's convention.  The video goes through in steps of `chunk` pairs: a step's frames are converted together and only
    its activations exist at a time, so the memory stays bounded whatever L is (a 1080p pair holds about 1 GB in the network's
    finest level in fp32).  Within a step the network runs one pair per call: the conv layers choose their kernels by the rows of a
    launch, and kernels round differently, so flows from calls of `chunk` pairs would change in their last bits with `chunk`
    (as inpaint_video(reuse=True) differs from reuse=False) -- a score must not depend on a memory knob.  One pair at full size
    is as many rows as sixteen at the forward's 1/4 size, and four 1080p pairs in one call would pass the 4 GiB a conv source may
    span.  Every pair table and frame list is uploaded before the first launch.
    `model` is the generator -- an object with ``engine()``; anything else raises TypeError.  The flows follow the engine's
    precision: score with an fp32 net (``model.precision = "fp32"``), the 16-bit paths round the flow network's activations.
    The paper's E_warp column used FlowNet2 flows: see warp_error."""
    from . import ops
    if not callable(getattr(model, "engine", None)):
        raise TypeError("video_flows needs the InpaintGenerator (its engine owns the SPyNet), got %s" % type(model).__name__)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1, got %d" % chunk)
    eng = model.engine()
    if isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda:
        frames_d = frames_u8.to(eng.device).contiguous()
    else:
        frames_d = torch.as_tensor(np.ascontiguousarray(frames_u8)).to(eng.device)
    if frames_d.dtype != torch.uint8 or frames_d.dim() != 4 or frames_d.shape[3] != 3 or frames_d.shape[0] < 2:
        raise ValueError("frames must be uint8 [L,H,W,3] with L >= 2, got %s %s" % (frames_d.dtype, tuple(frames_d.shape)))
    L, H, W, _ = frames_d.shape
    with torch.cuda.device(eng.device):
        # every upload in front of the first launch: the frames of each step and the table of one pair
        starts = list(range(0, L - 1, chunk))
        ids = [torch.arange(s, min(s + chunk, L - 1) + 1, dtype=torch.int32).to(eng.device) for s in starts]
        pair = eng.pair_table([(0, 1)])
        nomask = torch.zeros((L, H, W), dtype=torch.uint8, device=eng.device)
        fwd = torch.empty((L - 1, H, W, 2), dtype=torch.float32, device=eng.device)
        bwd = torch.empty_like(fwd)
        for s, i in zip(starts, ids):
            x = ops.masked_clip(frames_d, nomask, i, H, W)[0]           # [k + 1, 3, H, W] = frames / 255 * 2 - 1
            for j in range(i.numel() - 1):
                f, b = eng.pair_flows(x[j:j + 2], pair, downscale=1)
                fwd[s + j].copy_(f[0])
                bwd[s + j].copy_(b[0])
    return fwd, bwd


def evaluate_video(model, frames_u8, masks_u8, neighbor_stride=5, ref_length=10, win_size=65, warp=False, flows=None, valid=None,
                   scenes=None):
    """evaluate.py:75-125 for one video on the device: the sliding-window completion (no mask dilation, no padding --
    the dataset delivers frames at the model's size with binary masks) followed by per-frame PSNR / SSIM of the blended
    frames against the originals.  Returns (psnr[L], ssim[L]) float64 numpy arrays; their means are the video's scores.
    warp=True returns (psnr, ssim, warp): warp the [L-1, 2] float64 array of warp_error's rows (e_t, n_t) for the blended float
    frames (warp_score gives the video's E_warp; read warp_error on comparing it with the paper's column).  The flows are
    flows=(fwd, bwd) when given -- any callable model works then -- and otherwise video_flows(model, frames_u8): those of the
    ground-truth frames, as Lai et al. take them from the unprocessed video.  valid [L,H,W] uint8 is warp_error's.
    ``scenes`` is inpaint_video's (None, a list of cuts, or "auto"): the completion is windowed per scene, and with warp=True the
    row of every pair that straddles a cut -- (c - 1, c) for a cut c -- is set to (0, 0), so warp_score skips it: a flow between two
    shots means nothing.  warp_error itself is unchanged."""
    from . import video
    if warp and flows is None and not callable(getattr(model, "engine", None)):
        raise TypeError("warp=True without flows= takes them from the model's SPyNet (video_flows): that needs the InpaintGenerator, "
                        "got %s" % type(model).__name__)
    if isinstance(scenes, str) and scenes == "auto":
        scenes = video.detect_cuts(frames_u8)           # here, so that the rows dropped below are those of the cuts used
    comp = video.inpaint_video(model, frames_u8, masks_u8, neighbor_stride, ref_length, -1, dilate=False, pad=False,
                               keep_float=True, scenes=scenes)
    ori = torch.as_tensor(np.ascontiguousarray(frames_u8)).to(comp.device).float()
    r = psnr_ssim(ori, comp, win_size).cpu().numpy()
    if not warp:
        return r[:, 0], r[:, 1]
    fwd, bwd = flows if flows is not None else video_flows(model, frames_u8)
    rows = warp_error(comp, fwd, bwd, valid).cpu().numpy()
    for c in scenes or ():
        rows[int(c) - 1] = 0.0
    return r[:, 0], r[:, 1], rows
