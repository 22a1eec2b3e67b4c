"""E_warp (metrics.warp_error, csrc/metrics.hip) against a torch fp64 composition of the same definition on the device, and the
E_warp of the tennis clip under the drivers that change how a frame meets its neighbours in time.

  (1) PAIRS pairs at 432x240 and at 1080x1920 with given flows (smooth synthetic ones built on the device: a drift plus long waves,
      bwd = -fwd + waves of up to 0.9 px, so that every exclusion class occurs): device time of warp_error (fp32 and uint8 frames) and of
      the torch composition -- grid_sample(align_corners=True, zeros) of the next frame and of the backward flow in fp64, the two
      masks, the masked sums -- both warmed, alternating, device events around each call.  The kept counts n must be equal pair
      for pair (the composition's e agrees to rounding: it is printed, not asserted).  The bytes a pair must move at least
      (frames of both ends, both flows) over the kernel's time are given as GB/s; the gathers make the real traffic larger.
  (2) if tests/golden/tennis25.npz is there: flows of the clip's source frames (metrics.video_flows, fp32 net), then E_warp under
      those flows of the source frames themselves and of inpaint_video(size=(432, 240), restore=True) with region=None,
      region="track", and region="track" with feather=8.  Synthetic weights: the inpainted content is not meaningful, the rows say
      what the metric sees of each driver's seams, not how good an inpainting is.  SPyNet flows, not FlowNet2: not comparable with
      the paper's column.
One JSON line per measurement.
    python tools/warp_error_bench.py [PAIRS=50] [rounds=5]"""
import importlib
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F
from e2fgvi_amd import metrics, video
from e2fgvi_amd.synth import synth_state_dict

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")


def inputs(H, W, L, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    ys = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    xs = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]

    def waves(n, amp, lam0, lam1):
        out = torch.zeros((n, H, W), device=dev)
        for _ in range(3):
            a, lam, ph = r(n, 1, 1) * 6.2832, lam0 + r(n, 1, 1) * (lam1 - lam0), r(n, 1, 1) * 6.2832
            out += torch.sin((torch.cos(a) * xs + torch.sin(a) * ys) * 6.2832 / lam + ph)
        return out * (amp / 3)
    grey = (127 + waves(L, 100, 8, 60)).clamp(0, 255)
    frames = torch.stack([grey, 0.8 * grey + 20, 255 - grey], -1).round().contiguous()
    fwd = torch.stack([(r(L - 1, 1, 1) - 0.5) * 6 + waves(L - 1, 1.5, 40, 400), (r(L - 1, 1, 1) - 0.5) * 6 + waves(L - 1, 1.5, 40, 400)], -1)
    bwd = -fwd + torch.stack([waves(L - 1, 0.9, 30, 90), waves(L - 1, 0.9, 30, 90)], -1)
    return frames, fwd.contiguous(), bwd.contiguous()


def torch_warp_error(frames, fwd, bwd, step=10):
    """the definition composed from torch operators in fp64, `step` pairs at a time: [L-1, 2] rows (e, n)"""
    L, H, W, _ = frames.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    rows = []
    for s in range(0, L - 1, step):
        A = frames[s:s + step][:L - 1 - s].double()
        B = frames[s + 1:s + 1 + step].double().permute(0, 3, 1, 2)
        f, g = fwd[s:s + step].double(), bwd[s:s + step].double().permute(0, 3, 1, 2)
        qx, qy = xs + f[..., 0], ys + f[..., 1]
        inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
        grid = torch.stack([2 * qx / max(W - 1, 1) - 1, 2 * qy / max(H - 1, 1) - 1], -1)
        Bw = F.grid_sample(B, grid, mode="bilinear", padding_mode="zeros", align_corners=True).permute(0, 2, 3, 1)
        gw = F.grid_sample(g, grid, mode="bilinear", padding_mode="zeros", align_corners=True).permute(0, 2, 3, 1)
        dx, dy = torch.zeros_like(f), torch.zeros_like(f)
        dx[:, :, :-1] = f[:, :, 1:] - f[:, :, :-1]
        dy[:, :-1] = f[:, 1:] - f[:, :-1]
        ff = (f ** 2).sum(-1)
        occ = ((f + gw) ** 2).sum(-1) > 0.01 * (ff + (gw ** 2).sum(-1)) + 0.5
        mb = (dx ** 2).sum(-1) + (dy ** 2).sum(-1) > 0.01 * ff + 0.002
        keep = inside & ~occ & ~mb
        per = (((A - Bw) / 255.0) ** 2).sum(-1)
        n = keep.sum((1, 2)).double()
        e = torch.where(keep, per, torch.zeros_like(per)).sum((1, 2)) / n.clamp(min=1)
        rows.append(torch.stack([e, n], 1))
    return torch.cat(rows)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def stats(v):
    v = np.array(v)
    return {"mean": round(float(v.mean()), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


for (W, H) in ((432, 240), (1920, 1080)):
    frames, fwd, bwd = inputs(H, W, PAIRS + 1, 1)
    frames8 = frames.to(torch.uint8)
    arms = {"kernel_f32": lambda: metrics.warp_error(frames, fwd, bwd), "kernel_u8": lambda: metrics.warp_error(frames8, fwd, bwd),
            "torch_fp64": lambda: torch_warp_error(frames, fwd, bwd)}
    out = {k: fn() for k, fn in arms.items()}                     # warm every arm
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            out[k], t = timed(fn)
            ms[k].append(t)
    k32, k8, ref = (out[k].cpu().numpy() for k in ("kernel_f32", "kernel_u8", "torch_fp64"))
    same_n = bool(np.array_equal(k32[:, 1], ref[:, 1]) and np.array_equal(k8[:, 1], ref[:, 1]))
    rel = float(np.abs(k32[:, 0] - ref[:, 0]).max() / ref[:, 0].max())
    floor_bytes = PAIRS * H * W * (2 * 3 * 4 + 2 * 2 * 4)
    print(json.dumps({"size": "%dx%d" % (W, H), "pairs": PAIRS, "rounds": rounds, "ms": {k: stats(v) for k, v in ms.items()},
                      "torch_over_kernel_f32": round(float(np.mean(ms["torch_fp64"]) / np.mean(ms["kernel_f32"])), 1),
                      "kernel_f32_floor_GBps": round(floor_bytes / (np.mean(ms["kernel_f32"]) * 1e-3) / 1e9, 1),
                      "kept_share": round(float(ref[:, 1].mean() / (H * W)), 3), "same_n": same_n, "max_rel_diff_e": rel,
                      "same_bits_f32_rerun": bool(torch.equal(out["kernel_f32"].view(torch.int64), arms["kernel_f32"]().view(torch.int64)))}),
          flush=True)
    if not same_n:
        sys.exit("the kernel and the torch composition keep different pixels")
    del frames, frames8, fwd, bwd, out, arms

GOLD = os.path.join(ROOT, "tests", "golden", "tennis25.npz")
if os.path.exists(GOLD):
    z = np.load(GOLD)
    src, masks = z["frames"], z["masks_raw"]
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
    net = net.to(dev).eval()
    with torch.no_grad():
        fwd, bwd = metrics.video_flows(net, src)
        size = (src.shape[2], src.shape[1])
        clips = {"source": src}
        for name, kw in (("region=None", {}), ('region="track"', {"region": "track"}), ('region="track" feather=8', {"region": "track", "feather": 8})):
            clips[name] = video.inpaint_video(net, src, masks, device=dev, size=size, restore=True, **kw)
    for name, clip in clips.items():
        r = metrics.warp_error(np.ascontiguousarray(clip), fwd, bwd).cpu().numpy()
        print(json.dumps({"clip": "tennis25 %dx%d" % size, "frames": name, "weights": "synthetic (stress): content not meaningful",
                          "flows": "SPyNet of the source frames, fp32", "E_warp": float("%.6g" % metrics.warp_score(r)),
                          "kept_share": round(float(r[:, 1].mean() / (size[0] * size[1])), 3),
                          "e_min": float("%.4g" % r[:, 0].min()), "e_max": float("%.4g" % r[:, 0].max())}), flush=True)
else:
    print(json.dumps({"clip": "tennis25", "skipped": "tests/golden/tennis25.npz not found"}), flush=True)
