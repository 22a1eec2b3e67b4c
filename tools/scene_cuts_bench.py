"""The scene-cut kernels (ops.scene_diff, csrc/video.hip) against the two yardsticks that are not the kernel itself, and what
inpaint_video(scenes="auto") costs end to end.

  (1) L frames at 432x240 and at 1920x1080, three contents -- random bytes (no two lanes meet on a counter), smooth waves (the lanes
      of a wave mostly do) and one constant value (all of them do): device time of
        kernel      ops.scene_diff: the memset of the tables, the histogram pass, the difference pass;
        copy        a device-to-device copy of the same L H W 3 bytes (torch's copy_) -- the floor of a pass that reads every byte
                    once, although a copy also writes them;
        torch       the same definition from torch's integer operators: the luma and the cell index per pixel, one bincount over
                    `step` frames at a time, the absolute differences;
      all warmed, alternating, REPS calls between two device events.  The three results must be equal integer for integer.
  (2) if tests/golden/tennis25.npz is there: the clip played forwards and backwards until it has L frames (no cut: the windows are
      the same with and without the detector), the e2fgvi model with synthetic weights: host wall time of
      inpaint_video(scenes=None) and of inpaint_video(scenes="auto"), alternating, and of detect_cuts on the uploaded frames alone
      (its launches and the read-back of L - 1 integers).
One JSON line per measurement.
    python tools/scene_cuts_bench.py [L=100] [rounds=5]"""
import importlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from e2fgvi_amd import ops, video
from e2fgvi_amd.synth import synth_state_dict

L = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")


def frames_of(kind, H, W, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "random":
        return torch.randint(0, 256, (L, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    if kind == "constant":
        return torch.full((L, H, W, 3), 117, dtype=torch.uint8, device=dev)
    ys = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    xs = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    grey = torch.zeros((L, H, W), device=dev)
    for _ in range(3):
        a, lam, ph = (torch.rand(L, 1, 1, generator=g).to(dev) * s for s in (6.2832, 300.0, 6.2832))
        grey += torch.sin((torch.cos(a) * xs + torch.sin(a) * ys) * 6.2832 / (lam + 100.0) + ph)
    grey = (127 + grey * 33).clamp(0, 255)
    return torch.stack([grey, 0.8 * grey + 20, 255 - grey], -1).round().to(torch.uint8).contiguous()


def torch_scene_diff(frames, step=10):
    """the definition composed from torch's integer operators, `step` frames per bincount: int64 [L-1]"""
    n, H, W, _ = frames.shape
    cell = ((4 * torch.arange(H, device=dev)) // H)[:, None] * 4 + ((4 * torch.arange(W, device=dev)) // W)[None, :]
    hist = []
    for s in range(0, n, step):
        f = frames[s:s + step].to(torch.int32)
        k = f.shape[0]
        b = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 10
        idx = (b + cell[None] * 64 + torch.arange(k, device=dev)[:, None, None] * 1024).reshape(-1)
        hist.append(torch.bincount(idx, minlength=k * 1024).view(k, 1024))
    hist = torch.cat(hist)
    return (hist[1:] - hist[:-1]).abs().sum(1)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1) / reps


def stats(v):
    v = np.array(v)
    return {"mean": round(float(v.mean()), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


for (W, H) in ((432, 240), (1920, 1080)):
    nbytes = L * H * W * 3
    reps = 20 if nbytes < (1 << 28) else 5
    for kind in ("random", "smooth", "constant"):
        frames = frames_of(kind, H, W)
        spare = torch.empty_like(frames)
        arms = {"kernel": (lambda: ops.scene_diff(frames), reps), "copy": (lambda: spare.copy_(frames), reps),
                "torch": (lambda: torch_scene_diff(frames), 1)}
        out = {k: fn() for k, (fn, _) in arms.items()}                # warm every arm
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(rounds):
            for k, (fn, r) in arms.items():
                out[k], t = timed(fn, r)
                ms[k].append(t)
        same = bool(torch.equal(out["kernel"], out["torch"]))
        kmean, cmean = float(np.mean(ms["kernel"])), float(np.mean(ms["copy"]))
        print(json.dumps({"size": "%dx%d" % (W, H), "frames": L, "content": kind, "MB": round(nbytes / 1e6, 1), "rounds": rounds,
                          "calls_per_timing": reps, "ms": {k: stats(v) for k, v in ms.items()},
                          "kernel_read_GBps": round(nbytes / (kmean * 1e-3) / 1e9, 1),
                          "copy_read_GBps": round(nbytes / (cmean * 1e-3) / 1e9, 1),
                          "kernel_over_copy": round(kmean / cmean, 2), "torch_over_kernel": round(float(np.mean(ms["torch"])) / kmean, 1),
                          "same_integers_as_torch": same, "max_score": round(float(out["kernel"].max()) / (2.0 * H * W), 4),
                          "same_integers_rerun": bool(torch.equal(out["kernel"], ops.scene_diff(frames)))}), flush=True)
        if not same:
            sys.exit("the kernel and the torch composition count different integers")
        del frames, spare, out, arms

GOLD = os.path.join(ROOT, "tests", "golden", "tennis25.npz")
if os.path.exists(GOLD):
    z = np.load(GOLD)
    order = list(range(25)) + list(range(24, -1, -1))
    ids = [order[i % 50] for i in range(L)]
    src, masks = np.ascontiguousarray(z["frames"][ids]), np.ascontiguousarray(z["masks_raw"][ids])
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
    net = net.to(dev).eval()
    arms = {"scenes=None": {}, 'scenes="auto"': {"scenes": "auto"}}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    out = {k: video.inpaint_video(net, src, masks, device=dev, **kw) for k, kw in arms.items()}       # warm
    ms = {k: [] for k in arms}
    for _ in range(max(2, rounds // 2)):
        for k, kw in arms.items():
            out[k], t = wall(lambda: video.inpaint_video(net, src, masks, device=dev, **kw))
            ms[k].append(t)
    src_d = torch.from_numpy(src).to(dev)
    video.detect_cuts(src_d)
    det = [wall(lambda: video.detect_cuts(src_d))[1] for _ in range(10)]
    a, b = float(np.mean(ms["scenes=None"])), float(np.mean(ms['scenes="auto"']))
    print(json.dumps({"clip": "tennis25 forwards and backwards, %d frames 432x240" % L, "model": "e2fgvi, synthetic weights, fp32",
                      "cuts_found": video.detect_cuts(src_d), "max_score": round(float(video.scene_scores(src_d).max()), 4),
                      "same_bytes": bool(np.array_equal(out["scenes=None"], out['scenes="auto"'])),
                      "wall_ms": {k: stats(v) for k, v in ms.items()}, "auto_minus_none_ms": round(b - a, 2),
                      "auto_over_none": round(b / a, 4), "detect_cuts_alone_wall_ms": stats(det)}), flush=True)
else:
    print(json.dumps({"clip": "tennis25", "skipped": "tests/golden/tennis25.npz not found"}), flush=True)
