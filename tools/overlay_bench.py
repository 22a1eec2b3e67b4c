"""The overlay sums (ops.overlay_stats, csrc/video.hip overlay_stats_kernel) against ops.scene_diff, the other one-pass reader of the
same frame bytes, on the same tensors in one process.

L frames at 432x240 and at 1920x1080, three contents -- random bytes, smooth moving waves, and the waves with a static bright block in a
corner (the only one with an overlay to find: without a persistent edge overlay_mask returns before its labellings): device time of
    overlay_stats   the memset of the three planes when the frames are split into chunks, and the one launch
    scene_diff      ops.scene_diff: the memset of the tables, the histogram pass, the difference pass
    edges           ops.overlay_edges on the sums (threshold, dilation by radius 3, count): an H W pass, not an L H W one
    mask            video.overlay_mask on the uploaded frames, host clock: the two launches, the read of the count, two labellings
all warmed, alternating, `calls_per_timing` calls between two device events (1000 at 432x240 and 100 at 1920x1080, 500 for edges there:
every timing window is 8 ms or longer).  The sums must equal the composition of the definition
from torch's integer operators.  One JSON line per measurement.
    python tools/overlay_bench.py [L=100] [rounds=5]"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from e2fgvi_amd import ops, video

L = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")


def frames_of(kind, H, W, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "random":
        return torch.randint(0, 256, (L, H, W, 3), dtype=torch.uint8, device=dev)
    ys = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    xs = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    grey = torch.zeros((L, H, W), device=dev)
    for _ in range(3):
        a, lam, ph = (torch.rand(L, 1, 1, generator=g).to(dev) * s for s in (6.2832, 300.0, 6.2832))
        grey += torch.sin((torch.cos(a) * xs + torch.sin(a) * ys) * 6.2832 / (lam + 100.0) + ph)
    grey = (127 + grey * 33).clamp(0, 255)
    out = torch.stack([grey, 0.8 * grey + 20, 255 - grey], -1).round().to(torch.uint8).contiguous()
    if kind == "logo":                                             # a static bright block in a corner of the moving waves
        out[:, H // 8:H // 4, W // 8:W // 4] = 250
    return out


def torch_stats(frames, step=10):
    """the definition composed from torch's integer operators, `step` frames at a time: int32 [3,H,W]"""
    n, H, W, _ = frames.shape
    out = torch.zeros((3, H, W), dtype=torch.int64, device=dev)
    for s in range(0, n, step):
        f = frames[s:s + step].to(torch.int32)
        y = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8
        px = torch.cat([y[:, :, :1], y, y[:, :, -1:]], 2)
        py = torch.cat([y[:, :1], y, y[:, -1:]], 1)
        gx, gy = px[:, :, 2:] - px[:, :, :-2], py[:, 2:] - py[:, :-2]
        out[0] += gx.sum(0)
        out[1] += gy.sum(0)
        out[2] += (gx.abs() + gy.abs()).sum(0)
    return out.to(torch.int32)


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
    reps = 1000 if nbytes < (1 << 28) else 100                     # a timing window of 12 ms (scene_diff at 1080p) to 30 ms
    for kind in ("random", "smooth", "logo"):
        frames = frames_of(kind, H, W)
        sums = ops.overlay_stats(frames)
        same = bool(torch.equal(sums, torch_stats(frames)))
        arms = {"overlay_stats": lambda: ops.overlay_stats(frames), "scene_diff": lambda: ops.scene_diff(frames),
                "edges": lambda: ops.overlay_edges(sums, L, 32, 224, 3)}
        for fn in arms.values():                                   # warm every arm
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                ms[k].append(timed(fn, reps * 5 if k == "edges" and reps == 100 else reps)[1])    # 0.02 ms a call: 8 ms windows and more too
        wall = []
        for _ in range(rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            found = int((video.overlay_mask(frames, max_fraction=1.0) > 0).sum())
            wall.append((time.perf_counter() - t0) * 1e3)
        omean, smean = float(np.mean(ms["overlay_stats"])), float(np.mean(ms["scene_diff"]))
        print(json.dumps({"size": "%dx%d" % (W, H), "frames": L, "content": kind, "MB": round(nbytes / 1e6, 1), "rounds": rounds,
                          "calls_per_timing": reps, "ms": {k: stats(v) for k, v in ms.items()},
                          "overlay_stats_read_GBps": round(nbytes / (omean * 1e-3) / 1e9, 1),
                          "scene_diff_read_GBps": round(nbytes / (smean * 1e-3) / 1e9, 1),
                          "overlay_stats_over_scene_diff": round(omean / smean, 2), "same_integers_as_torch": same,
                          "same_integers_rerun": bool(torch.equal(sums, ops.overlay_stats(frames))),
                          "overlay_mask_wall_ms": stats(wall[1:]), "mask_pixels": found}), flush=True)
        if not same:
            sys.exit("the kernel and the torch composition sum different integers")
        del frames, sums, arms
