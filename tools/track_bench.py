"""End-to-end cost of inpaint_video(region="track") against region="hole" on a moving hole: L frames of 864x480 with a 90x60 hole
that moves 12 pixels right and 2 down per frame (wrapping at the frame's edge) through model.e2fgvi (synthetic weights, fp32) at
size=(432, 240) with restore=True, host arrays in and out.
  example  the worked example of tests/test_video_track.py: L = 30, frames 0 ... 14 carry the hole, frames 15 ... 29 none
  every    holes in every frame (the default for other L)
  (a) region="hole"   one box for the video: the bounding box of all masks, planned around it -- it grows with the hole's path
  (b) region="track"  one box per window, around the masks of the window's neighbour frames; a window without a hole runs no forward
One process, both arms warmed, then alternating; per round and arm one plain run (host clock around the call, which ends in the
copy to the host: video frames/s) and one with a counting model (the forwards).  Prints one JSON line per arm with mean / min /
max / std over the rounds, the number of forwards and the scale s = (right - left) / 432 of every box, and one with the comparison.
    python tools/track_bench.py [L=30] [rounds=6] [example|every]"""
import importlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from e2fgvi_amd import video
from e2fgvi_amd.synth import synth_state_dict

L = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
mode = sys.argv[3] if len(sys.argv) > 3 else ("example" if L == 30 else "every")
(W, H), size = (864, 480), (432, 240)
dev = torch.device("cuda:0")
rng = np.random.RandomState(0)
yy, xx = np.mgrid[0:H, 0:W]
base = np.stack([(xx * (3 + c) // 7 + yy * (5 - c) // 5) % 256 for c in range(3)], -1).astype(np.uint8)
frames = np.stack([np.roll(base, 3 * i, 1) for i in range(L)])
frames[:, 100:300, 200:600] = rng.randint(0, 256, (L, 200, 400, 3))
masks = np.zeros((L, H, W), np.uint8)
for i in range(L if mode == "every" else 15):
    x, y = (100 + 12 * i) % (W - 90), (150 + 2 * i) % (H - 60)            # wraps before the hole would leave the frame
    masks[i, y:y + 60, x:x + 90] = 255
net = importlib.import_module("model.e2fgvi").InpaintGenerator()
net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
net = net.to(dev).eval()
arms = ("hole", "track")


class Counted:
    def __init__(self, net):
        self.net, self.calls = net, 0

    def __call__(self, x, n_local):
        self.calls += 1
        return self.net(x, n_local)


def run(region, model=net):
    return video.inpaint_video(model, frames, masks, device=dev, size=size, restore=True, region=region)


out = {}
for region in arms:
    for _ in range(2):
        out[region] = run(region)
torch.cuda.synchronize()
hole = masks != 0
checks = {region + "_changes_hole": bool((out[region][hole] != frames[hole]).any()) for region in arms}
boxes = {"hole": [video.hole_region(masks, (W, H), size, device=dev)], "track": video.track_regions(masks, (W, H), size, device=dev)}
windows = video.plan_windows(L)
for region in arms:
    inside = np.zeros((L, H, W), bool)
    for (nb, _), b in zip(windows, boxes[region] * len(windows) if region == "hole" else boxes[region]):
        if b is not None:
            inside[nb, b[1]:b[3], b[0]:b[2]] = True
    checks[region + "_outside_boxes_is_source"] = bool(np.array_equal(out[region][~inside], frames[~inside]))
del out
sec = {region: [] for region in arms}
forwards = {}
for _ in range(rounds):
    for region in arms:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(region)
        sec[region].append(time.perf_counter() - t0)
        c = Counted(net)
        run(region, c)
        forwards[region] = c.calls


def stats(v, nd=3):
    v = np.array(v)
    return {"mean": round(float(v.mean()), nd), "min": round(float(v.min()), nd), "max": round(float(v.max()), nd),
            "std": round(float(v.std()), nd)}


for region in arms:
    s = np.array(sec[region])
    print(json.dumps({"arm": region, "frames": L, "holes": mode, "src": "%dx%d" % (W, H), "size": "%dx%d" % size, "rounds": rounds,
                      "forwards": forwards[region], "windows": len(windows),
                      "box_scale": [None if b is None else round((b[2] - b[0]) / size[0], 3) for b in boxes[region]],
                      "video_frames_per_s": stats(L / s, 2), "seconds": stats(s, 4)}), flush=True)
a, b = np.array(sec["hole"]), np.array(sec["track"])
verdict = {"track_minus_hole_mean_s": round(float(b.mean() - a.mean()), 4), "hole_spread_max_minus_min_s": round(float(a.max() - a.min()), 4),
           "track_spread_max_minus_min_s": round(float(b.max() - b.min()), 4)}
verdict.update(checks)
print(json.dumps(verdict), flush=True)
if not all(checks.values()):
    sys.exit("the two arms did not do what they are measured for")
