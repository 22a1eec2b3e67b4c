"""Real pixels for restored holes (video.propagate_pixels, ops.pixel_track_step, ops.pixel_fill, csrc/pixel_track.hip): what it
costs and what it reaches.

(1) 60 frames at 1920x1080, a static hole -- the size of a logo (160x90) and a quarter of the frame (960x540) -- and GIVEN flows
    (built on the device: a drift of up to 3 px per frame plus long waves, bwd = -fwd + waves of up to 0.3 px):
      steps_fill_ms  all launches of the lockstep plan (video.plan_pixel_chains: one launch per step) and the one of the fill, warmed,
                     one pair of device events around them; the planes are reset outside the timed window
      flows_s        metrics.video_flows of the synthetic-weights fp32 generator on the same number of frames of a synthetic moving
                     clip: host clock around the call and a synchronise, after a warm call on three frames
      filled         the share of hole pixels the fill wrote (source 1 or 2)
(2) the translated-tennis video of profiles/defects_stats.txt (frame 0 of tests/golden/tennis25.npz moved 1.5 / 0.5 px per frame,
    ideal flows), here 25 frames, with the static hole of a logo (60x34 at 432x240): the share of hole pixels filled, per frame and
    in all, the histogram of the ages they were fetched over, and the largest difference to the frame without the hole.
(3) a uniform pan of v pixels per frame behind a static 12x9 hole, 16 frames of 24x61 (the geometry of the tests' exact-truth
    case), ideal flows: the share of hole pixels filled against v.  The walk through the hole advances by the flow ROUNDED to whole
    pixels while the origin advances by the flow itself: where the two differ the share drops.
One JSON line per measurement.
    python tools/pixel_track_bench.py [rounds=5]"""
import importlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from e2fgvi_amd import metrics, ops, video
from e2fgvi_amd.synth import synth_clip, synth_state_dict

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = torch.device("cuda:0")


def smooth_flows(H, W, L, seed):
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
    fwd = torch.stack([(r(L - 1, 1, 1) - 0.5) * 6 + waves(L - 1, 1.5, 40, 400), (r(L - 1, 1, 1) - 0.5) * 6 + waves(L - 1, 1.5, 40, 400)], -1)
    bwd = -fwd + torch.stack([waves(L - 1, 0.3, 30, 90), waves(L - 1, 0.3, 30, 90)], -1)
    return fwd.contiguous(), bwd.contiguous()


def frames_u8(L, H, W, seed):
    x, _ = synth_clip(1, L, H, W, seed=seed, moving=True)
    return ((x[0] * 0.5 + 0.5) * 255).round().clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()


def stats(v):
    v = np.array(v)
    return {"mean": round(float(v.mean()), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def propagate(src, hole, fwd, bwd, filled, tables, age, origin, init):
    """the launches of video.propagate_pixels on prepared buffers -> (out, source)"""
    age.copy_(init)
    out = filled.clone()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for tb in tables:
        ops.pixel_track_step(hole, age, origin, fwd, bwd, tb, 254, True)
    out, source = ops.pixel_fill(src, hole, age, origin, out, True)
    e1.record()
    e1.synchronize()
    return out, source, e0.elapsed_time(e1)


def ages_of(source, age):
    a = torch.where(source == 1, age[0], age[1])[(source == 1) | (source == 2)]
    return torch.bincount(a.long(), minlength=1).cpu().tolist()


net = importlib.import_module("model.e2fgvi").InpaintGenerator()
net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
net = net.to(dev).eval()

W, H, L = 1920, 1080, 60
frames = frames_u8(L, H, W, 11)
with torch.no_grad():
    metrics.video_flows(net, frames[:3])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nf, nb = metrics.video_flows(net, frames)
    torch.cuda.synchronize()
    flows_s = time.perf_counter() - t0
del nf, nb
torch.cuda.empty_cache()
src = torch.from_numpy(frames).to(dev)
fwd, bwd = smooth_flows(H, W, L, 2)
steps = video.plan_pixel_chains(L)
tables = [torch.tensor(s, dtype=torch.int32).to(dev) for s in steps]
origin = torch.empty((2, L, H, W, 2), dtype=torch.float32, device=dev)
for name, (hw, hh) in (("logo 160x90", (160, 90)), ("quarter 960x540", (960, 540))):
    hole = torch.zeros((L, H, W), dtype=torch.uint8, device=dev)
    y0, x0 = (H - hh) // 3, (W - hw) // 3
    hole[:, y0:y0 + hh, x0:x0 + hw] = 1
    init = (hole * 255).unsqueeze(0).repeat(2, 1, 1, 1)
    age = init.clone()
    ms = []
    for r in range(rounds + 1):                          # round 0 warms
        out, source, t = propagate(src, hole, fwd, bwd, src, tables, age, origin, init)
        if r:
            ms.append(t)
    n_hole = int(hole.sum())
    got = int(((source == 1) | (source == 2)).sum())
    hist = ages_of(source, age)
    print(json.dumps({"size": "%dx%d" % (W, H), "frames": L, "hole": name, "hole_pixels_per_frame": n_hole // L, "rounds": rounds,
                      "launches": {"steps": len(steps), "fill": 1}, "steps_fill_ms": stats(ms),
                      "flows_s": round(flows_s, 3), "share_of_flows": round(float(np.mean(ms)) / (flows_s * 1e3), 5),
                      "filled": round(got / n_hole, 4), "largest_age": len(hist) - 1,
                      "age_median": int(np.searchsorted(np.cumsum(hist), sum(hist) / 2))}), flush=True)
    del hole, init, age, out, source
del src, fwd, bwd, origin
torch.cuda.empty_cache()

GOLD = os.path.join(ROOT, "tests", "golden", "tennis25.npz")
if os.path.exists(GOLD):
    from tests import defect_cases as D
    L = 25
    truth, fwd, bwd, _ = D.tennis_video(ROOT, length=L)
    H, W = truth.shape[1:3]
    hole = np.zeros((L, H, W), np.uint8)
    hole[:, 40:74, 300:360] = 1
    frames = truth.copy()
    frames[hole == 1] = 255                             # the logo, in the caller's frames
    filled = truth.copy()
    filled[hole == 1] = 128                             # what stands in for the prediction
    out, source = video.propagate_pixels(None, frames, hole * np.uint8(255), filled, flows=(fwd, bwd), dilate=False,
                                         return_source=True, device=dev)
    got = (source == 1) | (source == 2)
    # the ages, from the planes of the same launches
    hd = torch.from_numpy(hole).to(dev)
    age = (hd * 255).unsqueeze(0).repeat(2, 1, 1, 1)
    origin = torch.empty((2, L, H, W, 2), dtype=torch.float32, device=dev)
    for s in video.plan_pixel_chains(L):
        ops.pixel_track_step(hd, age, origin, fwd, bwd, torch.tensor(s, dtype=torch.int32).to(dev))
    hist = ages_of(torch.from_numpy(source).to(dev), age)
    diff = np.abs(out.astype(np.int32) - truth.astype(np.int32)).max(-1)
    print(json.dumps({"clip": "tennis25 frame 0 translated 1.5 / 0.5 px per frame, %d frames %dx%d, ideal flows" % (L, W, H),
                      "hole": "static 60x34", "hole_pixels_per_frame": int(hole[0].sum()),
                      "filled": round(float(got.sum()) / float(hole.sum()), 4),
                      "filled_per_frame": [round(float(got[t].sum()) / float(hole[t].sum()), 3) for t in range(L)],
                      "age_histogram": hist,
                      "max_abs_diff_to_the_frame_without_the_hole": int(diff[got].max()),
                      "mean_abs_diff": round(float(diff[got].mean()), 3)}), flush=True)
else:
    print(json.dumps({"clip": "tennis25", "skipped": "tests/golden/tennis25.npz not found"}), flush=True)

shares = {}
L, H, W = 16, 24, 61
hole = np.zeros((L, H, W), np.uint8)
hole[:, 8:17, 24:36] = 1
rng = np.random.RandomState(0)
frames = rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)
for v in (0.25, 0.4, 0.5, 0.6, 1.0, 1.25, 1.4, 1.5, 1.6, 1.75, 2.0, 2.4, 2.6, 3.0):
    fwd = np.zeros((L - 1, H, W, 2), np.float32)
    fwd[..., 0] = v
    _, source = video.propagate_pixels(None, frames, hole * np.uint8(255), frames, flows=(fwd, -fwd), dilate=False, return_source=True,
                                       device=dev)
    shares[str(v)] = round(float(((source == 1) | (source == 2)).sum()) / float(hole.sum()), 3)
print(json.dumps({"clip": "uniform pan of v px per frame, 16 frames 61x24, static hole 12x9, ideal flows", "filled_by_v": shares}), flush=True)
