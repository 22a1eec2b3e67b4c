"""Masks from keyframes (video.propagate_masks, ops.mask_track_step, csrc/mask_track.hip): what the two pieces cost.

For 100 frames at 432x240 and 60 frames at 1920x1080, a key every KEY_EVERY frames:
  flows      metrics.video_flows of the synthetic-weights fp32 generator on a synthetic moving clip: host clock around the call and a
             synchronise, after a warm call on three frames (the weights are packed, the code objects loaded)
  chains     all launches of the propagation with GIVEN flows (smooth synthetic ones built on the device: a drift of up to 3 px plus
             long waves, bwd = -fwd + waves of up to 0.9 px, so that the consistency test takes both outcomes) and a key mask of about
             a tenth of the frame: the lockstep plan of video.plan_mask_chains (one launch per step) against the same chains run one
             job per launch, both warmed, alternating, one pair of device events around all launches of an arm; the planes are
             reset outside the timed window.  The two arms must leave the same bytes.
  gather     the share of destination pixels that took the 32-byte gather of the check flow (inside and s >= 0.5), counted job by
             job with the test switched off on a copy of the planes
One JSON line per size.
    python tools/mask_keys_bench.py [rounds=5]"""
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
KEY_EVERY = 20
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
    bwd = -fwd + torch.stack([waves(L - 1, 0.9, 30, 90), waves(L - 1, 0.9, 30, 90)], -1)
    return fwd.contiguous(), bwd.contiguous()


def frames_u8(L, H, W, seed):
    x, _ = synth_clip(1, L, H, W, seed=seed, moving=True)
    return ((x[0] * 0.5 + 0.5) * 255).round().clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()


def stats(v):
    v = np.array(v)
    return {"mean": round(float(v.mean()), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


net = importlib.import_module("model.e2fgvi").InpaintGenerator()
net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
net = net.to(dev).eval()

for (W, H, L) in ((432, 240, 100), (1920, 1080, 60)):
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

    fwd, bwd = smooth_flows(H, W, L, 2)
    keys = list(range(0, L, KEY_EVERY))
    init = torch.zeros((2, L, H, W), dtype=torch.uint8, device=dev)
    init[:, keys, H // 3:H // 3 + H // 3, W // 3:W // 3 + W // 3] = 1
    steps = video.plan_mask_chains(L, keys)
    chains = {}                                         # the same jobs, chain after chain
    for s in steps:
        for t, d in s:
            key = max(k for k in keys if k <= t) if d == 0 else min(k for k in keys if k > t)
            chains.setdefault((key, d), []).append((t, d))
    single = [[j] for ch in chains.values() for j in ch]
    up = lambda tables: [torch.tensor(tb, dtype=torch.int32).to(dev) for tb in tables]
    arms = {"lockstep": up(steps), "one_job_per_launch": up(single)}
    planes = init.clone()

    def run(tables):
        for tb in tables:
            ops.mask_track_step(planes, fwd, bwd, tb, True)

    out, ms = {}, {k: [] for k in arms}
    for r in range(rounds + 1):                          # round 0 warms both arms
        for k, tables in arms.items():
            planes.copy_(init)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(tables)
            e1.record()
            e1.synchronize()
            if r:
                ms[k].append(e0.elapsed_time(e1))
            out[k] = planes.clone()
    same = bool(torch.equal(out["lockstep"], out["one_job_per_launch"]))
    result = out["lockstep"][0] | out["lockstep"][1]
    del out
    # the gather's share, job by job: what the step keeps with the test off is what the test is asked about
    planes.copy_(init)
    scratch = torch.empty_like(planes)
    cand = kept = 0
    for tb in arms["one_job_per_launch"]:
        t, d = (int(v) for v in tb[0].tolist())
        dst = (d, t + 1 if d == 0 else t)
        scratch.copy_(planes)
        ops.mask_track_step(scratch, fwd, bwd, tb, False)
        cand += int(scratch[dst].sum())
        ops.mask_track_step(planes, fwd, bwd, tb, True)
        kept += int(planes[dst].sum())
    njobs = len(single)
    print(json.dumps({"size": "%dx%d" % (W, H), "frames": L, "keys": keys, "rounds": rounds,
                      "flows_s": round(flows_s, 3), "flows_ms_per_pair": round(flows_s * 1e3 / (L - 1), 2),
                      "launches": {"lockstep": len(steps), "one_job_per_launch": njobs},
                      "chains_ms": {k: stats(v) for k, v in ms.items()},
                      "lockstep_us_per_job": round(float(np.mean(ms["lockstep"])) * 1e3 / njobs, 2),
                      "same_bytes": same, "check_gather_share": round(cand / (njobs * H * W), 4),
                      "kept_of_candidates": round(kept / max(cand, 1), 4),
                      "mask_share_first_last": [round(float(result[0].float().mean()), 4), round(float(result[L - 1].float().mean()), 4)]}),
          flush=True)
    if not same:
        sys.exit("the lockstep launches and the single jobs leave different bytes")
    del fwd, bwd, init, planes, scratch, result, arms
    torch.cuda.empty_cache()
