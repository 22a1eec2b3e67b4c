"""Frame interpolation (video.retime, ops.interpolate, csrc/interpolate.hip): what it costs.

    python tools/interpolate_bench.py [rounds=11] [--kernels] > profiles/interpolate.txt
60 frames at 1920x1080, one scene: the 25 frames of tests/golden/tennis25.npz resized on the device (video.resize_frames) and
repeated; rate = 2, so 119 output frames of which 60 are copies and 59 are made at the fraction 1/2; the flows are the net's own
between these frames (metrics.video_flows with the synthetic-weights generator), and a second pair that certainly stays in the
frame: a pan of (-2, -1) px under a slow wave of 1.5 px.
    interpolate_ms, interpolate_it0_ms, interpolate_it8_ms   one call of ops.interpolate with video.plan_retime's table at the
                     default setting (3 fixed-point iterations), and at 0 and 8 iterations, into buffers that are there, with the
                     source codes
    interpolate_new_ms   the 59 new frames alone (the copies left out of the table)
    interpolate_smooth_ms   the default setting along the smooth flows
    denoise_s1_ms    ops.denoise at search 1 on the same frames along the same flows: the yardstick for gathers along flows
    flicker_apply_ms ops.flicker_apply on the same frames (reads 3 L H W, writes 3 L H W): the traffic floor of reading and writing
                     the frames once
each warmed; `rounds` rounds, and in every round each of them once, in this order, one pair of device events around each -- so the
passes alternate in one process: median / min / max, the interpolation as a ratio to the two yardsticks, the share of each source
code, and the bytes the call has to move at the least over its median time.  One JSON line.  --kernels: the interpolation and
the two yardsticks alone, two rounds, for a run under rocprofv3 (kernel times from --kernel-trace --stats; counters from a run of
its own with --pmc).  The library is the one E2FGVI_LIB names, or the product build."""
import importlib
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def device(rounds, kernels_only):
    import torch
    from e2fgvi_amd import lib, metrics, ops, video
    from e2fgvi_amd.synth import synth_state_dict
    from tests import denoise_cases as DN
    dev = torch.device("cuda:0")
    L, W, H = 60, 1920, 1080
    big = video.resize_frames(DN.tennis25(ROOT), (W, H), device=dev)
    frames = torch.cat([big] * 3)[:L].contiguous()
    del big
    net = importlib.import_module("model.e2fgvi_hq").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi_hq", "stress", 0))
    net = net.to(dev).eval()
    with torch.no_grad():
        fwd, bwd = (f.contiguous() for f in metrics.video_flows(net, frames))
    rows, pairs = video.plan_retime(L, 2)
    assert pairs == list(range(L - 1))
    jobs = torch.tensor(rows, dtype=torch.int32).to(dev)
    new = torch.tensor([r for r in rows if r[3]], dtype=torch.int32).to(dev)
    n = len(rows)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    src = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    dn_out = torch.empty_like(frames)
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    hist = ops.flicker_hist(frames)
    _, d = ops.flicker_curves(hist, scene, H * W, 4, 32)
    ys = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xs = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    wave = torch.stack([1.5 * torch.sin(xs / 97 + ys / 61), 1.5 * torch.cos(xs / 83 - ys / 71)], dim=-1)
    sfwd = (wave + torch.tensor([-2.0, -1.0], device=dev)).expand(L - 1, H, W, 2).contiguous()
    sbwd = (-sfwd).contiguous()
    k = len(new)
    passes = {
        "interpolate": lambda: ops.interpolate(frames, fwd, bwd, jobs, 3, 8, 96, out=out, source=src),
        "denoise_s1": lambda: ops.denoise(frames, fwd, bwd, scene, 8, 1, 255, out=dn_out),
        "flicker_apply": lambda: ops.flicker_apply(frames, d, out=dn_out),
    }
    if not kernels_only:
        passes.update({
            "interpolate_it0": lambda: ops.interpolate(frames, fwd, bwd, jobs, 0, 8, 96, out=out, source=src),
            "interpolate_it8": lambda: ops.interpolate(frames, fwd, bwd, jobs, 8, 8, 96, out=out, source=src),
            "interpolate_new": lambda: ops.interpolate(frames, fwd, bwd, new, 3, 8, 96, out=out[:k], source=src[:k]),
            "interpolate_smooth": lambda: ops.interpolate(frames, sfwd, sbwd, jobs, 3, 8, 96, out=out, source=src),
        })
    for fn in passes.values():
        fn()
    ms = {name: [] for name in passes}
    for _ in range(rounds):
        for name, fn in passes.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    rec = {"video": "tennis25 resized", "size": "%dx%d" % (W, H), "frames": L, "rate": 2, "frames_out": n, "frames_new": k, "rounds": rounds,
           "library": os.path.basename(lib.LIB_PATH), "flows": "metrics.video_flows, synthetic weights",
           "finite_flows": bool(torch.isfinite(fwd).all() and torch.isfinite(bwd).all()),
           "mean_abs_flow_px": round(float(fwd[torch.isfinite(fwd)].abs().mean()), 3)}
    for name, v in ms.items():
        rec[name + "_ms"] = {"median": round(med[name], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    for name in [p for p in passes if p.startswith("interpolate")]:
        rec[name + "_over_denoise_s1"] = round(med[name] / med["denoise_s1"], 3)
        rec[name + "_over_flicker_apply"] = round(med[name] / med["flicker_apply"], 3)
    # the least the call moves: a copy reads and writes 3 bytes a pixel and writes a code; a new frame reads two frames and two flows
    # once (6 + 16 bytes a pixel) and writes 3 + 1
    px = H * W
    rec["interpolate_least_TB_per_s"] = round(((n - k) * 7 + k * 26) * px / (med["interpolate"] * 1e-3) / 1e12, 3)
    for label, fn in (("net", passes["interpolate"]),) + ((("smooth", passes["interpolate_smooth"]),) if not kernels_only else ()):
        fn()
        counts = torch.bincount(src[1::2].reshape(-1).to(torch.int64), minlength=6).float()
        rec["source_share_%s_flows" % label] = [round(float(c), 5) for c in counts / counts.sum()]
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    only = "--kernels" in sys.argv
    device(2 if only else next((int(a) for a in sys.argv[1:] if a.isdigit()), 11), only)
