"""Temporal denoiser (video.denoise, ops.denoise, csrc/denoise.hip): what it costs.

    python tools/denoise_bench.py [rounds=11] [--no-inpaint] > profiles/denoise.txt
60 frames at 1920x1080, one scene: the 25 frames of tests/golden/tennis25.npz resized on the device (video.resize_frames) and
repeated, under uniform noise of +- 8 levels from a seeded generator; the flows are the net's own between these frames
(metrics.video_flows with the synthetic-weights generator), so the gathers follow a field that is smooth but not constant.
    denoise_s0_ms, denoise_s1_ms, denoise_s2_ms   one call of ops.denoise at strength 8 and search 0, 1, 2 into a buffer that is
                     there: the luma pass and the filter pass (and the allocation of the workspace)
    candidates_ms    ops.defect_candidates on the same frames along the same flows, every frame with both neighbours a centre
                     frame: the yardstick for the gather pattern
    denoise_s1_smooth_ms, candidates_smooth_ms   the two along flows that certainly stay in the frame -- a pan of (-2, -1) px under a
                     slow wave of 1.5 px -- whatever the synthetic weights make of the net's flows (inside_share_* says)
    flicker_apply_ms ops.flicker_apply on the same frames (reads 3 L H W, writes 3 L H W): the traffic floor of reading and writing
                     the frames once
each warmed; `rounds` rounds, and in every round each of them once, in this order, one pair of device events around each -- so the
passes alternate in one process: median / min / max, each denoise pass as a ratio to the two yardsticks, and the bytes it has to
move at the least (frames read once and written once, both flows read once: 3 + 3 + 16 bytes a pixel) over its median time.
    flows_s          metrics.video_flows on these frames, host clock and a synchronise, the smaller of two after a warm call
    inpaint_s        inpaint_video(size=(432, 240), restore=True) on these frames with a hole over a ninth of the frame
and the share of the flows and of the filter in video.denoise with the net's flows.  One JSON line.  The library is the one
E2FGVI_LIB names, or the product build.  Kernel times come from a run of this file under rocprofv3 --kernel-trace --stats with
--no-inpaint; counters from another run."""
import importlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def device(rounds, inpaint):
    import torch
    from e2fgvi_amd import lib, metrics, ops, video
    from e2fgvi_amd.synth import synth_state_dict
    from tests import denoise_cases as C
    dev = torch.device("cuda:0")
    L, W, H = 60, 1920, 1080
    big = video.resize_frames(C.tennis25(ROOT), (W, H), device=dev)
    frames = torch.cat([big] * 3)[:L].to(torch.int16)
    del big
    g = torch.Generator(device="cpu").manual_seed(1)
    for t in range(L):
        frames[t] += torch.randint(-8, 9, (H, W, 3), generator=g, dtype=torch.int16).to(dev)
    frames = frames.clamp_(0, 255).to(torch.uint8).contiguous()
    net = importlib.import_module("model.e2fgvi_hq").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi_hq", "stress", 0))
    net = net.to(dev).eval()
    stamp = lambda: (torch.cuda.synchronize(), time.perf_counter())[1]
    with torch.no_grad():
        metrics.video_flows(net, frames[:3].contiguous())
        flows_all = []
        for _ in range(2):
            t0 = stamp()
            fwd, bwd = metrics.video_flows(net, frames)
            flows_all.append(stamp() - t0)
    fwd, bwd = fwd.contiguous(), bwd.contiguous()
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    ids = torch.tensor(video.plan_defect_frames(L), dtype=torch.int32).to(dev)
    out = torch.empty_like(frames)
    cand = torch.zeros((L, H, W), dtype=torch.uint8, device=dev)
    hist = ops.flicker_hist(frames)
    _, d = ops.flicker_curves(hist, scene, H * W, 4, 32)
    # a second pair of flows that certainly stays in the frame: a pan of (-2, -1) px under a slow wave of 1.5 px
    ys = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xs = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    wave = torch.stack([1.5 * torch.sin(xs / 97 + ys / 61), 1.5 * torch.cos(xs / 83 - ys / 71)], dim=-1)
    sfwd = (wave + torch.tensor([-2.0, -1.0], device=dev)).expand(L - 1, H, W, 2).contiguous()
    sbwd = (-sfwd).contiguous()
    passes = {
        "denoise_s1_smooth": lambda: ops.denoise(frames, sfwd, sbwd, scene, 8, 1, 255, out=out),
        "candidates_smooth": lambda: ops.defect_candidates(frames, sfwd, sbwd, ids, video.DEFECT_THRESHOLD, video.DEFECT_SLACK, out=cand),
        "denoise_s0": lambda: ops.denoise(frames, fwd, bwd, scene, 8, 0, 255, out=out),
        "candidates": lambda: ops.defect_candidates(frames, fwd, bwd, ids, video.DEFECT_THRESHOLD, video.DEFECT_SLACK, out=cand),
        "denoise_s1": lambda: ops.denoise(frames, fwd, bwd, scene, 8, 1, 255, out=out),
        "flicker_apply": lambda: ops.flicker_apply(frames, d, out=out),
        "denoise_s2": lambda: ops.denoise(frames, fwd, bwd, scene, 8, 2, 255, out=out),
    }
    for fn in passes.values():
        fn()
    ms = {k: [] for k in passes}
    for _ in range(rounds):
        for k, fn in passes.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    px = L * H * W
    changed = ops.denoise(frames, fwd, bwd, scene, 8, 1, 255, out=out).ne(frames).float().mean().item()
    rec = {"video": "tennis25 resized, uniform noise of +- 8", "size": "%dx%d" % (W, H), "frames": L, "rounds": rounds,
           "library": os.path.basename(lib.LIB_PATH), "flows": "metrics.video_flows, synthetic weights",
           "finite_flows": bool(torch.isfinite(fwd).all() and torch.isfinite(bwd).all()),
           "mean_abs_flow_px": round(float(fwd[torch.isfinite(fwd)].abs().mean()), 3), "bytes_changed_s1": round(changed, 4)}
    for k, v in ms.items():
        rec[k + "_ms"] = {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    for k in ("denoise_s0", "denoise_s1", "denoise_s2"):
        rec[k + "_over_candidates"] = round(med[k] / med["candidates"], 3)
        rec[k + "_over_flicker_apply"] = round(med[k] / med["flicker_apply"], 3)
        rec[k + "_least_TB_per_s"] = round(22 * px / (med[k] * 1e-3) / 1e12, 3)
    rec["denoise_s1_smooth_over_candidates_smooth"] = round(med["denoise_s1_smooth"] / med["candidates_smooth"], 3)
    rec["denoise_s1_smooth_over_flicker_apply"] = round(med["denoise_s1_smooth"] / med["flicker_apply"], 3)
    inside = lambda f: float(((xs + f[..., 0] >= 0) & (xs + f[..., 0] <= W - 1) & (ys + f[..., 1] >= 0) & (ys + f[..., 1] <= H - 1)).float().mean())
    rec["inside_share_net_flows"] = round(0.5 * (inside(fwd) + inside(bwd)), 4)
    rec["inside_share_smooth_flows"] = round(0.5 * (inside(sfwd) + inside(sbwd)), 4)
    rec["flows_s"] = round(min(flows_all), 4)
    rec["flows_s_all"] = [round(v, 4) for v in flows_all]
    rec["flows_share_of_denoise_s1"] = round(min(flows_all) / (min(flows_all) + med["denoise_s1"] * 1e-3), 4)
    del out, cand
    torch.cuda.empty_cache()
    if inpaint:
        host = frames.cpu().numpy()
        m = np.zeros((L, H, W), np.uint8)
        m[:, H // 3:2 * H // 3, W // 3:2 * W // 3] = 1
        with torch.no_grad():
            video.inpaint_video(net, host[:12], m[:12], size=(432, 240), restore=True)
            t0 = stamp()
            video.inpaint_video(net, host, m, size=(432, 240), restore=True)
            rec["inpaint_s"] = round(stamp() - t0, 3)
            t0 = stamp()
            video.denoise(net, host)
            rec["denoise_with_flows_upload_and_download_s"] = round(stamp() - t0, 4)
        rec["denoise_s1_share_of_inpaint"] = round(med["denoise_s1"] * 1e-3 / rec["inpaint_s"], 5)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    device(next((int(a) for a in sys.argv[1:] if a.isdigit()), 11), "--no-inpaint" not in sys.argv)
