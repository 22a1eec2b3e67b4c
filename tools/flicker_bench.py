"""Deflicker (video.deflicker, ops.flicker_hist, ops.flicker_curves, ops.flicker_apply, csrc/flicker.hip): what it costs, and what
it does to planted flicker.

    python tools/flicker_bench.py [rounds=11] [--no-inpaint]
60 frames at 1920x1080, the defaults, one scene, two videos: "natural" -- the 25 frames of tests/golden/tennis25.npz resized on the
device (video.resize_frames) and repeated -- and "flat", mid grey everywhere: every pixel in one histogram bin, the worst case for
the LDS atomics of the histogram pass.
    hist_ms      the memset and the one launch of ops.flicker_hist (reads every frame byte once: 3 L H W bytes)
    curves_ms    the one launch of ops.flicker_curves over L x 256 counts
    apply_ms     the one launch of ops.flicker_apply into a buffer that is there (reads and writes 6 L H W bytes)
    line_sums_ms the project's own pass over the same bytes, ops.line_sums(rows=16), on the same frames in the same run: the
                 yardstick for hist_ms
each warmed, `rounds` repetitions, one pair of device events around each: median / min / max, and the rate the bytes above make;
deflicker_ms the three calls in a row (video._deflicker_device); and beside them, on the natural video,
    inpaint_s    video.inpaint_video of the synthetic-weights fp32 generator on the same frames with a box hole (size=(432, 240),
                 restore=True): host clock around the call and a synchronise, after a warm call on 12 frames
Then, from the device: tests/golden/tennis25.npz under flicker_cases.plant (gain +-10 %, offset +-8 levels per frame; seeds 0, 1, 2)
through video.deflicker at spans 1, 2, 4 and 8 -- the roughness (the mean |second difference| along time of the frames' mean luma)
before and after and the ratio -- and the clean video through it at the defaults: the share of pixels it changes and by how much.
One JSON line each.  --no-inpaint leaves the generator out: the form to run under rocprofv3 --kernel-trace --stats."""
import importlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def device(rounds):
    import torch
    from e2fgvi_amd import ops, video
    from e2fgvi_amd.synth import synth_state_dict
    from tests import flicker_cases as C
    dev = torch.device("cuda:0")
    span, max_shift = video.FLICKER_SPAN, video.FLICKER_MAX_SHIFT

    def stats(v):
        v = np.array(v)
        return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}

    def timed(fn):
        fn()
        ms = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    L, W, H = 60, 1920, 1080
    tennis = C.tennis25(ROOT)
    big = video.resize_frames(tennis, (W, H), device=dev)
    natural = torch.cat([big, big, big[:L - 2 * len(big)]]).contiguous()
    del big
    flat = torch.full((L, H, W, 3), 128, dtype=torch.uint8, device=dev)
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    out = torch.empty_like(flat)
    hist = torch.empty((L, 256), dtype=torch.int32, device=dev)
    rate = lambda b, ms: round(b / (float(np.median(ms)) * 1e-3) / 1e12, 3)
    recs = {}
    for name, src in (("natural", natural), ("flat", flat)):
        ops.flicker_hist(src, out=hist)
        Q, d = ops.flicker_curves(hist, scene, H * W, span, max_shift)
        t_hist = timed(lambda: ops.flicker_hist(src, out=hist))
        t_curves = timed(lambda: ops.flicker_curves(hist, scene, H * W, span, max_shift))
        t_apply = timed(lambda: ops.flicker_apply(src, d, out=out))
        t_sums = timed(lambda: ops.line_sums(src, 16))
        t_all = timed(lambda: video._deflicker_device(src, np.zeros(L, np.int32), span, max_shift))
        b_hist, b_apply = 3 * L * H * W, 6 * L * H * W
        b_sums = 3 * L * (H // 16) * 16 * W
        recs[name] = {"video": name, "size": "%dx%d" % (W, H), "frames": L, "rounds": rounds, "span": span, "max_shift": max_shift,
                      "max_abs_shift": int(d.abs().max()), "bins_used_frame0": int((hist[0] != 0).sum()),
                      "hist_ms": stats(t_hist), "hist_bytes": b_hist, "hist_TB_per_s": rate(b_hist, t_hist),
                      "line_sums_ms": stats(t_sums), "line_sums_bytes": b_sums, "line_sums_TB_per_s": rate(b_sums, t_sums),
                      "hist_over_line_sums": round(float(np.median(t_hist)) / float(np.median(t_sums)), 3),
                      "curves_ms": stats(t_curves), "apply_ms": stats(t_apply), "apply_bytes": b_apply,
                      "apply_TB_per_s": rate(b_apply, t_apply), "deflicker_ms": stats(t_all)}
    del flat, out
    torch.cuda.empty_cache()
    if "--no-inpaint" not in sys.argv:
        net = importlib.import_module("model.e2fgvi_hq").InpaintGenerator()
        net.load_state_dict(synth_state_dict("e2fgvi_hq", "stress", 0))
        net = net.to(dev).eval()
        frames = natural.cpu().numpy()
        m = np.zeros((L, H, W), np.uint8)
        m[:, H // 3:H // 2, W // 3:W // 2] = 1
        with torch.no_grad():
            video.inpaint_video(net, frames[:12], m[:12], size=(432, 240), restore=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            video.inpaint_video(net, frames, m, size=(432, 240), restore=True)
            torch.cuda.synchronize()
            recs["natural"]["inpaint_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            video.deflicker(frames, device=dev)
            recs["natural"]["deflicker_with_upload_and_download_s"] = round(time.perf_counter() - t0, 4)
        recs["natural"]["deflicker_share_of_inpaint"] = round(recs["natural"]["deflicker_ms"]["median"] * 1e-3 / recs["natural"]["inpaint_s"], 5)
    for rec in recs.values():
        print(json.dumps(rec), flush=True)
    del natural
    print(json.dumps({"video": "tennis25 clean", "roughness": round(C.roughness(tennis), 4)}), flush=True)
    for seed in (0, 1, 2):
        planted = C.plant(tennis, seed)
        before = C.roughness(planted)
        row = {"video": "tennis25 planted", "seed": seed, "roughness": round(before, 4)}
        for s in (1, 2, 4, 8):
            got, d = video.deflicker(planted, span=s, return_curves=True, device=dev)
            after = C.roughness(got)
            moved = np.arange(256)[None, :] + d.astype(np.int64)
            row["span_%d" % s] = {"roughness": round(after, 4), "ratio": round(after / before, 4),
                                  "level_plus_shift_non_decreasing": bool((np.diff(moved, axis=1) >= 0).all())}
        print(json.dumps(row), flush=True)
    got = video.deflicker(tennis, device=dev)
    diff = np.abs(got.astype(np.int64) - tennis).max(axis=-1)
    print(json.dumps({"video": "tennis25 clean through deflicker", "roughness": round(C.roughness(got), 4),
                      "pixels_changed": round(float((diff > 0).mean()), 4), "largest_change": int(diff.max())}), flush=True)


if __name__ == "__main__":
    device(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 11)
