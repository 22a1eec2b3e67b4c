"""Weave stabiliser (video.stabilize, ops.weave_profiles, ops.weave_match, ops.weave_path, ops.weave_apply, csrc/weave.hip): what it
costs, and what it does to planted weave.

    python tools/weave_bench.py [rounds=11] [--no-inpaint]
60 frames at 1920x1080, the defaults, one scene: the 25 frames of tests/golden/tennis25.npz resized on the device
(video.resize_frames) and repeated, each frame moved by whole and fractional pixels (ops.weave_apply) so that the apply pass has
fractions on both axes to blend.
    profiles_ms  the memset and the one launch of ops.weave_profiles (reads every frame byte once: 3 L H W bytes)
    hist_ms      ops.flicker_hist into a buffer that is there, on the same frames in the same run: it moves the same bytes and is
                 the yardstick for profiles_ms
    match_ms     the one launch of ops.weave_match;  path_ms: the one launch of ops.weave_path
    apply_ms     the one launch of ops.weave_apply with the mask, into buffers that are there (reads 3 L H W bytes -- each about
                 four times, from the caches -- and writes 4 L H W); apply_whole_ms: the same with whole-pixel shifts (a copy)
    flicker_apply_ms  ops.flicker_apply on the same frames in the same run (reads and writes 6 L H W bytes): the yardstick for apply_ms
each warmed, `rounds` repetitions, one pair of device events around each: median / min / max;  stabilize_ms the four calls in a row
(video._stabilize_device, allocations included); and beside them
    inpaint_s    video.inpaint_video of the synthetic-weights fp32 generator on the same frames with a box hole (size=(432, 240),
                 restore=True): host clock around the call and a synchronise, after a warm call on 12 frames
Then, from the device: tests/golden/tennis25.npz under weave_cases.plant (whole-pixel weave of +-3 px, replicated borders; seeds 0,
1, 2) through video.stabilize at radius 24 and spans 1, 2, 4 and 8: per axis the rms in px of the planted weave before, and of
plant + (correction - the clean video's own correction) after, each with its mean taken out; how many of the 24 pairs' motions are
within 8/16 px of the clean video's motion plus the planted difference; and the largest error.  One JSON line each.  --no-inpaint
leaves the generator out: the form to run under rocprofv3 --kernel-trace --stats."""
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
    from tests import weave_cases as C
    dev = torch.device("cuda:0")
    span, radius, max_shift, tex = video.WEAVE_SPAN, video.WEAVE_RADIUS, video.WEAVE_MAX_SHIFT, video.WEAVE_TEX

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
    still = torch.cat([big, big, big[:L - 2 * len(big)]]).contiguous()
    del big
    weave = torch.from_numpy(np.random.default_rng(0).integers(-40, 41, (L, 2)).astype(np.int32)).to(dev)
    src = ops.weave_apply(still, weave)
    del still
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    out, mask = torch.empty_like(src), torch.empty((L, H, W), dtype=torch.uint8, device=dev)
    hist = torch.empty((L, 256), dtype=torch.int32, device=dev)
    col, row = ops.weave_profiles(src)
    motion = ops.weave_match(col, row, scene, radius, tex)
    shifts = ops.weave_path(motion, scene, span, max_shift)
    whole = ((shifts + 8) >> 4) << 4
    ops.flicker_hist(src, out=hist)
    _, d = ops.flicker_curves(hist, scene, H * W, 4, 32)
    t_prof = timed(lambda: ops.weave_profiles(src))
    t_hist = timed(lambda: ops.flicker_hist(src, out=hist))
    t_match = timed(lambda: ops.weave_match(col, row, scene, radius, tex))
    t_path = timed(lambda: ops.weave_path(motion, scene, span, max_shift))
    t_apply = timed(lambda: ops.weave_apply(src, shifts, out=out, mask=mask))
    t_whole = timed(lambda: ops.weave_apply(src, whole, out=out, mask=mask))
    t_fapply = timed(lambda: ops.flicker_apply(src, d, out=out))
    t_all = timed(lambda: video._stabilize_device(src, np.zeros(L, np.int32), span, radius, max_shift, tex, True, True))
    med = lambda v: float(np.median(v))
    rec = {"video": "natural with weave", "size": "%dx%d" % (W, H), "frames": L, "rounds": rounds, "span": span, "radius": radius,
           "max_shift": max_shift, "tex": tex, "trusted_pairs_x_y": [int((motion[:, 2] >= 4).sum()), int((motion[:, 3] >= 4).sum())],
           "max_abs_shift_16ths": int(shifts.abs().max()), "fractional_shifts": int((shifts & 15).ne(0).sum()),
           "profiles_ms": stats(t_prof), "hist_ms": stats(t_hist), "profiles_over_hist": round(med(t_prof) / med(t_hist), 3),
           "profiles_TB_per_s": round(3 * L * H * W / (med(t_prof) * 1e-3) / 1e12, 3),
           "match_ms": stats(t_match), "path_ms": stats(t_path), "apply_ms": stats(t_apply), "apply_whole_ms": stats(t_whole),
           "flicker_apply_ms": stats(t_fapply), "apply_over_flicker_apply": round(med(t_apply) / med(t_fapply), 3),
           "apply_whole_over_flicker_apply": round(med(t_whole) / med(t_fapply), 3), "stabilize_ms": stats(t_all)}
    del out, mask
    torch.cuda.empty_cache()
    if "--no-inpaint" not in sys.argv:
        net = importlib.import_module("model.e2fgvi_hq").InpaintGenerator()
        net.load_state_dict(synth_state_dict("e2fgvi_hq", "stress", 0))
        net = net.to(dev).eval()
        frames = src.cpu().numpy()
        m = np.zeros((L, H, W), np.uint8)
        m[:, H // 3:H // 2, W // 3:W // 2] = 1
        with torch.no_grad():
            video.inpaint_video(net, frames[:12], m[:12], size=(432, 240), restore=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            video.inpaint_video(net, frames, m, size=(432, 240), restore=True)
            torch.cuda.synchronize()
            rec["inpaint_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            video.stabilize(frames, device=dev)
            rec["stabilize_with_upload_and_download_s"] = round(time.perf_counter() - t0, 4)
        rec["stabilize_share_of_inpaint"] = round(rec["stabilize_ms"]["median"] * 1e-3 / rec["inpaint_s"], 5)
    print(json.dumps(rec), flush=True)
    del src
    rms = lambda v: round(float(np.sqrt(((v - v.mean()) ** 2).mean())), 4)
    _, _, clean_motion = video.stabilize(tennis, radius=24, return_shifts=True, device=dev)
    for seed in (0, 1, 2):
        planted, plant = C.plant(tennis, seed)
        row = {"video": "tennis25 planted", "seed": seed, "radius": 24,
               "weave_rms_px_x_y": [rms(plant[:, 0].astype(np.float64)), rms(plant[:, 1].astype(np.float64))]}
        for s in (1, 2, 4, 8):
            _, sh, mo = video.stabilize(planted, radius=24, span=s, return_shifts=True, device=dev)
            _, own, _ = video.stabilize(tennis, radius=24, span=s, return_shifts=True, device=dev)
            left = plant + (sh.astype(np.float64) - own) / 16
            row["span_%d" % s] = {"left_rms_px_x_y": [rms(left[:, 0]), rms(left[:, 1])]}
        err = np.abs(mo[1:, :2] - (clean_motion[1:, :2] + 16 * np.diff(plant, axis=0)))
        row["pairs_within_8_16ths_x_y"] = [(err[:, 0] <= 8).sum().item(), (err[:, 1] <= 8).sum().item()]
        row["largest_error_16ths_x_y"] = err.max(axis=0).tolist()
        row["errors_sorted_16ths_x"] = sorted(err[:, 0].tolist())[-4:]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    device(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 11)
