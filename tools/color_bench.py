"""Colour restoration (video.restore_color, ops.color_hist, ops.color_nodes, ops.color_lut, ops.color_apply, csrc/color.hip): what it
costs beside the deflicker's passes over the same frames, and what it does to planted fades.

    python tools/color_bench.py [rounds=11] [--passes-only]
60 frames at 1920x1080, the defaults, one scene, two videos: "natural" -- the 25 frames of tests/golden/tennis25.npz resized on the
device (video.resize_frames) and repeated -- and "flat", mid grey everywhere: every pixel in one histogram bin per channel, the
worst case for the LDS atomics of the histogram pass.
    color_hist_ms    the memset and the one launch of ops.color_hist (reads every frame byte once: 3 L H W bytes)
    color_nodes_ms   the one launch of ops.color_nodes over the L x 3 x 256 counts, one group of all frames
    color_lut_ms     the one launch of ops.color_lut
    color_apply_ms   the one launch of ops.color_apply into a buffer that is there (reads and writes 6 L H W bytes)
    flicker_hist_ms, flicker_curves_ms, flicker_apply_ms    the deflicker's three passes on the same frames: the yardstick
The seven are warmed and then timed in turn, one after the other in each of `rounds` rounds, one pair of device events around each
call: median / min / max, the rate the bytes above make, and each colour pass over its deflicker counterpart.  restore_color_ms and
deflicker_ms are the whole tools after the upload (video._restore_color_device, video._deflicker_device).
The library is the one e2fgvi_amd.lib loads: E2FGVI_LIB=<an A/B build> python tools/color_bench.py 11 --passes-only times
build.build_variant("tag", "-DCOL_COPIES=1") / "-DCOL_MERGE=0" / "-DCOL_PACKED=0" (one copy of the histograms in LDS; equal bytes of
a group not merged; the apply pass's table as three byte tables), one process per library.
Then, without --passes-only, from the device: tests/golden/tennis25.npz under color_cases.plant_fade (both fades) through
video.restore_color -- automatic levels, frame 0 or frame 12 with its clean version as the only key -- in dB against the clean
video, and the clean video through automatic levels.  One JSON line each."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def device(rounds, passes_only):
    import torch
    from e2fgvi_amd import lib, ops, video
    from tests import color_cases as C
    dev = torch.device("cuda:0")

    def stats(v):
        v = np.array(v)
        return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}

    def timed_in_turn(fns):
        """every function warmed, then `rounds` rounds that run each once, in turn"""
        for fn in fns.values():
            fn()
        ms = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return ms

    L, W, H = 60, 1920, 1080
    tennis = C.tennis25(ROOT)
    big = video.resize_frames(tennis, (W, H), device=dev)
    natural = torch.cat([big, big, big[:L - 2 * len(big)]]).contiguous()
    del big
    flat = torch.full((L, H, W, 3), 128, dtype=torch.uint8, device=dev)
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    starts = torch.tensor([0, L], dtype=torch.int32, device=dev)
    ids = torch.arange(L, dtype=torch.int32, device=dev)
    mode = torch.ones(1, dtype=torch.int32, device=dev)
    out = torch.empty_like(flat)
    chist = torch.empty((L, 3, 256), dtype=torch.int32, device=dev)
    fhist = torch.empty((L, 256), dtype=torch.int32, device=dev)
    med =lambda v: float(np.median(v))
    rate = lambda b, v: round(b / (med(v) * 1e-3) / 1e12, 3)
    for name, src in (("natural", natural), ("flat", flat)):
        ops.color_hist(src, out=chist)
        Q = ops.color_nodes(chist, starts, ids)
        lut = ops.color_lut(Q, mode)
        ops.flicker_hist(src, out=fhist)
        _, d = ops.flicker_curves(fhist, scene, H * W, video.FLICKER_SPAN, video.FLICKER_MAX_SHIFT)
        # a clip of frames as the tool's own check sees it
        plan = video._check_restore_color_args(src, None, None, None, "levels", video.COLOR_CLIP, None, video.COLOR_MIN_RANGE,
                                               video.COLOR_MAX_GAIN, video.COLOR_STRENGTH, False)
        t = timed_in_turn({
            "color_hist": lambda: ops.color_hist(src, out=chist),
            "flicker_hist": lambda: ops.flicker_hist(src, out=fhist),
            "color_nodes": lambda: ops.color_nodes(chist, starts, ids),
            "color_lut": lambda: ops.color_lut(Q, mode),
            "flicker_curves": lambda: ops.flicker_curves(fhist, scene, H * W, video.FLICKER_SPAN, video.FLICKER_MAX_SHIFT),
            "color_apply": lambda: ops.color_apply(src, lut, scene, out=out),
            "flicker_apply": lambda: ops.flicker_apply(src, d, out=out),
            "restore_color": lambda: video._restore_color_device(src, None, plan),
            "deflicker": lambda: video._deflicker_device(src, np.zeros(L, np.int32), video.FLICKER_SPAN, video.FLICKER_MAX_SHIFT)})
        b_hist, b_apply = 3 * L * H * W, 6 * L * H * W
        rec = {"video": name, "size": "%dx%d" % (W, H), "frames": L, "rounds": rounds, "library": os.path.basename(lib.LIB_PATH),
               "bins_used_frame0": [int((chist[0, c] != 0).sum()) for c in range(3)],
               "table_changes_a_byte": bool((lut.cpu() != torch.arange(256, dtype=torch.uint8)).any())}
        for k, v in t.items():
            rec[k + "_ms"] = stats(v)
        rec.update(hist_bytes=b_hist, apply_bytes=b_apply,
                   color_hist_TB_per_s=rate(b_hist, t["color_hist"]), flicker_hist_TB_per_s=rate(b_hist, t["flicker_hist"]),
                   color_apply_TB_per_s=rate(b_apply, t["color_apply"]), flicker_apply_TB_per_s=rate(b_apply, t["flicker_apply"]),
                   color_hist_over_flicker_hist=round(med(t["color_hist"]) / med(t["flicker_hist"]), 3),
                   color_apply_over_flicker_apply=round(med(t["color_apply"]) / med(t["flicker_apply"]), 3),
                   restore_color_over_deflicker=round(med(t["restore_color"]) / med(t["deflicker"]), 3))
        print(json.dumps(rec), flush=True)
    del flat, out, natural
    torch.cuda.empty_cache()
    if passes_only:
        return
    db = lambda a: round(C.psnr(a, tennis), 2)
    for fade, kw in C.FADES.items():
        faded = C.plant_fade(tennis, **kw)
        row = {"video": "tennis25 faded", "fade": fade, "faded_dB": db(faded)}
        got, luts = video.restore_color(faded, return_curves=True, device=dev)
        row["levels_dB"] = db(got)
        mono = bool((np.diff(luts.astype(np.int64), axis=-1) >= 0).all())
        for k in (0, 12):
            got, luts = video.restore_color(faded, graded=tennis[k:k + 1], keys=[k], return_curves=True, device=dev)
            row["key_%d_dB" % k] = db(got)
            row["key_%d_worst_frame_dB" % k] = round(min(C.psnr_frames(got, tennis)), 2)
            mono = mono and bool((np.diff(luts.astype(np.int64), axis=-1) >= 0).all())
        row["tables_monotone"] = mono
        print(json.dumps(row), flush=True)
    got = video.restore_color(tennis, device=dev)
    diff = np.abs(got.astype(np.int64) - tennis)
    print(json.dumps({"video": "tennis25 clean through automatic levels", "dB": db(got), "largest_change": int(diff.max()),
                      "bytes_changed_by_more_than_3": round(float((diff > 3).mean()), 4)}), flush=True)


if __name__ == "__main__":
    device(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 11, "--passes-only" in sys.argv)
