"""Local deflicker (video.deflicker_local, ops.flicker_local_hist, ops.flicker_local_curves, ops.flicker_local_apply,
csrc/flicker_local.hip): what it costs beside the global deflicker of the same tree, and what it does to planted flicker.

    python tools/flicker_local_bench.py [rounds=11]
60 frames at 1920x1080, the defaults, one scene, the "natural" video of tools/flicker_bench.py -- the 25 frames of
tests/golden/tennis25.npz resized on the device and repeated -- and a "flat" one, mid grey everywhere.  In ONE process, per round
one after the other: the three global passes (ops.flicker_hist, ops.flicker_curves, ops.flicker_apply) and the three local passes
at grids (2,2) and (3,4), each call between a pair of device events after a warm-up round; median / min / max over the rounds.
    hist     reads every frame byte once: 3 L H W bytes
    curves   L (gy gx) rows of 256 counts, each workgroup over its window
    apply    reads and writes 6 L H W bytes, into a buffer that is there
and the ratio of every local median to its global counterpart of the same run, which is the yardstick.  Then, from the device:
tennis25 under flicker_local_cases.plant_tilted (seeds 1, 2) through video.deflicker and video.deflicker_local at (2,2) and (3,4)
-- block_roughness before and after -- and the clean clip through grids (1,1), (2,2), (3,4), (4,6): the share of pixels changed by
more than 3 levels, the largest change, the PSNR.  One JSON line each."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

GRIDS = ((2, 2), (3, 4))


def device(rounds):
    import torch
    from e2fgvi_amd import ops, video
    from tests import flicker_cases as C
    from tests import flicker_local_cases as LC
    dev = torch.device("cuda:0")
    span, max_shift = video.FLICKER_SPAN, video.FLICKER_MAX_SHIFT

    def stats(v):
        v = np.array(v)
        return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}

    def once(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    L, W, H = 60, 1920, 1080
    tennis = C.tennis25(ROOT)
    big = video.resize_frames(tennis, (W, H), device=dev)
    natural = torch.cat([big, big, big[:L - 2 * len(big)]]).contiguous()
    del big
    flat = torch.full((L, H, W, 3), 128, dtype=torch.uint8, device=dev)
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    out = torch.empty_like(flat)
    rate = lambda b, ms: round(b / (ms * 1e-3) / 1e12, 3)
    b_hist, b_apply = 3 * L * H * W, 6 * L * H * W
    for name, src in (("natural", natural), ("flat", flat)):
        hist = ops.flicker_hist(src)
        _, d = ops.flicker_curves(hist, scene, H * W, span, max_shift)
        calls = {("global", "hist"): lambda: ops.flicker_hist(src, out=hist),
                 ("global", "curves"): lambda: ops.flicker_curves(hist, scene, H * W, span, max_shift),
                 ("global", "apply"): lambda: ops.flicker_apply(src, d, out=out)}
        held = {}
        for g in GRIDS:
            hl = ops.flicker_local_hist(src, g)
            _, dl = ops.flicker_local_curves(hl, scene, H, W, span, max_shift)
            held[g] = (hl, dl)
            calls[(g, "hist")] = lambda g=g: ops.flicker_local_hist(src, g, out=held[g][0])
            calls[(g, "curves")] = lambda g=g: ops.flicker_local_curves(held[g][0], scene, H, W, span, max_shift)
            calls[(g, "apply")] = lambda g=g: ops.flicker_local_apply(src, held[g][1], out=out)
        ms = {k: [] for k in calls}
        for r in range(rounds + 1):                    # the first round warms every call up; then alternating, round by round
            for k, fn in calls.items():
                t = once(fn)
                if r:
                    ms[k].append(t)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for who in ("global",) + GRIDS:
            rec = {"video": name, "size": "%dx%d" % (W, H), "frames": L, "rounds": rounds, "span": span, "max_shift": max_shift,
                   "passes": "global" if who == "global" else "local %dx%d" % who}
            for p, b in (("hist", b_hist), ("curves", None), ("apply", b_apply)):
                rec[p + "_ms"] = stats(ms[(who, p)])
                if b:
                    rec[p + "_TB_per_s"] = rate(b, med[(who, p)])
                if who != "global":
                    rec[p + "_over_global"] = round(med[(who, p)] / med[("global", p)], 3)
            rec["sum_ms"] = round(sum(med[(who, p)] for p in ("hist", "curves", "apply")), 4)
            print(json.dumps(rec), flush=True)
    del natural, flat, out
    torch.cuda.empty_cache()
    print(json.dumps({"video": "tennis25 clean", "block_roughness": round(LC.block_roughness(tennis), 4)}), flush=True)
    for seed in (1, 2):
        planted = LC.plant_tilted(tennis, seed)
        glob = LC.block_roughness(video.deflicker(planted, device=dev))
        row = {"video": "tennis25 plant_tilted", "seed": seed, "block_roughness": round(LC.block_roughness(planted), 4),
               "global": round(glob, 4)}
        for g in GRIDS:
            after = LC.block_roughness(video.deflicker_local(planted, grid=g, device=dev))
            row["local %dx%d" % g] = {"block_roughness": round(after, 4), "over_global": round(after / glob, 4)}
        print(json.dumps(row), flush=True)
    for g in ((1, 1), (2, 2), (3, 4), (4, 6)):
        got = video.deflicker_local(tennis, grid=g, device=dev).astype(np.int64)
        diff = np.abs(got - tennis).max(axis=-1)
        mse = float(((got - tennis) ** 2).mean())
        print(json.dumps({"video": "tennis25 clean through deflicker_local", "grid": list(g),
                          "changed_by_more_than_3": round(float((diff > 3).mean()), 4), "largest_change": int(diff.max()),
                          "psnr_dB": round(10 * np.log10(255.0 ** 2 / mse), 2) if mse else None}), flush=True)


if __name__ == "__main__":
    device(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 11)
