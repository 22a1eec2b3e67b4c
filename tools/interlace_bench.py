"""Deinterlacer (video.deinterlace, video.detect_interlace, ops.deinterlace, ops.interlace_scores, csrc/interlace.hip): what it costs.

    python tools/interlace_bench.py [rounds=11]
60 interlaced frames at 1920x1080, one scene: the 25 frames of tests/golden/tennis25.npz resized on the device
(video.resize_frames), repeated to 120 and woven pair by pair, top field first.
    scores_ms        the memset and the one launch of ops.interlace_scores (reads every frame byte twice: 6 (L - 1) H W bytes)
    field_ms         the one launch of ops.deinterlace at field rate with the defaults, into a buffer that is there (writes 6 L H W
                     bytes; by traffic alone it reads 3 L H W -- every frame once -- and at most 9 L H W, every frame as P, C and N)
    frame_ms         the same at frame rate, the first field kept (writes 3 L H W)
    field_noguard_ms, field_edges2_ms   field rate with guard=False, and with edges=2 (the byte-load path of the direction search)
    hist_ms          ops.flicker_hist into a buffer that is there, on the same frames (reads 3 L H W bytes): the yardstick for scores_ms
    flicker_apply_ms ops.flicker_apply on the same frames (reads 3 L H W, writes 3 L H W): the yardstick for the fields pass
each warmed; `rounds` rounds, and in every round each of them once, in this order, one pair of device events around each -- so the
passes alternate in one process: median / min / max, each pass as a ratio to the two yardsticks, and the bytes it has to move at
the least (reads of every frame once, twice for the scores, plus the writes) over its median time.  One JSON line.  The library
is the one E2FGVI_LIB names, or the product build."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def device(rounds):
    import torch
    from e2fgvi_amd import lib, ops, video
    from tests import interlace_cases as C
    dev = torch.device("cuda:0")
    L, W, H = 60, 1920, 1080
    big = video.resize_frames(C.tennis25(ROOT), (W, H), device=dev)
    src = torch.cat([big] * 5)[:2 * L]
    del big
    frames = src[0::2].clone()
    frames[:, 1::2] = src[1::2, 1::2]
    del src
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    field = torch.empty((2 * L, H, W, 3), dtype=torch.uint8, device=dev)
    frame = torch.empty((L, H, W, 3), dtype=torch.uint8, device=dev)
    hist = torch.empty((L, 256), dtype=torch.int32, device=dev)
    ops.flicker_hist(frames, out=hist)
    _, d = ops.flicker_curves(hist, scene, H * W, 4, 32)
    passes = {
        "scores": lambda: ops.interlace_scores(frames, scene),
        "hist": lambda: ops.flicker_hist(frames, out=hist),
        "field": lambda: ops.deinterlace(frames, scene, True, 0, True, 0, out=field),
        "flicker_apply": lambda: ops.flicker_apply(frames, d, out=frame),
        "frame": lambda: ops.deinterlace(frames, scene, True, 1, True, 0, out=frame),
        "field_noguard": lambda: ops.deinterlace(frames, scene, True, 0, False, 0, out=field),
        "field_edges2": lambda: ops.deinterlace(frames, scene, True, 0, True, 2, out=field),
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
    least = {"scores": 6 * (L - 1) * H * W, "hist": 3 * px, "field": 9 * px, "flicker_apply": 6 * px, "frame": 6 * px,
             "field_noguard": 9 * px, "field_edges2": 9 * px}
    verdict, D, votes = video.detect_interlace(frames, return_scores=True)
    rec = {"video": "tennis25 woven, top field first", "size": "%dx%d" % (W, H), "frames": L, "rounds": rounds,
           "library": os.path.basename(lib.LIB_PATH), "verdict": verdict, "votes_plus_minus": [int((votes == 1).sum()), int((votes == -1).sum())]}
    for k, v in ms.items():
        rec[k + "_ms"] = {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        rec[k + "_least_TB_per_s"] = round(least[k] / (med[k] * 1e-3) / 1e12, 3)
    for k in ("scores", "field", "frame", "field_noguard", "field_edges2"):
        rec[k + "_over_hist"] = round(med[k] / med["hist"], 3)
        rec[k + "_over_flicker_apply"] = round(med[k] / med["flicker_apply"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    device(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 11)
