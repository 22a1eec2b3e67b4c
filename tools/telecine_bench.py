"""Inverse telecine (video.inverse_telecine, video.detect_telecine, ops.telecine_scores, ops.field_weave, csrc/telecine.hip): what it
costs.

    python tools/telecine_bench.py [rounds=11]
60 video frames at 1920x1080, one scene: the 25 frames of tests/golden/tennis25.npz resized on the device
(video.resize_frames), repeated to 48 film frames and put through 3:2 pulldown, top field first (tests/telecine_cases.py).
    scores_ms            the memset and the one launch of ops.telecine_scores (reads every frame byte three times but for the
                         first and the last frame: 3 (3 L - 2) H W bytes)
    weave_ms             the one launch of ops.field_weave with the jobs of the plan, into a buffer that is there (reads and writes
                         3 n H W bytes each, n = 48); the upload of the jobs is inside
    interlace_scores_ms  ops.interlace_scores on the same frames (reads 6 (L - 1) H W bytes): unchanged code, a third of the sums
    hist_ms              ops.flicker_hist into a buffer that is there, on the same frames (reads 3 L H W bytes): unchanged code
    copy_ms              a device copy of the weave's bytes (Tensor.copy_ of n frames: reads and writes 3 n H W each)
each warmed; `rounds` rounds, and in every round each of them once, in this order, one pair of device events around each -- so the
passes alternate in one process: median / min / max, the bytes each has to move at the least over its median time, the scores
as a ratio to interlace_scores and to the histogram, the weave as a ratio to the copy.  One JSON line.  The library is the one
E2FGVI_LIB names, or the product build."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def device(rounds):
    import torch
    from e2fgvi_amd import lib, ops, video
    from tests import telecine_cases as C
    dev = torch.device("cuda:0")
    W, H, films = 1920, 1080, 48
    big = video.resize_frames(C.tennis25(ROOT), (W, H), device=dev)
    film = torch.cat([big, big])[:films]
    del big
    origin = torch.from_numpy(C.telecine_origin(films, True, 0)).to(dev)
    frames = film[origin[:, 0]].clone()
    frames[:, 1::2] = film[origin[:, 1]][:, 1::2]
    L = int(frames.shape[0])
    scene = torch.zeros(L, dtype=torch.int32, device=dev)
    out, plan = video.inverse_telecine(frames, return_plan=True)
    exact = bool(torch.equal(out, film))
    del film
    jobs, n = plan["source"], int(out.shape[0])
    spare = torch.empty_like(out)
    hist = torch.empty((L, 256), dtype=torch.int32, device=dev)
    passes = {
        "scores": lambda: ops.telecine_scores(frames, scene),
        "interlace_scores": lambda: ops.interlace_scores(frames, scene),
        "hist": lambda: ops.flicker_hist(frames, out=hist),
        "weave": lambda: ops.field_weave(frames, jobs, 0, out=out),
        "copy": lambda: spare.copy_(out),
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
    least = {"scores": 3 * (3 * L - 2) * H * W, "interlace_scores": 6 * (L - 1) * H * W, "hist": 3 * L * H * W, "weave": 6 * n * H * W,
             "copy": 6 * n * H * W}
    verdict, M, k, locks = video.detect_telecine(frames, return_scores=True)
    rec = {"video": "tennis25 under 3:2 pulldown, top field first", "size": "%dx%d" % (W, H), "frames": L, "frames_out": n, "rounds": rounds,
           "library": os.path.basename(lib.LIB_PATH), "verdict": verdict, "locks": locks, "film_frames_back_byte_for_byte": exact}
    for name, v in ms.items():
        rec[name + "_ms"] = {"median": round(med[name], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        rec[name + "_least_TB_per_s"] = round(least[name] / (med[name] * 1e-3) / 1e12, 3)
    rec["scores_over_interlace_scores"] = round(med["scores"] / med["interlace_scores"], 3)
    rec["scores_over_hist"] = round(med["scores"] / med["hist"], 3)
    rec["weave_over_copy"] = round(med["weave"] / med["copy"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    device(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 11)
