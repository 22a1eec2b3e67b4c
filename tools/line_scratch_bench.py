"""Line scratches (video.detect_line_scratches, ops.line_sums, ops.line_columns, ops.line_paint, csrc/line_scratch.hip): what the
detector costs, and what its defaults do on the host restatement.

    python tools/line_scratch_bench.py [rounds=11] [--no-inpaint]
100 frames at 432x240 and 60 frames at 1920x1080 of a synthetic moving clip with three planted scratches that wander as
x0 + round(1.5 sin(0.7 t + i)), the defaults, one scene:
    sums_ms      the one launch of ops.line_sums (reads every frame byte of a band once: 3 bytes per pixel at the least)
    columns_ms   the one launch of ops.line_columns over the L x nb x W sums
    paint_ms     the two launches of ops.line_paint: keep and counts over L x 2 x W, then every mask byte once (1 byte per pixel)
each warmed, `rounds` repetitions, one pair of device events around each: median / min / max per repetition, the bytes each must
move at the least (computed from the shapes) and the rate that makes; detect_ms the three calls in a row; and beside them
    inpaint_s    video.inpaint_video of the synthetic-weights fp32 generator on the same frames with the detected masks (at
                 1920x1080 with size=(432, 240), restore=True): host clock around the call and a synchronise, after a warm call
                 on 12 frames; detect_with_upload_and_download_s: numpy in, numpy out
One JSON line per size.  --no-inpaint leaves the generator out: the form to run under rocprofv3 --kernel-trace --stats, which gives
the four kernels' own times.

    python tools/line_scratch_bench.py --host
needs no device: the restatement of tests/line_scratch_cases.py at the defaults on the two clean videos (tau 4, 6, 8, 12), with three
planted scratches (seeds 0 to 5), with one 1-pixel scratch of amplitude 8 ... 24, the limits (a slowly moving bar, 40 % of the
height), and the cross-section test against the median of the side columns in place of their envelope."""
import importlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def host():
    from tests import line_scratch_cases as C

    def median_candidates(S, rows, tau, gap, side):
        """candidates_np with the median of the 2 side columns in the envelope's place"""
        S = S.astype(np.int64)
        m = gap + side
        xs = np.arange(m, S.shape[2] - m)
        med = np.median(np.stack([S[..., xs + s * d] for d in range(gap + 1, m + 1) for s in (-1, 1)]), axis=0)
        bits = np.zeros(S.shape, np.uint8)
        bits[..., xs] = (S[..., xs] > med + tau * rows) | ((S[..., xs] < med - tau * rows).astype(np.uint8) << 1)
        return bits

    d = C.DEFAULTS
    for which in ("translated", "raw"):
        fr = C.stats_video(ROOT, which)
        for tau in (4, 6, 8, 12):
            w = C.detect_np(fr, **dict(d, tau=tau))
            print(json.dumps({"video": which, "frames": len(fr), "tau": tau, "set_pixels": int((w["masks"] > 0).sum()),
                              "kept_columns": int(w["counts"].sum()), "columns_with_the_height": int(w["col"].sum()),
                              "band_candidates": int((w["cand"] > 0).sum())}), flush=True)
        S = C.sums_np(fr, d["rows"])
        _, _, col, b0, b1 = C.columns_np(median_candidates(S, d["rows"], d["tau"], d["gap"], d["side"]), d["drift"], d["coverage"])
        keep, counts = C.keep_np(col, C.scene_of_np(len(fr)), d["drift"], d["span"], d["persist"])
        masks = C.paint_np(keep, b0, b1, fr.shape[1], d["rows"], d["radius"])
        print(json.dumps({"video": which, "form": "median of the sides", "tau": d["tau"], "set_pixels": int((masks > 0).sum()),
                          "kept_columns": int(counts.sum()), "columns_with_the_height": int(col.sum())}), flush=True)
        runs = []
        for seed in range(6):
            planted, marks = C.plant(fr, seed)
            recall, strays = C.recall_and_strays(C.detect_np(planted, **d)["masks"], marks)
            runs.append((round(recall, 4), strays))
        print(json.dumps({"video": which, "planted": "3 scratches, seeds 0-5", "recall": [r for r, _ in runs],
                          "set_pixels_beyond_4_columns": [s for _, s in runs]}), flush=True)
        for amp in (8, 12, 16, 24):
            planted, marks = C.plant(fr, 0, n=1, amplitude=amp, width=1)
            m = C.detect_np(planted, **d)["masks"]
            print(json.dumps({"video": which, "planted": "one 1-pixel scratch", "amplitude": amp,
                              "frames_masked": int(m.reshape(len(fr), -1).any(axis=1).sum()), "frames": len(fr)}), flush=True)
    fr = C.stats_video(ROOT, "translated")
    for step in (1, 2, 3, 4, 6):                          # a 3-pixel bright bar over the full height that moves `step` px per frame
        bar = fr.astype(np.int64)
        for t in range(len(fr)):
            bar[t, :, 100 + step * t:103 + step * t] += 40
        m = C.detect_np(np.clip(bar, 0, 255).astype(np.uint8), **d)["masks"]
        print(json.dumps({"limit": "3-pixel bar moving", "px_per_frame": step,
                          "frames_masked": int(m.reshape(len(fr), -1).any(axis=1).sum()), "frames": len(fr)}), flush=True)
    for share in (0.4, 0.5, 0.6):
        part = fr.astype(np.int64)
        part[:, :int(round(share * fr.shape[1])), 200] += 40
        m = C.detect_np(np.clip(part, 0, 255).astype(np.uint8), **d)["masks"]
        print(json.dumps({"limit": "scratch over a share of the height", "share": share, "set_pixels": int((m > 0).sum())}), flush=True)


def device(rounds):
    import torch
    from e2fgvi_amd import ops, video
    from e2fgvi_amd.synth import synth_clip, synth_state_dict
    dev = torch.device("cuda:0")
    d = dict(rows=video.LINE_ROWS, tau=video.LINE_TAU, gap=video.LINE_GAP, side=video.LINE_SIDE, drift=video.LINE_DRIFT,
             coverage=video.LINE_COVERAGE, span=video.LINE_SPAN, persist=video.LINE_PERSIST, radius=video.LINE_RADIUS)

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

    net = None
    if "--no-inpaint" not in sys.argv:
        net = importlib.import_module("model.e2fgvi_hq").InpaintGenerator()
        net.load_state_dict(synth_state_dict("e2fgvi_hq", "stress", 0))
        net = net.to(dev).eval()
    for L, W, H in ((100, 432, 240), (60, 1920, 1080)):
        x, _ = synth_clip(1, L, H, W, seed=11, moving=True)
        g = ((x[0] * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.int16).permute(0, 2, 3, 1).contiguous()
        del x
        for i, (x0, amp) in enumerate(((W // 5, 40), (W // 2, -45), (4 * W // 5, 30))):
            for t in range(L):
                g[t, :, x0 + int(round(1.5 * np.sin(0.7 * t + i)))] += amp
        frames = g.clamp(0, 255).to(torch.uint8).numpy()
        del g
        src = torch.from_numpy(frames).to(dev)
        scene = torch.zeros(L, dtype=torch.int32, device=dev)
        S = ops.line_sums(src, d["rows"])
        cand, cnt, col, b0, b1 = ops.line_columns(S, d["rows"], d["tau"], d["gap"], d["side"], d["drift"], d["coverage"])
        out = torch.empty((L, H, W), dtype=torch.uint8, device=dev)
        paint = lambda: ops.line_paint(col, b0, b1, scene, H, d["rows"], d["drift"], d["span"], d["persist"], d["radius"], out=out)
        keep, counts, masks = paint()
        t_sums = timed(lambda: ops.line_sums(src, d["rows"]))
        t_cols = timed(lambda: ops.line_columns(S, d["rows"], d["tau"], d["gap"], d["side"], d["drift"], d["coverage"]))
        t_paint = timed(paint)
        t_all = timed(lambda: video._detect_line_scratches_device(src, np.zeros(L, np.int32), *d.values()))
        nb = H // d["rows"]
        b_sums = L * nb * d["rows"] * W * 3                # the bytes of the bands; S written on top: L nb W 4
        b_paint = L * H * W
        rate = lambda b, ms: round(b / (float(np.median(ms)) * 1e-3) / 1e12, 3)
        rec = {"size": "%dx%d" % (W, H), "frames": L, "rounds": rounds, "settings": d, "kept_columns_per_frame": counts[:4].tolist(),
               "mask_share": round(float((masks != 0).float().mean()), 5),
               "sums_ms": stats(t_sums), "sums_least_bytes": b_sums, "sums_TB_per_s": rate(b_sums, t_sums),
               "columns_ms": stats(t_cols), "columns_values": L * nb * W,
               "paint_ms": stats(t_paint), "paint_least_bytes": b_paint, "paint_TB_per_s": rate(b_paint, t_paint),
               "detect_ms": stats(t_all)}
        if net is None:
            print(json.dumps(rec), flush=True)
            continue
        del S, cand, cnt, col, b0, b1, out, keep, src
        torch.cuda.empty_cache()
        m = masks.cpu().numpy()
        kw = dict(size=(432, 240), restore=True) if W > 432 else {}
        with torch.no_grad():
            video.inpaint_video(net, frames[:12], m[:12], **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            video.inpaint_video(net, frames, m, **kw)
            torch.cuda.synchronize()
            rec["inpaint_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            video.detect_line_scratches(frames, device=dev)
            rec["detect_with_upload_and_download_s"] = round(time.perf_counter() - t0, 4)
        rec["detect_share_of_inpaint"] = round(float(np.median(t_all)) * 1e-3 / rec["inpaint_s"], 5)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if "--host" in sys.argv:
        host()
    else:
        device(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 11)
