"""Film grain (video.match_grain, ops.grain_blocks, ops.grain_lut, ops.grain_apply, csrc/grain.hip): what the regrain step costs.

60 frames at 1920x1080 of a synthetic moving clip with Gaussian noise of sigma 4 on top, ``where`` a static rectangle the size of
a logo (160x90) and a quarter of the frame (960x540), hole = where, one scene:
    blocks_ms   the one launch of ops.grain_blocks over all frames (reads every frame byte and the hole plane)
    lut_ms      ops.grain_lut: the integer torch ops between the two launches, of which
    sort_ms     the one torch sort of the 6 x (blocks) int64 keys, timed alone on the same keys
    apply_ms    the one launch of ops.grain_apply, out of place (every byte is copied) and in place (a thread without a ``where``
                pixel is done after one dword)
each warmed, `rounds` repetitions between one pair of device events, mean / min / max per repetition; the bytes each launch must
move at the least (computed from the shapes) and the rate that makes; and beside them
    inpaint_s   video.inpaint_video(size=(432, 240), restore=True) of the synthetic-weights fp32 generator on the same frames and
                the same rectangle as mask: host clock around the call, after a warm call on 12 frames
One JSON line per measurement.
    python tools/grain_bench.py [rounds=10] [frames=60]"""
import importlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from e2fgvi_amd import ops, video
from e2fgvi_amd.synth import synth_clip, synth_state_dict

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
L = int(sys.argv[2]) if len(sys.argv) > 2 else 60
dev = torch.device("cuda:0")
W, H = 1920, 1080


def stats(v):
    v = np.array(v)
    return {"mean": round(float(v.mean()), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def timed(fn):
    """per-call milliseconds of fn over `rounds` repetitions, one pair of device events each, after one warm call"""
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


x, _ = synth_clip(1, L, H, W, seed=11, moving=True)
frames = ((x[0] * 0.5 + 0.5) * 255 + 4.0 * torch.randn(L, 3, H, W, generator=torch.Generator().manual_seed(5)))
frames = frames.round().clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()
del x
src = torch.from_numpy(frames).to(dev)
scene_of = torch.zeros(L, dtype=torch.int32, device=dev)
Hb, Wb = (H - 2) // 8, (W - 2) // 8

for name, (ww, wh) in (("logo 160x90", (160, 90)), ("quarter 960x540", (960, 540))):
    where = torch.zeros((L, H, W), dtype=torch.uint8, device=dev)
    y0, x0 = (H - wh) // 3, (W - ww) // 3
    where[:, y0:y0 + wh, x0:x0 + ww] = 1
    filled = src.clone()
    filled[:, y0:y0 + wh, x0:x0 + ww] = 128
    energy, band = ops.grain_blocks(src, where)
    lut, scale = ops.grain_lut(energy, band, scene_of, 1)
    keys = torch.cat([energy.to(torch.int64).reshape(-1)] * 2)
    out = torch.empty_like(filled)
    work = filled.clone()
    t_blocks = timed(lambda: ops.grain_blocks(src, where))
    t_lut = timed(lambda: ops.grain_lut(energy, band, scene_of, 1))
    t_sort = timed(lambda: keys.sort())
    t_apply = timed(lambda: ops.grain_apply(filled, where, lut, scene_of, 7, out=out))
    t_place = timed(lambda: ops.grain_apply(work, where, lut, scene_of, 7, out=work))
    n_where = int(where.sum())
    px = L * H * W
    b_blocks = px * 4 + L * Hb * Wb * 13                 # frames and hole read once, energy and band written
    b_apply = px * 7                                      # filled and where read, out written
    b_place = px + n_where * 6                            # where read; the pixels of where read and written
    rate = lambda b, ms: round(b / (float(np.mean(ms)) * 1e-3) / 1e12, 3)
    print(json.dumps({"size": "%dx%d" % (W, H), "frames": L, "where": name, "where_pixels_per_frame": n_where // L, "rounds": rounds,
                      "blocks_per_frame": Hb * Wb, "measured_blocks": int((band != 255).sum()),
                      "sigma_green_per_band": [round(float(v) * video._GRAIN_SIGMA_PER_SCALE, 2) for v in scale[0, :, 1].tolist()],
                      "blocks_ms": stats(t_blocks), "blocks_least_bytes": b_blocks, "blocks_TB_per_s": rate(b_blocks, t_blocks),
                      "lut_ms": stats(t_lut), "sort_ms": stats(t_sort), "sort_keys": int(keys.numel()),
                      "sort_share_of_lut": round(float(np.mean(t_sort)) / float(np.mean(t_lut)), 3),
                      "apply_ms": stats(t_apply), "apply_least_bytes": b_apply, "apply_TB_per_s": rate(b_apply, t_apply),
                      "apply_in_place_ms": stats(t_place), "apply_in_place_least_bytes": b_place,
                      "apply_in_place_TB_per_s": rate(b_place, t_place),
                      "regrain_ms": round(float(np.mean(t_blocks) + np.mean(t_lut) + np.mean(t_apply)), 4)}), flush=True)
    del where, filled, energy, band, lut, scale, keys, out, work
del src
torch.cuda.empty_cache()

net = importlib.import_module("model.e2fgvi_hq").InpaintGenerator()
net.load_state_dict(synth_state_dict("e2fgvi_hq", "stress", 0))
net = net.to(dev).eval()
for name, (ww, wh) in (("logo 160x90", (160, 90)), ("quarter 960x540", (960, 540))):
    masks = np.zeros((L, H, W), np.uint8)
    y0, x0 = (H - wh) // 3, (W - ww) // 3
    masks[:, y0:y0 + wh, x0:x0 + ww] = 255
    with torch.no_grad():
        video.inpaint_video(net, frames[:12], masks[:12], size=(432, 240), restore=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = video.inpaint_video(net, frames, masks, size=(432, 240), restore=True)
        torch.cuda.synchronize()
        inpaint_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        video.match_grain(frames, done, masks, device=dev)
        torch.cuda.synchronize()
        grain_s = time.perf_counter() - t0
    print(json.dumps({"size": "%dx%d" % (W, H), "frames": L, "mask": name, "inpaint_s": round(inpaint_s, 3),
                      "match_grain_with_upload_and_download_s": round(grain_s, 3)}), flush=True)
