"""The dust-and-dirt detector (video.detect_defects, ops.defect_candidates / defect_clean, csrc/defects.hip): what its pieces cost.

For 100 frames at 432x240 and 60 frames at 1920x1080, every frame with both neighbours a centre frame:
  video      a smooth synthetic texture under a drift of up to 3 px per frame with a little noise, 30 planted blotches per 432x240
             of frame area; GIVEN flows: the drift itself, exact (built on the device)
  kernels    the candidate launch and the cleaning launch at detect_defects' defaults, each between its own pair of device events,
             warmed, the arms alternating; with csrc/libe2fgvi_hip_luma.so present (build.build_variant("luma",
             "-DE2_DEFECT_BPP=1")) a third arm runs the candidate kernel on a ready-made luma plane -- the 1-byte gathers of the form
             that was not kept -- and must leave the same bytes; `plane_copy_ms` is a device copy of the RGB frames (6 bytes per
             pixel moved), an upper bound for the pass that would make that plane (4 bytes per pixel)
  traffic    achieved bytes/s against the least traffic per pixel of a centre frame: candidates 3 (centre RGB) + 2 x 8 (flows) + 1
             (written) = 20 bytes with the envelope bytes taken as L2-resident; cleaning 1 + 1 = 2 bytes
  flows      the share of metrics.video_flows in a whole detect_defects call with the synthetic-weights fp32 generator: host clock
             around each and a synchronise, after a warm call on three frames; the two alternate three times and the first pass
             (which fills the allocator's cache) is left out: the smaller of the other two each
One JSON line per size.
    python tools/defects_bench.py [rounds=7] > profiles/defects.txt"""
import ctypes as C
import importlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from e2fgvi_amd import lib, metrics, ops, video
from e2fgvi_amd.synth import synth_state_dict

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda:0")
LUMA_LIB = os.path.join(ROOT, "e2fgvi_amd", "csrc", "libe2fgvi_hip_luma.so")


def make_video(L, H, W, seed):
    """(frames uint8 [L,H,W,3], fwd, bwd) on the device"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    drift = torch.cumsum((r(L, 2) - 0.5) * 6, 0).to(dev)                # c_t: frame t shows the texture at p + c_t
    ys = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xs = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    waves = [(float(a), float(lam), float(ph)) for a, lam, ph in zip(r(6) * 6.2832, 8 + r(6) * 52, r(6) * 6.2832)]
    frames = torch.empty((L, H, W, 3), dtype=torch.uint8, device=dev)
    for t in range(L):
        u, v = xs + drift[t, 0], ys + drift[t, 1]
        tex = sum(torch.sin((np.cos(a) * u + np.sin(a) * v) * 6.2832 / lam + ph) for a, lam, ph in waves) * (50.0 / 3) + 128
        noise = (torch.rand((H, W, 3), generator=g) * 5 - 2).to(dev)
        frames[t] = (tex[..., None] + noise + torch.tensor([4.0, 0.0, -6.0], device=dev)).round().clamp(0, 255).to(torch.uint8)
    rng = np.random.RandomState(seed)
    for t in range(L):
        for _ in range(max(1, 30 * H * W // (432 * 240))):
            h, w = rng.randint(2, 8, 2)
            y, x = rng.randint(0, H - h), rng.randint(0, W - w)
            frames[t, y:y + h, x:x + w] = 235 if rng.rand() < 0.5 else 20
    d = (drift[:-1] - drift[1:])[:, None, None, :]                      # fwd[t] = c_t - c_{t+1}
    fwd = d.expand(L - 1, H, W, 2).contiguous()
    return frames, fwd, (-fwd).contiguous()


def stats(v):
    v = np.array(v)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def luma_entry():
    if not os.path.exists(LUMA_LIB):
        return None
    fn = C.CDLL(LUMA_LIB).e2fgvi_defect_candidates
    fn.restype, fn.argtypes = lib.SYMBOLS["e2fgvi_defect_candidates"]
    return fn


net = importlib.import_module("model.e2fgvi").InpaintGenerator()
net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
net = net.to(dev).eval()
luma_fn = luma_entry()
S = dict(threshold=video.DEFECT_THRESHOLD, slack=video.DEFECT_SLACK, support=video.DEFECT_SUPPORT, radius=video.DEFECT_RADIUS)

for (W, H, L) in ((432, 240, 100), (1920, 1080, 60)):
    frames, fwd, bwd = make_video(L, H, W, 5)
    ids = video.plan_defect_frames(L)
    ids_d = torch.tensor(ids, dtype=torch.int32).to(dev)
    px = len(ids) * H * W
    cand = torch.zeros((L, H, W), dtype=torch.uint8, device=dev)
    cand_luma = torch.zeros_like(cand)
    masks = torch.zeros_like(cand)
    f = frames.to(torch.int32)
    plane = ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).to(torch.uint8).contiguous()
    del f
    spare = torch.empty_like(frames)
    counts = [None]

    def arm_candidates():
        ops.defect_candidates(frames, fwd, bwd, ids_d, S["threshold"], S["slack"], out=cand)

    def arm_clean():
        counts[0] = ops.defect_clean(cand, ids_d, S["support"], S["radius"], out=masks)[1]

    def arm_luma():
        lib.check(luma_fn(ops._ptr(plane), ops._ptr(fwd), ops._ptr(bwd), ops._ptr(ids_d), len(ids), L, H, W, S["threshold"], S["slack"],
                          ops._ptr(cand_luma), ops._stream()), "defect_candidates (luma build)")

    def arm_copy():
        spare.copy_(frames)

    arms = {"candidates": arm_candidates, "clean": arm_clean, "plane_copy": arm_copy}
    if luma_fn is not None:
        arms["candidates_luma_plane"] = arm_luma
    ms = {k: [] for k in arms}
    for r in range(rounds + 2):                          # rounds 0 and 1 warm every arm
        for k, fn in arms.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r > 1:
                ms[k].append(e0.elapsed_time(e1))
    same = None if luma_fn is None else bool(torch.equal(cand, cand_luma))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    del spare, plane, cand_luma
    torch.cuda.empty_cache()

    with torch.no_grad():
        small = frames[:3].contiguous()
        video._detect_defects_device(net, small, [1], None, None, max_fraction=video.DEFECT_MAX_FRACTION, **S)
        flows_all, whole_all = [], []
        for _ in range(3):                               # alternating; the first pass also fills the allocator's cache
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nf, nb = metrics.video_flows(net, frames)
            torch.cuda.synchronize()
            flows_all.append(time.perf_counter() - t0)
            del nf, nb
            t0 = time.perf_counter()
            m, n = video._detect_defects_device(net, frames, ids, None, None, max_fraction=video.DEFECT_MAX_FRACTION, **S)
            torch.cuda.synchronize()
            whole_all.append(time.perf_counter() - t0)
            del m, n
        flows_s, whole_s = min(flows_all[1:]), min(whole_all[1:])
    print(json.dumps({"size": "%dx%d" % (W, H), "frames": L, "centre_frames": len(ids), "rounds": rounds, "settings": S,
                      "ms": {k: stats(v) for k, v in ms.items()},
                      "us_per_centre_frame": {k: round(med[k] * 1e3 / len(ids), 2) for k in ("candidates", "clean")},
                      "least_bytes": {"candidates": 20 * px, "clean": 2 * px},
                      "achieved_GBps_of_least": {"candidates": round(20 * px / med["candidates"] / 1e6, 1),
                                                 "clean": round(2 * px / med["clean"] / 1e6, 1),
                                                 "plane_copy": round(6 * L * H * W / med["plane_copy"] / 1e6, 1)},
                      "luma_plane_same_bytes": same,
                      "candidate_share": round(float(cand[ids_d.long()].float().mean()), 6),
                      "mask_share": round(float(counts[0].sum()) / px, 6),
                      "flows_s": round(flows_s, 4), "detect_defects_s": round(whole_s, 4),
                      "flows_s_all": [round(v, 4) for v in flows_all], "detect_defects_s_all": [round(v, 4) for v in whole_all],
                      "flows_share_of_detect_defects": round(flows_s / whole_s, 4)}), flush=True)
    if same is False:
        sys.exit("the luma-plane build leaves other bytes than the product")
    del frames, fwd, bwd, cand, masks
    torch.cuda.empty_cache()
