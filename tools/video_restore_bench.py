"""Device cost of the paste-back at source size (video.restore_frames: csrc/video.hip restore_u8_kernel) against the composition
of the package's other public pieces that computes the same bytes: the two resample_u8 passes of video.resize_frames up to the
source size, the mask gathered through the two NEAREST tables, torch.where.  432x240 -> 1920x1080, the tennis masks (dilated as
the driver dilates them) tiled over L frames; everything on the device and every table uploaded before the clock starts.  The
feathered paste (feather=4 and 16, fused_f4 / fused_f16) runs beside them, and composed_f4, the same bytes from torch: max_pool2d
for the dilation, an integer box sum (cumulative sums) for c and n, int64 arithmetic for the blend.  The
arms alternate in one process, one pair of events per call; prints one JSON line per arm (mean / min / max ms over the rounds,
bytes each arm moves by its shapes, the 2 L H W 3 floor, the time over the `fused` arm's) and checks once that the fused and the
composed arm of each paste return the same bytes.
    python tools/video_restore_bench.py [L=50] [rounds=20]"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from e2fgvi_amd import ops, video

L = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
(w, h), (W, H) = (432, 240), (1920, 1080)
dev = torch.device("cuda:0")
raw = np.load(os.path.join(ROOT, "tests", "golden", "tennis25.npz"))["masks_raw"]
raw = np.concatenate([raw] * (L // len(raw) + 1))[:L]
m = video.prepare_masks(raw, (h, w), dev)
g = torch.Generator(device=dev).manual_seed(0)
lo = torch.randint(0, 256, (L, h, w, 3), dtype=torch.uint8, device=dev, generator=g)
src = torch.randint(0, 256, (L, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
t = lambda a: torch.from_numpy(a).to(dev)
ytab, xtab = t(video.nearest_table(h, H)), t(video.nearest_table(w, W))
bx, cx = (t(a) for a in video.bicubic_tables(w, W))
by, cy = (t(a) for a in video.bicubic_tables(h, H))
yl, xl = ytab.long(), xtab.long()


def fused():
    return ops.restore_u8(lo, m, src, ytab, xtab, bx, cx, by, cy)


def composed():
    up = ops.resample_u8(ops.resample_u8(lo, W, 2, bx, cx), H, 1, by, cy)
    M = m.index_select(1, yl).index_select(2, xl)
    return torch.where(M[..., None] != 0, up, src)


def fused_f4():
    return ops.restore_u8(lo, m, src, ytab, xtab, bx, cx, by, cy, feather=4)


def fused_f16():
    return ops.restore_u8(lo, m, src, ytab, xtab, bx, cx, by, cy, feather=16)


def _box_sum(a, r):
    """sum over the (2r+1) x (2r+1) window of int32 [L,H,W], zeros outside"""
    for axis in (2, 1):
        pad = [0, 0, 0, 0]
        pad[(2 - axis) * 2], pad[(2 - axis) * 2 + 1] = r + 1, r
        c = torch.cumsum(torch.nn.functional.pad(a, pad), axis)
        n = a.shape[axis]
        a = c.narrow(axis, 2 * r + 1, n) - c.narrow(axis, 0, n)
    return a


def composed_f4(r=4):
    up = ops.resample_u8(ops.resample_u8(lo, W, 2, bx, cx), H, 1, by, cy)
    M = m.index_select(1, yl).index_select(2, xl)
    D = torch.nn.functional.max_pool2d((M != 0).half()[:, None], 2 * r + 1, 1, r)[:, 0]
    c = _box_sum(D.int(), r).long()[..., None]
    n = _box_sum(torch.ones((1, H, W), dtype=torch.int32, device=dev), r).long()[..., None]
    return ((c * up.long() + (n - c) * src.long() + n // 2) // n).to(torch.uint8)


arms = (("fused", fused), ("composed", composed), ("fused_f4", fused_f4), ("fused_f16", fused_f16), ("composed_f4", composed_f4))
for _, fn in arms:
    for _ in range(3):
        out = fn()
torch.cuda.synchronize()
same = bool(torch.equal(fused(), composed())) and bool(torch.equal(fused_f4(), composed_f4()))
ms = {name: [] for name, _ in arms}
for _ in range(rounds):
    for name, fn in arms:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1))
        del out
full, small = L * H * W * 3, L * h * w * 3
floor = 2 * full
nbytes = {
    # reads src and writes out once (tiles with a hole read src too), reads lo and the mask once
    "fused": 2 * full + small + small // 3,
    "fused_f4": 2 * full + small + small // 3,
    "fused_f16": 2 * full + small + small // 3,
    # W pass: lo -> [L,h,W,3]; H pass: that -> [L,H,W,3]; mask rows, then columns; the compare's bool; where reads mask, up, src
    "composed": (small + L * h * W * 3) + (L * h * W * 3 + full) + (L * h * w + L * H * w) + (L * H * w + L * H * W)
                + 2 * L * H * W + (L * H * W + 2 * full + full),
    # composed's resize and mask gather; M != 0 -> half, the pool, -> int32; two cumulative sums and two differences of int32; c and
    # n as int64; up and src as int64; five int64 elementwise passes over [L,H,W,3]; the uint8 result
    "composed_f4": (small + L * h * W * 3) + (L * h * W * 3 + full) + (L * h * w + L * H * w) + (L * H * w + L * H * W)
                   + L * H * W * (1 + 2 + 2 + 2 + 2 + 4) + 4 * 2 * 4 * L * H * W + 12 * L * H * W + 2 * 9 * full
                   + 5 * 3 * 8 * full + 9 * full,
}
coverage = float(m.float().mean())
base = float(np.mean(ms["fused"]))
for name, _ in arms:
    v = np.array(ms[name])
    print(json.dumps({"arm": name, "frames": L, "lo": "%dx%d" % (w, h), "src": "%dx%d" % (W, H), "mask_coverage": round(coverage, 4),
                      "rounds": rounds, "ms_mean": round(float(v.mean()), 4), "ms_min": round(float(v.min()), 4),
                      "ms_max": round(float(v.max()), 4), "ms_std": round(float(v.std()), 4), "bytes": nbytes[name],
                      "bytes_over_floor": round(nbytes[name] / floor, 3), "GB_per_s": round(nbytes[name] / v.mean() / 1e6, 1),
                      "floor_GB_per_s": round(floor / v.mean() / 1e6, 1), "over_fused": round(float(v.mean()) / base, 3),
                      "arms_equal": same}), flush=True)
if not same:
    sys.exit("a fused arm and its composed arm disagree")
