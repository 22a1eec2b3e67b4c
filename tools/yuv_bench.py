"""The pixel-format kernels (ops.yuv420_to_rgb / ops.rgb_to_yuv420, csrc/yuv.hip) beside two yardsticks, on the same tensors in one
process: L frames of 1920x1080 NV12, bt709 limited range, "left" chroma.

    decode          [L,3H/2,W] -> [L,H,W,3]: one launch; reads 1.5 and writes 3 bytes per pixel
    encode          [L,H,W,3] -> [L,3H/2,W]: one launch; reads 3 and writes 1.5 bytes per pixel
    paste           the same launch with like / like_rgb: reads 3 + 3 + 1.5 and writes 1.5 bytes per pixel
    copy_4.5 / _9   a device-to-device copy (Tensor.copy_) that moves as many bytes as the kernel beside it reads + writes
    torch_decode    the float torch expression a caller of the RGB-only driver writes today: planes to float, bilinear chroma,
    torch_encode    the 3x3 matrix, round, clamp, to uint8 (and the way back with a 2x2 mean) -- several passes over the frames

All warmed, alternating over `rounds`, `calls` launches between two device events (windows of 20 ms and more); effective GB/s =
(bytes read + written by the definition) / time.  One JSON line per arm and a table.
    python tools/yuv_bench.py [L=60] [rounds=5]"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F
from e2fgvi_amd import ops, video

L = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
H, W = 1080, 1920
dev = torch.device("cuda:0")
fmt = video.yuv_format()
dec, enc = video.yuv_coefficients(fmt.matrix, fmt.full_range)
dec, enc = dec + (16,), enc + (16,)
px = L * H * W

g = torch.Generator(device="cpu").manual_seed(1)
ys = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
xs = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
ph = torch.rand(L, 1, 1, generator=g).to(dev) * 6.2832
grey = 127 + 90 * torch.sin(xs / 37.0 + ys / 53.0 + ph)
rgb0 = torch.stack([grey, 0.8 * grey + 20, 255 - grey], -1).round().clamp(0, 255).to(torch.uint8).contiguous()
del grey
yuv = ops.rgb_to_yuv420(rgb0, fmt.layout, enc)
like_rgb = ops.yuv420_to_rgb(yuv, fmt.layout, fmt.chroma, dec)
edited = like_rgb.clone()
edited[:, H // 8:H // 4, W // 8:W // 4] = 250                        # a logo's worth of changed pixels: 1.6 % of the frame
assert torch.equal(ops.rgb_to_yuv420(like_rgb, fmt.layout, enc, like=yuv, like_rgb=like_rgb), yuv)
del rgb0


def torch_decode(x):
    y = (x[:, :H].float() - 16.0) * (255.0 / 219.0)
    uv = x[:, H:].reshape(L, H // 2, W // 2, 2).permute(0, 3, 1, 2).float() - 128.0
    uv = F.interpolate(uv, size=(H, W), mode="bilinear", align_corners=False) * (255.0 / 224.0)
    u, v = uv[:, 0], uv[:, 1]
    out = torch.stack([y + 1.5748 * v, y - 0.1873 * u - 0.4681 * v, y + 1.8556 * u], -1)
    return out.round().clamp(0, 255).to(torch.uint8)


def torch_encode(x):
    f = x.float()
    r, gch, b = f[..., 0], f[..., 1], f[..., 2]
    y = 16.0 + (0.2126 * r + 0.7152 * gch + 0.0722 * b) * (219.0 / 255.0)
    u = 128.0 + (-0.1146 * r - 0.3854 * gch + 0.5 * b) * (224.0 / 255.0)
    v = 128.0 + (0.5 * r - 0.4542 * gch - 0.0458 * b) * (224.0 / 255.0)
    uv = F.avg_pool2d(torch.stack([u, v], 1), 2).permute(0, 2, 3, 1).reshape(L, H // 2, W)
    return torch.cat([y, uv], 1).round().clamp(0, 255).to(torch.uint8)


def copy_of(nbytes):
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256)
    b = torch.empty_like(a)
    return lambda: b.copy_(a)


# (arm, call, bytes read + written per pixel, calls per timing)
arms = [("decode", lambda: ops.yuv420_to_rgb(yuv, fmt.layout, fmt.chroma, dec), 4.5, 200),
        ("copy_4.5", copy_of(int(4.5 * px)), 4.5, 200),
        ("encode", lambda: ops.rgb_to_yuv420(edited, fmt.layout, enc), 4.5, 200),
        ("paste", lambda: ops.rgb_to_yuv420(edited, fmt.layout, enc, like=yuv, like_rgb=like_rgb), 9.0, 100),
        ("copy_9", copy_of(int(9.0 * px)), 9.0, 100),
        ("torch_decode", lambda: torch_decode(yuv), 4.5, 5),
        ("torch_encode", lambda: torch_encode(edited), 4.5, 5)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps                         # us per call


for _, fn, _, _ in arms:
    fn()
torch.cuda.synchronize()
us = {name: [] for name, _, _, _ in arms}
for _ in range(rounds):
    for name, fn, _, reps in arms:
        us[name].append(timed(fn, reps))
diff_d = int((torch_decode(yuv).int() - like_rgb.int()).abs().max())
diff_e = int((torch_encode(edited).int() - ops.rgb_to_yuv420(edited, fmt.layout, enc).int()).abs().max())
rows = []
for name, _, bpp, reps in arms:
    v = np.array(us[name])
    row = {"arm": name, "size": "%dx%d" % (W, H), "frames": L, "MB_moved": round(bpp * px / 1e6, 1), "rounds": rounds,
           "calls_per_timing": reps, "us": {"mean": round(float(v.mean()), 1), "min": round(float(v.min()), 1),
                                            "max": round(float(v.max()), 1)},
           "effective_GBps": round(bpp * px / (float(v.mean()) * 1e-6) / 1e9, 1)}
    rows.append(row)
    print(json.dumps(row), flush=True)
print(json.dumps({"max_abs_levels_torch_float_vs_kernel": {"decode": diff_d, "encode": diff_e}}))
by = {r["arm"]: r for r in rows}
print("\n%-14s %12s %10s %16s" % ("arm", "us / launch", "GB/s", "of the copy"))
for name, ref in (("decode", "copy_4.5"), ("copy_4.5", None), ("encode", "copy_4.5"), ("paste", "copy_9"), ("copy_9", None),
                  ("torch_decode", "copy_4.5"), ("torch_encode", "copy_4.5")):
    r = by[name]
    share = "%.2f" % (r["effective_GBps"] / by[ref]["effective_GBps"]) if ref else ""
    print("%-14s %12.1f %10.1f %16s" % (name, r["us"]["mean"], r["effective_GBps"], share))
