"""Device cost of the bicubic frame resize (video.resize_frames: csrc/video.hip resample_u8, test.py:97-104) on frames already
on the device, at the sizes users run: 854x480 -> 432x240 (DAVIS, e2fgvi) and 1920x1080 -> 1296x720 (e2fgvi_hq --set_size).
Prints one JSON line per pair: event-timed ms per call (both passes and the table uploads) and the bytes the two passes move.
Kernel times: run it under rocprofv3 --kernel-trace --stats.
    python tools/resize_bench.py [L=100] [reps=20]"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from e2fgvi_amd import video

L = int(sys.argv[1]) if len(sys.argv) > 1 else 100
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda:0")
for (W, H), (w, h) in (((854, 480), (432, 240)), ((1920, 1080), (1296, 720))):
    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.randint(0, 256, (L, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    for _ in range(3):
        out = video.resize_frames(src, (w, h))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = video.resize_frames(src, (w, h))
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    # width pass: reads the source, writes [L,H,w,3]; height pass: reads that, writes [L,h,w,3]
    nbytes = L * 3 * (H * W + 2 * H * w + h * w)
    print(json.dumps({"frames": L, "src": "%dx%d" % (W, H), "dst": "%dx%d" % (w, h), "ms_per_call": round(ms, 4),
                      "us_per_frame": round(1e3 * ms / L, 3), "pass_bytes": nbytes, "GB_per_s": round(nbytes / ms / 1e6, 1)}),
          flush=True)
    del src, out
