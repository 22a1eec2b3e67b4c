"""The component labelling of inpaint_video(region="holes") (ops.hole_components, csrc/video.hip) against the yardstick that is not
the kernel itself: L mask frames of 1080x1920, three contents --
  rects    two rectangles, a logo in a corner and a band at the bottom (2 components);
  glyphs   subtitle-like blobs: rows of small rectangles in the bottom quarter, another choice of them in every frame;
  noise    a footprint of 40 % random pixels, every frame holding half of them (the most components and the most unions);
device time of
  components    ops.hole_components: the OR over the frames, the labelling, the read of K, the table of boxes;
  label         the C entry e2fgvi_hole_label alone on the same masks (no host read);
  label_1frame  the same entry on ONE frame that holds the whole footprint: everything but the OR over L frames;
  boxes         e2fgvi_label_boxes alone;
  copy          a device-to-device copy of the same L Hm Wm mask bytes (torch's copy_) -- the floor of a pass that must read them,
                although a copy also writes them;
all warmed, alternating, REPS calls between two device events.  same_integers_rerun: a second call returns the same labels and boxes.
One JSON line per content.
    python tools/hole_label_bench.py [L=100] [rounds=5]"""
import ctypes
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from e2fgvi_amd import lib, ops

L = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
Hm, Wm = 1080, 1920
dev = torch.device("cuda:0")
so = lib.load()


def masks_of(kind, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = torch.zeros((L, Hm, Wm), dtype=torch.uint8, device=dev)
    if kind == "rects":
        m[:, 40:140, 1700:1880] = 255
        m[:, 940:1040, 300:1620] = 1
    elif kind == "glyphs":
        for l in range(L):
            on = torch.rand((3, 60), generator=g) < 0.7
            for r in range(3):
                for c in range(60):
                    if on[r, c]:
                        m[l, 830 + 80 * r:830 + 80 * r + 50, 40 + 30 * c:40 + 30 * c + 22] = 255
    else:
        U = (torch.rand((Hm, Wm), generator=g) < 0.4).to(dev)
        for l in range(L):
            m[l] = (U & ((torch.rand((Hm, Wm), generator=g) < 0.5).to(dev) | (l == 0))).to(torch.uint8)
    return m


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1) / reps


def stats(v):
    v = np.array(v)
    return {"mean": round(float(v.mean()), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


p = lambda t: ctypes.c_void_p(t.data_ptr())
st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
work = torch.empty(so.e2fgvi_hole_label_workspace(Hm, Wm), dtype=torch.uint8, device=dev)
labels = torch.empty((Hm, Wm), dtype=torch.int32, device=dev)
count = torch.empty(1, dtype=torch.int32, device=dev)

for kind in ("rects", "glyphs", "noise"):
    m = masks_of(kind)
    nbytes = m.numel()
    spare = torch.empty_like(m)
    foot = (m != 0).any(0).to(torch.uint8).unsqueeze(0).contiguous()
    ref_labels, ref_boxes = ops.hole_components(m)
    K = int(ref_boxes.shape[0])
    boxes = torch.empty((max(K, 1), 5), dtype=torch.int32, device=dev)

    def label(x):
        lib.check(so.e2fgvi_hole_label(p(x), x.shape[0], Hm, Wm, p(work), p(labels), p(count), st()), "hole_label")

    def table():
        lib.check(so.e2fgvi_label_boxes(p(ref_labels), Hm, Wm, K, p(boxes), st()), "label_boxes")

    reps = 10
    arms = {"components": lambda: ops.hole_components(m), "label": lambda: label(m), "label_1frame": lambda: label(foot),
            "boxes": table, "copy": lambda: spare.copy_(m)}
    for fn in arms.values():                                        # warm every arm
        fn()
    torch.cuda.synchronize()
    one = bool(torch.equal(labels, ref_labels))                     # the one-frame footprint labels like the video
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn, reps)[1])
    again = ops.hole_components(m)
    mean = {k: float(np.mean(v)) for k, v in ms.items()}
    print(json.dumps({"size": "%dx%d" % (Wm, Hm), "frames": L, "content": kind, "MB": round(nbytes / 1e6, 1), "components": K,
                      "hole_fraction": round(float(foot.float().mean()), 4), "rounds": rounds, "calls_per_timing": reps,
                      "ms": {k: stats(v) for k, v in ms.items()},
                      "label_read_GBps": round(nbytes / (mean["label"] * 1e-3) / 1e9, 1),
                      "copy_read_GBps": round(nbytes / (mean["copy"] * 1e-3) / 1e9, 1),
                      "components_over_copy": round(mean["components"] / mean["copy"], 2),
                      "label_over_copy": round(mean["label"] / mean["copy"], 2),
                      "or_over_frames_ms": round(mean["label"] - mean["label_1frame"], 4),
                      "one_frame_same_labels": one,
                      "same_integers_rerun": bool(torch.equal(again[0], ref_labels) and torch.equal(again[1], ref_boxes))}), flush=True)
    del m, spare, arms
