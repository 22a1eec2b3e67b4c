"""End-to-end throughput of the sliding-window driver (e2fgvi_amd/video.py) on a synthetic 432x240 video:
upload of the uint8 frames, all windows (11 local + reference frames each), compositing, download.
    python tools/video_bench.py [L=100] [batch_windows=1] [in_flight=1] [source=WxH]
With a source size the frames (and masks) have that size and the driver resizes them to 432x240 on the device
(inpaint_video(size=(432, 240)), test.py:97-104); the same video pre-resized with PIL on the host is timed against it,
alternating, and the host's PIL time per frame is reported beside.
    python tools/video_bench.py --reuse [L=100] [model=e2fgvi] [WxH=432x240] [precision=fp32] [repeats=4]
times inpaint_video(reuse=False) against inpaint_video(reuse=True) on the same video in one process, alternating, after one
warm-up call of each, and prints every run's seconds, the best rates, the run-to-run spread of each mode, the frames / pairs
the engine counted through its encoder, SPyNet and decoder, and the bytes of the reuse caches."""
import os, sys, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, importlib
from e2fgvi_amd import video
from e2fgvi_amd.synth import synth_state_dict


def reuse_ab(argv):
    L = int(argv[0]) if len(argv) > 0 else 100
    model = argv[1] if len(argv) > 1 else "e2fgvi"
    W, H = (int(v) for v in (argv[2] if len(argv) > 2 else "432x240").split("x"))
    precision = argv[3] if len(argv) > 3 else "fp32"
    reps = int(argv[4]) if len(argv) > 4 else 4
    dev = torch.device("cuda:0")
    net = importlib.import_module("model." + model).InpaintGenerator()
    net.load_state_dict(synth_state_dict(model, "default", 0)); net = net.to(dev).eval()
    net.precision = precision
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)
    masks = np.zeros((L, H, W), np.uint8); masks[:, H // 4:H // 2, W // 4:W // 2] = 255
    eng = net.engine()
    secs, counts, outs = {False: [], True: []}, {}, {}
    for rep in range(reps + 1):                # rep 0: warm-up of every shape either mode launches (not timed)
        for reuse in (False, True):
            before = dict(eng.counters)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            outs[reuse] = video.inpaint_video(net, frames, masks, reuse=reuse)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            counts[reuse] = {k: eng.counters[k] - before[k] for k in before}
            if rep:
                secs[reuse].append(dt)
    Hp, Wp = video.padded_size(H, W)
    plan = video.plan_reuse(video.plan_windows(L))
    d = np.abs(outs[True].astype(int) - outs[False].astype(int))
    spread = lambda v: (max(v) - min(v)) / min(v)
    print(json.dumps({
        "video_frames": L, "model": model, "size": "%dx%d" % (W, H), "precision": precision, "repeats": reps,
        "seconds_reuse_off": [round(v, 3) for v in secs[False]], "seconds_reuse_on": [round(v, 3) for v in secs[True]],
        "video_frames_per_s_reuse_off": round(L / min(secs[False]), 2), "video_frames_per_s_reuse_on": round(L / min(secs[True]), 2),
        "speedup_best_of": round(min(secs[False]) / min(secs[True]), 3),
        "speedup_slowest_on_vs_fastest_off": round(min(secs[False]) / max(secs[True]), 3),
        "spread_reuse_off": round(spread(secs[False]), 4), "spread_reuse_on": round(spread(secs[True]), 4),
        "counted_reuse_off": counts[False], "counted_reuse_on": counts[True],
        "cache_slots": plan.slots, "cache_pair_slots": plan.pair_slots,
        "cache_bytes": plan.cache_bytes(Hp // 4, Wp // 4, 2 if precision in ("bf16", "fp16") else 4),
        "on_vs_off_max_byte_difference": int(d.max()), "on_vs_off_share_of_differing_bytes": round(float((d > 0).mean()), 6)}))


if "--reuse" in sys.argv:
    reuse_ab([a for a in sys.argv[1:] if a != "--reuse"])
    sys.exit(0)
L = int(sys.argv[1]) if len(sys.argv) > 1 else 100
bw = int(sys.argv[2]) if len(sys.argv) > 2 else 1
fl = int(sys.argv[3]) if len(sys.argv) > 3 else 1
src = sys.argv[4] if len(sys.argv) > 4 else None
SW, SH = (int(v) for v in src.split("x")) if src else (432, 240)
size = (432, 240) if src else None
dev = torch.device("cuda:0")
net = importlib.import_module("model.e2fgvi").InpaintGenerator()
net.load_state_dict(synth_state_dict("e2fgvi", "default", 0)); net = net.to(dev).eval()
rng = np.random.RandomState(0)
frames = rng.randint(0, 256, (L, SH, SW, 3)).astype(np.uint8)
masks = np.zeros((L, SH, SW), np.uint8); masks[:, SH // 4:SH // 2, SW // 4:SW // 2] = 255
video.inpaint_video(net, frames[:12], masks[:12], size=size)            # engine build, allocator
res = {}
for tag in ("first_call", "steady"):
    # first_call: includes the one-off tile tuning of every new window shape (GEMM-shaped layers, a few hundred timed
    # launches per size class); steady: the same video again, every decision cached in the process
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = video.inpaint_video(net, frames, masks, batch_windows=bw, in_flight=fl, size=size)
    torch.cuda.synchronize(); res[tag] = time.perf_counter() - t0
nwin = len(range(0, L, 5))
dt = res["steady"]
ref = video.inpaint_video(net, frames, masks, size=size)
same = bool(np.array_equal(np.asarray(out), np.asarray(ref)))
line = {"video_frames": L, "windows": nwin, "batch_windows": bw, "in_flight": fl, "same_bytes_as_one_at_a_time": same, "seconds": round(dt, 3),
        "video_frames_per_s": round(L / dt, 1), "ms_per_window": round(1e3 * dt / nwin, 2),
        "first_call_seconds": round(res["first_call"], 3)}
if src:
    from PIL import Image
    t0 = time.perf_counter()
    pre = np.stack([np.asarray(Image.fromarray(f).resize(size)) for f in frames])
    pil_s = time.perf_counter() - t0
    t_size, t_pre = [dt], []
    for _ in range(2):                     # alternate the two forms; best of each
        torch.cuda.synchronize(); t0 = time.perf_counter()
        b = video.inpaint_video(net, pre, masks, batch_windows=bw, in_flight=fl)
        torch.cuda.synchronize(); t_pre.append(time.perf_counter() - t0)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        video.inpaint_video(net, frames, masks, batch_windows=bw, in_flight=fl, size=size)
        torch.cuda.synchronize(); t_size.append(time.perf_counter() - t0)
    line.update({"source": src, "video_frames_per_s": round(L / min(t_size), 1),
                 "pre_resized_video_frames_per_s": round(L / min(t_pre), 1),
                 "same_bytes_as_pre_resized": bool(np.array_equal(np.asarray(out), np.asarray(b))),
                 "host_pil_resize_ms_per_frame": round(1e3 * pil_s / L, 2)})
print(json.dumps(line))
