"""Speed of the fp16 data path against the bf16 one, in alternating fresh processes (one forward configuration per process).
    python tools/fp16_vs_bf16.py [rounds] [iters]        (default 3 rounds of 10 timed forwards each)
    python tools/fp16_vs_bf16.py --child MODEL HxW T ITERS PRECISION
Configurations: e2fgvi 432x240 T=10, e2fgvi_hq 720x1296 T=10 and 1080x1944 T=20 (timed like tools/hq_run.py: random-init
weights, synthetic clip, l_t = T)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("e2fgvi", "240x432", 10), ("e2fgvi_hq", "720x1296", 10), ("e2fgvi_hq", "1080x1944", 20)]


def child(model, hw, t, iters, prec):
    sys.path.insert(0, ROOT)
    import importlib
    import torch
    from e2fgvi_amd.synth import synth_clip, synth_state_dict
    H, W = [int(v) for v in hw.split("x")]
    dev = torch.device("cuda:0")
    net = importlib.import_module("model." + model).InpaintGenerator()
    net.load_state_dict(synth_state_dict(model, "default", 0))
    net = net.to(dev).eval()
    net.precision = prec
    x = synth_clip(1, t, H, W, seed=9)[0].to(dev)
    for _ in range(2):
        out, _ = net(x, t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out, _ = net(x, t)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    print(json.dumps({"model": model, "hw": hw, "t": t, "precision": prec, "ms_per_forward": round(ms, 3),
                      "frames_per_s": round(1e3 * t / ms, 2), "finite": bool(torch.isfinite(out).all())}))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    res = {}
    for model, hw, t in CONFIGS:
        for r in range(rounds):
            for prec in (("bf16", "fp16") if r % 2 == 0 else ("fp16", "bf16")):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", model, hw, str(t), str(iters), prec],
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    print("child failed (%d): %s %s %s\n%s" % (p.returncode, model, hw, prec, p.stderr[-2000:]), flush=True)
                    sys.exit(1)
                line = json.loads(p.stdout.strip().splitlines()[-1])
                print(json.dumps(line), flush=True)
                res.setdefault((model, hw, t), {}).setdefault(prec, []).append(line["frames_per_s"])
    print("\n%-10s %-10s %3s %28s %28s %9s" % ("model", "H x W", "T", "bf16 frames/s (runs)", "fp16 frames/s (runs)", "fp16/bf16"))
    for (model, hw, t), v in res.items():
        b, f = v["bf16"], v["fp16"]
        mb, mf = sorted(b)[len(b) // 2], sorted(f)[len(f) // 2]
        print("%-10s %-10s %3d %28s %28s %9.3f" % (model, hw, t, " ".join("%.1f" % x for x in b), " ".join("%.1f" % x for x in f), mf / mb))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[6])
    else:
        main()
