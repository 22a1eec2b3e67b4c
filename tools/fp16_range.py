"""Range of the fp16 data path: for every stage (layer / helper) of the fp16 forward, the largest |x| of each 16-bit tensor it
writes and the share of its values that are fp16 subnormals (0 < |x| < 2^-14), on the default, stress and peaked weights
(synth.synth_state_dict) at e2fgvi 432x240 T=10, e2fgvi_hq 720x1296 T=10 and 1080x1944 T=8.  fp16 overflows above 65504: a
tensor within 4x of it (max |x| > 16376) would have to stay fp32.

    python tools/fp16_range.py [--quick] > profiles/fp16_range.txt

Every 16-bit result is read back after a device synchronisation (slow; a measurement, not a benchmark)."""
import collections
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from e2fgvi_amd import ops
from e2fgvi_amd.synth import synth_clip, synth_state_dict

SUB = 2.0 ** -14
LIMIT = 65504.0 / 4
CONFIGS = [("e2fgvi", 240, 432, 10), ("e2fgvi_hq", 720, 1296, 10), ("e2fgvi_hq", 1080, 1944, 8)]
stats = collections.OrderedDict()


def record(stage, t):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float16 or t.numel() == 0:
        return
    torch.cuda.synchronize()
    a = t.detach().float().abs()
    s = stats.setdefault(stage, [0.0, 0, 0, 0, 0])        # max |x|, subnormals, nonzero, elements, non-finite
    s[0] = max(s[0], float(a[torch.isfinite(a)].max()) if bool(torch.isfinite(a).any()) else 0.0)
    s[1] += int(((a > 0) & (a < SUB)).sum())
    s[2] += int((a > 0).sum())
    s[3] += a.numel()
    s[4] += int((~torch.isfinite(a)).sum())


def wrap_method(cls, attr, slice_out):
    fn = getattr(cls, attr)

    def call(self, *a, **k):
        r = fn(self, *a, **k)
        record(getattr(self, "name", cls.__name__), slice_out(self, r, k))
        return r
    setattr(cls, attr, call)


def wrap_function(name, pick=lambda r: r):
    fn = getattr(ops, name)

    def call(*a, **k):
        r = fn(*a, **k)
        for t in (pick(r) if isinstance(pick(r), (list, tuple)) else [pick(r)]):
            record(name, t)
        return r
    setattr(ops, name, call)


def _conv_slice(self, r, k):                     # only the channels this call wrote (out may be a wider buffer)
    if not isinstance(r, torch.Tensor) or r.dim() != 4 or k.get("out_nchw"):
        return r
    c0 = k.get("out_coff", 0)
    return r[..., c0:c0 + self.Cout]


wrap_method(ops.PackedConvX, "__call__", _conv_slice)
wrap_method(ops.PackedDcn, "__call__", lambda self, r, k: r)
wrap_method(ops.SoftCompGather, "__call__", lambda self, r, k: r)
for f in ("nchw_to_nhwc", "layernorm", "window_pool", "ffn_fold", "ffn_fold_gelu", "ffn_unfold", "ffn_unfold_gelu",
          "softcomp_fold", "resize_bilinear", "focal_attention_bf16", "cast"):
    wrap_function(f)
wrap_function("prop_cond", lambda r: [r[0], r[2]] if len(r) > 2 else [r[0]])
wrap_function("spynet_level_input", lambda r: r[1] if isinstance(r, tuple) else None)


def main():
    quick = "--quick" in sys.argv
    dev = torch.device("cuda")
    print("# fp16 data path: per stage, the largest |x| of its 16-bit results and the share of fp16 subnormals among the non-zero")
    print("# values (0 < |x| < 2^-14 = 6.1e-5); flag '!!' = within 4x of the fp16 maximum 65504 (> %.0f)" % LIMIT)
    worst = {}
    for model, H, W, t in (CONFIGS[:1] if quick else CONFIGS):
        for kind in ("default", "stress", "peaked"):
            stats.clear()
            net = importlib.import_module("model." + model).InpaintGenerator()
            net.load_state_dict(synth_state_dict(model, kind, 0))
            net = net.to(dev).eval()
            net.precision = "fp16"
            x = synth_clip(1, t, H, W, seed=9, moving=True)[0].to(dev)
            with torch.no_grad():
                out, _ = net(x, t)
            torch.cuda.synchronize()
            print("\n## %s %dx%d T=%d, %s weights: output finite %s, max |out| %.4f"
                  % (model, W, H, t, kind, bool(torch.isfinite(out).all()), float(out.abs().max())))
            print("%-58s %12s %12s %10s" % ("stage", "max |x|", "subnormal", "non-finite"))
            for stage, (mx, sub, nz, n, nf) in stats.items():
                print("%-58s %12.4g %11.2e%% %10d %s" % (stage[:58], mx, 100.0 * sub / max(nz, 1), nf, "!!" if mx > LIMIT else ""))
                w = worst.setdefault(stage, [0.0, 0.0, ""])
                if mx > w[0]:
                    w[0], w[2] = mx, "%s %dx%d %s" % (model, W, H, kind)
                w[1] = max(w[1], 100.0 * sub / max(nz, 1))
            del net, out
            torch.cuda.empty_cache()
    print("\n## every regime: per stage, the largest |x| (where) and the largest subnormal share")
    for stage, (mx, sub, where) in sorted(worst.items(), key=lambda kv: -kv[1][0]):
        print("%-58s %12.4g  %-32s %9.2e%% %s" % (stage[:58], mx, where, sub, "!!" if mx > LIMIT else ""))
    top = max(worst.values(), key=lambda v: v[0])
    print("\nlargest |x| of any 16-bit tensor: %.4g (%s) = 65504 / %.1f" % (top[0], top[2], 65504.0 / max(top[0], 1e-30)))


if __name__ == "__main__":
    main()
