"""Where the fp16 data path's error comes from, stage by stage, next to bf16: every traced tensor of the fp16 and the bf16 forward of a
golden fixture's clip (tests/golden, rebuilt from its seed) against the CPU oracle's trace of the same clip (oracle/e2fgvi_oracle.py,
within ~1e-6 of the real reference on these fixtures) -- flows, encoder output, propagated features, the token stream behind every
transformer block, the decoder input, the frames -- as rms of the difference / rms of the reference and max abs, with the ratio
bf16 / fp16 per stage.  Then the same forwards with the ORACLE's flows fed in (the engine's given-flows hook), which takes SPyNet's
own rounding out of everything downstream.

    python tools/fp16_stage_errors.py g14_hq_default_720x1296_t10_lt10_benchclip.npz g13_hq_peaked_720x1296_t4_lt3.npz
"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    from e2fgvi_amd.synth import synth_state_dict
    from oracle import e2fgvi_oracle as O
    from tests.util import golden_case
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    for fx in sys.argv[1:]:
        z, model, kind, x, lt, so, sf = golden_case(os.path.join(ROOT, "tests", "golden", fx))
        sd = synth_state_dict(model, kind, 0)
        b, t, _, H, W = x.shape
        h, w = H // 4, W // 4
        tr = {}
        ref, (rf, rb) = O.forward(sd, x, lt, model, tr)
        C = tr["enc"].shape[1]

        def nhwc_ref(v):                                  # oracle NCHW [b*t, C, h, w] (or [b, t, C, h, w]) -> NHWC
            return v.reshape(b * t, C, h, w).permute(0, 2, 3, 1)

        def rows(got, out, ff, fb):
            r = [("flows (SPyNet)", torch.cat([ff.cpu().reshape(-1), fb.cpu().reshape(-1)]), torch.cat([rf.reshape(-1), rb.reshape(-1)])),
                 ("encoder output", got["enc"].reshape(b * t, h, w, C), nhwc_ref(tr["enc"])),
                 ("propagated features", got["prop"].reshape(b * t, h, w, C), nhwc_ref(tr["prop"])),
                 ("tokens0 (soft split)", got["tokens0"].reshape(-1, 512), tr["tokens0"].reshape(-1, 512))]
            r += [("tokens%d (block %d)" % (i, i - 1), got["tokens%d" % i].reshape(-1, 512), tr["tokens%d" % i].reshape(-1, 512))
                  for i in range(1, 9)]
            r += [("decoder input", got["dec_in"].reshape(b * t, h, w, C), nhwc_ref(tr["dec_in"])), ("frames", out, ref)]
            return r

        def err(g, r):
            g, r = g.detach().double().cpu(), r.detach().double()
            return ((g - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt()).item(), (g - r).abs().max().item()

        res = {}
        for precision in ("fp16", "bf16"):
            net = importlib.import_module("model." + model).InpaintGenerator()
            net.load_state_dict(sd)
            net = net.to(dev).eval()
            net.precision = precision
            eng = net.engine()
            with torch.no_grad():
                got = {}
                out, (ff, fb) = eng.forward(x.to(dev), lt, trace=got)
                torch.cuda.synchronize()
                res[precision] = [(n, err(g, r)) for n, g, r in rows(got, out, ff, fb)]
                # the oracle's flows in place of SPyNet's (NHWC [b, l_t-1, h, w, 2]); the encoder of this precision
                enc = eng.encode(x.to(dev).float().contiguous())
                given = (rf.permute(0, 1, 3, 4, 2).contiguous().to(dev), rb.permute(0, 1, 3, 4, 2).contiguous().to(dev))
                eng._given = (given, enc)
                try:
                    got2 = {}
                    out2, _ = eng.forward(x.to(dev), lt, trace=got2)
                    torch.cuda.synchronize()
                finally:
                    eng._given = None
                res[precision + "+oracle flows"] = [(n, err(g, r)) for n, g, r in rows(got2, out2, rf, rb)][1:]
            del net, eng
            torch.cuda.empty_cache()
        print("\n== %s: %s %dx%d T=%d l_t=%d, %s weights" % (fx, model, W, H, t, lt, kind))
        print("%-22s %21s %21s %13s" % ("stage", "fp16 rms / max", "bf16 rms / max", "bf16/fp16 rms / max"))
        for (n, (r16, m16)), (_, (rb16, mb16)) in zip(res["fp16"], res["bf16"]):
            print("%-22s %9.3e / %9.3e %9.3e / %9.3e %6.2f / %6.2f" % (n, r16, m16, rb16, mb16, rb16 / max(r16, 1e-30), mb16 / max(m16, 1e-30)))
        print("-- with the oracle's flows fed in (SPyNet's rounding removed):")
        for (n, (r16, m16)), (_, (rb16, mb16)) in zip(res["fp16+oracle flows"], res["bf16+oracle flows"]):
            print("%-22s %9.3e / %9.3e %9.3e / %9.3e %6.2f / %6.2f" % (n, r16, m16, rb16, mb16, rb16 / max(r16, 1e-30), mb16 / max(m16, 1e-30)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
