"""Device-side execution plan of the E2FGVI / E2FGVI-HQ inference forward on MI355X.

``Engine`` is built once from a checkpoint-format ``state_dict`` (reference format):
it re-lays-out every weight for the HIP kernels and then runs the forward as a sequence of
C-ABI kernel launches (ops.py).  The staging mirrors the reference's module boundaries so each
stage can be checked against the oracle on the same inputs:

    flows()      e2fgvi.py:210-234 + flow_comp.py:84-169      SPyNet, both directions batched
    encode()     e2fgvi.py:96-109                             9 convs, grouped concat by pointers
    propagate()  feat_prop.py:81-149, :35-58                  2 x l_t sequential steps
    transformer()tfocal_transformer.py:466-536, :210-399      8 blocks, fused focal attention
    compose()    tfocal_transformer.py:65-72 (+ e2fgvi.py:258)
    decode()     e2fgvi.py:126-150, :261-262

Nothing here computes on the CPU or through torch ops -- torch only owns the buffers (and does index-only copies when clips
are batched).  The precision is data: the layer classes a checkpoint layer gets, the dtype of the activations and the input
padding; both precisions run the same stage methods.

  * fp32 (the default and the parity configuration): all activations are NHWC fp32.
  * bf16 (BASELINE.json configs 4 / 5: e2fgvi_hq at 720p / 1080p, "bf16 MFMA"): activations are bf16 NHWC tensors in HBM (half
    the traffic of the fp32 path), every conv / linear runs in csrc/conv_bf16x.hip (bf16 operands by LDS-DMA,
    v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogue).  Kept in fp32: the SPyNet flow pyramid and the flows (sub-pixel
    sampling positions), the DCN offsets / masks (output of conv_offset.6 incl. its 10 tanh + flow post-processing), the token
    residual stream between transformer blocks (LayerNorm input) and the output frames; the recurrent propagation features are
    ONE bf16 tensor per step (conv source, flow-warp source, and -- re-laid out [group][pixel][16] -- the deformable conv's
    gather source).  LayerNorm, window pooling, fold / unfold + GELU, SoftComp fold and the x2 upsamples read / write bf16 and
    compute in fp32 (typed variants of the fp32 kernels, csrc/misc.hip).
  * fp16: the bf16 data path with IEEE half as the 16-bit type -- the same stage methods, layers, tiles and fp32 tensors
    (self.x16 is the 16-bit data path, self.dtype its element type); the kernels' fp16 instantiations run fp16 MFMA.  8x finer
    rounding than bf16 (11 significand bits against 8); range: profiles/fp16_range.txt, DESIGN.md section 1.
"""
import numpy as np
import os

import torch

from . import ops
from .ops import ACT_DCNPOST, ACT_LRELU, ACT_RELU, ACT_TANH, PackedConvX

BF16 = torch.bfloat16
F16 = torch.float16
# fp32 path: the FFN's second Linear as a conv of the folded tensor (as the bf16 path runs it).  Measured neutral on the fp32
# MFMA kernels (15.785 vs 15.775 ms, profiles/r02_fc2_conv.txt: the 16-byte tap-packed fetches cost what the unfold kernel
# saved); with the split-operand kernels (ops.X3_ENABLED) the conv form wins -- 743 -> 750 frames/s, same box, two runs each
# (profiles/r03_fc2_conv_x3.txt) -- and is the default
FC2_CONV = ops.X3_ENABLED          # (bench.py's E2FGVI_X3=0 secondary line sets both to False for its engine)
# bf16 path, settled in rounds 2-5 and no longer switchable (round 6): decoder.6 on csrc/conv_tail.hip; the deformable conv gathers
# from [group][pixel][16] copies of the propagated features; the recurrent propagation state and the flow-warp sources are the bf16
# copies (an fp32 state changes the end-to-end error by < 1 % of itself: tools/bf16_error_growth.py); the FFN's second Linear is
# the 7x7 / stride-3 conv of the folded tensor; SoftComp (HQ) runs in gather form.
WIN = (5, 9)
# where the side stream (SPyNet) joins the main one: in front of encoder.layers.<JOIN_AT> (18 = behind the encoder).  Round 4 joined in
# front of layer 10 (its wide-tile kernel was fenced to layers with the chip to themselves); with encoder.layers.2 / 6 / 8 on that
# kernel the main stream reaches layer 10 before SPyNet has finished and waited there: 787.9 frames/s joined at 10, 801-808 joined
# at 12 ... 18, best at 16 (same box, two runs each: profiles/r05_join_position.txt)
# With several clips per forward the batched encoder layers fill the chip on their own and the early join is 0.5 % ahead (8 clips: 974.7
# vs 969.5 frames/s), so: 16 at one clip, 10 otherwise; E2FGVI_JOIN_AT overrides both.  (The bf16 path joins behind the encoder.)
JOIN_AT = int(os.environ.get("E2FGVI_JOIN_AT", "0") or 0)
if JOIN_AT not in (0, 10, 12, 14, 16, 18):
    raise ValueError("E2FGVI_JOIN_AT=%d: the join sits in front of encoder.layers.10 / 12 / 14 / 16 or behind the encoder (18)" % JOIN_AT)
PROP_SPLIT = os.environ.get("E2FGVI_PROP_SPLIT", "1") != "0"       # 0: conv_offset.0 / backbone.0 whole in every propagation step (A/B)


def token_grid(h, w):
    """Unfold(7, stride 3, pad 3) output grid (tfocal_transformer.py:30-37)."""
    return (h + 6 - 7) // 3 + 1, (w + 6 - 7) // 3 + 1


def build_key_table(fh, fw, valid_ind_rolled):
    """Per-window key references for the fused attention kernel.

    Row ``win`` lists, for one frame, the keys window ``win`` attends to besides nothing else:
    its own 45 tokens, the 120 ring tokens of the four circularly rolled maps (positions from
    ``valid_ind_rolled``; wrap-around and the 12 duplicates kept exactly as torch.roll +
    window_partition produce them, tfocal_transformer.py:235-273) as ``y*fw+x`` >= 0, then the
    valid pooled windows of the 5x9 neighbourhood (:328-333) as ``-(index+1)``.  ``nkeys`` is the
    count; the other pooled slots are the zero-padded ones (score -100).
    """
    nwh, nww = fh // WIN[0], fw // WIN[1]
    ex = (WIN[0] // 2, WIN[1] // 2)
    shifts = ((-ex[0], -ex[1]), (-ex[0], ex[1]), (ex[0], -ex[1]), (ex[0], ex[1]))   # tl, tr, bl, br
    vi = [int(v) for v in valid_ind_rolled]
    tab = np.zeros((nwh * nww, 212), np.int32)
    nk = np.zeros((nwh * nww,), np.int32)
    for wy in range(nwh):
        for wx in range(nww):
            refs = []
            for p in range(45):
                refs.append((wy * 5 + p // 9) * fw + wx * 9 + p % 9)
            for v in vi:
                n, p = divmod(v, 45)
                sy, sx = shifts[n]
                # rolled[y,x] = k[(y - sy) % fh, (x - sx) % fw]
                y = (wy * 5 + p // 9 - sy) % fh
                x = (wx * 9 + p % 9 - sx) % fw
                refs.append(y * fw + x)
            for ki in range(5):
                for kj in range(9):
                    py, px = wy - 2 + ki, wx - 4 + kj
                    if 0 <= py < nwh and 0 <= px < nww:
                        refs.append(-(py * nww + px + 1))
            w = wy * nww + wx
            nk[w] = len(refs)
            tab[w, :len(refs)] = refs
    return tab, nk


def split_prop_weights(w_off0, w_bb0, ch=128):
    """The propagation split as weight slices.  conv_offset.0 reads cat(cond_n1, current frame, cond_n2, flow_1,
    flow_2) (feat_prop.py:27-35,117-123) and backbone.0 cat(current frame[, the other direction's feature], feat_prop)
    (feat_prop.py:131-137): `*_rec` keep the input channels that depend on the recurrence -- sources (cond_n1, cond_n2, flows) and
    (feat_prop) --, `off_cur` / `bb_pre` the rest; conv(whole) == conv(rec part) + conv(other part), bias counted once
    (tests/test_identities.py)."""
    return dict(off_rec=torch.cat([w_off0[:, :ch], w_off0[:, 2 * ch:]], 1).contiguous(), off_cur=w_off0[:, ch:2 * ch].contiguous(),
                bb_rec=w_bb0[:, -ch:].contiguous(), bb_pre=w_bb0[:, :-ch].contiguous())


class Engine:
    def __init__(self, state_dict, model="e2fgvi", device="cuda", precision="fp32", winograd=True, autotune=True):
        """precision="fp32": fp32 tensors, every contraction with fp32-level rounding (the default and the parity configuration):
        on the fp32 MFMA instructions (bit-equivalent to an fp32 FMA chain) or -- ops.X3_ENABLED, the default -- on the bf16 matrix
        pipe with exactly split operands (three bf16 pieces per fp32 value, six of the nine cross terms, fp32 accumulation: fp32-
        level, not bit-identical to an FMA chain; tests/test_gpu_x3.py).  Which of the two a layer runs comes from the decision
        table (ops.py); E2FGVI_X3=0 gives the pure fp32-MFMA configuration.
        precision="bf16": the bf16 data path (BASELINE.json HQ configurations): bf16 activations in HBM, every conv / linear /
        attention product on bf16 MFMA with fp32 accumulation; SPyNet, the flows, the DCN offsets and masks, the deformable conv's
        arithmetic and the token residual stream stay fp32.
        precision="fp16": the same data path with fp16 in place of bf16 (fp16 MFMA, same fp32 tensors)."""
        if precision not in ("fp32", "bf16", "fp16"):
            raise ValueError("precision must be 'fp32', 'bf16' or 'fp16'")
        self.precision = precision
        self.hq = model == "e2fgvi_hq"
        self.device = torch.device(device)
        sd = {k: v.detach().to(self.device) for k, v in state_dict.items()}
        self.sd = sd
        f = lambda k: sd[k].float().contiguous()
        self.x16 = x16 = precision in ("bf16", "fp16")        # the 16-bit data path (bf16 or fp16 activations)
        self.dtype = {"bf16": BF16, "fp16": F16}.get(precision, torch.float32)     # of the activations between the layers
        x3 = not x16 and ops.X3_ENABLED
        # wide 3x3 / stride-1 layers: fp32 Winograd F(2x2,3x3) whenever the call qualifies (even H, W), else implicit GEMM (the
        # other geometries stay on the implicit GEMM under algo="auto": ops.PackedConv)
        algo = "auto" if winograd else "igemm"

        def layer(name, key, cpg=None, w=None, b=None, tune=False, nopk=False, **geom):
            """One checkpoint layer in this engine's precision: weights <key>.weight / <key>.bias unless `w` / `b` are given (key
            None: both are); cpg None: a Linear.  fp32: ops.PackedConv / PackedLinear, or PackedConvX on fp32 operands when `taps`
            is given; 16-bit: ops.PackedConvX / PackedLinearX.
            tune (fp32): the GEMM-shaped layers (token Linears, soft split / composite): the best implicit-GEMM tile depends on
            the token count; their tile code comes from the decision table of ops.py (e2fgvi_amd/tile_table.py by default, timed on
            the first eager call of each size class under E2FGVI_AUTOTUNE=1).  (Winograd block shapes are NOT tuned at run time:
            measured in round 2, the timing-based choice between the 16x16 / 8x16-pixel blocks moved the forward by -1 ... -2 % and
            added run-to-run variance; the static rule of e2fgvi_conv3x3_winograd stays.)  In bf16 every layer is tuned: the best
            tile of conv_bf16x depends on the layer's M x N x K and on how many tiles that makes for 256 CUs (timed on the first
            eager call of each size class, never under graph capture).
            try_x3: every fp32 conv / linear may run on the bf16 matrix pipe instead (ops.PackedConvX x3: operands split exactly
            into three bf16 pieces, six bf16 MFMA terms per product, fp32-level rounding): timed against the layer's fp32 kernel
            on the first eager call of each size class, kept where it is faster (the GEMM-shaped layers: token Linears, soft split
            / composite, the stride-2 and 1x1 convs; the Winograd layers mostly keep Winograd).  SPyNet's 7x7 layers are candidates
            too since round 5 (the split-operand GEMM is built without packed-fp32 VALU like every kernel that can run on the side
            stream): the two wide layers of the upper levels take it, 221 -> 199 and 239 -> 223 us alone and -- what matters beside
            the encoder -- at a third of the matrix-pipe time (profiles/r05_spynet_x3.txt).
            nopk (fp32): the side stream's layers run the build without packed-fp32 VALU (build.py; every bf16 kernel is built so)."""
            if key is not None:
                w = f(key + ".weight") if w is None else w
                b = f(key + ".bias") if b is None else b
            if cpg is None:
                c = ops.PackedLinearX(w, b, dtype=self.dtype) if x16 else ops.PackedLinear(w, b, precision="fp32")
            elif x16 or "taps" in geom:
                c = ops.PackedConvX(w, b, cpg, dtype=self.dtype, **geom)
            else:
                c = ops.PackedConv(w, b, cpg, precision="fp32", algo=algo, **geom)
            c.name = name
            c.tune = autotune and (x16 or tune)
            c.try_x3 = x3
            if nopk and not x16:
                c.nopk = True
            return c

        # ---- encoder (e2fgvi.py:75-94): the 3-channel frames are carried as 4 fp32 / 8 bf16 channels (16-byte pixels), layer 0's
        # weight is zero-padded to match
        cin0 = 8 if x16 else 4
        w0 = torch.zeros(64, cin0, 3, 3, device=self.device)
        w0[:, :3] = f("encoder.layers.0.weight")
        self.enc = [layer("encoder.layers.0", "encoder.layers.0", [cin0], w=w0, stride=2, pad=1)]
        for i, (cpg, g, s) in zip((2, 4, 6, 8, 10, 12, 14, 16),
                                  (([64], 1, 1), ([64], 1, 2), ([128], 1, 1), ([256], 1, 1), ([128, 192], 2, 1),
                                   ([64, 128], 4, 1), ([32, 48], 8, 1), ([256, 256], 1, 1))):
            self.enc.append(layer("encoder.layers.%d" % i, "encoder.layers.%d" % i, cpg, groups=g, stride=s, pad=1))

        # ---- decoder (e2fgvi.py:143-150); decoder.6 (64 -> 3) on csrc/conv_tail.hip, reading the activations' dtype
        self.dec = [layer(n, n, [c], pad=1) for n, c in (("decoder.0.conv", 128), ("decoder.2", 128), ("decoder.4.conv", 64))]
        tail = ops.PackedTailConv(f("decoder.6.weight"), f("decoder.6.bias"), dtype=self.dtype)
        tail.name = "decoder.6"
        if x16 and autotune:
            tail.tune = True
        self.dec.append(tail)

        # ---- propagation (feat_prop.py:61-79, :15-33)
        # conv_offset.0 and backbone.0 are linear in their input channels, and a third / a half / two thirds of those do not
        # depend on the recurrence (the current frame's features, the other direction's result): at one clip per forward that
        # part is computed for all frames at once on the side stream, beside the chain of one-frame launches that leaves most
        # of the chip idle, and enters the per-step layer -- now 260 / 128 input channels instead of 388 / 256 / 384 -- as its
        # residual (PROP_SPLIT, propagate(); fp32 only).  Round 2 measured the same split as a net loss (42 -> 34 and 37 -> 26 us
        # per step against 537 us of batched launches in the critical path, profiles/r02_c2_layer_fp32_base.md): the batched half
        # was four fp32-MFMA launches on the main stream then, it is three split-operand launches beside the chain now.
        self.prop = {}
        self.prop_split = {}
        for d, nparts in (("backward_", 2), ("forward_", 3)):
            p = "feat_prop_module.deform_align.%s." % d
            b = "feat_prop_module.backbone.%s." % d
            # conv_offset.0 input = cat(cond_n1, cur, cond_n2, flow_1, flow_2): sources (cond|0), cur, (cond|128), flows (4 fp32
            # channels; 8 bf16 channels, the weight zero-padded to match)
            w_off0 = f(p + "conv_offset.0.weight")
            if x16:
                w_off0 = torch.cat([w_off0, w_off0.new_zeros(128, 4, 3, 3)], 1)
            off = [layer("deform_align.%sconv_offset.0" % d, p + "conv_offset.0", [128, 128, 128, 8 if x16 else 4], w=w_off0, pad=1)]
            off += [layer("deform_align.%sconv_offset.%d" % (d, k), p + "conv_offset.%d" % k, [128], pad=1) for k in (2, 4, 6)]
            # the deformable conv: split-operand MFMA with the other x3 kernels (ops.X3_ENABLED); bf16 products in the bf16 path
            dcn = ops.PackedDcn(f(p + "weight"), f(p + "bias"), 16, pad=1, mfma=precision if x16 else ("x3" if x3 else "fp32"))
            dcn.name = "deform_align.%sdcn" % d
            bb = [layer("backbone.%s0" % d, b + "0", [128] * nparts, pad=1), layer("backbone.%s2" % d, b + "2", [128], pad=1)]
            self.prop[d] = (off, dcn, bb)
            if PROP_SPLIT and not x16:
                ws = split_prop_weights(f(p + "conv_offset.0.weight"), f(b + "0.weight"))
                self.prop_split[d] = dict(
                    off_rec=layer("deform_align.%sconv_offset.0 (recurrent part)" % d, None, [128, 128, 4], w=ws["off_rec"],
                                  b=f(p + "conv_offset.0.bias"), pad=1),
                    off_cur=layer("deform_align.%sconv_offset.0 (current-frame part)" % d, None, [128], w=ws["off_cur"], pad=1),
                    bb_rec=layer("backbone.%s0 (recurrent part)" % d, None, [128], w=ws["bb_rec"], b=f(b + "0.bias"), pad=1),
                    bb_pre=layer("backbone.%s0 (non-recurrent part)" % d, None, [128] * (nparts - 1), w=ws["bb_pre"], pad=1))
        self.fusion = layer("fusion", "feat_prop_module.fusion", [128, 128], tune=True)

        # ---- soft split / composite (tfocal_transformer.py:19-72)
        self.ss = layer("ss.embedding", "ss.embedding", [128], w=f("ss.embedding.weight").view(512, 128, 7, 7), stride=3, pad=3,
                        tune=True)
        # patch channel order c*49+tap -> tap*128+c (private layout of the fold kernels)
        wsc = f("sc.embedding.weight").view(128, 49, 512).permute(1, 0, 2).reshape(6272, 512).contiguous()
        bsc = f("sc.embedding.bias").view(128, 49).t().reshape(6272).contiguous()
        self.sc = layer("sc.embedding", None, w=wsc, b=bsc, tune=True)
        self.sc_bias_conv = layer("sc.bias_conv", "sc.bias_conv", [128], pad=1) if self.hq else None
        self.sc_bias_hwc = None if self.hq else f("sc.bias").permute(1, 2, 0).contiguous()
        # bf16 HQ: SoftComp in gather form (nine phase convolutions writing the folded image directly: no [tokens, 6272] tensor,
        # 813 MB at 720p T=10, and no fold kernel); other token grids than 3 x the feature size take the Linear + fold pair
        self.sc_gather = (ops.SoftCompGather(f("sc.embedding.weight"), f("sc.embedding.bias"), 128, dtype=self.dtype)
                          if x16 and self.hq else None)

        # ---- transformer blocks
        self.blocks = []
        for i in range(8):
            p = "transformer.%d." % i
            w1 = f(p + "mlp.conv1.0.weight").view(40, 49, 512).permute(1, 0, 2).reshape(1960, 512).contiguous()
            b1 = f(p + "mlp.conv1.0.bias").view(40, 49).t().reshape(1960).contiguous()
            if FC2_CONV or x16:
                # fc2: Linear(1960 -> 512) of the unfolded 7x7 patches == the 7x7 / stride 3 / pad 3 convolution of the folded
                # [F, H, W, 40] tensor (tfocal_transformer.py:81,95-97): no unfold kernel, no [rows, 1960] tensor
                fc2 = layer(p + "fc2", p + "mlp.conv2.1", [40], w=f(p + "mlp.conv2.1.weight").view(512, 40, 7, 7), stride=3, pad=3,
                            taps=True, tune=True)
            else:
                w2 = f(p + "mlp.conv2.1.weight").view(512, 40, 49).permute(0, 2, 1).reshape(512, 1960).contiguous()
                fc2 = layer(p + "fc2", p + "mlp.conv2.1", w=w2, tune=True)
            self.blocks.append(dict(
                pool_w=f(p + "pool_layers.0.weight").view(45), pool_b=f(p + "pool_layers.0.bias"),
                n1w=f(p + "norm1.weight"), n1b=f(p + "norm1.bias"), n2w=f(p + "norm2.weight"), n2b=f(p + "norm2.bias"),
                qkv=layer(p + "qkv", p + "attn.qkv", tune=True),
                proj=layer(p + "proj", p + "attn.proj", tune=True),
                fc1=layer(p + "fc1", None, w=w1, b=b1, tune=True),
                fc2=fc2,
                valid=sd[p + "attn.valid_ind_rolled"].cpu().tolist()))

        # ---- SPyNet (flow_comp.py:49-82,172-215).  In bf16 the conv stacks of the six pyramid levels run on bf16 MFMA (they are
        # 15 % of the 720p forward in fp32); the geometry stays fp32 -- pyramid images, warps, the flow itself and the residual sum
        # flow = up(flow) + net(...) (the last conv of a level adds the fp32 upsampled flow and stores fp32).
        self.spy = [[layer("spynet.%d.%d" % (lv, j), "update_spynet.basic_module.%d.basic_module.%d.conv" % (lv, j), [cin], pad=3,
                           nopk=True)
                     for j, cin in enumerate((8, 32, 64, 32, 16))] for lv in range(6)]
        mean = f("update_spynet.mean").view(3)
        std = f("update_spynet.std").view(3)
        one = torch.ones(1, device=self.device)
        self.spy_scale = torch.cat([1.0 / std, one]).contiguous()
        self.spy_shift = torch.cat([-mean / std, 0 * one]).contiguous()
        self.half = torch.full((4,), 0.5, device=self.device)
        self._tables = {}
        self._zeros = {}
        # SPyNet runs on a side stream next to the encoder, in both precision modes.  Round 1 found the side stream's
        # kernels corrupted beside bf16 MFMA tiles; round 2 traced it to packed-fp32 VALU instructions consuming freshly
        # loaded registers (tools/probe/overlap_probe.hip, DESIGN.md "Stream overlap"): every kernel that can run on the
        # side stream is built without them (csrc/misc.hip and the `nopk` build of conv.hip, e2fgvi_amd/build.py).
        self.overlap_flows = True
        self._side = None
        self._given = None         # (flows, encoder output) of segment graphs: runner.ShardedStep._capture_segments
        # frames through the encoder and the decoder, pairs through SPyNet, since construction (host integers: what
        # video.inpaint_video(reuse=True) saves is counted, not timed)
        self.counters = {"encoder_frames": 0, "flow_pairs": 0, "decoder_frames": 0}
        torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ helpers
    def weight_bytes(self):
        """device bytes of the packed weights the layers hold right now (each layer packs what the kernels it has run need:
        ops.PackedConv); the checkpoint's own tensors are not counted"""
        seen, total = set(), 0

        def walk(o):
            nonlocal total
            if id(o) in seen:
                return
            seen.add(id(o))
            if isinstance(o, (list, tuple)):
                for v in o:
                    walk(v)
            elif isinstance(o, dict):
                for v in o.values():
                    walk(v)
            elif hasattr(o, "weight_bytes") and o is not self:
                total += o.weight_bytes()
            elif isinstance(getattr(o, "wpacked", None), torch.Tensor):
                total += o.wpacked.numel() * o.wpacked.element_size()
            elif hasattr(o, "__dict__") and type(o).__module__.startswith("e2fgvi_amd") and o is not self:
                walk(list(vars(o).values()))
        walk(list(vars(self).values()))
        return total

    def _fork_ok(self):
        """Whether this forward may fork work onto a side stream: eager forwards only.  A forward being captured into a HIP graph
        stays on the capture stream, so that no captured graph has parallel branches -- the HIP runtime assigns a graph's branches
        to streams of its own at launch, and with a process's hardware queues at the runtime's default (4) replays of such graphs
        after earlier graphs were destroyed corrupted its state: the SIGSEGV in hip::Graph::UpdateStreams of DESIGN.md C8, and a
        host-heap corruption (`free(): invalid next size`) in a later capture of `bench.py`'s secondary lines.  Forwards in flight
        still overlap: each pipeline's graph replays whole on a stream of its own (runner.ShardedStep)."""
        return self.overlap_flows and not torch.cuda.is_current_stream_capturing()

    def _side_stream(self):
        """The side stream that belongs to the CURRENT stream: one per main stream a forward has been issued on.  With a single
        shared side stream, two eager forwards on two main streams (video.inpaint_video(in_flight=2)) raced through the caching
        allocator: a tensor allocated on the side stream is returned to that stream's pool when its forward ends on the HOST, the
        other forward's side work takes the block while the first forward's main-stream kernels -- which no wait of the second
        forward covers -- are still reading it (round 6: different bytes from the one-at-a-time run; graph replay, with its private
        pools and static buffers, was never exposed)."""
        if self._side is None:
            self._side = {}
        key = torch.cuda.current_stream(self.device).cuda_stream
        if key not in self._side:
            # (default priority on purpose: with a priority on EITHER branch of the captured forward -- this stream or the capture
            #  stream -- the replayed graph takes 21.9 ms instead of 12.0, profiles/r05_tile8_priority_ab.txt)
            self._side[key] = torch.cuda.Stream(device=self.device)
        return self._side[key]

    def _zero(self, shape, dtype=torch.float32):
        """a shared all-zero buffer (read-only), filled on first use: ops._lazy orders the fill before readers on other streams"""
        return ops._lazy(self._zeros, (dtype,) + tuple(shape), "zero buffer %s" % (tuple(shape),),
                         lambda: torch.zeros(tuple(shape), dtype=dtype, device=self.device))

    def _table(self, fh, fw, blk):
        key = (fh, fw, tuple(blk["valid"]))
        if key not in self._tables:
            tab, nk = build_key_table(fh, fw, blk["valid"])
            self._tables[key] = (torch.from_numpy(tab).to(self.device), torch.from_numpy(nk).to(self.device))
        return self._tables[key]

    # ------------------------------------------------------------------ flows
    def pair_table(self, pairs):
        """Device index tables of SPyNet runs for `pairs`, a host list of (i, j) frame positions: int32 [2, 2 P] -- row 0 the
        reference image and row 1 the support image of 2 P flow computations, the P flows i -> j first, then the P flows j -> i
        (e2fgvi.py:222-229 batches both directions the same way).  An upload: build it before the forwards that use it."""
        ref = [int(i) for i, _ in pairs]
        supp = [int(j) for _, j in pairs]
        return torch.tensor([ref + supp, supp + ref], dtype=torch.int32, device=self.device)

    def flows(self, frames, l_t):
        """frames: [b,t,3,H,W] in [-1,1].  Returns (fwd, bwd) NHWC [b, l_t-1, h, w, 2]."""
        b, t, c, H, W = frames.shape
        h, w = H // 4, W // 4
        local = frames[:, :l_t].reshape(b * l_t, c, H, W)
        if not local.is_contiguous():
            local = local.contiguous()
        key = ("pairs", b, l_t)
        if key not in self._tables:          # host->device uploads happen once (HIP-graph capture safe)
            self._tables[key] = self.pair_table([(bi * l_t + i, bi * l_t + i + 1) for bi in range(b) for i in range(l_t - 1)])
        fwd, bwd = self.pair_flows(local, self._tables[key])
        return fwd.view(b, l_t - 1, h, w, 2), bwd.view(b, l_t - 1, h, w, 2)

    def pair_flows(self, frames, pairs, downscale=4):
        """SPyNet on explicit pairs of a flat list of frames (the body of flows(): flow_comp.py:84-169, one pair at a time and
        independent of every other pair).  frames: [n,3,H,W] in [-1,1]; pairs: int32 device [2, 2 P] as pair_table() builds it
        (positions into `frames`).  Returns (forward, backward) NHWC fp32 [P, h, w, 2]: the flows i -> j and j -> i of pair (i, j).
        downscale = 4: h, w = H / 4, W / 4, the forward's flows on the 1/4 downsample (e2fgvi.py:214-219); downscale = 1: the same
        pyramid on the frames themselves, flows [P, H, W, 2] in pixels of the frames (metrics.video_flows); anything else raises
        ValueError."""
        ops._chk(pairs, "pairs", torch.int32)
        if pairs.dim() != 2 or pairs.shape[0] != 2 or pairs.shape[1] % 2 or pairs.shape[1] == 0:
            raise ValueError("pairs must be int32 [2, 2 P] (Engine.pair_table), got %s" % (tuple(pairs.shape),))
        if downscale not in (1, 4):
            raise ValueError("downscale must be 4 (the forward's 1/4-size flows) or 1 (flows at the frames' own size), got %r"
                             % (downscale,))
        n, c, H, W = frames.shape
        if downscale == 1:
            # a same-size resize with align_corners=True is the identity: only the layout change and [-1,1] -> [0,1] remain
            h, w = H, W
            small = ops.nchw_to_nhwc(frames, ld=4, scale=0.5, shift=0.5)
        else:
            h, w = H // 4, W // 4
            small = ops.resize_bilinear(frames, (h, w), True, src_nchw=True, out_ld=4, scale=self.half, shift=self.half)
        w_up = w if w % 32 == 0 else 32 * (w // 32 + 1)
        h_up = h if h % 32 == 0 else 32 * (h // 32 + 1)
        pyr = [ops.resize_bilinear(small, (h_up, w_up), False, channels=3, out_ld=4, scale=self.spy_scale,
                                   shift=self.spy_shift)]
        for _ in range(5):
            pyr.append(ops.avgpool2(pyr[-1]))
        pyr = pyr[::-1]
        nf = pairs.shape[1] // 2
        self.counters["flow_pairs"] += nf
        key = ("flow scale", h, w)
        if key not in self._tables:          # host->device uploads happen once (HIP-graph capture safe)
            self._tables[key] = torch.tensor([float(w) / float(w_up), float(h) / float(h_up)], dtype=torch.float32, device=self.device)
        sc = self._tables[key]
        ref_idx, supp_idx = pairs[0], pairs[1]
        flow = None
        for lv in range(6):
            # the fp32 level input (images, warped support image, upsampled flow); the bf16 path's convs read its bf16 copy
            if self.x16:
                inp, x = ops.spynet_level_input(pyr[lv], ref_idx, supp_idx, flow, copy_dtype=self.dtype)
            else:
                inp = x = ops.spynet_level_input(pyr[lv], ref_idx, supp_idx, flow)
            cv = self.spy[lv]
            x = cv[0]([x], act=ACT_RELU)
            x = cv[1]([x], act=ACT_RELU)
            x = cv[2]([x], act=ACT_RELU)
            x = cv[3]([x], act=ACT_RELU)
            flow = cv[4]([x], out_dtype=torch.float32, residual=inp, res_coff=6)          # + fp32 upsampled flow
        flow = ops.resize_bilinear(flow, (h, w), False, scale=sc)
        return flow[:nf], flow[nf:]

    def start_pair_flows(self, frames, pairs, fork=True):
        """pair_flows(frames, pairs) beside whatever the caller issues next on the current stream (the encoder on new frames, in the
        video driver's reuse=True): returns collect() -> (forward, backward), to be called once, on the same stream, when the flows
        are needed.  With a fork -- ``fork`` and an eager forward (_fork_ok) -- SPyNet is issued now on the current stream's side
        stream, which waits for the current stream first, and collect() makes the current stream wait for the side stream.  Without
        one nothing is issued now and collect() computes the flows on the current stream."""
        if not (fork and self._fork_ok()):
            return lambda: self.pair_flows(frames, pairs)
        main, side = torch.cuda.current_stream(self.device), self._side_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            flows = self.pair_flows(frames, pairs)

        def collect():
            main.wait_stream(side)
            return flows
        return collect

    # ------------------------------------------------------------------ encoder
    def encode(self, frames, join=None):
        """join: called in front of encoder.layers.<join_at> (16 at one clip: the fork's other branch, SPyNet, overlaps layers 0 .. 14;
        the bf16 path joins behind the encoder)"""
        b, t, c, H, W = frames.shape
        return self._encode(frames.reshape(b * t, c, H, W).contiguous(), b, join)

    def encode_frames(self, frames):
        """The encoder on a flat list of frames (e2fgvi.py:96-109 sees one frame at a time): [n,3,H,W] in [-1,1] ->
        [n, H/4, W/4, 128] in the engine's dtype."""
        return self._encode(ops._chk(frames, "frames"), 1, None)

    def _encode(self, frames, b, join):
        self.counters["encoder_frames"] += frames.shape[0]
        x = ops.nchw_to_nhwc(frames, ld=8 if self.x16 else 4, out_dtype=self.dtype)
        e = self.enc
        lr = dict(act=ACT_LRELU, slope=0.2)
        x = e[0]([x], **lr)
        x = e[1]([x], **lr)
        x = e[2]([x], **lr)
        x0 = e[3]([x], **lr)
        x = e[4]([x0], **lr)
        join_at = 18 if self.x16 else (JOIN_AT or (16 if b == 1 else 10))
        joined = join is None
        if not joined and join_at <= 10:
            join()
            joined = True
        for k in (5, 6, 7, 8):
            x = e[k]([x0, x], **lr)
            if not joined and (join_at <= 2 * k + 2 or k == 8):        # never leave the encoder with the fork open
                join()
                joined = True
        return x                                            # [n, h, w, 128]

    # ------------------------------------------------------------------ propagation
    def propagate(self, loc, flows_a, flows_b, inplace=False):
        """loc: [l_t, b, h, w, 128] frame-major local features.  flows_a / flows_b: fp32 NHWC [b,l_t-1,h,w,2]; they are
        bound positionally like the reference (e2fgvi.py:249-250): flows_a drives 'backward_', flows_b 'forward_'.
        Returns the propagated features [l_t, b, h, w, 128]; inplace: written over `loc` (the fusion layer's residual is `loc`
        itself: its epilogue reads a residual element and writes the same element in the same thread)."""
        l_t, b, h, w, ch = loc.shape
        dev = loc.device
        x16 = self.x16
        feats = {}
        zero = self._zero((b, h, w, ch), self.dtype)
        # 16-bit: the deformable conv gathers from copies of the propagated features re-laid out [group][pixel][16]: the 32-byte runs a
        # deform group's samples fetch are then adjacent for neighbouring pixels and share cache lines (NHWC: one run per 256-byte
        # pixel) -- tools/dcn_bench_x.py
        zero_dcn = self._zero((ch // 16, b, h, w, 16), self.dtype) if x16 else zero
        lk = dict(act=ACT_LRELU, slope=0.1)
        # the non-recurrent parts of conv_offset.0 / backbone.0 for the frames of steps 1 .. l_t - 1, all at once (see __init__);
        # step 0 of a direction (backbone only, needed at once) keeps the whole layer
        split = bool(self.prop_split) and b == 1 and l_t >= 3
        main = torch.cuda.current_stream()
        side = self._side_stream() if (split and self._fork_ok()) else None
        pre, ready = {}, {}
        if split:
            n1 = (l_t - 1) * b
            for k in ("off backward_", "bb backward_", "off forward_", "bb forward_"):
                pre[k] = torch.empty((l_t - 1, b, h, w, ch), dtype=torch.float32, device=dev)
            flat = lambda t: t.reshape(n1, h, w, ch)
            lb, lf = flat(loc[:l_t - 1]), flat(loc[1:])       # backward: steps 1.. are frames l_t-2 .. 0; forward: frames 1 .. l_t-1

            def beside(jobs):
                """jobs: (key, layer, sources) in the order the chain needs them; on the side stream when there is one"""
                if side is not None:
                    side.wait_stream(main)
                for key, layer, srcs in jobs:
                    if side is None:
                        layer(srcs, out=flat(pre[key]))
                        continue
                    with torch.cuda.stream(side):
                        layer(srcs, out=flat(pre[key]))
                        ready[key] = torch.cuda.Event()
                        ready[key].record(side)
            sb, sf = self.prop_split["backward_"], self.prop_split["forward_"]
            beside([("off backward_", sb["off_cur"], [lb]), ("bb backward_", sb["bb_pre"], [lb]), ("off forward_", sf["off_cur"], [lf])])

        def partial(key, slot):
            ev = ready.pop(key, None)
            if ev is not None:
                main.wait_event(ev)
            return pre[key][slot]
        for name, flows in (("backward_", flows_a), ("forward_", flows_b)):
            off_convs, dcn, bb = self.prop[name]
            sp = self.prop_split.get(name) if split else None
            if sp is not None and name == "forward_":
                beside([("bb forward_", sp["bb_pre"], [lf, flat(feats["backward_"][1:])])])
            store = torch.empty((l_t, b, h, w, ch), dtype=self.dtype, device=dev)
            order = list(range(l_t))
            if name == "backward_":
                order = order[::-1]
            img_stride = (l_t - 1) * h * w * 2
            hist = []                       # the propagated features in processing order: conv and flow-warp sources
            hist_dcn = [] if x16 else hist     # ... and the deformable conv's (16-bit: the [group][pixel][16] copies)
            aligned = zero
            for i, idx in enumerate(order):
                cur = loc[idx]
                if i > 0:
                    flow_a = flows[0, i - 1]
                    flow_b = flows[0, i - 2] if i > 1 else None
                    feat_n2 = hist[-2] if i > 1 else None
                    if x16:        # 16-bit warped features, and the flows as an 8-channel 16-bit source of conv_offset.0
                        cond, fl, fl_src = ops.prop_cond(hist[-1], feat_n2, flow_a, flow_b, img_stride, cond_dtype=self.dtype, flows8=True)
                    else:
                        cond, fl = ops.prop_cond(hist[-1], feat_n2, flow_a, flow_b, img_stride)
                        fl_src = fl
                    if sp is not None:
                        slot = idx if name == "backward_" else idx - 1
                        x = sp["off_rec"]([(cond, 0), (cond, ch), fl], residual=partial("off " + name, slot), **lk)
                    else:
                        x = off_convs[0]([(cond, 0), cur, (cond, ch), fl_src], **lk)
                    x = off_convs[1]([x], **lk)
                    x = off_convs[2]([x], **lk)
                    # 10*tanh + flow.flip / sigmoid (feat_prop.py:38-53) applied in the epilogue of the last conv_offset
                    # layer: the deformable conv then reads finished (fp32) offsets and masks
                    offs = off_convs[3]([x], out_dtype=torch.float32, residual=fl, act=ACT_DCNPOST, slope=10.0)
                    aligned = dcn([hist_dcn[-1], hist_dcn[-2] if i > 1 else zero_dcn], offs, out_dtype=self.dtype, planar=x16)
                if sp is not None and i > 0:
                    y = sp["bb_rec"]([aligned], residual=partial("bb " + name, idx if name == "backward_" else idx - 1), **lk)
                else:
                    srcs = [cur, feats["backward_"][idx], aligned] if name == "forward_" else [cur, aligned]
                    y = bb[0](srcs, **lk)
                hist.append(bb[1]([y], residual=aligned, out=store[idx]))
                if x16 and i + 1 < l_t:
                    hist_dcn.append(ops.to_planar16(store[idx]))
            feats[name] = store
        out = self.fusion([feats["backward_"].view(l_t * b, h, w, ch), feats["forward_"].view(l_t * b, h, w, ch)],
                          residual=loc.view(l_t * b, h, w, ch), out=loc.view(l_t * b, h, w, ch) if inplace else None)
        return out.view(l_t, b, h, w, ch)

    # ------------------------------------------------------------------ transformer
    def soft_split(self, feat):
        return self.ss([feat], out_dtype=torch.float32)     # [b*t, fh, fw, 512] fp32 tokens

    def block(self, i, x, b, t, fh, fw, hw, out2=None):
        """x: fp32 [b*t*fh*fw, 512] tokens in (b,t,y,x) order (the residual stream).  Returns (x_out fp32, attention-branch output
        fp32).  out2: a bf16 [b*t*fh*fw, 512] buffer that receives a bf16 copy of x_out (the bf16 path's compose() source)."""
        blk = self.blocks[i]
        H, W = hw
        tab, nk = self._table(fh, fw, blk)
        # LayerNorm output and the pooled windows share one buffer, and so do their qkv rows: ONE qkv GEMM for both
        # (and one buffer resource in the attention kernel)
        rows = x.shape[0]
        prow = b * t * (fh // 5) * (fw // 9)
        nbuf = torch.empty((rows + prow, 512), dtype=self.dtype, device=x.device)
        n1 = ops.layernorm(x, blk["n1w"], blk["n1b"], out=nbuf[:rows])
        ops.window_pool(n1, blk["pool_w"], blk["pool_b"], b * t, fh, fw, out=nbuf[rows:])
        if self.x16:
            both = blk["qkv"](nbuf)                                   # bf16 [rows + prow, 1536]
            att = ops.focal_attention_bf16(both[:rows], both[rows:], tab, nk, b, t, fh, fw)
        elif ops.attention_x3_applies(b, t, fh, fw):
            # both products on the bf16 matrix pipe (exactly split operands).  The k / v columns of all rows as three bf16 planes:
            # written by the qkv GEMM's epilogue when the split-operand GEMM runs it (round 5: no separate pass over the rows, and
            # the fp32 K / V columns are never stored), by e2fgvi_split3_kv otherwise (ops.PackedConv.__call__, kv_planes)
            planes = torch.empty((3, rows + prow, 1024), dtype=torch.bfloat16, device=x.device)
            both = blk["qkv"](nbuf, kv_planes=planes)
            att = ops.focal_attention_x3(both[:rows], planes, tab, nk, b, t, fh, fw)
        else:
            both = blk["qkv"](nbuf)
            att = ops.focal_attention(both[:rows], both[rows:], tab, nk, b, t, fh, fw)
        x1 = blk["proj"](att, out_dtype=torch.float32, residual=x)
        n2 = ops.layernorm(x1, blk["n2w"], blk["n2b"], out_dtype=self.dtype)
        hid = blk["fc1"](n2)
        # GELU in front of the unfold (a gather with zero padding: GELU commutes with it, 5.4x fewer erf evaluations)
        folded = ops.ffn_fold_gelu(hid, b * t, fh, fw, H, W, 40)
        if isinstance(blk["fc2"], PackedConvX):
            y = torch.empty((rows, 512), dtype=torch.float32, device=x.device)
            blk["fc2"]([folded], out=y.view(b * t, fh, fw, 512), residual=x1.view(b * t, fh, fw, 512),
                       out2=None if out2 is None else out2.view(b * t, fh, fw, 512))
            return y, x1
        unf = ops.ffn_unfold(folded, fh, fw, out=hid)
        return blk["fc2"](unf, residual=x1), x1

    def compose(self, tokens, enc, b, t, fh, fw):
        """SoftComp + residual with the encoder features (tfocal_transformer.py:65-72, e2fgvi.py:258).  tokens: in the
        activations' dtype."""
        _, h, w, ch = enc.shape
        if self.sc_gather is not None and (h, w) == (3 * fh, 3 * fw):
            folded = self.sc_gather(tokens.view(b * t, fh, fw, 512))
            return self.sc_bias_conv([folded], residual=enc)
        emb = self.sc(tokens)
        if self.hq:
            folded = ops.softcomp_fold(emb, b * t, fh, fw, h, w, ch)
            return self.sc_bias_conv([folded], residual=enc)
        return ops.softcomp_fold(emb, b * t, fh, fw, h, w, ch, bias_hwc=self.sc_bias_hwc, residual=enc)

    # ------------------------------------------------------------------ decoder
    def decode(self, x):
        n, h, w, _ = x.shape
        self.counters["decoder_frames"] += n
        lr = dict(act=ACT_LRELU, slope=0.2)
        d = self.dec
        x = ops.resize_bilinear(x, (2 * h, 2 * w), True)
        x = d[0]([x], **lr)
        x = d[1]([x], **lr)
        x = ops.resize_bilinear(x, (4 * h, 4 * w), True)
        x = d[2]([x], **lr)
        return d[3]([x], act=ACT_TANH, out_nchw=True)             # 64 -> 3, tanh, fp32 NCHW frames

    # ------------------------------------------------------------------ whole forward (e2fgvi_hq.py:235-263)
    def forward(self, frames, l_t, trace=None, given=None, decode_local=False):
        """trace: a dict that receives fp32 copies of the stage outputs (flows, encoder, propagation, tokens, decoder input)

        given = ((fwd, bwd), enc): the per-pair and per-frame stages computed by the caller -- flows fp32 NHWC [b, l_t-1, h, w, 2]
        (pair_flows / flows) and encoder features [b*t, h, w, 128] in the engine's dtype (encode_frames / encode) -- instead of
        running SPyNet and the encoder here; no side-stream fork then.  `enc` is CONSUMED: at one clip the propagated features
        are written over its local frames, so hand in a copy of anything that is to be used again (video.inpaint_video(reuse=True)
        gathers a fresh window tensor from its cache).  `frames` may then be None: only its shape is used.

        decode_local=True: compose and decode only the first l_t frames of the clip -- all t frames still pass through the
        transformer -- and return [l_t,3,H,W] frames.  One clip only: at b == 1 the local frames' tokens are the leading rows;
        b > 1 raises ValueError."""
        if given is None:
            given = self._given
        if frames is None:
            if given is None:
                raise ValueError("frames may be None only with given=((fwd, bwd), enc)")
            (g_fwd, _), g_enc = given
            b = g_fwd.shape[0]
            t, c, H, W = g_enc.shape[0] // b, 3, 4 * g_enc.shape[1], 4 * g_enc.shape[2]
        else:
            b, t, c, H, W = frames.shape
        if H % 4 or W % 4:
            raise ValueError("H and W must be multiples of 4")
        h, w = H // 4, W // 4
        fh, fw = token_grid(h, w)
        if fh % 5 or fw % 9:
            raise ValueError("token grid %dx%d is not a multiple of (5,9): pad H to a multiple of 60 and W to a "
                             "multiple of 108 (reference test.py:156-165)" % (fh, fw))
        if not self.hq and (h, w) != (60, 108):
            raise ValueError("model 'e2fgvi' is fixed to 432x240 inputs (sc.bias is [128,60,108]); use e2fgvi_hq")
        if not (1 <= l_t <= t):
            raise ValueError("num_local_frames must be in [1, t]")
        if decode_local and b != 1:
            raise ValueError("decode_local=True takes one clip per forward (b == 1), got b = %d" % b)
        if frames is not None:
            frames = ops._chk(frames.float().contiguous(), "masked_frames")
        if given is not None:
            (fwd, bwd), enc = given
            ops._chk(fwd, "given flows (forward)"); ops._chk(bwd, "given flows (backward)"); ops._chk(enc, "given encoder features", self.dtype)
            if tuple(fwd.shape) != (b, l_t - 1, h, w, 2) or tuple(bwd.shape) != tuple(fwd.shape) or tuple(enc.shape) != (b * t, h, w, 128):
                raise ValueError("given: flows must be [%d,%d,%d,%d,2] and the encoder features [%d,%d,%d,128], got %s, %s and %s"
                                 % (b, l_t - 1, h, w, b * t, h, w, tuple(fwd.shape), tuple(bwd.shape), tuple(enc.shape)))
        elif l_t == 1:
            # a one-frame local window (test.py on a 1-frame video): the reference's flow tensors are empty
            # [b,0,2,h,w] and each propagation direction is backbone(cat(x, 0)) (feat_prop.py:105,131-137)
            fwd = bwd = torch.empty((b, 0, h, w, 2), dtype=torch.float32, device=frames.device)
            enc = self.encode(frames)
        elif self._fork_ok():
            # SPyNet (many short, small-channel launches) and the encoder (few large launches) are independent:
            # run them on two HIP streams so the flow pyramid fills the gaps of the encoder (eager forwards only: _fork_ok)
            main = torch.cuda.current_stream()
            side = self._side_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                fwd, bwd = self.flows(frames, l_t)
            enc = self.encode(frames, join=lambda: main.wait_stream(side))
        else:
            fwd, bwd = self.flows(frames, l_t)
            enc = self.encode(frames)
        ch = enc.shape[3]
        if trace is not None:
            trace["flow_fwd"], trace["flow_bwd"], trace["enc"] = fwd, bwd, enc.to(torch.float32, copy=True)
        enc5 = enc.view(b, t, h, w, ch)
        if b == 1:
            loc = enc5[0, :l_t].unsqueeze(1)                 # view: [l_t, 1, h, w, C]
            # one clip, fp32: the local frames are a view of the encoder output and the propagated features replace them in place
            # (no 33 MB copy; under E2FGVI_AUTOTUNE=1 the fusion layer writes a fresh tensor so that its candidates can be timed)
            inplace = not (ops.AUTOTUNE or self.x16)
            prop = self.propagate(loc, fwd, bwd, inplace=inplace)
            if not inplace:
                enc5[0, :l_t].copy_(prop[:, 0])
        else:
            loc = enc5[:, :l_t].permute(1, 0, 2, 3, 4).contiguous()
            prop = self.propagate(loc, fwd, bwd)
            enc5[:, :l_t].copy_(prop.permute(1, 0, 2, 3, 4))
        if trace is not None:
            trace["prop"] = enc.to(torch.float32, copy=True)
        tok = self.soft_split(enc).view(b * t * fh * fw, 512)
        if trace is not None:
            trace["tokens0"] = tok.clone()
        tok16 = None
        for i in range(8):
            if self.x16 and i == 7:        # the 16-bit path's compose() reads a 16-bit copy of the last block's tokens
                tok16 = torch.empty((b * t * fh * fw, 512), dtype=self.dtype, device=tok.device)
            tok, x1 = self.block(i, tok, b, t, fh, fw, (h, w), out2=tok16)
            if trace is not None:
                trace["block%d_attn_out" % i] = x1
                trace["tokens%d" % (i + 1)] = tok
        last = tok if tok16 is None else tok16
        if decode_local:                   # b == 1: the local frames are the leading rows of the tokens and of `enc`
            dec_in = self.compose(last[:l_t * fh * fw], enc[:l_t], 1, l_t, fh, fw)
        else:
            dec_in = self.compose(last, enc, b, t, fh, fw)
        if trace is not None:
            trace["dec_in"] = dec_in.float()
        out = self.decode(dec_in)
        if l_t == 1:
            empty = torch.empty((b, 0, 2, h, w), dtype=torch.float32, device=out.device)
            return out, (empty, empty.clone())
        flows_out = (ops.nhwc_to_nchw(fwd.reshape(b * (l_t - 1), h, w, 2)).view(b, l_t - 1, 2, h, w),
                     ops.nhwc_to_nchw(bwd.reshape(b * (l_t - 1), h, w, 2)).view(b, l_t - 1, 2, h, w))
        return out, flows_out
