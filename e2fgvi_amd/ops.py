"""Host-side operator layer: torch tensors in, libe2fgvi_hip.so kernels out.

torch is used only as device-memory owner and stream provider; all arithmetic happens in the
hand-written HIP kernels behind the C ABI (include/e2fgvi_hip.h).  Activations are NHWC
``[N, H, W, ld]`` fp32 contiguous CUDA tensors.  Every wrapper validates device / dtype / layout
and raises on error -- there is no eager fallback.
"""
import collections
import ctypes as C
import math
import numbers
import os

import torch

from . import lib as _L

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_DCNPOST = _L.ACT_NONE, _L.ACT_RELU, _L.ACT_LRELU, _L.ACT_TANH, _L.ACT_DCNPOST


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA (ROCm) tensor -- the HIP path has no CPU fallback" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def empty_nhwc(n, h, w, c, device):
    return torch.empty((n, h, w, c), dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------ conv / linear
# implicit-GEMM tile codes worth timing on GEMM-shaped layers (64x64 / 128x128 / 64x128 / 128x256 / 256x128 shapes with
# 16- and 32-deep K steps); 0 = the library's static choice
TUNE_CANDIDATES = (0, 213, 223, 211, 219, 216)
# Winograd block shapes: 16x16-pixel blocks x 64 / 32 couts, 8x16-pixel blocks x 32 / 64 couts
WINO_CANDIDATES = (64, 132, 164, 32)
# wide-tile Winograd variant (csrc/conv_wino4.hip): tile code -> (fy, couts per workgroup); F(2x4,3x3) issues 3 multiplies per
# output and input channel (F(2x2,3x3): 4).  Round 6 pruned the shapes that never won a layer (F(2x4) x 32 couts, F(4x4) x 32:
# profiles/r02_wino4_bench.txt) together with their instantiations and the E2FGVI_WINO4* switches that forced them.
W4_CODES = {2464: (2, 64)}
_W4_MINPIX = 20000          # output pixels from which PackedConv._wino4_rule hands a qualifying layer to F(2x4)
# bf16 data path (conv_bf16x): 128x128, 64x128, 256x128 and 256x256 (8 waves), 128x64, 64x64, 128x32 tiles; tile codes +10
# are the row-shift variants for 3x3 stride-1 pad-1 layers (the three horizontal taps share one A stage).
# 107 / 108: the ping-pong forms of 7 / 8, split-operand layers only (others: EUNSUP, skipped)
# 51 / 52: split-operand 7x7 stride-1 layers from an LDS halo patch (conv_bf16x.hip conv_halo_x3_kernel: 16x16- and 8x16-pixel tiles);
#          timed only where PackedConvX._halo_x3 says the geometry qualifies (SPyNet's 32 -> 64 and 64 -> 32 layers), EUNSUP anywhere else
XTUNE_CANDIDATES = (1, 4, 6, 7, 8, 2, 5, 3, 107, 108, 51, 52)
XTUNE_HALO = (51, 52)
XTUNE_ROWSHIFT = (11, 16, 17, 12, 13, 18)
# fp32 layers on the bf16 matrix pipe by exact operand splitting (conv_bf16x.hip MODE 2, PackedConvX(x3=True)): a tuning
# alternative of every fp32 layer that asks for it (PackedConv.try_x3 / PackedConvX.try_x3); taken when its best tile beats
# the fp32 kernel of the call by more than X3_MARGIN.  Tile codes X3_BASE + tile in the decision table (clear of the Winograd
# code 2464 and of the DMA_BASE + tile codes of the LDS-DMA fp32 kernel).  E2FGVI_X3=0: never.
X3_ENABLED = os.environ.get("E2FGVI_X3", "1") != "0"
X3_MARGIN = 0.97
X3_BASE = 30000
# ... and the Winograd F(2x2,3x3) kernel with split operands (conv_wino.hip, X3 build): codes W3_BASE + its block shape
W3_BASE = 40000
# (+ 1000: LDS-DMA patch staging with two stages of lookahead -- measured slower everywhere; 5132: four positions per wave in
#  four-wave workgroups, two per CU: 5-20 % ahead of 132 on the batched layers, level with 164 where 64 couts per workgroup fit;
#  6064 (round 4): 16x16-pixel blocks x 64 couts, single-buffered weights reloaded in place, patch by LDS-DMA)
W3_CANDIDATES = (132, 164, 32, 5132, 6064)
# The wide-tile split-operand Winograd kernel (6064) is a candidate of every 3x3 layer, whatever runs beside it (round 5).  Round 4
# restricted it to layers with the chip to themselves (a per-layer flag): beside the SPyNet stream it returned wrong 16x16-pixel
# blocks.  Root cause: the weight loads for the stage past the end were in flight while the compiler had reused their
# registers for the epilogue's addresses; fixed in conv_wino.hip for every Winograd kernel, guarded by build.verify_exit_reuse() and
# by tests/test_gpu_hazards.py (every selectable kernel beside device copies, bit-equal to the unaccompanied launch).
# (The A/B switches of rounds 3-5 whose verdict is in: E2FGVI_W3_WIDE, _W3_SKIP, _KV_EPILOGUE, _DCN_TILE, _TAPS, _SCG_TILE, _ATT_X3
#  are gone since round 6; what remains selectable from the environment is listed once)
W3_WIDE = 6064
W3_WIDE_FALLBACK = 164
# the LDS-DMA fp32 GEMM (PackedConvX on fp32 operands) as the alternative of a tuned PackedConv: codes DMA_BASE + its tile
DMA_BASE = 2000


def _decode(code):
    """(family, arg) of a tile code -- the one place that knows the number space of the decision table and of the `tile` argument:
    "own"  the layer's own kernel, arg = its tile (0: the library's static choice; Winograd block shapes; halo ids from 10000)
    "w4"   the wide-tile fp32 Winograd kernel, arg = the code itself, a key of W4_CODES
    "dma"  the LDS-DMA fp32 GEMM, arg = code - DMA_BASE, its tile
    "x3"   the split-operand GEMM, arg = code - X3_BASE, its tile
    "w3"   the split-operand Winograd kernel, arg = code - W3_BASE, its block shape"""
    if code >= W3_BASE:
        return "w3", code - W3_BASE
    if code >= X3_BASE:
        return "x3", code - X3_BASE
    if code in W4_CODES:
        return "w4", code
    if DMA_BASE <= code < DMA_BASE + 100:
        return "dma", code - DMA_BASE
    return "own", code


_TUNED = {}      # (layer geometry, input size class) -> tile code; shared by all layers of the same geometry (the 8 blocks)
# Kernel selection is DETERMINISTIC by default (round 4): the decisions come from the checked-in table e2fgvi_amd/tile_table.py
# (generated on an MI355X by tools/make_tile_table.py from timed runs of the BASELINE configurations), looked up by layer
# geometry and size class; a geometry the table does not hold at this size takes its decision at the nearest tabled size class,
# and one it does not hold at all runs the library's static default.  No timing, no files: two processes -- and every rank of a
# sharded job -- run the same kernels in the same accumulation order and return the same bits.
#   E2FGVI_AUTOTUNE=1   time the candidates on the first eager call of each (geometry, size class) instead (what generates the
#                       table); those decisions are persisted per library build under e2fgvi_amd/.tile_cache/ (or
#                       $E2FGVI_CACHE_DIR; E2FGVI_TUNE_FILE=<path> names the file, =0 disables) so that a profiled run replays them
#   E2FGVI_TILE_TABLE=0 ignore the table (every layer on its static default kernel); =<file.py>: that table instead of the checked-in one
AUTOTUNE = os.environ.get("E2FGVI_AUTOTUNE", "0") == "1"
TUNE_REPS = max(1, int(os.environ.get("E2FGVI_TUNE_REPS", "1") or 1))      # x the timed launches per candidate (table generation: 4)
TABLE_FORMAT = 2          # bump when the meaning of a key field or of a tile code changes: older tables / cache files are ignored
_SIZE_FIELD = 8           # position of the size class in both key layouts (PackedConv / PackedConvX)


def _default_tune_file():
    try:
        st = os.stat(_L.LIB_PATH)
        d = os.environ.get("E2FGVI_CACHE_DIR") or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".tile_cache")
        os.makedirs(d, exist_ok=True)
        dev = "gpu"
        if torch.cuda.is_available():
            dev = "".join(ch for ch in torch.cuda.get_device_properties(0).gcnArchName.split(":")[0] if ch.isalnum())
        return os.path.join(d, "tiles_v%d_%s_%x_%x.txt" % (TABLE_FORMAT, dev, st.st_size, int(st.st_mtime)))
    except (OSError, RuntimeError):
        return None


_TUNE_FILE = None
if AUTOTUNE:
    _TUNE_FILE = os.environ.get("E2FGVI_TUNE_FILE")
    if _TUNE_FILE is None:
        _TUNE_FILE = _default_tune_file()
    elif _TUNE_FILE in ("", "0"):
        _TUNE_FILE = None
    if _TUNE_FILE and os.path.exists(_TUNE_FILE):
        import ast
        for _line in open(_TUNE_FILE):
            try:
                _k, _v = ast.literal_eval(_line)
                _TUNED[_k] = _v
            except Exception:           # a torn line of a concurrent writer: that geometry is simply tuned again
                pass
elif os.environ.get("E2FGVI_TILE_TABLE", "1") != "0":
    try:
        if os.environ.get("E2FGVI_TILE_TABLE", "1").endswith(".py"):       # another table of the same format (A/B runs, integrators)
            import importlib.util
            _spec = importlib.util.spec_from_file_location("e2fgvi_tile_table_override", os.environ["E2FGVI_TILE_TABLE"])
            _tt = importlib.util.module_from_spec(_spec)
            _spec.loader.exec_module(_tt)
        else:
            from . import tile_table as _tt
        if getattr(_tt, "TABLE_FORMAT", None) == TABLE_FORMAT:
            _TUNED.update(_tt.TILES)
    except ImportError:
        pass


def _remember(key, tile):
    _TUNED[key] = tile
    if _TUNE_FILE:
        try:
            with open(_TUNE_FILE, "a") as fh:
                fh.write(repr((key, tile)) + "\n")
        except OSError:
            pass
    return tile


def _decision(key):
    """the tile code recorded for `key`; without timing-based tuning also the one of the nearest tabled size class of the same
    geometry (a decision taken a quarter octave away is still a good one, and it is the same in every process)"""
    best = _TUNED.get(key)
    if best is not None or AUTOTUNE:
        return best
    hit = _NEAREST.get(key)
    if hit is None:
        sc = key[_SIZE_FIELD]
        cands = [(abs(k[_SIZE_FIELD] - sc), k[_SIZE_FIELD], v) for k, v in _TUNED.items()
                 if len(k) == len(key) and k[:_SIZE_FIELD] == key[:_SIZE_FIELD] and k[_SIZE_FIELD + 1:] == key[_SIZE_FIELD + 1:]]
        hit = _NEAREST[key] = (min(cands)[2] if cands else -1)
    return None if hit < 0 else hit


_NEAREST = {}


def sync_tile_decisions(group=None, src=0):
    """Sharded jobs under E2FGVI_AUTOTUNE=1: every rank adopts rank `src`'s tile table, so that all ranks run the same kernels
    in the same accumulation order (timed choices differ per process, and the alternatives order their K loop differently).
    Call after the first (tuning) forward.  With the default table-driven selection every rank already holds the same table
    and the broadcast only confirms it."""
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return False
    box = [dict(_TUNED) if dist.get_rank(group) == src else None]
    dist.broadcast_object_list(box, src=src, group=group)
    _TUNED.clear()
    _TUNED.update(box[0])
    _NEAREST.clear()
    return True


def _no_capture(what):
    """Weight packings are built lazily, on the first call that runs their kernel.  That first call must be an eager one: under
    HIP-graph capture the allocation would come from the graph's private pool and the pack kernel would be captured -- re-packed on
    every replay, dangling for eager calls once the graph is freed (advisor finding of round 4).  runner.ShardedStep runs an eager
    forward before it captures; a caller that captures without one is told so here instead of getting a stale pointer later."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("%s: first use of this kernel's weight packing under HIP-graph capture -- run one eager forward of the "
                           "same shapes before capturing (runner.ShardedStep does)" % what)


# Lazily built device state (weight packings, zero buffers, bias images, the engine itself) is built on whatever stream is current
# at its first use and then read by kernels of ANY stream: video.inpaint_video(in_flight=K) runs consecutive windows on K streams
# that nothing orders with each other.  Every such object is built and fetched through _lazy(), the one seam: the build records
# an event on its stream, and a fetch on another stream makes that stream wait for it.  Once the event has
# completed the entry is dropped, so a warm forward pays one truth test of an empty list per fetch and nothing else.
_PENDING = []    # [id of the producer's stream, event recorded behind the producer, ids of the streams that wait on it already]


def _await_pending():
    """The current stream waits for every lazily built object whose producer (on another stream) may not have run yet: device-side
    waits, never a host synchronisation.  Under graph capture nothing is pending by contract: torch.cuda.graph synchronises
    the device before it begins to capture, and _lazy() builds nothing under capture."""
    if torch.cuda.is_current_stream_capturing():
        return
    cur = torch.cuda.current_stream()
    live = []
    for ent in _PENDING:
        sid, ev, waiting = ent
        if ev.query():
            continue
        live.append(ent)
        if sid != cur.cuda_stream and cur.cuda_stream not in waiting:
            cur.wait_event(ev)
            waiting.add(cur.cuda_stream)
    _PENDING[:] = live


def _lazy(store, key, what, build):
    """``store[key]``, built by ``build()`` on the current stream if it is not there yet (never under HIP-graph capture:
    _no_capture), and safe to hand to a kernel on the current stream either way.  ``store`` is a dict, or ``vars(obj)`` for an
    attribute that starts out as None."""
    obj = store.get(key)
    if obj is None:
        _no_capture(what)
        obj = store[key] = build()
        if torch.cuda.is_available():
            ev = torch.cuda.Event()
            ev.record()
            _PENDING.append([torch.cuda.current_stream().cuda_stream, ev, set()])
    elif _PENDING:
        _await_pending()
    return obj


def _time_launches(launch, reps):
    """device time in ms per launch of `reps` back-to-back `launch()` calls on the current stream (hip events); the one event
    loop of table generation"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _pack_weights(size_fn, pack_fn, src, dtype, what, *geom, extra=()):
    """`src` (fp32 checkpoint weights) re-laid-out for one kernel: the library's size query `size_fn(*geom)`, a `dtype` tensor of
    that many elements on src's device, filled by `pack_fn(src, dst, *geom, *extra, stream)`.  `what` names both in error messages."""
    n = size_fn(*geom)
    if n < 0:
        _L.check(int(n), "packed_%s_size" % what)
    t = torch.empty(int(n), dtype=dtype, device=src.device)
    _L.check(pack_fn(_ptr(src), _ptr(t), *geom, *extra, _stream()), "pack_" + what)
    return t


def _image_chunks(N, per_img):
    """(n0, n1) image ranges of a batch whose kernel addresses each tensor through a 32-bit buffer resource: a batch that spans
    >= 4 GiB (`per_img` bytes per image in its largest tensor) is processed in chunks of images -- images are independent"""
    step = max(1, N)
    if N > 1 and N * per_img >= (1 << 32) - 1:
        step = max(1, ((1 << 32) - 2) // per_img)
    for n0 in range(0, N, step):
        yield n0, min(N, n0 + step)


class _ConvLayer:
    """What the two conv / linear layer classes share: the layer geometry, the image chunks and the call descriptor's common
    fields (ConvDesc and ConvXDesc agree on them by name)."""

    def _init_layer(self, weight, bias, cpg, groups, stride, pad):
        """geometry, bias and the defaults the engine overwrites; returns the fp32 OIHW weight (a Linear's [Cout, Cin] as 1x1)"""
        if weight.dim() == 2:
            weight = weight[:, :, None, None]
        w = _chk(weight.detach().float().contiguous(), "weight")
        self.Cout, cin_g, self.KH, self.KW = w.shape
        self.cpg = [int(c) for c in cpg]
        if sum(self.cpg) != cin_g:
            raise ValueError("sum(cpg)=%d != weight input channels %d" % (sum(self.cpg), cin_g))
        self.groups, self.stride, self.pad = groups, stride, pad
        self.bias = None if bias is None else _chk(bias.detach().float().contiguous(), "bias")
        self.name = "conv"         # layer name for launch traces (the engine sets the checkpoint key)
        self.tune = False          # take the tile from the decision table (E2FGVI_AUTOTUNE=1: time the candidates per size class)
        self.try_x3 = False        # fp32 layers: the split-bf16 kernels (PackedConvX x3, codes X3_BASE + tile) are alternatives
        self.alt3 = None
        return w

    def out_hw(self, H, W):
        return ((H + 2 * self.pad - self.KH) // self.stride + 1, (W + 2 * self.pad - self.KW) // self.stride + 1)

    def _cpg_arr(self):
        return (C.c_int32 * len(self.cpg))(*self.cpg)

    def _srcs_out(self, sources, out, out_nchw, out_dtype):
        """the sources as (tensor, channel offset) pairs, and `out` -- a fresh tensor if the caller gave none"""
        srcs = [(s, 0) if isinstance(s, torch.Tensor) else s for s in sources]
        if len(srcs) != len(self.cpg):
            raise ValueError("expected %d sources, got %d" % (len(self.cpg), len(srcs)))
        if out is None:
            N, H, W, _ = srcs[0][0].shape
            Ho, Wo = self.out_hw(H, W)
            out = torch.empty((N, self.Cout, Ho, Wo) if out_nchw else (N, Ho, Wo, self.Cout),
                              dtype=torch.float32 if out_nchw else out_dtype, device=srcs[0][0].device)
        return srcs, out

    def _x_alternative(self, **kw):
        """this fp32 layer as a PackedConvX on fp32 operands (the build function of the _alt / _alt3 accessors)"""
        alt = PackedConvX(self._w_raw, self.bias, self.cpg, groups=self.groups, stride=self.stride, pad=self.pad, dtype=torch.float32, **kw)
        alt.name = self.name
        return alt

    def _fill(self, d, src_dtype, chk, srcs, out, out_coff, act, slope, out_nchw):
        """validates sources (`src_dtype`) and out (by `chk`: _chk or _chk_any) and fills the fields ConvDesc and ConvXDesc have
        in common; the residual's follow from _fill_residual"""
        N, H, W, _ = srcs[0][0].shape
        Ho, Wo = self.out_hw(H, W)
        for i, (t, coff) in enumerate(srcs):
            _chk(t, "source %d" % i, src_dtype)
            if t.dim() != 4 or tuple(t.shape[:3]) != (N, H, W):
                raise ValueError("source %d shape %s does not match [%d,%d,%d,*]" % (i, tuple(t.shape), N, H, W))
            d.src[i], d.src_ld[i], d.src_coff[i], d.src_cpg[i] = t.data_ptr(), t.shape[3], coff, self.cpg[i]
        d.nsrc = len(srcs)
        d.N, d.H, d.W, d.Ho, d.Wo = N, H, W, Ho, Wo
        d.KH, d.KW, d.stride, d.pad = self.KH, self.KW, self.stride, self.pad
        d.groups, d.Cout = self.groups, self.Cout
        d.bias = self.bias.data_ptr() if self.bias is not None else None
        chk(out, "out")
        if out_nchw:
            if tuple(out.shape) != (N, self.Cout, Ho, Wo) or out.dtype != torch.float32:
                raise ValueError(self._NCHW_ERROR % dict(got=tuple(out.shape), want=(N, self.Cout, Ho, Wo)))
            d.dst_ld, d.dst_coff, d.dst_nchw = 0, 0, 1
        else:
            if out.dim() != 4 or tuple(out.shape[:3]) != (N, Ho, Wo):
                raise ValueError("out shape %s != [%d,%d,%d,*]" % (tuple(out.shape), N, Ho, Wo))
            d.dst_ld, d.dst_coff, d.dst_nchw = out.shape[3], out_coff, 0
        d.dst = out.data_ptr()
        d.act, d.slope, d.tile = act, slope, 0
        return d

    @staticmethod
    def _fill_residual(d, chk, residual, res_coff):
        if residual is not None:
            chk(residual, "residual")
            if residual.dim() != 4 or tuple(residual.shape[:3]) != (d.N, d.Ho, d.Wo):
                raise ValueError("residual shape %s != [%d,%d,%d,*]" % (tuple(residual.shape), d.N, d.Ho, d.Wo))
            d.residual, d.res_ld, d.res_coff = residual.data_ptr(), residual.shape[3], res_coff


# what PackedConv._select hands to PackedConv._launch: the kernel family and tile to run (_decode), the static rule's (family,
# tile) that a rejected alternative falls back to, whether the decision came from the table, whether the call is a Winograd one
_Plan = collections.namedtuple("_Plan", "family tile static from_table use_wino")
# one PackedConv call on its way through the steps: the C descriptor, the sources as (tensor, channel offset) pairs, the call's
# other arguments by keyword (as PackedConvX.__call__ and both _desc take them) and the K / V planes to write, or None
_Call = collections.namedtuple("_Call", "d srcs kw kv_planes")


class PackedConv(_ConvLayer):
    """A conv / linear layer with weights re-laid-out once for the MFMA kernel.

    weight: torch OIHW ``[Cout, sum(cpg), KH, KW]`` (a Linear weight ``[Cout, Cin]`` is 1x1).
    cpg:    channels per group contributed by each source of the virtual input concat.

    A call is four steps: _desc (the C descriptor), _select (static rule and decision table -> a _Plan; _tune times the
    candidates for a new table row under E2FGVI_AUTOTUNE=1), _launch.
    """

    _NCHW_ERROR = "NCHW out shape %(got)s != %(want)s"

    def __init__(self, weight, bias, cpg, groups=1, stride=1, pad=0, bk=None, precision="fp32", algo="igemm"):
        """precision: "fp32" only: fp32 tensors and fp32-level rounding -- the layer's own kernels are fp32 MFMA (bit-equivalent
        to an fp32 FMA chain); with try_x3 the decision table may hand the call to the split-operand kernels (three exact bf16
        pieces per operand, six bf16 MFMA terms per product: fp32-level, not bit-identical).  The bf16 data path has its own
        layer class, PackedConvX.
        algo: "igemm" (implicit GEMM), "winograd" (fp32 F(2x2,3x3) only; 3x3 / stride 1 / pad 1, every cpg % 4 == 0,
        even H and W at call time, NHWC output) or "auto" (both packings; Winograd whenever a call qualifies)."""
        lib = _L.load()
        w = self._init_layer(weight, bias, cpg, groups, stride, pad)
        if precision != "fp32":
            raise ValueError("PackedConv is the fp32 layer; the bf16 data path uses PackedConvX")
        self.precision = precision
        self.nopk = False          # True: the build without packed-fp32 VALU (side-stream launches beside bf16 MFMA tiles)
        self.alt = None
        self._w_raw = w            # for the alternative LDS-DMA kernels (built on the first tuned call)
        if algo not in ("igemm", "winograd", "auto"):
            raise ValueError("algo must be 'igemm', 'winograd' or 'auto'")
        wino_ok = (self.KH, self.KW, stride, pad) == (3, 3, 1, 1) and not any(c % 4 for c in self.cpg)
        if algo == "winograd" and not wino_ok:
            raise ValueError("winograd needs fp32, 3x3 / stride 1 / pad 1 and channels per source in multiples of 4")
        if algo == "auto":
            algo = "auto" if wino_ok else "igemm"
        self.algo = algo
        self._w4 = {}              # fy -> packed F(fy x 4, 3x3) weights, built on first use
        self._w3 = None            # packed weights of the split-bf16 Winograd kernel, built on first use
        self._w_oihw = w if algo in ("winograd", "auto") else None
        # every packing (implicit GEMM, Winograd F(2x2), F(2x4), the three-plane split ones, the LDS-DMA alternatives) is built from
        # _w_raw on the first call that runs it: with the kernel table (tile_table.py) a layer holds the packing of the kernel it
        # runs and nothing else; E2FGVI_AUTOTUNE=1 builds every candidate's (weight memory)
        self._own = {}
        if algo in ("winograd", "auto"):       # a geometry the library rejects raises here, not on the first call
            _L.check(min(0, int(lib.e2fgvi_packed_winograd_weight_size(*self._wgeom()))), "packed_winograd_weight_size")
        if algo == "winograd":
            self.bk = 8
            return
        if bk is None:
            # K-chunk granule: 32 unless padding every source up to a multiple of 32 wastes more than ~8 % of K
            pad32 = sum((c + 31) // 32 * 32 for c in self.cpg)
            pad16 = sum((c + 15) // 16 * 16 for c in self.cpg)
            bk = 32 if pad32 <= 1.08 * sum(self.cpg) else (16 if pad16 <= 1.08 * sum(self.cpg) else 8)
        self.bk = bk
        _L.check(min(0, int(lib.e2fgvi_packed_conv_weight_size(self.Cout, groups, self.KH, self.KW, len(self.cpg), self._cpg_arr(), bk))),
                 "packed_conv_weight_size")

    def _wgeom(self):
        """the geometry arguments the Winograd packers share"""
        return self.Cout, self.groups, len(self.cpg), self._cpg_arr()

    @property
    def wino_packed(self):
        """packed weights of the fp32 F(2x2,3x3) kernel (conv_wino.hip), built on first use"""
        if self.algo not in ("winograd", "auto"):
            return None

        def build():
            lib = _L.load()
            return _pack_weights(lib.e2fgvi_packed_winograd_weight_size, lib.e2fgvi_pack_winograd_weight, self._w_raw, torch.float32,
                                 "winograd_weight", *self._wgeom())
        return _lazy(self._own, "wino", self.name + " (Winograd F(2x2,3x3) weights)", build)

    @property
    def wpacked(self):
        """packed weights of the register-staged implicit GEMM (conv.hip), built on first use"""
        if self.algo == "winograd":
            return None

        def build():
            lib = _L.load()
            return _pack_weights(lib.e2fgvi_packed_conv_weight_size, lib.e2fgvi_pack_conv_weight, self._w_raw, torch.float32,
                                 "conv_weight", self.Cout, self.groups, self.KH, self.KW, len(self.cpg), self._cpg_arr(), self.bk)
        return _lazy(self._own, "igemm", self.name + " (implicit-GEMM weights)", build)

    def weight_bytes(self):
        """device bytes of the packings this layer holds right now (the checkpoint tensor _w_raw not counted)"""
        ts = list(self._own.values()) + list(self._w4.values()) + ([self._w3] if self._w3 is not None else [])
        return sum(t.numel() * t.element_size() for t in ts) + sum(a.weight_bytes() for a in (self.alt, self.alt3) if a is not None)

    def _wino4(self, fy):
        """packed weights of the wide-tile Winograd kernel (conv_wino4.hip), built on first use"""
        def build():
            lib = _L.load()
            return _pack_weights(lib.e2fgvi_packed_winograd4_weight_size, lib.e2fgvi_pack_winograd4_weight, self._w_oihw, torch.float32,
                                 "winograd4_weight", *self._wgeom(), fy)
        return _lazy(self._w4, fy, self.name + " (Winograd F(%dx4,3x3) weights)" % fy, build)

    def _wino4_rule(self, N, H, W):
        """tile code of the wide-tile Winograd variant for this call, or 0 for the F(2x2,3x3) kernel"""
        if W % 4 or self._w_oihw is None:
            return 0
        # Measured on MI355X (tools/wino_bench.py, profiles/r02_wino4_bench.txt): F(2x4) x 64 couts beats the F(2x2) kernel
        # by 6-8 % on the batched layers with >= 256 output channels per group (encoder.layers.8 / .10) and loses
        # everywhere else (one workgroup per CU: the 16x16-pixel x 32-cout F(2x2) shape runs two); F(4x4) ties at best.
        # (... and >= 256 input channels per group: on encoder.layers.6, 128 -> 256, the 8x16x32 F(2x2) shape is 6-10 % faster)
        if self.Cout // self.groups >= 256 and sum(self.cpg) >= 256 and N * H * W >= _W4_MINPIX:
            return 2464
        return 0

    def _alt(self):
        """the LDS-DMA fp32 kernel (conv_bf16x.hip, F32 variant) as a tuning alternative of the implicit GEMM"""
        return _lazy(vars(self), "alt", self.name + " (LDS-DMA fp32 alternative)", self._x_alternative)

    def _wino_x3(self):
        """packed weights of the split-bf16 Winograd kernel (three bf16 planes of the transformed weights), built on first use"""
        if self._w_oihw is None:
            return None

        def build():
            lib = _L.load()
            return _pack_weights(lib.e2fgvi_packed_winograd_weight_x3_size, lib.e2fgvi_pack_winograd_weight_x3, self._w_oihw,
                                 torch.bfloat16, "winograd_weight_x3", *self._wgeom())
        return _lazy(vars(self), "_w3", self.name + " (split-operand Winograd weights)", build)

    def _alt3(self):
        """the same layer on the bf16 matrix pipe (three-way split operands, six exact bf16 MFMA terms per product)"""
        if any(c % 4 for c in self.cpg):
            return self.alt3
        return _lazy(vars(self), "alt3", self.name + " (split-operand GEMM alternative)", lambda: self._x_alternative(x3=True))

    def _work(self, d, use_wino, family, tile):
        """Launch-trace record: algorithmic MACs (direct convolution) and the MACs the matrix pipe is ISSUED.
        Winograd F(2x2,3x3): 16 multiplies per 2x2 outputs and input channel instead of 36, on pixel blocks of 16x16 /
        8x16 and 32 / 64-wide cout tiles (the tile rule of e2fgvi_conv3x3_winograd), input channels in chunks of 8.
        Implicit GEMM: output channels padded to 32, every source's channels to the K granule."""
        N, H, W, Ho, Wo = d.N, d.H, d.W, d.Ho, d.Wo
        cin_g, cout_g, K2 = sum(self.cpg), self.Cout // self.groups, self.KH * self.KW
        macs = N * Ho * Wo * self.Cout * cin_g * K2
        asked = int(tile)                      # the tile code handed to the launcher
        if family == "w4":
            fy, bn = W4_CODES[tile]
            pix = N * (-(-H // (8 * fy)) * 8 * fy) * (-(-W // 16) * 16)
            cin_p = sum(-(-c // 8) * 8 for c in self.cpg)
            # (fy+2)*6 positions per fy x 4 pixels
            issued = pix * (-(-cout_g // bn) * bn) * self.groups * cin_p * (fy + 2) * 6 // (fy * 4)
            kern = "conv_wino4<F(%dx4),%d>" % (fy, bn)
        elif family == "w3":
            asked = W3_BASE + tile             # (W3_BASE + block shape for the split Winograd kernel)
            shape = tile % 1000
            mt, bn = (2, shape) if shape < 100 else (1, shape - 100)
            pix = N * (-(-H // (8 * mt)) * 8 * mt) * (-(-W // 16) * 16)
            cin_p = -(-sum(-(-c // 8) for c in self.cpg) // 2) * 16           # 16-channel stages
            # 16 positions per 4 pixels, six bf16 MACs per product, in fp32-pipe equivalents (see PackedConvX's trace record)
            issued = int(pix * (-(-cout_g // bn) * bn) * self.groups * cin_p * 4 * 6 * 157.3 / 2500.0)
            kern = ("conv_wino_x3w<%d>" % bn) if tile >= 6000 else ("conv_wino_x3p4<%d>" % bn) if tile >= 5000 else "conv_wino_x3<%d,%d>" % (mt, bn)
        elif use_wino:
            if not tile:
                big = N * -(-H // 16) * -(-W // 16) * -(-cout_g // 64) * self.groups
                tile = 64 if (cout_g >= 256 and big >= 128) else 132
            mt, bn = (2, tile) if tile < 100 else (1, tile - 100)
            pix = N * (-(-H // (8 * mt)) * 8 * mt) * (-(-W // 16) * 16)
            cin_p = sum(-(-c // 8) * 8 for c in self.cpg)
            issued = pix * (-(-cout_g // bn) * bn) * self.groups * cin_p * 4       # 16 positions per 4 pixels
            kern = "conv_wino<%d,%d>" % (mt, bn)
        else:
            g = self.bk
            cin_p = sum(-(-c // g) * g for c in self.cpg)
            issued = N * Ho * Wo * (-(-cout_g // 32) * 32) * self.groups * cin_p * K2
            kern = "conv_igemm/halo tile=%d" % tile
        return dict(layer=self.name, kernel=kern, shape="N%d %dx%d %d->%d k%d s%d g%d" % (
            N, H, W, cin_g * self.groups, self.Cout, self.KH, self.stride, self.groups), macs=macs, issued=issued, tile=asked)

    def __call__(self, sources, out=None, out_coff=0, residual=None, res_coff=0, act=ACT_NONE, slope=0.0,
                 out_nchw=False, tile=0, kv_planes=None, out_dtype=None):
        """sources: list of NHWC tensors or (tensor, channel_offset) pairs, one per cpg entry.
        out_dtype: None or torch.float32 (the keyword of PackedConvX, so that callers pass the same ones to both).
        kv_planes (a qkv Linear, Cout = 1536): [3, rows, 1024] bf16 -- the K / V columns as the three exact planes the split-operand
        attention reads.  When the decision table hands the call to the split-operand GEMM its epilogue writes them (and skips the
        fp32 K / V columns); any other kernel writes the fp32 rows and e2fgvi_split3_kv makes the planes from them."""
        if out_dtype not in (None, torch.float32):
            raise ValueError("PackedConv writes fp32 results")
        srcs, out = self._srcs_out(sources, out, out_nchw, torch.float32)
        N, H, W, _ = srcs[0][0].shape
        kw = dict(out_coff=out_coff, res_coff=res_coff, act=act, slope=slope, out_nchw=out_nchw)
        chunks = list(_image_chunks(N, max(H * W * t.shape[3] * 4 for t, _ in srcs)))
        if len(chunks) > 1:
            for n0, n1 in chunks:
                self([(t[n0:n1], c) for t, c in srcs], out=out[n0:n1], residual=None if residual is None else residual[n0:n1],
                     tile=tile, **kw)
        else:
            kw.update(out=out, residual=residual)
            call = _Call(self._desc(srcs, **kw), srcs, kw, kv_planes)
            if self._launch(call, self._select(call, tile)):
                return out                         # the kernel's epilogue has written kv_planes
        if kv_planes is not None:
            split3_kv(out.view(-1, out.shape[-1]), out=kv_planes)
        return out

    def _desc(self, srcs, out, out_coff, residual, res_coff, act, slope, out_nchw):
        """the C descriptor of one call (srcs: list of (tensor, channel offset)); wpacked and tile are set by what launches: a
        layer packs the weights of the kernels it runs, only"""
        d = self._fill(_L.ConvDesc(), torch.float32, _chk, srcs, out, out_coff, act, slope, out_nchw)
        self._fill_residual(d, _chk, residual, res_coff)
        d.bk = self.bk
        return d

    def _select(self, call, tile):
        """The kernel of this call as a _Plan: the caller's tile code, or (tile == 0) the static rule and, on layers that ask for it,
        the decision table's row for (layer geometry, size class).  No launch, no timing -- except through _tune, which fills a
        missing row under E2FGVI_AUTOTUNE=1."""
        d, kw = call.d, call.kw
        N, H, W, Ho, Wo = d.N, d.H, d.W, d.Ho, d.Wo
        out, residual = kw["out"], kw["residual"]
        use_wino = self.algo == "winograd" or (self.algo == "auto" and H % 2 == 0 and W % 2 == 0 and not kw["out_nchw"]
                                               and (tile in (0, 32, 64, 132, 164) or _decode(tile)[0] in ("w4", "w3")))
        asked = _decode(tile) if use_wino else ("own", tile)
        # the static rule's kernel: what runs when nothing else is decided, and what a rejected alternative falls back to
        static = self._wino4_rule(N, H, W) if use_wino and (tile == 0 or asked[0] == "w3") else tile
        own = ("w4" if use_wino and static in W4_CODES else "own", static)
        family, arg = asked if asked[0] == "w3" else own
        plan = _Plan(family, arg, own, False, use_wino)
        # (a layer of the side stream may take it too: conv_bf16x.o is one of the packed-math-free objects, build.NOPK_OBJECTS)
        x3 = self.try_x3 and X3_ENABLED
        if not (tile == 0 and (static == 0 or not self.tune) and (self.tune or x3) and N * Ho * Wo >= 2048):
            return plan
        # one decision per (layer geometry, size class): row counts within a quarter octave share the tile, so the
        # slightly different window lengths of a video (t = 17 ... 21 frames) do not each pay for a tuning pass
        # (the fp32 baseline the alternatives are measured against is part of the key: a tuned layer and an untuned one of the
        #  same geometry, or the F(2x4) / F(2x2) Winograd baselines, do not share a verdict)
        key = (self.Cout, tuple(self.cpg), self.KH, self.KW, self.stride, self.pad, self.groups, self.bk,
               int(4.0 * math.log2(N * Ho * Wo)), residual is not None, kw["act"], use_wino, bool(self.tune), int(static)) + (("x3",) if x3 else ())
        best = _decision(key)
        from_table = best is not None
        if best is None and AUTOTUNE and not torch.cuda.is_current_stream_capturing() and (
                residual is None or residual.data_ptr() != out.data_ptr()):
            best = _remember(key, self._tune(call, own, use_wino, x3))
        family, arg = _decode(best or 0)
        # the split kernels wherever the key asked for them; tiles of the own and the LDS-DMA kernel on tuned layers only (the own
        # kernel's halo ids, from 10000, are for callers that name them: no table row does)
        if family in ("w3", "x3") or (self.tune and (family == "dma" or (family == "own" and arg < DMA_BASE))):
            plan = plan._replace(family=family, tile=arg)
        return plan._replace(from_table=from_table)

    def _tune(self, call, own, use_wino, x3):
        """E2FGVI_AUTOTUNE=1, first eager call of a (geometry, size class): device time of every candidate kernel on this exact
        call -- the launches rewrite the same output, so the result of the call is unaffected.  Returns the winner's tile code."""
        d, srcs, kw, kv_planes = call
        best = self._autotune(d, use_wino) if self.tune else own[1]
        base = own if own[0] == "w4" else ("own", best)
        mine = None

        def time_mine():
            self._run(d, *base, use_wino)
            return min(_time_launches(lambda: self._run(d, *base, use_wino), 3) for _ in range(TUNE_REPS))
        if self.tune and not use_wino and not self.nopk:
            # the LDS-DMA fp32 kernel on the very same call: codes DMA_BASE + its tile
            alt = self._alt()
            mine = time_mine()
            res = alt._time_tiles(alt._desc(srcs, out2=None, **kw))
            if res and min(res.values()) < mine:
                best, mine = DMA_BASE + min(res, key=res.get), min(res.values())
        if x3 and self._alt3() is not None:
            # ... and the split-bf16 kernel: codes X3_BASE + its tile
            if mine is None:
                mine = time_mine()
            d3 = self.alt3._desc(srcs, out2=None, **kw)
            if kv_planes is not None:            # timed as it will run: with the K / V planes written by the epilogue
                self.alt3._set_planes(d3, kv_planes, self.Cout - kv_planes.shape[2], d.N * d.Ho * d.Wo)
            res = self.alt3._time_tiles(d3)
            if res and min(res.values()) < X3_MARGIN * mine:
                best, mine = X3_BASE + min(res, key=res.get), min(res.values())
        if x3 and use_wino and self._wino_x3() is not None:
            # ... and the Winograd kernel with split operands: codes W3_BASE + its block shape
            w3 = {}
            for shape in W3_CANDIDATES:
                def run():
                    return self._run(d, "w3", shape, use_wino)[0]
                if run() == 0:
                    w3[shape] = min(_time_launches(run, 3) for _ in range(TUNE_REPS))
            # the margin is for leaving the fp32 kernel; among the block shapes of the split kernel the fastest wins
            if w3 and min(w3.values()) < X3_MARGIN * mine:
                best, mine = W3_BASE + min(w3, key=w3.get), min(w3.values())
        return best

    def _autotune(self, d, wino):
        """the fastest of the own kernel's candidate tile codes on this exact call (best of TUNE_REPS measurements of 2 launches)"""
        lib = _L.load()
        best, best_ms = 0, float("inf")
        st = _stream()
        fn = lib.e2fgvi_conv3x3_winograd if wino else lib.e2fgvi_conv2d_nhwc
        d.tile, d.wpacked = 0, (self.wino_packed if wino else self.wpacked).data_ptr()
        for _ in range(3):                                       # bring clocks / caches to steady state first
            fn(C.byref(d), st)
        for code in (WINO_CANDIDATES if wino else TUNE_CANDIDATES):
            d.tile = code
            if fn(C.byref(d), st) != 0:                          # not instantiated / not applicable to this packing
                continue
            ms = min(_time_launches(lambda: fn(C.byref(d), st), 2) for _ in range(TUNE_REPS))
            if ms < best_ms:
                best, best_ms = code, ms
        return best

    def _run(self, d, family, tile, use_wino):
        """one launch of a kernel of this layer's own on descriptor `d`: (return code, entry point's name)"""
        lib, st = _L.load(), _stream()
        if family == "w3":
            d.tile, d.wpacked = tile, self._wino_x3().data_ptr()
            return lib.e2fgvi_conv3x3_winograd_x3(C.byref(d), st), "conv3x3_winograd_x3"
        if family == "w4":
            fy, d.tile = W4_CODES[tile]
            d.wpacked = self._wino4(fy).data_ptr()
            return lib.e2fgvi_conv3x3_winograd4(C.byref(d), fy, st), "conv3x3_winograd4"
        d.tile = tile
        d.wpacked = (self.wino_packed if use_wino else self.wpacked).data_ptr()
        if use_wino:
            return lib.e2fgvi_conv3x3_winograd(C.byref(d), st), "conv3x3_winograd"
        if self.nopk:
            return lib.e2fgvi_conv2d_nhwc_nopk(C.byref(d), st), "conv2d_nhwc_nopk"
        return lib.e2fgvi_conv2d_nhwc(C.byref(d), st), "conv2d_nhwc"

    def _launch(self, call, plan):
        """runs `plan`, one trace record announced before the launch; True when the kernel's epilogue has written kv_planes (the
        split-operand GEMM's does)"""
        d, srcs, kw, kv_planes = call
        family, tile = plan.family, plan.tile
        try:
            if family == "x3" and self._alt3() is not None:
                self.alt3(srcs, tile=tile, planes=kv_planes, split_from=(self.Cout - kv_planes.shape[2]) if kv_planes is not None else 0,
                          **kw)
                return True
            if family == "dma":
                self._alt()(srcs, tile=tile, **kw)
                return False
            if family == "x3" or (family == "w3" and self._wino_x3() is None):
                family, tile = plan.static
        except _L.HipError:
            # a decision taken at a neighbouring size class (or an older cache entry) that this call's shape rejects: the
            # layer's own fp32 kernel runs instead
            if not plan.from_table:
                raise
            family, tile = plan.static
        if _L.TRACE is not None:
            _L.annotate(**self._work(d, plan.use_wino, family, tile))
        rc, what = self._run(d, family, tile, plan.use_wino)
        if rc != 0 and (family, tile) != plan.static:
            rc, what = self._run(d, *plan.static, plan.use_wino)       # a tabled block shape this call's geometry rejects: the static default
        _L.check(rc, what)
        return False


HALF16 = (torch.bfloat16, torch.float16)     # the two element types of the 16-bit data path


_DT_CODE = {torch.float32: _L.DT_F32, torch.bfloat16: _L.DT_BF16, torch.float16: _L.DT_F16}      # the C ABI's element codes


def _dt(t):
    try:
        return _DT_CODE[t.dtype]
    except KeyError:
        raise TypeError("tensor must be float32, bfloat16 or float16, got %s" % t.dtype) from None


def _dt_key(t):
    """the element-type field of a tuning key: fp16 layers share the bf16 entries (same kernels, same tiles, same data movement:
    conv_bf16x.hip MODE 3 is MODE 0 with another MFMA instruction and conversion).  On purpose, also under E2FGVI_AUTOTUNE=1: an
    fp16 layer that times its tiles records the winner under the bf16 key and may replace a bf16 decision held in memory (or in
    the tune file) -- the measurement is one of the same kernel body on the same shape, so it is as valid for bf16 as for fp16."""
    return _L.DT_BF16 if t.dtype == torch.float16 else _dt(t)


def _chk_any(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA (ROCm) tensor -- the HIP path has no CPU fallback" % name)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    _dt(t)
    return t


class PackedConvX(_ConvLayer):
    """Conv / linear layer on the LDS-DMA implicit-GEMM kernel (csrc/conv_bf16x.hip).

    dtype=torch.bfloat16 (default): the bf16 data path -- bf16 NHWC sources (virtual concat, channels per source in
    multiples of 8), bf16 packed weights, v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
    dtype=torch.float16: the same with fp16 sources / weights / 16-bit results on v_mfma_f32_32x32x16_f16 (mode E2FGVI_F16),
    same tiles; its tuning keys are the bf16 ones.
    dtype=torch.float32: the same kernel on fp32 operands (channels in multiples of 4, exact fp32 MFMA) -- the fp32 path's
    tuning alternative to PackedConv's register-staged implicit GEMM.
    Either way: fp32 epilogue (bias, fp32 / bf16 residual, activation or the DCN offset post-processing), bf16 or fp32
    result (NHWC, or fp32 NCHW), optional second bf16 copy (`out2`)."""

    _NCHW_ERROR = "NCHW out must be fp32 %(want)s"

    def __init__(self, weight, bias, cpg, groups=1, stride=1, pad=0, dtype=torch.bfloat16, taps=None, x3=False):
        """taps: None = tap-packed K-steps whenever the layer qualifies (one bf16 source of <= 32 channels, no groups, more
        than one tap), False = never (A/B measurements).
        x3 (fp32 sources only): fp32 on the bf16 matrix pipe -- weights stored as three bf16 planes whose sum is the fp32
        weight, activations split the same way in registers, six exact bf16 MFMA terms per product (kernel MODE 2)"""
        lib = _L.load()
        w = self._init_layer(weight, bias, cpg, groups, stride, pad)
        self.dtype = dtype
        self.f32 = dtype == torch.float32
        self.x3 = bool(x3)
        if self.x3 and not self.f32:
            raise ValueError("x3 splitting is for fp32 sources")
        self.f16 = dtype == torch.float16
        if not self.f32 and dtype not in HALF16:
            raise TypeError("PackedConvX: dtype must be float32, bfloat16 or float16")
        self._mode = mode = _L.DT_BF16X3 if self.x3 else _DT_CODE[dtype]      # the `mode` of e2fgvi_conv2d_x and of its packers
        conv2d_x = lib.e2fgvi_conv2d_x
        self._fn = lambda desc_ref, stream: conv2d_x(desc_ref, mode, stream)
        self._w_raw = w if (self.f32 and not self.x3) else None
        self._taps_arg = taps
        # narrow single-source layers (SPyNet's 7x7 stacks, the encoder's first layer): K-steps that carry several taps
        # (fp32 operands: only on request -- the one fp32 user is the FFN's second Linear as a conv, engine.py)
        self.taps = (len(self.cpg) == 1 and groups == 1 and self.cpg[0] <= 56 and self.KW > 1
                     and (taps is True if self.f32 else taps is not False))
        self._wdtype = torch.bfloat16 if self.x3 else dtype
        self._wp = None
        if self._w_raw is None:
            self._wp = self._pack(w)       # bf16 layers and the split-operand ones: packed now, the fp32 tensor is not kept
        else:                              # a geometry the library rejects raises here, not on the first call
            _L.check(min(0, int(lib.e2fgvi_packed_conv_weight_x_size(*self._wgeom()))), "packed_conv_weight_x_size")

    @property
    def wpacked(self):
        """packed weights; an fp32 layer (whose split-operand alternative alt3 may be what runs) packs its own on first use"""
        return _lazy(vars(self), "_wp", self.name + " (LDS-DMA GEMM weights)", lambda: self._pack(self._w_raw))

    def weight_bytes(self):
        return (0 if self._wp is None else self._wp.numel() * self._wp.element_size()) + (self.alt3.weight_bytes() if self.alt3 is not None else 0)

    def _wgeom(self):
        return self._mode, int(self.taps), self.Cout, self.groups, self.KH, self.KW, len(self.cpg), self._cpg_arr()

    def _pack(self, w):
        lib = _L.load()
        return _pack_weights(lib.e2fgvi_packed_conv_weight_x_size, lib.e2fgvi_pack_conv_weight_x, w, self._wdtype, "conv_weight_x",
                             *self._wgeom())

    def _alt3(self):
        """this fp32 layer on the bf16 matrix pipe (x3=True), built on first use"""
        if self._w_raw is None:
            return self.alt3
        return _lazy(vars(self), "alt3", self.name + " (split-operand GEMM alternative)",
                     lambda: self._x_alternative(taps=self._taps_arg, x3=True))

    def _desc(self, srcs, out, out_coff, residual, res_coff, act, slope, out2, out_nchw):
        """the C descriptor of one call (srcs: list of (tensor, channel offset))"""
        d = self._fill(_L.ConvXDesc(), self.dtype, _chk_any, srcs, out, out_coff, act, slope, out_nchw)
        d.wpacked = None if self._wp is None else self._wp.data_ptr()      # an fp32 layer's own packing: set by what launches it
        d.dst_dtype = _dt(out)
        if out2 is not None:
            _chk(out2, "out2", torch.float16 if self.f16 else torch.bfloat16)
            if out2.dim() != 4 or tuple(out2.shape[:3]) != (d.N, d.Ho, d.Wo):
                raise ValueError("out2 shape %s != [%d,%d,%d,*]" % (tuple(out2.shape), d.N, d.Ho, d.Wo))
            d.dst2, d.dst2_ld, d.dst2_coff = out2.data_ptr(), out2.shape[3], 0
        self._fill_residual(d, _chk_any, residual, res_coff)
        if residual is not None:
            d.res_dtype = _dt(residual)
        d.tap_packed = 1 if self.taps else 0
        return d

    @staticmethod
    def _set_planes(d, planes, split_from, rows):
        """ABI 8: output channels from `split_from` on go to `planes` ([3, rows, Cout - split_from] bf16: hi / mid / lo, their sum is
        the fp32 result bit for bit) instead of to the fp32 rows"""
        _chk(planes, "planes", torch.bfloat16)
        if planes.dim() != 3 or planes.shape[0] != 3 or planes.shape[1] != rows or planes.shape[2] != d.Cout - split_from:
            raise ValueError("planes must be [3, %d, %d] bf16, got %s" % (rows, d.Cout - split_from, tuple(planes.shape)))
        d.dst2, d.dst2_ld, d.dst2_coff = planes.data_ptr(), planes.shape[2], 0
        d.dst2_split_from, d.dst2_plane_stride = split_from, planes.shape[1] * planes.shape[2]

    def __call__(self, sources, out=None, out_dtype=None, out_coff=0, residual=None, res_coff=0, act=ACT_NONE,
                 slope=0.0, out2=None, tile=0, out_nchw=False, planes=None, split_from=0):
        """planes / split_from (fp32 results): see _set_planes -- the qkv Linear writes the attention's K / V operand planes.
        The steps of PackedConv.__call__: _desc, _select (_tune under E2FGVI_AUTOTUNE=1), launch."""
        if out_dtype is None:
            out_dtype = self.dtype
        srcs, out = self._srcs_out(sources, out, out_nchw, out_dtype)
        N, H, W, _ = srcs[0][0].shape
        Ho, Wo = self.out_hw(H, W)
        kw = dict(out_coff=out_coff, res_coff=res_coff, act=act, slope=slope, out_nchw=out_nchw)
        chunks = list(_image_chunks(N, max(H * W * t.shape[3] * (4 if self.f32 else 2) for t, _ in srcs)))
        if len(chunks) > 1:
            if planes is not None:
                raise ValueError("split planes: the batch spans >= 4 GiB (call in chunks)")
            for n0, n1 in chunks:
                self([(t[n0:n1], c) for t, c in srcs], out=out[n0:n1], residual=None if residual is None else residual[n0:n1],
                     out2=None if out2 is None else out2[n0:n1], tile=tile, **kw)
            return out
        kw.update(out=out, residual=residual, out2=out2)
        d = self._desc(srcs, **kw)
        if planes is not None:
            self._set_planes(d, planes, split_from, N * Ho * Wo)
        if tile == 0 and self.tune and N * Ho * Wo >= 2048:
            family, tile = self._select(d, srcs, kw)
            if family == "x3":
                try:
                    return self.alt3(srcs, out_dtype=out_dtype, tile=tile, planes=planes, split_from=split_from, **kw)
                except _L.HipError:                       # a neighbouring size class's tile that this shape rejects
                    tile = 0
        d.tile = tile
        if _L.TRACE is not None:
            _L.annotate(**self._work(d))
        d.wpacked = self.wpacked.data_ptr()
        rc = self._fn(C.byref(d), _stream())
        if rc != 0 and d.tile and self.tune:
            d.tile = 0                                    # a tabled tile this call's geometry rejects: the library's default
            rc = self._fn(C.byref(d), _stream())
        _L.check(rc, "conv2d_x")
        return out

    def _select(self, d, srcs, kw):
        """(family, tile) of a call that leaves the tile to the layer: the decision table's row for (layer geometry, size class) --
        "own" and a tile of this kernel, or "x3" and a tile of the split-operand alternative.  No launch, no timing -- except
        through _tune, which fills a missing row under E2FGVI_AUTOTUNE=1."""
        out, residual = kw["out"], kw["residual"]
        x3 = self.try_x3 and X3_ENABLED and self.f32 and not self.x3
        key = (("x3" if self.x3 else ("x32+3" if x3 else "x32")) if self.f32 else "x", self.Cout, tuple(self.cpg), self.KH, self.KW, self.stride, self.pad, self.groups,
               int(4.0 * math.log2(d.N * d.Ho * d.Wo)), _dt_key(out), kw["out_nchw"], self.taps)
        best = _decision(key)
        if best is None and AUTOTUNE and not torch.cuda.is_current_stream_capturing() and (
                residual is None or residual.data_ptr() != out.data_ptr()):
            best = _remember(key, self._tune(d, srcs, kw, x3))
        if _decode(best or 0)[0] in ("x3", "w3"):      # (a Winograd code counts from X3_BASE here: a tile the launcher rejects)
            return ("x3", best - X3_BASE) if self._alt3() is not None else ("own", 0)
        return "own", best or 0

    def _tune(self, d, srcs, kw, x3):
        """E2FGVI_AUTOTUNE=1: the fastest tile of this exact call, or X3_BASE + the split-operand alternative's where that is
        faster by more than X3_MARGIN"""
        res = self._time_tiles(d)
        best = min(res, key=res.get) if res else 0
        if x3 and self._alt3() is not None:
            res3 = self.alt3._time_tiles(self.alt3._desc(srcs, **kw))
            if res3 and (not res or min(res3.values()) < X3_MARGIN * min(res.values())):
                best = X3_BASE + min(res3, key=res3.get)
        return best

    def _work(self, d):
        """launch-trace record of the call `d` describes (see PackedConv._work)"""
        N, H, W, Ho, Wo, tile = d.N, d.H, d.W, d.Ho, d.Wo, d.tile
        cin_g, cout_g, K2 = sum(self.cpg), self.Cout // self.groups, self.KH * self.KW
        kc = 32 if self.f32 else 64
        cin_p = sum(-(-c // kc) * kc for c in self.cpg)
        if self.taps:                                   # K-steps of several taps: issued K = steps * 64
            cin_p = -(-K2 * (self.cpg[0] // (4 if self.f32 else 8)) // 8) * kc / K2
        return dict(layer=self.name, kernel="conv_%s tile=%d%s" % (("f32x3" if self.x3 else "f32x") if self.f32 else
                                                                   "f16x" if self.f16 else "bf16x", tile, " taps" if self.taps else ""),
                    shape="N%d %dx%d %d->%d k%d s%d g%d" % (N, H, W, cin_g * self.groups, self.Cout, self.KH, self.stride, self.groups),
                    macs=N * Ho * Wo * self.Cout * cin_g * K2, tile=int(tile),
                    # x3: six bf16 MACs per product, counted in fp32-pipe equivalents (a bf16 MAC occupies the matrix
                    # pipe for 157.3 / 2500 of the time of an fp32 MAC): `issued / fp32 peak` stays matrix-pipe time
                    issued=int(N * Ho * Wo * (-(-cout_g // 32) * 32) * self.groups * cin_p * K2 * (_L.X3_PIPE if self.x3 else 1)))

    def _halo_x3(self):
        """whether the halo tiles (XTUNE_HALO) take this layer: split operands, 7x7 stride 1 pad 3, one source of a multiple of 16
        channels in the plain packing, no groups, at most 64 output channels (the launcher checks the call's epilogue itself)"""
        return (self.x3 and not self.taps and (self.KH, self.KW, self.stride, self.pad, self.groups) == (7, 7, 1, 3, 1)
                and len(self.cpg) == 1 and self.cpg[0] % 16 == 0 and self.Cout <= 64)

    def _time_tiles(self, d, reps=3, rounds=2):
        """{tile code: best device time in ms} of every tile shape on this exact call (the launches rewrite the same
        output); best of `rounds` measurements of `reps` launches each"""
        st = _stream()
        res = {}
        d.tile = 0
        d.wpacked = self.wpacked.data_ptr()

        def run():
            return self._fn(C.byref(d), st)
        for _ in range(2):
            run()
        for _ in range(rounds * TUNE_REPS):
            rowshift = (self.KH, self.KW, self.stride, self.pad) == (3, 3, 1, 1) and not self.f32 and not self.taps
            for code in XTUNE_CANDIDATES + (XTUNE_ROWSHIFT if rowshift else ()):
                if code in XTUNE_HALO and not self._halo_x3():
                    continue
                if code % 10 == 3 and self.Cout // self.groups > 64:  # 32-wide tiles only make sense for narrow layers
                    continue
                if code in (12, 18) and self.Cout // self.groups > 64:
                    continue
                d.tile = code
                if run() == 0:
                    res[code] = min(res.get(code, float("inf")), _time_launches(run, reps))
        d.tile = 0
        return res


class SoftCompGather:
    """SoftComp's Linear(512 -> 49 C) + nn.Fold(7x7, stride 3, padding 3) (tfocal_transformer.py:49-72,
    tfocal_transformer_hq.py:49-79) in GATHER form: pixel (Y, X) of the folded image receives the taps (ki, kj) with
    ki = Y + 3 - 3 ly, kj = X + 3 - 3 lx of the tokens (ly, lx) around it, so the pixels of phase (py, px) = (Y % 3, X % 3)
    are a small convolution over the token grid -- 3 taps per axis for phase 0 (token rows ty-1, ty, ty+1 with ki = 6, 3, 0),
    2 for phases 1 and 2 (rows ty, ty+1 with ki = p+3, p) -- written to every third pixel.  Nine launches of the LDS-DMA
    conv kernel (explicit output grid + output scatter), 49 x 512 x C MACs per token as before, but no [tokens, 49 C]
    tensor between the Linear and the Fold (813 MB at 720x1296 T=10 in bf16) and no fold kernel.  The Linear's bias folds
    to a per-pixel image (fewer taps reach the border pixels), added as a residual broadcast over the frames."""

    def __init__(self, weight, bias, channels=128, dtype=torch.bfloat16):
        w = _chk(weight.detach().float().contiguous(), "weight")            # [49 C, 512], row c*49 + ki*7 + kj
        if w.dim() != 2 or w.shape[0] != 49 * channels:
            raise ValueError("SoftComp embedding weight must be [%d, hidden]" % (49 * channels))
        self.C, self.hidden, self.dtype = channels, w.shape[1], dtype
        w4 = w.view(channels, 7, 7, self.hidden)
        self.phases = []
        for py in range(3):
            ky_taps = [6, 3, 0] if py == 0 else [py + 3, py]                 # kernel row -> ki; input row = ty - pad + ky
            for px in range(3):
                kx_taps = [6, 3, 0] if px == 0 else [px + 3, px]
                wp = w4[:, ky_taps][:, :, kx_taps].permute(0, 3, 1, 2).contiguous()          # [C, hidden, kh, kw]
                layer = PackedConvX(wp, None, [self.hidden], dtype=dtype)
                layer.name = "sc.embedding phase (%d,%d)" % (py, px)
                self.phases.append((py, px, 1 if py == 0 else 0, 1 if px == 0 else 0, layer))
        self.bias = None if bias is None else _chk(bias.detach().float().contiguous(), "bias")
        self._bias_img = {}
        self.tile = 0

    def bias_image(self, fh, fw):
        """fold of the Linear's bias: [3 fh, 3 fw, C] fp32 (computed once per token grid with the fold kernel)"""
        if self.bias is None:
            return None

        def build():
            rows = self.bias.view(self.C, 49).t().reshape(1, 49 * self.C).expand(fh * fw, 49 * self.C).contiguous()
            return softcomp_fold(rows, 1, fh, fw, 3 * fh, 3 * fw, self.C)[0].contiguous()
        return _lazy(self._bias_img, (fh, fw), "sc.embedding (folded bias image)", build)

    def __call__(self, tokens, out=None, out_dtype=None):
        """tokens [F, fh, fw, hidden] -> folded [F, 3 fh, 3 fw, C]"""
        _chk(tokens, "tokens", self.dtype)
        F_, fh, fw, hid = tokens.shape
        if hid != self.hidden:
            raise ValueError("tokens must be [F, fh, fw, %d]" % self.hidden)
        H, W = 3 * fh, 3 * fw
        if out is None:
            out = torch.empty((F_, H, W, self.C), dtype=out_dtype or self.dtype, device=tokens.device)
        if tuple(out.shape) != (F_, H, W, self.C):
            raise ValueError("out must be [%d,%d,%d,%d]" % (F_, H, W, self.C))
        chunks = list(_image_chunks(F_, fh * fw * hid * tokens.element_size()))
        if len(chunks) > 1:
            for n0, n1 in chunks:
                self(tokens[n0:n1], out=out[n0:n1])
            return out
        bimg = self.bias_image(fh, fw)
        for py, px, pad_y, pad_x, layer in self.phases:
            d = _L.ConvXDesc()
            d.src[0], d.src_ld[0], d.src_coff[0], d.src_cpg[0], d.nsrc = tokens.data_ptr(), hid, 0, hid, 1
            d.N, d.H, d.W, d.Ho, d.Wo = F_, fh, fw, fh, fw
            d.KH, d.KW, d.stride, d.pad = layer.KH, layer.KW, 1, pad_y
            d.groups, d.Cout = 1, self.C
            d.wpacked = layer.wpacked.data_ptr()
            d.dst, d.dst_ld, d.dst_coff, d.dst_dtype = out.data_ptr(), self.C, 0, _dt(out)
            if bimg is not None:
                d.residual, d.res_ld, d.res_coff, d.res_dtype, d.res_bcast = bimg.data_ptr(), self.C, 0, _L.DT_F32, 1
            d.out_grid, d.pad_left = 1, pad_x
            d.out_sy, d.out_sx, d.out_py, d.out_px, d.out_H, d.out_W = 3, 3, py, px, H, W
            d.act, d.slope, d.tile = ACT_NONE, 0.0, self.tile
            if _L.TRACE is not None:
                kc = 32 if layer.f32 else 64
                macs = F_ * fh * fw * self.C * hid * layer.KH * layer.KW
                _L.annotate(layer=layer.name, kernel="conv_%s (gather-form SoftComp)" % ("f32x" if layer.f32 else "f16x" if layer.f16 else "bf16x"),
                            shape="N%d %dx%d %d->%d k%dx%d scatter s3" % (F_, fh, fw, hid, self.C, layer.KH, layer.KW),
                            macs=macs, issued=macs // hid * (-(-hid // kc) * kc))
            _L.check(layer._fn(C.byref(d), _stream()), "conv2d_x (SoftComp phase)")
        return out


class PackedLinearX(PackedConvX):
    """y[rows, Cout] = x[rows, Cin] @ W^T + b (+ residual) on the bf16 data path, rows treated as 1x1 images."""

    def __init__(self, weight, bias, dtype=torch.bfloat16):
        super().__init__(weight, bias, [weight.shape[1]], dtype=dtype)

    def __call__(self, x, out=None, out_dtype=None, residual=None, act=ACT_NONE, slope=0.0, out2=None, tile=0):
        rows = x.numel() // x.shape[-1]
        if out is None:
            out = torch.empty((rows, self.Cout), dtype=out_dtype or self.dtype, device=x.device)
        r4 = None if residual is None else residual.view(rows, 1, 1, residual.shape[-1])
        o2 = None if out2 is None else out2.view(rows, 1, 1, out2.shape[-1])
        super().__call__([x.view(rows, 1, 1, x.shape[-1])], out=out.view(rows, 1, 1, out.shape[-1]), residual=r4, act=act,
                         slope=slope, out2=o2, tile=tile)
        return out


class PackedLinear(PackedConv):
    """y[rows, Cout] = x[rows, Cin] @ W^T + b (+ residual), rows treated as 1x1 images."""

    def __init__(self, weight, bias, bk=None, precision="fp32"):
        super().__init__(weight, bias, [weight.shape[1]], bk=bk, precision=precision)

    def __call__(self, x, out=None, residual=None, act=ACT_NONE, slope=0.0, tile=0, kv_planes=None, out_dtype=None):
        if out_dtype not in (None, torch.float32):
            raise ValueError("PackedLinear writes fp32 results")
        _chk(x, "x")
        rows = x.numel() // x.shape[-1]
        x4 = x.view(rows, 1, 1, x.shape[-1])
        if out is None:
            out = torch.empty((rows, self.Cout), dtype=torch.float32, device=x.device)
        o4 = out.view(rows, 1, 1, out.shape[-1])
        r4 = None if residual is None else residual.view(rows, 1, 1, residual.shape[-1])
        super().__call__([x4], out=o4, residual=r4, act=act, slope=slope, tile=tile, kv_planes=kv_planes)
        return out


class PackedTailConv:
    """The decoder's last layer, Conv2d(64, 3, 3, padding=1) + activation -> fp32 NCHW frames (csrc/conv_tail.hip): the nine
    taps on the N side of one [pixels x 64] x [64 x 27] GEMM, shifted sum in LDS.  dtype = the source's (fp32 / bf16 / fp16)."""

    def __init__(self, weight, bias, dtype=torch.float32):
        lib = _L.load()
        w = _chk(weight.detach().float().contiguous(), "weight")
        self.Cout, self.Cin, self.KH, self.KW = w.shape
        if (self.KH, self.KW) != (3, 3):
            raise ValueError("PackedTailConv: 3x3 kernels only")
        self.dtype = dtype
        if dtype not in _DT_CODE:
            raise TypeError("tensor must be float32, bfloat16 or float16, got %s" % dtype)
        self.wpacked = _pack_weights(lib.e2fgvi_packed_tail_weight_size, lib.e2fgvi_pack_tail_weight, w, dtype, "tail_weight",
                                     self.Cout, self.Cin, extra=(_DT_CODE[dtype],))
        self.bias = None if bias is None else _chk(bias.detach().float().contiguous(), "bias")
        self.name = "conv_tail"

    def __call__(self, sources, out=None, act=ACT_NONE, slope=0.0, out_nchw=True, tile=0):
        """call-compatible with PackedConv / PackedConvX for one NHWC source and an NCHW fp32 result"""
        x = sources[0] if isinstance(sources, (list, tuple)) else sources
        if not out_nchw:
            raise ValueError("PackedTailConv writes NCHW frames")
        _chk(x, "x", self.dtype)
        N, H, W, ld = x.shape
        if out is None:
            out = torch.empty((N, self.Cout, H, W), dtype=torch.float32, device=x.device)
        _chk(out, "out")
        if tuple(out.shape) != (N, self.Cout, H, W):
            raise ValueError("out shape %s != %s" % (tuple(out.shape), (N, self.Cout, H, W)))
        macs = N * H * W * self.Cout * self.Cin * 9
        tiles = N * -(-H // 16) * -(-W // 32)
        _L.annotate(layer=self.name, kernel="conv_tail", shape="N%d %dx%d %d->%d k3 s1 g1" % (N, H, W, self.Cin, self.Cout),
                    macs=macs, issued=tiles * 640 * 64 * 32)
        _L.check(_L.load().e2fgvi_conv3x3_tail(_ptr(x), _dt(x), ld, _ptr(self.wpacked), _ptr(self.bias), _ptr(out), N, H, W, act,
                                               float(slope), _stream()), "conv3x3_tail")
        return out


# ------------------------------------------------------------------------------------------ deformable conv
# PackedDcn(mfma=...) -> (mfma_dtype of the C ABI, element type of the packed weights, kernel name of the trace record)
_DCN_PACKING = {"fp32": (_L.DT_F32, torch.float32, "mdcn"), "bf16": (_L.DT_BF16, torch.bfloat16, "mdcn_bf16"),
                "fp16": (_L.DT_F16, torch.float16, "mdcn_f16"), "x3": (_L.DT_BF16X3, torch.bfloat16, "mdcn_x3")}


class PackedDcn:
    def __init__(self, weight, bias, deform_groups, stride=1, pad=0, dil=1, mfma="fp32"):
        """mfma="bf16": the sampled columns and the weights are rounded to bf16 for the MFMA (bf16 data path); the gather,
        the bilinear blend and the accumulation stay fp32.
        mfma="x3": the fp32 layer on the bf16 matrix pipe -- blended values and weights split exactly into three bf16 pieces,
        six bf16 MFMA terms per product (fp32-level rounding; fp32 sources)."""
        lib = _L.load()
        if mfma not in _DCN_PACKING:
            raise ValueError("mfma must be 'fp32', 'bf16', 'fp16' or 'x3'")
        self._mfma_dtype, wdtype, self._kernel = _DCN_PACKING[mfma]       # ("fp16": "bf16" on fp16 sources, products and 16-bit result)
        self.mfma_bf16, self.mfma_f16, self.mfma_x3 = mfma == "bf16", mfma == "fp16", mfma == "x3"
        w = _chk(weight.detach().float().contiguous(), "weight")
        self.Cout, self.C, self.KH, self.KW = w.shape
        self.dg, self.stride, self.pad, self.dil = deform_groups, stride, pad, dil
        self.wpacked = _pack_weights(lib.e2fgvi_packed_dcn_weight_size, lib.e2fgvi_pack_dcn_weight, w, wdtype, "dcn_weight",
                                     self._mfma_dtype, self.Cout, self.C, self.KH, self.KW, extra=(deform_groups,))
        self.bias = None if bias is None else _chk(bias.detach().float().contiguous(), "bias")
        self.name = "dcn"

    def __call__(self, sources, offset, mask=None, off_cols=None, flows=None, max_residue=10.0, out=None, tile=0,
                 out_dtype=torch.float32, planar=False):
        """sources: 1 or 2 NHWC tensors (virtual concat).  offset: [N,Ho,Wo,*] pixel-major; if ``mask`` is None
        the mask words live in the same tensor starting at column dg*2*K (raw conv_offset layout).
        planar=True: the (bf16) sources are [C/16, N, H, W, 16] tensors from ops.to_planar16."""
        lib = _L.load()
        d = _L.MdcnDesc()
        if planar:
            _, N, H, W, _ = sources[0].shape
        else:
            N, H, W, _ = sources[0].shape
        d.src_planar = 1 if planar else 0
        ctot = 0
        for i, t in enumerate(sources):
            _chk_any(t, "source %d" % i)
            if t.dtype != sources[0].dtype:
                raise ValueError("sources must share one dtype")
            c = t.shape[0] * 16 if planar else t.shape[3]
            if planar and (t.dim() != 5 or t.shape[4] != 16 or tuple(t.shape[1:4]) != (N, H, W)):
                raise ValueError("planar source %d must be [C/16, N, H, W, 16]" % i)
            d.src[i], d.src_ld[i], d.src_c[i] = t.data_ptr(), c, c
            ctot += c
        d.src_dtype = _dt(sources[0])                 # bf16 sources: only with mfma="bf16" (checked by the library)
        if ctot != self.C:
            raise ValueError("sources carry %d channels, weight expects %d" % (ctot, self.C))
        d.nsrc = len(sources)
        Ho = (H + 2 * self.pad - (self.dil * (self.KH - 1) + 1)) // self.stride + 1
        Wo = (W + 2 * self.pad - (self.dil * (self.KW - 1) + 1)) // self.stride + 1
        d.N, d.H, d.W, d.Ho, d.Wo = N, H, W, Ho, Wo
        d.KH, d.KW, d.stride, d.pad, d.dil = self.KH, self.KW, self.stride, self.pad, self.dil
        d.deform_groups, d.Cout = self.dg, self.Cout
        K = self.KH * self.KW
        _chk(offset, "offset")
        if tuple(offset.shape[:3]) != (N, Ho, Wo):
            raise ValueError("offset shape %s" % (tuple(offset.shape),))
        d.offset, d.off_ld = offset.data_ptr(), offset.shape[3]
        if mask is None:
            if offset.shape[3] < self.dg * 3 * K:
                raise ValueError("fused offset tensor too narrow")
            d.mask, d.mask_ld = offset.data_ptr() + 4 * self.dg * 2 * K, offset.shape[3]
        else:
            _chk(mask, "mask")
            d.mask, d.mask_ld = mask.data_ptr(), mask.shape[3]
        if flows is not None:
            _chk(flows, "flows")
            if tuple(flows.shape) != (N, Ho, Wo, 4):
                raise ValueError("flows must be [N,Ho,Wo,4]")
            d.flows = flows.data_ptr()
        d.max_residue = max_residue
        d.wpacked = self.wpacked.data_ptr()
        d.bias = self.bias.data_ptr() if self.bias is not None else None
        if out is None:
            out = torch.empty((N, Ho, Wo, self.Cout), dtype=out_dtype, device=sources[0].device)
        _chk_any(out, "out")
        d.dst, d.dst_ld, d.dst_coff, d.tile, d.dst_dtype = out.data_ptr(), out.shape[3], 0, tile, _dt(out)
        d.mfma_dtype = self._mfma_dtype
        if _L.TRACE is not None:
            m = N * Ho * Wo * self.Cout * self.C * K
            _L.annotate(layer=self.name, kernel=self._kernel, shape="N%d %dx%d %d->%d dg%d" % (N, H, W, self.C, self.Cout, self.dg),
                        macs=m, issued=int(m * 6 * 157.3 / 2500.0) if self._mfma_dtype == _L.DT_BF16X3 else m)
        _L.check(lib.e2fgvi_mdcn_nhwc(C.byref(d), _stream()), "mdcn_nhwc")
        return out


# ------------------------------------------------------------------------------------------ attention
def _attn_work(B, T, fh, fw, nkeys):
    """launch-trace record of a focal attention call without its `layer` / `kernel`: algorithmic = the reference's [T*45] x [T*210]
    score and PV products per (window, head); issued = the keys the kernel actually multiplies (zero-padded pooled slots are
    handled analytically), in 32-key tiles, 32-query waves"""
    qpad = -(-(45 * T) // 32) * 32
    return dict(shape="B%d T%d grid %dx%d" % (B, T, fh, fw), macs=B * (fh // 5) * (fw // 9) * 4 * (45 * T) * (210 * T) * 128 * 2,
                issued=B * 4 * qpad * 128 * 2 * sum(-(-(T * k) // 32) * 32 for k in nkeys.tolist()))


def focal_attention(qkv, kv_pool, key_tab, nkeys, B, T, fh, fw, out=None, waves=0):
    lib = _L.load()
    _chk(qkv, "qkv"); _chk(kv_pool, "kv_pool")
    _chk(key_tab, "key_tab", torch.int32); _chk(nkeys, "nkeys", torch.int32)
    rows = B * T * fh * fw
    if tuple(qkv.shape) != (rows, 1536):
        raise ValueError("qkv must be [%d,1536], got %s" % (rows, tuple(qkv.shape)))
    nwin = (fh // 5) * (fw // 9)
    if tuple(kv_pool.shape) != (B * T * nwin, 1536):
        raise ValueError("kv_pool must be [%d,1536], got %s" % (B * T * nwin, tuple(kv_pool.shape)))
    if key_tab.shape[0] != nwin or nkeys.shape[0] != nwin:
        raise ValueError("key table must have %d rows" % nwin)
    if out is None:
        out = torch.empty((rows, 512), dtype=torch.float32, device=qkv.device)
    _chk(out, "out")
    # 32-bit buffer addressing inside the kernel: batches whose qkv spans >= 4 GiB go clip by clip
    rpc, ppc = T * fh * fw, T * nwin
    chunks = list(_image_chunks(B, rpc * 1536 * 4))
    if len(chunks) > 1:
        for b0, b1 in chunks:
            focal_attention(qkv[b0 * rpc:b1 * rpc], kv_pool[b0 * ppc:b1 * ppc], key_tab, nkeys, b1 - b0, T, fh, fw,
                            out=out[b0 * rpc:b1 * rpc], waves=waves)
        return out
    if _L.TRACE is not None:
        _L.annotate(layer="attention", kernel="focal_attn", **_attn_work(B, T, fh, fw, nkeys))
    _L.check(lib.e2fgvi_focal_attention(_ptr(qkv), _ptr(kv_pool), _ptr(key_tab), key_tab.shape[1], _ptr(nkeys),
                                        _ptr(out), B, T, fh, fw, waves, _stream()), "focal_attention")
    return out


def split3_kv(rows_1536, out=None):
    """the k / v columns of fp32 qkv rows ([rows, 1536], token rows followed by the pooled rows) as three bf16 planes
    [3, rows, 1024] whose sum is the fp32 value bit for bit -- the K / V operand of focal_attention_x3"""
    lib = _L.load()
    _chk(rows_1536, "qkv rows")
    if rows_1536.dim() != 2 or rows_1536.shape[1] != 1536:
        raise ValueError("split3_kv takes [rows, 1536] fp32 rows")
    rows = rows_1536.shape[0]
    if out is None:
        out = torch.empty((3, rows, 1024), dtype=torch.bfloat16, device=rows_1536.device)
    _chk(out, "planes", torch.bfloat16)
    _L.check(lib.e2fgvi_split3_kv(_ptr(rows_1536), _ptr(out), rows, _stream()), "split3_kv")
    return out


def focal_attention_x3(qkv, planes, key_tab, nkeys, B, T, fh, fw, out=None, waves=0):
    """focal_attention (fp32 in / out, fp32 softmax) with both products on the bf16 matrix pipe: six exact bf16 MFMA terms
    per fp32 product of three-way split operands (csrc/attention_x3.hip).  qkv: the fp32 token rows [B*T*fh*fw, 1536];
    planes: split3_kv of those rows followed by the B*T*nWin pooled rows."""
    lib = _L.load()
    _chk(qkv, "qkv"); _chk(planes, "planes", torch.bfloat16)
    _chk(key_tab, "key_tab", torch.int32); _chk(nkeys, "nkeys", torch.int32)
    rows = B * T * fh * fw
    nwin = (fh // 5) * (fw // 9)
    if tuple(qkv.shape) != (rows, 1536):
        raise ValueError("qkv must be [%d,1536], got %s" % (rows, tuple(qkv.shape)))
    if tuple(planes.shape) != (3, rows + B * T * nwin, 1024):
        raise ValueError("planes must be [3,%d,1024], got %s" % (rows + B * T * nwin, tuple(planes.shape)))
    if key_tab.shape[0] != nwin or nkeys.shape[0] != nwin:
        raise ValueError("key table must have %d rows" % nwin)
    if out is None:
        out = torch.empty((rows, 512), dtype=torch.float32, device=qkv.device)
    _chk(out, "out")
    if _L.TRACE is not None:
        work = _attn_work(B, T, fh, fw, nkeys)
        # six bf16 MACs per product, in fp32-pipe equivalents (PackedConvX's trace record)
        work["issued"] = int(work["issued"] * 6 * 157.3 / 2500.0)
        _L.annotate(layer="attention", kernel="focal_attn_x3", **work)
    _L.check(lib.e2fgvi_focal_attention_x3(_ptr(qkv), _ptr(planes), _ptr(key_tab), key_tab.shape[1], _ptr(nkeys), _ptr(out),
                                           B, T, fh, fw, waves, _stream()), "focal_attention_x3")
    return out


def attention_x3_applies(B, T, fh, fw):
    """the split-operand attention takes the call: enabled, the three planes inside one 4 GiB buffer resource, and the
    window's key table + two 48 KB stages inside the LDS"""
    rows = B * T * (fh * fw + (fh // 5) * (fw // 9))
    return (X3_ENABLED and 3 * rows * 2048 < 0xFFFFF000
            and -(-(T * 210) // 32) * 128 + 2 * 49152 + 1280 <= 160 * 1024)


def focal_attention_bf16(qkv, kv_pool, key_tab, nkeys, B, T, fh, fw, out=None, variant=None):
    """16-bit data path: qkv [rows,1536] / kv_pool [B*T*nWin,1536] / out [rows,512] are bf16 -- or all fp16
    (the same kernels on fp16 MFMA).
    variant (tests / A-B measurements): kernel variant for this call (see e2fgvi_focal_attention_16_variant)"""
    lib = _L.load()
    if variant is not None:
        prev = lib.e2fgvi_focal_attention_16_variant(int(variant))
        try:
            return focal_attention_bf16(qkv, kv_pool, key_tab, nkeys, B, T, fh, fw, out=out)
        finally:
            lib.e2fgvi_focal_attention_16_variant(prev)
    dt = qkv.dtype if isinstance(qkv, torch.Tensor) and qkv.dtype == torch.float16 else torch.bfloat16
    _chk(qkv, "qkv", dt); _chk(kv_pool, "kv_pool", dt)
    _chk(key_tab, "key_tab", torch.int32); _chk(nkeys, "nkeys", torch.int32)
    rows = B * T * fh * fw
    nwin = (fh // 5) * (fw // 9)
    if tuple(qkv.shape) != (rows, 1536) or tuple(kv_pool.shape) != (B * T * nwin, 1536):
        raise ValueError("qkv must be [%d,1536] and kv_pool [%d,1536]" % (rows, B * T * nwin))
    if key_tab.shape[0] != nwin or nkeys.shape[0] != nwin:
        raise ValueError("key table must have %d rows" % nwin)
    if out is None:
        out = torch.empty((rows, 512), dtype=dt, device=qkv.device)
    _chk(out, "out", dt)
    if _L.TRACE is not None:
        _L.annotate(layer="attention", kernel="focal_attn_f16" if dt == torch.float16 else "focal_attn_bf16",
                    **_attn_work(B, T, fh, fw, nkeys))
    _L.check(lib.e2fgvi_focal_attention_16(_ptr(qkv), _ptr(kv_pool), _ptr(key_tab), key_tab.shape[1], _ptr(nkeys), _ptr(out),
                                           _dt(qkv), B, T, fh, fw, _stream()),
             "focal_attention_f16" if dt == torch.float16 else "focal_attention_bf16")
    return out


# ------------------------------------------------------------------------------------------ small kernels
def nchw_to_nhwc(x, ld=None, scale=1.0, shift=0.0, out_dtype=torch.float32):
    lib = _L.load()
    _chk(x, "x")
    N, Cc, H, W = x.shape
    ld = Cc if ld is None else ld
    out = torch.empty((N, H, W, ld), dtype=out_dtype, device=x.device)
    _L.check(lib.e2fgvi_nchw_to_nhwc(_ptr(x), _ptr(out), _dt(out), N, Cc, H, W, ld, scale, shift, _stream()), "nchw_to_nhwc")
    return out


def cast(x, dtype):
    """fp32 <-> bf16 / fp16 copy of a tensor (round to nearest even; fp16: the bits of torch's .half()); numel must be a
    multiple of 4"""
    lib = _L.load()
    _chk_any(x, "x")
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _L.check(lib.e2fgvi_cast(_ptr(x), _dt(x), _ptr(out), _dt(out), x.numel(), _stream()), "cast")
    return out


def nhwc_to_nchw(x, channels=None):
    lib = _L.load()
    _chk(x, "x")
    N, H, W, ld = x.shape
    Cc = ld if channels is None else channels
    out = torch.empty((N, Cc, H, W), dtype=torch.float32, device=x.device)
    _L.check(lib.e2fgvi_nhwc_to_nchw(_ptr(x), ld, _ptr(out), N, Cc, H, W, _stream()), "nhwc_to_nchw")
    return out


def resize_bilinear(x, out_hw, align_corners, src_nchw=False, channels=None, out_ld=None, scale=None, shift=None):
    lib = _L.load()
    if isinstance(x, torch.Tensor) and x.dtype in HALF16:                # 16-bit data path: NHWC -> NHWC only
        _chk(x, "x", x.dtype)
        if src_nchw or scale is not None or shift is not None or channels is not None or out_ld is not None:
            raise ValueError("16-bit resize: plain NHWC -> NHWC only")
        N, H, W, Cc = x.shape
        out = torch.empty((N, out_hw[0], out_hw[1], Cc), dtype=x.dtype, device=x.device)
        _L.check(lib.e2fgvi_resize_bilinear(_ptr(x), _dt(x), 0, Cc, _ptr(out), Cc, N, Cc, H, W, out_hw[0], out_hw[1],
                                            int(align_corners), None, None, _stream()), "resize_bilinear_16")
        return out
    _chk(x, "x")
    if src_nchw:
        N, Cc, H, W = x.shape
        src_ld = 0
    else:
        N, H, W, src_ld = x.shape
        Cc = src_ld if channels is None else channels
    Ho, Wo = out_hw
    out_ld = Cc if out_ld is None else out_ld
    if out_ld > Cc:
        out = torch.zeros((N, Ho, Wo, out_ld), dtype=torch.float32, device=x.device)
    else:
        out = empty_nhwc(N, Ho, Wo, out_ld, x.device)
    for v, nm in ((scale, "scale"), (shift, "shift")):
        if v is not None:
            _chk(v, nm)
            if v.numel() < Cc:
                raise ValueError("%s needs %d entries" % (nm, Cc))
    _L.check(lib.e2fgvi_resize_bilinear(_ptr(x), _L.DT_F32, int(src_nchw), src_ld, _ptr(out), out_ld, N, Cc, H, W, Ho, Wo,
                                        int(align_corners), _ptr(scale), _ptr(shift), _stream()), "resize_bilinear")
    return out


def avgpool2(x):
    lib = _L.load()
    _chk(x, "x")
    N, H, W, Cc = x.shape
    out = empty_nhwc(N, H // 2, W // 2, Cc, x.device)
    _L.check(lib.e2fgvi_avgpool2_nhwc(_ptr(x), _ptr(out), N, H, W, Cc, _stream()), "avgpool2")
    return out


def spynet_level_input(pyr, ref_idx, supp_idx, flow_prev, copy_dtype=None):
    """copy_dtype (torch.bfloat16 / torch.float16): also return the 8 channels as a 16-bit copy of that type, the source of the
    level's 16-bit conv stack"""
    lib = _L.load()
    _chk(pyr, "pyr"); _chk(ref_idx, "ref_idx", torch.int32); _chk(supp_idx, "supp_idx", torch.int32)
    F_, h, w, c = pyr.shape
    if c != 4:
        raise ValueError("pyramid images must be NHWC4")
    Np = ref_idx.numel()
    if flow_prev is not None:
        _chk(flow_prev, "flow_prev")
        if tuple(flow_prev.shape) != (Np, h // 2, w // 2, 2):
            raise ValueError("flow_prev must be [%d,%d,%d,2], got %s" % (Np, h // 2, w // 2, tuple(flow_prev.shape)))
    out = empty_nhwc(Np, h, w, 8, pyr.device)
    if copy_dtype not in (None,) + HALF16:
        raise TypeError("copy_dtype must be None, torch.bfloat16 or torch.float16")
    out16 = torch.empty((Np, h, w, 8), dtype=copy_dtype, device=pyr.device) if copy_dtype is not None else None
    _L.check(lib.e2fgvi_spynet_level_input(_ptr(pyr), _ptr(ref_idx), _ptr(supp_idx), _ptr(flow_prev), _ptr(out), _ptr(out16),
                                           _dt(out16) if out16 is not None else _L.DT_F32, Np, h, w, _stream()),
             "spynet_level_input")
    return (out, out16) if copy_dtype is not None else out


def prop_cond(feat_prop, feat_n2, flow_a, flow_b, flow_img_stride, cond=None, flows=None, cond_dtype=torch.float32,
              flows8=False):
    """flow_a / flow_b: tensors whose data_ptr is image 0's [H,W,2] flow; image n is at +n*flow_img_stride floats.
    cond_dtype=torch.bfloat16 / torch.float16 writes the warped features as 16-bit (16-bit data path); flows8=True additionally
    returns the four flow values as a [N,H,W,8] conv source (channels 4..7 zero) of the cond's 16-bit type (bf16 beside an fp32
    cond).  16-bit feat_prop / feat_n2 (with a cond of their type): the warp reads the 16-bit copies -- half the gather bytes."""
    lib = _L.load()
    _chk_any(feat_prop, "feat_prop")
    N, H, W, Cc = feat_prop.shape
    if cond is None:
        cond = torch.empty((N, H, W, 2 * Cc), dtype=cond_dtype, device=feat_prop.device)
    if flows is None:
        flows = empty_nhwc(N, H, W, 4, feat_prop.device)
    fl8 = (torch.empty((N, H, W, 8), dtype=cond.dtype if cond.dtype == torch.float16 else torch.bfloat16, device=feat_prop.device)
           if flows8 else None)
    f2_ld = 0
    if flow_b is not None:
        _chk(feat_n2, "feat_n2", feat_prop.dtype)
        f2_ld = feat_n2.shape[3]
    _L.check(lib.e2fgvi_prop_cond(_ptr(feat_prop), Cc, _ptr(feat_n2) if flow_b is not None else None, f2_ld, _dt(feat_prop),
                                  C.c_void_p(flow_a.data_ptr()),
                                  C.c_void_p(flow_b.data_ptr()) if flow_b is not None else None,
                                  flow_img_stride, _ptr(cond), _dt(cond), _ptr(flows), _ptr(fl8), N, H, W, Cc, _stream()),
             "prop_cond")
    return (cond, flows, fl8) if flows8 else (cond, flows)


def layernorm(x, gamma, beta, out=None, out_dtype=torch.float32):
    lib = _L.load()
    _chk(x, "x"); _chk(gamma, "gamma"); _chk(beta, "beta")
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    _chk_any(out, "out")
    _L.check(lib.e2fgvi_layernorm(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), _dt(out), rows, Cc, _stream()), "layernorm")
    return out


def window_pool(x, w45, bias1, BT, fh, fw, out=None):
    lib = _L.load()
    _chk_any(x, "x"); _chk(w45, "w45"); _chk(bias1, "bias1")
    Cc = x.shape[-1]
    rows = BT * (fh // 5) * (fw // 9)
    if out is None:
        out = torch.empty((rows, Cc), dtype=x.dtype, device=x.device)
    elif tuple(_chk(out, "out", x.dtype).shape) != (rows, Cc):
        raise ValueError("window_pool out must be [%d,%d]" % (rows, Cc))
    _L.check(lib.e2fgvi_window_pool(_ptr(x), _dt(x), _ptr(w45), _ptr(bias1), _ptr(out), BT, fh, fw, Cc, _stream()), "window_pool")
    return out


def _ffn_fold(hid, F_, fh, fw, H, W, Cc, gelu):
    lib = _L.load()
    _chk_any(hid, "hid")
    out = torch.empty((F_, H, W, Cc), dtype=hid.dtype, device=hid.device)
    _L.check(lib.e2fgvi_ffn_fold(_ptr(hid), _ptr(out), _dt(hid), gelu, F_, fh, fw, H, W, Cc, _stream()),
             "ffn_fold_gelu" if gelu else "ffn_fold")
    return out


def ffn_fold(hid, F_, fh, fw, H, W, Cc):
    return _ffn_fold(hid, F_, fh, fw, H, W, Cc, 0)


def ffn_fold_gelu(hid, F_, fh, fw, H, W, Cc):
    """GELU(fold(hid) / count): the FFN middle with the GELU in front of the (pure-gather) unfold -- see ffn_unfold"""
    return _ffn_fold(hid, F_, fh, fw, H, W, Cc, 1)


def _ffn_unfold(folded, fh, fw, out, gelu):
    lib = _L.load()
    _chk_any(folded, "folded")
    F_, H, W, Cc = folded.shape
    if out is None:
        out = torch.empty((F_ * fh * fw, 49 * Cc), dtype=folded.dtype, device=folded.device)
    _chk(out, "out", folded.dtype)
    _L.check(lib.e2fgvi_ffn_unfold(_ptr(folded), _ptr(out), _dt(folded), gelu, F_, fh, fw, H, W, Cc, _stream()),
             "ffn_unfold_gelu" if gelu else "ffn_unfold")
    return out


def ffn_unfold(folded, fh, fw, out=None):
    return _ffn_unfold(folded, fh, fw, out, 0)


def ffn_unfold_gelu(folded, fh, fw, out=None):
    return _ffn_unfold(folded, fh, fw, out, 1)


def to_planar16(x, out=None):
    """16-bit NHWC [N,H,W,C] -> [C/16, N, H, W, 16]: the deformable conv's planar source layout (PackedDcn(..., planar=True))"""
    dt = x.dtype if isinstance(x, torch.Tensor) and x.dtype == torch.float16 else torch.bfloat16
    _chk(x, "x", dt)
    N, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((Cc // 16, N, H, W, 16), dtype=dt, device=x.device)
    _chk(out, "out", dt)
    _L.check(_L.load().e2fgvi_nhwc_to_planar16(_ptr(x), _ptr(out), N * H * W, Cc, _stream()), "nhwc_to_planar16")
    return out


def softcomp_fold(emb, F_, fh, fw, H, W, Cc, bias_hwc=None, residual=None):
    """emb, residual and the result share one element type (fp32, or bf16 / fp16 on the 16-bit data path); bias_hwc is fp32"""
    lib = _L.load()
    dt = emb.dtype if isinstance(emb, torch.Tensor) and emb.dtype in HALF16 else torch.float32
    _chk(emb, "emb", dt)
    out = torch.empty((F_, H, W, Cc), dtype=dt, device=emb.device)
    if bias_hwc is not None:
        _chk(bias_hwc, "bias_hwc")
    if residual is not None:
        _chk(residual, "residual", dt)
    _L.check(lib.e2fgvi_softcomp_fold(_ptr(emb), _ptr(bias_hwc), _ptr(residual), _ptr(out), _dt(out), F_, fh, fw, H, W, Cc,
                                      _stream()), "softcomp_fold")
    return out


# ------------------------------------------------------------------------------------------ video driver (byte side)
def _u8(t, name):
    return _chk(t, name, torch.uint8)


def _frame_ids(ids, device):
    """a device int32 table [n], n > 0, of frame numbers (range-checked in the kernels, not here: no host read)"""
    _chk(ids, "ids", torch.int32)
    if ids.dim() != 1 or ids.numel() == 0 or ids.device != device:
        raise ValueError("ids must be a non-empty int32 [n] on the device of the frames")
    return ids.numel()


def _int_arg(name, v, lo, hi):
    """``v`` as an int: an integer in [lo, hi], no bool; ValueError that names the argument otherwise"""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
        raise ValueError("%s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
    return int(v)


def _flag_arg(check):
    """check= as 0 / 1: a bool, or the integer 0 or 1; ValueError otherwise"""
    if not isinstance(check, (bool, numbers.Integral)) or check not in (0, 1):
        raise ValueError("check must be a bool (or 0 / 1), got %r" % (check,))
    return int(check)


def _device_inputs(named, first, written=()):
    """``named`` = ((name, value, dtype), ...) -> the tensors on the device of the first one that is there already (anything else
    through torch.as_tensor and uploaded); a wrong dtype, a non-contiguous input, a tensor on another device than the first (the
    message calls it ``first``) and a name of ``written`` that is no device tensor raise ValueError"""
    for nm, t, _ in named:
        if nm in written and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError("%s is written: it must be a device tensor, got %s" % (nm, type(t).__name__))
    device = next((t.device for _, t, _ in named if isinstance(t, torch.Tensor) and t.is_cuda), "cuda")
    up = [t if isinstance(t, torch.Tensor) and t.is_cuda else torch.as_tensor(t).to(device) for _, t, _ in named]
    for t, (nm, _, dt) in zip(up, named):
        if t.dtype != dt:
            raise ValueError("%s must be %s, got %s" % (nm, dt, t.dtype))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % nm)
        if t.device != up[0].device:
            raise ValueError("%s is on %s, the %s on %s" % (nm, t.device, first, up[0].device))
    return up


def _alloc(work, shape, dtype, device, out=None):
    """the buffer a launch fills: empty when the launch writes every entry (``work``), zeros when there is no work and the zeros
    are the answer; ``out`` when given, zeroed when there is no work"""
    if out is not None:
        return out if work else out.zero_()
    return (torch.empty if work else torch.zeros)(shape, dtype=dtype, device=device)


def _frames_shape(t, name):
    """(L, H, W) of ``t`` as [L,H,W,3]; ValueError that names it otherwise"""
    if t.dim() != 4 or t.shape[3] != 3:
        raise ValueError("%s must be [L,H,W,3], got %s" % (name, tuple(t.shape)))
    return tuple(t.shape[:3])


def _scene_table(t, name, L):
    """a scene table is int32 [L] (the dtype is _device_inputs'); ValueError that names it otherwise"""
    if tuple(t.shape) != (L,):
        raise ValueError("%s must be int32 [%d], got %s" % (name, L, tuple(t.shape)))


def mask_prepare(masks_u8, ytab, xtab, H, W, iterations=4, ids=None):
    """masks_u8 [L,Hin,Win] uint8 -> [L,H,W] uint8 of 0/1 (NEAREST resize by the given tables, > 0, cross dilation).
    ``ids`` device int32 [n]: -> [n,H,W], output frame l from masks_u8[ids[l]] (an id outside [0, L): an empty mask)."""
    lib = _L.load()
    _u8(masks_u8, "masks")
    _chk(ytab, "ytab", torch.int32); _chk(xtab, "xtab", torch.int32)
    L, Hin, Win = masks_u8.shape
    if ytab.numel() != H or xtab.numel() != W:
        raise ValueError("ytab / xtab must have H / W entries")
    if ids is not None:
        n = _frame_ids(ids, masks_u8.device)
        out = torch.empty((n, H, W), dtype=torch.uint8, device=masks_u8.device)
        _L.check(lib.e2fgvi_mask_prepare_ids(_ptr(masks_u8), L, _ptr(ids), n, Hin, Win, _ptr(ytab), _ptr(xtab), _ptr(out), H, W,
                                             iterations, _stream()), "mask_prepare_ids")
        return out
    out = torch.empty((L, H, W), dtype=torch.uint8, device=masks_u8.device)
    _L.check(lib.e2fgvi_mask_prepare(_ptr(masks_u8), L, Hin, Win, _ptr(ytab), _ptr(xtab), _ptr(out), H, W, iterations, _stream()),
             "mask_prepare")
    return out


def masked_clip(frames_u8, masks01, ids, Hp, Wp):
    """frames_u8 [L,H,W,3], masks01 [L,H,W], ids int32 [t] -> fp32 [1,t,3,Hp,Wp] masked clip in [-1,1], mirror padded."""
    lib = _L.load()
    _u8(frames_u8, "frames"); _u8(masks01, "masks"); _chk(ids, "ids", torch.int32)
    L, H, W, _ = frames_u8.shape
    t = ids.numel()
    out = torch.empty((1, t, 3, Hp, Wp), dtype=torch.float32, device=frames_u8.device)
    _L.check(lib.e2fgvi_masked_clip(_ptr(frames_u8), _ptr(masks01), _ptr(ids), t, H, W, _ptr(out), Hp, Wp, _stream()), "masked_clip")
    return out


def composite(pred, ids, first, frames_u8, masks01, comp):
    """pred fp32 [>=n,3,Hp,Wp]; ids int32 [n]; first uint8 [n]; comp fp32 [L,H,W,3] updated in place (test.py:168-179)."""
    lib = _L.load()
    _chk(pred, "pred"); _chk(ids, "ids", torch.int32); _u8(first, "first"); _u8(frames_u8, "frames"); _u8(masks01, "masks")
    _chk(comp, "comp")
    L, H, W, _ = frames_u8.shape
    n = ids.numel()
    if pred.shape[0] < n or pred.shape[1] != 3:
        raise ValueError("pred must hold at least %d frames of 3 channels" % n)
    _L.check(lib.e2fgvi_composite(_ptr(pred), _ptr(ids), _ptr(first), n, _ptr(frames_u8), _ptr(masks01), _ptr(comp), H, W,
                                  pred.shape[2], pred.shape[3], _stream()), "composite")
    return comp


def _taps_of(span, n_out):
    """ksize of video.bicubic_tables for `span` source pixels resized to n_out"""
    return 2 * math.ceil(2.0 * max(span / n_out, 1.0)) + 1


def resample_u8(frames_u8, n_out, axis, bounds, coeffs, span=None, ids=None):
    """frames_u8 [L,H,W,3] uint8 -> uint8 with dimension `axis` (1: H, 2: W) resized to n_out: one bicubic pass of PIL's
    Image.resize with the tables of video.bicubic_tables (bounds int32 [n_out,2], coeffs int32 [n_out,ksize]).  ``span``: the
    number of source pixels the tables were built for when that is a box of the axis (bicubic_tables(box=)), not all of it.
    ``ids`` device int32 [n]: the result has n frames, frame l the pass over frames_u8[ids[l]] (an id outside [0, L): zeros)."""
    lib = _L.load()
    _u8(frames_u8, "frames"); _chk(bounds, "bounds", torch.int32); _chk(coeffs, "coeffs", torch.int32)
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError("frames must be [L,H,W,3], got %s" % (tuple(frames_u8.shape),))
    if axis not in (1, 2):
        raise ValueError("axis must be 1 (H) or 2 (W), got %r" % (axis,))
    if bounds.device != frames_u8.device or coeffs.device != frames_u8.device:
        raise ValueError("frames, bounds and coeffs must be on one device")
    if bounds.dim() != 2 or tuple(bounds.shape) != (n_out, 2) or coeffs.dim() != 2 or coeffs.shape[0] != n_out:
        raise ValueError("bounds must be [n_out,2] and coeffs [n_out,ksize] for n_out = %d" % n_out)
    L, H, W, _ = frames_u8.shape
    n_in = frames_u8.shape[axis]
    ksize = coeffs.shape[1]
    if span is not None and not 0 < span <= n_in:
        raise ValueError("span must be in (0, %d], got %r" % (n_in, span))
    if ksize != _taps_of(n_in if span is None else span, n_out):
        raise ValueError("coeffs of %d taps do not belong to a %d -> %d resize" % (ksize, n_in if span is None else span, n_out))
    n = L if ids is None else _frame_ids(ids, frames_u8.device)
    shape = (n, n_out, W, 3) if axis == 1 else (n, H, n_out, 3)
    out = torch.empty(shape, dtype=torch.uint8, device=frames_u8.device)
    if ids is not None:
        _L.check(lib.e2fgvi_resample_ids_u8(_ptr(frames_u8), L, _ptr(ids), n, _ptr(out), H, W, n_out, axis, _ptr(bounds), _ptr(coeffs),
                                            ksize, _stream()), "resample_ids_u8")
        return out
    _L.check(lib.e2fgvi_resample_u8(_ptr(frames_u8), _ptr(out), L, H, W, n_out, axis, _ptr(bounds), _ptr(coeffs), ksize, _stream()),
             "resample_u8")
    return out


def resample_rows_u8(frames_u8, n_out, row0, rows, bounds, coeffs, ids=None):
    """The width pass of resample_u8 over rows [row0, row0 + rows) of every frame: frames_u8 [L,H,W,3] uint8 -> [L,rows,n_out,3].
    bounds int32 [n_out,2] hold absolute source columns (video.bicubic_tables(W, n_out, box=(left, right)), or one-tap tables of
    a crop), coeffs int32 [n_out,ksize], ksize >= 1 the tables' own; entries are clipped to the frame in the kernel.
    ``ids`` device int32 [n]: -> [n,rows,n_out,3], frame l the pass over frames_u8[ids[l]] (an id outside [0, L): zeros)."""
    lib = _L.load()
    _u8(frames_u8, "frames"); _chk(bounds, "bounds", torch.int32); _chk(coeffs, "coeffs", torch.int32)
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError("frames must be [L,H,W,3], got %s" % (tuple(frames_u8.shape),))
    if bounds.device != frames_u8.device or coeffs.device != frames_u8.device:
        raise ValueError("frames, bounds and coeffs must be on one device")
    if bounds.dim() != 2 or tuple(bounds.shape) != (n_out, 2) or coeffs.dim() != 2 or coeffs.shape[0] != n_out or coeffs.shape[1] < 1:
        raise ValueError("bounds must be [n_out,2] and coeffs [n_out,ksize] for n_out = %d" % n_out)
    L, H, W, _ = frames_u8.shape
    row0, rows = int(row0), int(rows)
    if row0 < 0 or rows < 1 or row0 + rows > H:
        raise ValueError("rows [%d, %d) are not rows of a %d-row frame" % (row0, row0 + rows, H))
    n = L if ids is None else _frame_ids(ids, frames_u8.device)
    out = torch.empty((n, rows, n_out, 3), dtype=torch.uint8, device=frames_u8.device)
    if ids is not None:
        _L.check(lib.e2fgvi_resample_rows_ids_u8(_ptr(frames_u8), L, _ptr(ids), n, _ptr(out), H, W, n_out, row0, rows, _ptr(bounds),
                                                 _ptr(coeffs), coeffs.shape[1], _stream()), "resample_rows_ids_u8")
        return out
    _L.check(lib.e2fgvi_resample_rows_u8(_ptr(frames_u8), _ptr(out), L, H, W, n_out, row0, rows, _ptr(bounds), _ptr(coeffs),
                                         coeffs.shape[1], _stream()), "resample_rows_u8")
    return out


def hole_bbox(masks_u8):
    """masks_u8 [L,Hm,Wm] uint8 on the device (any non-zero byte is hole) -> device int32 [4] = (x0, y0, x1, y1), the hole's
    bounding box over all frames, upper ends exclusive; x1 <= x0: no hole.  No host read (csrc/video.hip hole_bbox_kernel)."""
    lib = _L.load()
    _u8(masks_u8, "masks")
    if masks_u8.dim() != 3:
        raise ValueError("masks must be [L,Hm,Wm], got %s" % (tuple(masks_u8.shape),))
    L, Hm, Wm = masks_u8.shape
    out = torch.empty(4, dtype=torch.int32, device=masks_u8.device)
    _L.check(lib.e2fgvi_hole_bbox(_ptr(masks_u8), L, Hm, Wm, _ptr(out), _stream()), "hole_bbox")
    return out


def hole_bbox_frames(masks_u8):
    """hole_bbox per frame: masks_u8 [L,Hm,Wm] uint8 on the device -> device int32 [L,4], row l = (x0, y0, x1, y1) of frame l in
    hole_bbox's convention (upper ends exclusive; x1 <= x0: no hole in that frame).  One pass over the masks, no host read."""
    lib = _L.load()
    _u8(masks_u8, "masks")
    if masks_u8.dim() != 3:
        raise ValueError("masks must be [L,Hm,Wm], got %s" % (tuple(masks_u8.shape),))
    L, Hm, Wm = masks_u8.shape
    out = torch.empty((L, 4), dtype=torch.int32, device=masks_u8.device)
    _L.check(lib.e2fgvi_hole_bbox_frames(_ptr(masks_u8), L, Hm, Wm, _ptr(out), _stream()), "hole_bbox_frames")
    return out


def scene_diff(frames_u8):
    """frames_u8 [L,H,W,3] uint8 on the device, L >= 2 -> device int64 [L-1]: the block-histogram difference of every pair of
    adjacent frames (csrc/video.hip scene_hist_kernel / scene_diff_kernel; include/e2fgvi_hip.h has the definition), an exact
    integer in 0 .. 2 H W.  No host read; video.scene_scores normalises it, video.cuts_from_scores turns it into cuts."""
    lib = _L.load()
    _u8(frames_u8, "frames")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError("frames must be [L,H,W,3], got %s" % (tuple(frames_u8.shape),))
    L, H, W, _ = frames_u8.shape
    if L < 2:
        raise ValueError("scene_diff needs at least two frames, got %d" % L)
    nbytes = lib.e2fgvi_scene_diff_workspace(L, H, W)
    if nbytes < 0:
        _L.check(int(nbytes), "scene_diff_workspace")
    with torch.cuda.device(frames_u8.device):
        work = torch.empty(int(nbytes) // 4, dtype=torch.int32, device=frames_u8.device)
        out = torch.empty(L - 1, dtype=torch.int64, device=frames_u8.device)
        _L.check(lib.e2fgvi_scene_diff(_ptr(frames_u8), L, H, W, _ptr(work), _ptr(out), _stream()), "scene_diff")
    return out


LABEL_TILE_W, LABEL_TILE_H = 64, 32        # csrc/video.hip LB_TW, LB_TH: the tile one workgroup labels in LDS


def hole_components(masks_u8):
    """masks_u8 [L,Hm,Wm] uint8 on the device (any non-zero byte is hole) -> (labels, boxes), both on the device: labels int32
    [Hm,Wm] is 0 outside the footprint of the masks (the OR over the frames) and elsewhere the number 1 .. K of the pixel's
    8-connected component, numbered in raster order of the components' first pixels (scipy.ndimage.label's order; the integers
    do not depend on how the threads ran); boxes int32 [K,5], row k - 1 = (x0, y0, x1, y1, area) of component k, upper ends
    exclusive as for hole_bbox.  One host read, of K, to size the table (csrc/video.hip label_*_kernel; include/e2fgvi_hip.h has
    the definition)."""
    lib = _L.load()
    _u8(masks_u8, "masks")
    if masks_u8.dim() != 3:
        raise ValueError("masks must be [L,Hm,Wm], got %s" % (tuple(masks_u8.shape),))
    L, Hm, Wm = masks_u8.shape
    dev = masks_u8.device
    if Hm * Wm == 0:
        return torch.zeros((Hm, Wm), dtype=torch.int32, device=dev), torch.zeros((0, 5), dtype=torch.int32, device=dev)
    nbytes = lib.e2fgvi_hole_label_workspace(Hm, Wm)
    if nbytes < 0:
        _L.check(int(nbytes), "hole_label_workspace")
    with torch.cuda.device(dev):
        work = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        labels = torch.empty((Hm, Wm), dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        _L.check(lib.e2fgvi_hole_label(_ptr(masks_u8), L, Hm, Wm, _ptr(work), _ptr(labels), _ptr(count), _stream()), "hole_label")
        K = int(count.item())
        boxes = torch.empty((K, 5), dtype=torch.int32, device=dev)
        if K:
            _L.check(lib.e2fgvi_label_boxes(_ptr(labels), Hm, Wm, K, _ptr(boxes), _stream()), "label_boxes")
    return labels, boxes


OVERLAY_TILE_W, OVERLAY_TILE_H = 64, 32    # csrc/video.hip OV_TW, OV_TH: the pixel tile of a workgroup of both overlay kernels
OVERLAY_CHUNK = 8                          # csrc/video.hip OV_CHUNK: overlay_stats splits L frames into at most L // 8 chunks of
                                           # equal length (to within one frame), so none is shorter; fewer than 16 frames are one chunk
OVERLAY_FRAMES_MAX = 1 << 22               # csrc/video.hip OV_LMAX: more frames would overflow the int32 sums
OVERLAY_RADIUS_MAX = 16                    # csrc/video.hip OV_RMAX: the largest dilation radius overlay_edges keeps in LDS


def overlay_stats(frames_u8):
    """frames_u8 [L,H,W,3] uint8 on the device, 1 <= L <= OVERLAY_FRAMES_MAX -> device int32 [3,H,W] = (Sx, Sy, M): per pixel the
    sums over the frames of the luma gradient's two components and of |gx| + |gy|, central differences of the scene detector's
    integer luma with clamped borders (csrc/video.hip overlay_stats_kernel; include/e2fgvi_hip.h has the definition).  One pass
    over the frames, exact integers that do not depend on how the threads ran, no host read; overlay_edges thresholds them."""
    lib = _L.load()
    _u8(frames_u8, "frames")
    L, H, W = _frames_shape(frames_u8, "frames")
    if not 1 <= L <= OVERLAY_FRAMES_MAX:
        raise ValueError("overlay_stats needs between 1 and %d frames, got %d" % (OVERLAY_FRAMES_MAX, L))
    if H * W == 0:
        raise ValueError("overlay_stats needs frames with pixels, got %d x %d" % (H, W))
    with torch.cuda.device(frames_u8.device):
        out = torch.empty((3, H, W), dtype=torch.int32, device=frames_u8.device)
        _L.check(lib.e2fgvi_overlay_stats(_ptr(frames_u8), L, H, W, _ptr(out), _stream()), "overlay_stats")
    return out


def overlay_edges(stats, L, g_min, coherence, radius):
    """stats: overlay_stats's int32 [3,H,W] of L frames -> (D, count), both on the device.  A pixel is a persistent edge when
    M >= g_min L and 256 (|Sx| + |Sy|) >= coherence M (64-bit integers); D uint8 [H,W] is 1 where the (2 radius + 1)-pixel box
    around the pixel, clipped at the frame, holds a persistent edge and 0 elsewhere; count int32 [1] is the number of set pixels
    of D.  Threshold and dilation are one launch (csrc/video.hip overlay_edges_kernel), no host read.  g_min >= 1, coherence in
    [1, 256], radius in [0, OVERLAY_RADIUS_MAX], L in [1, OVERLAY_FRAMES_MAX]: integers (ValueError otherwise, bools included)."""
    lib = _L.load()
    _chk(stats, "stats", torch.int32)
    if stats.dim() != 3 or stats.shape[0] != 3 or stats.shape[1] * stats.shape[2] == 0:
        raise ValueError("stats must be [3,H,W] with H, W >= 1, got %s" % (tuple(stats.shape),))
    L = _int_arg("L", L, 1, OVERLAY_FRAMES_MAX)
    g_min = _int_arg("g_min", g_min, 1, 2 ** 31 - 1)
    coherence = _int_arg("coherence", coherence, 1, 256)
    radius = _int_arg("radius", radius, 0, OVERLAY_RADIUS_MAX)
    _, H, W = stats.shape
    with torch.cuda.device(stats.device):
        out = torch.empty((H, W), dtype=torch.uint8, device=stats.device)
        count = torch.empty(1, dtype=torch.int32, device=stats.device)
        _L.check(lib.e2fgvi_overlay_edges(_ptr(stats), L, H, W, g_min, coherence, radius, _ptr(out), _ptr(count), _stream()),
                 "overlay_edges")
    return out, count


def mask_track_step(planes, fwd, bwd, jobs, check=True):
    """One step of carrying binary masks along a video's flows (csrc/mask_track.hip; include/e2fgvi_hip.h has the definition;
    video.propagate_masks runs the chains): planes uint8 [2,L,H,W] of 0 / 1, L >= 2, plane 0 carried forward in time and plane 1
    backward, updated in place; fwd, bwd fp32 [L-1,H,W,2] in metrics.warp_error's convention; jobs int32 [n,2] of (pair t, dir):
    dir 0 writes plane 0 frame t+1 from frame t, pulled along bwd[t] and checked against fwd[t]; dir 1 writes plane 1 frame t from
    frame t+1, pulled along fwd[t] and checked against bwd[t].  One launch runs all n jobs; no job of a call may write a frame of a
    plane that another reads or writes (video.plan_mask_chains).  check=False switches the forward / backward consistency test
    off.  Device tensors, or anything torch.as_tensor accepts (uploaded first); wrong dtypes, shapes that do not fit,
    non-contiguous inputs and tensors on different devices raise ValueError.  Returns the planes on the device (the tensor that
    was passed when it was there already).  The same inputs give the same bits in every run."""
    lib = _L.load()
    check = _flag_arg(check)
    named = (("planes", planes, torch.uint8), ("fwd", fwd, torch.float32), ("bwd", bwd, torch.float32), ("jobs", jobs, torch.int32))
    pl, fw, bw, jb = _device_inputs(named, "planes")
    if pl.dim() != 4 or pl.shape[0] != 2:
        raise ValueError("planes must be [2,L,H,W], got %s" % (tuple(pl.shape),))
    _, L, H, W = pl.shape
    if L < 2:
        raise ValueError("mask_track_step needs at least two frames, got planes %s" % (tuple(pl.shape),))
    for t, nm in ((fw, "fwd"), (bw, "bwd")):
        if tuple(t.shape) != (L - 1, H, W, 2):
            raise ValueError("%s must be [%d,%d,%d,2] for planes %s, got %s" % (nm, L - 1, H, W, tuple(pl.shape), tuple(t.shape)))
    if jb.dim() != 2 or jb.shape[1] != 2:
        raise ValueError("jobs must be int32 [n,2] of (pair, dir), got %s" % (tuple(jb.shape),))
    with torch.cuda.device(pl.device):
        _L.check(lib.e2fgvi_mask_track_step(_ptr(pl), _ptr(fw), _ptr(bw), _ptr(jb), jb.shape[0], L, H, W, check, _stream()),
                 "mask_track_step")
    return pl


DEFECT_THRESHOLD_MAX = 254                 # csrc/defects.hip: tau, slack, support and radius outside these are E2FGVI_EINVAL
DEFECT_SLACK_MAX = 2
DEFECT_RADIUS_MAX = 16                     # csrc/defects.hip DF_RMAX: the largest dilation radius defect_clean keeps in LDS


def defect_candidates(frames, fwd, bwd, ids, threshold, slack, out=None):
    """The candidates of the dust-and-dirt detector (csrc/defects.hip; include/e2fgvi_hip.h has the definition; video.detect_defects
    is the caller): frames uint8 [L,H,W,3]; fwd, bwd fp32 [L-1,H,W,2] in metrics.warp_error's convention; ids int32 [n], the centre
    frames to do (distinct; one outside [1, L-2] writes nothing) -> device uint8 [L,H,W] of 0 / 1: a pixel of a listed frame is 1
    when its integer luma lies more than ``threshold`` above the largest or below the smallest luma of the pixels around its
    motion-compensated position in BOTH neighbouring frames (``slack`` more pixels on every side of the 2 x 2 the bilinear sample
    would read).  One launch, no host read.  ``out``: a device uint8 [L,H,W] to write the listed frames into (its other frames stay
    as they are); without it a buffer of zeros.  threshold in [0, 254], slack in [0, 2]: integers, no bools.  Device tensors, or
    anything torch.as_tensor accepts (uploaded first); wrong dtypes, shapes that do not fit, non-contiguous inputs and tensors on
    different devices raise ValueError.  There is no CPU path.  The same inputs give the same bits in every run."""
    lib = _L.load()
    threshold = _int_arg("threshold", threshold, 0, DEFECT_THRESHOLD_MAX)
    slack = _int_arg("slack", slack, 0, DEFECT_SLACK_MAX)
    named = [("frames", frames, torch.uint8), ("fwd", fwd, torch.float32), ("bwd", bwd, torch.float32), ("ids", ids, torch.int32)]
    if out is not None:
        named.append(("out", out, torch.uint8))
    up = _device_inputs(named, "frames")
    fr, fw, bw, idt = up[:4]
    L, H, W = _frames_shape(fr, "frames")
    if idt.dim() != 1:
        raise ValueError("ids must be int32 [n], got %s" % (tuple(idt.shape),))
    for t, nm in ((fw, "fwd"), (bw, "bwd")):
        if L >= 1 and tuple(t.shape) != (L - 1, H, W, 2):
            raise ValueError("%s must be [%d,%d,%d,2] for frames %s, got %s" % (nm, L - 1, H, W, tuple(fr.shape), tuple(t.shape)))
    if out is not None and tuple(up[4].shape) != (L, H, W):
        raise ValueError("out must be [%d,%d,%d], got %s" % (L, H, W, tuple(up[4].shape)))
    with torch.cuda.device(fr.device):
        cand = up[4] if out is not None else torch.zeros((L, H, W), dtype=torch.uint8, device=fr.device)
        _L.check(lib.e2fgvi_defect_candidates(_ptr(fr), _ptr(fw), _ptr(bw), _ptr(idt), idt.shape[0], L, H, W, threshold, slack,
                                              _ptr(cand), _stream()), "defect_candidates")
    return cand


def defect_clean(cand, ids, support, radius, out=None):
    """The support test and the dilation of the dust-and-dirt detector, one launch (csrc/defects.hip defect_clean_kernel;
    include/e2fgvi_hip.h has the definition): cand uint8 [L,H,W] (any non-zero byte is a candidate), ids int32 [n] as for
    defect_candidates -> (masks, counts) on the device: in a listed frame a candidate stays when the 3 x 3 box around it, clipped
    at the frame, holds at least ``support`` candidates (itself included), masks uint8 [L,H,W] is 255 where the (2 radius + 1)-pixel
    box around the pixel holds one that stayed and 0 elsewhere, and counts int32 [L] is the number of set pixels of the frame -- 0
    for a frame that is not listed.  ``out``: a device uint8 [L,H,W] to write the listed frames' masks into (its other frames stay
    as they are); without it a buffer of zeros.  support in [1, 9], radius in [0, DEFECT_RADIUS_MAX]: integers, no bools.  The
    checks of defect_candidates; no host read; exact integers, the same in every run."""
    lib = _L.load()
    support = _int_arg("support", support, 1, 9)
    radius = _int_arg("radius", radius, 0, DEFECT_RADIUS_MAX)
    named = [("cand", cand, torch.uint8), ("ids", ids, torch.int32)]
    if out is not None:
        named.append(("out", out, torch.uint8))
    up = _device_inputs(named, "candidates")
    cd, idt = up[:2]
    if cd.dim() != 3:
        raise ValueError("cand must be [L,H,W], got %s" % (tuple(cd.shape),))
    L, H, W = cd.shape
    if idt.dim() != 1:
        raise ValueError("ids must be int32 [n], got %s" % (tuple(idt.shape),))
    if out is not None and tuple(up[2].shape) != (L, H, W):
        raise ValueError("out must be [%d,%d,%d], got %s" % (L, H, W, tuple(up[2].shape)))
    with torch.cuda.device(cd.device):
        masks = up[2] if out is not None else torch.zeros((L, H, W), dtype=torch.uint8, device=cd.device)
        counts = torch.zeros(L, dtype=torch.int32, device=cd.device)
        _L.check(lib.e2fgvi_defect_clean(_ptr(cd), _ptr(idt), idt.shape[0], L, H, W, support, radius, _ptr(masks), _ptr(counts),
                                         _stream()), "defect_clean")
    return masks, counts


PIXEL_REACH_MAX = 254                      # csrc/pixel_track.hip: the largest age a byte of the planes can hold


def pixel_track_step(hole, age, origin, fwd, bwd, jobs, reach=PIXEL_REACH_MAX, check=True):
    """One step of carrying, for every hole pixel, the place its colour can be seen at along a video's flows
    (csrc/pixel_track.hip; include/e2fgvi_hip.h has the definition; video.propagate_pixels runs the chains): hole uint8 [L,H,W] of
    0 / 1, L >= 2; age uint8 [2,L,H,W] (255 = not reached, 0 = known, a = reached after a steps; both planes start as 255 * hole;
    plane 0 travels forward in time, plane 1 backward) and origin fp32 [2,L,H,W,2], both updated in place at hole pixels only; fwd,
    bwd fp32 [L-1,H,W,2] in metrics.warp_error's convention; jobs int32 [n,2] of (pair t, dir): dir 0 writes plane 0 frame t+1 from
    frame t, pulled along bwd[t] and checked against fwd[t]; dir 1 writes plane 1 frame t from frame t+1, pulled along fwd[t] and
    checked against bwd[t].  One launch runs all n jobs; no job of a call may write a frame of a plane that another reads or writes
    (video.plan_pixel_chains).  ``reach``: the largest age, an integer in [1, 254]; check=False switches the forward / backward
    consistency test off.  age and origin must be device tensors (they are written); the others device tensors or anything
    torch.as_tensor accepts (uploaded first); wrong dtypes, shapes that do not fit, non-contiguous inputs and tensors on different
    devices raise ValueError.  Returns (age, origin).  The same inputs give the same bits in every run."""
    lib = _L.load()
    reach = _int_arg("reach", reach, 1, PIXEL_REACH_MAX)
    check = _flag_arg(check)
    named = (("age", age, torch.uint8), ("hole", hole, torch.uint8), ("origin", origin, torch.float32), ("fwd", fwd, torch.float32),
             ("bwd", bwd, torch.float32), ("jobs", jobs, torch.int32))
    ag, ho, og, fw, bw, jb = _device_inputs(named, "age", written=("age", "origin"))
    if ag.dim() != 4 or ag.shape[0] != 2:
        raise ValueError("age must be [2,L,H,W], got %s" % (tuple(ag.shape),))
    _, L, H, W = ag.shape
    if L < 2:
        raise ValueError("pixel_track_step needs at least two frames, got age %s" % (tuple(ag.shape),))
    for t, nm, shape in ((ho, "hole", (L, H, W)), (og, "origin", (2, L, H, W, 2)), (fw, "fwd", (L - 1, H, W, 2)),
                         (bw, "bwd", (L - 1, H, W, 2))):
        if tuple(t.shape) != shape:
            raise ValueError("%s must be %s for age %s, got %s" % (nm, list(shape), tuple(ag.shape), tuple(t.shape)))
    if jb.dim() != 2 or jb.shape[1] != 2:
        raise ValueError("jobs must be int32 [n,2] of (pair, dir), got %s" % (tuple(jb.shape),))
    with torch.cuda.device(ag.device):
        _L.check(lib.e2fgvi_pixel_track_step(_ptr(ho), _ptr(ag), _ptr(og), _ptr(fw), _ptr(bw), _ptr(jb), jb.shape[0], L, H, W, reach,
                                             check, _stream()), "pixel_track_step")
    return ag, og


def pixel_fill(src, hole, age, origin, out, return_source=False):
    """The colours of the hole pixels pixel_track_step reached, one launch over all frames (csrc/pixel_track.hip
    pixel_fill_kernel; include/e2fgvi_hip.h has the definition): src uint8 [L,H,W,3], the frames the colours are read from; hole
    uint8 [L,H,W] of 0 / 1; age uint8 [2,L,H,W] and origin fp32 [2,L,H,W,2] as the steps left them; out uint8 [L,H,W,3], a device
    tensor updated in place: a hole pixel gets one bilinear sample of src[f] at its origin, from the plane of the smaller age (a tie:
    plane 0) whose four corners are known pixels of that frame, and keeps its bytes when neither plane has one; no other byte is
    written.  Returns out, or with ``return_source`` (out, source): device uint8 [L,H,W] of 0 (no hole pixel), 1 (plane 0), 2
    (plane 1), 3 (a hole pixel left as it was).  The checks of pixel_track_step; no host read; the same bits in every run."""
    lib = _L.load()
    named = (("out", out, torch.uint8), ("src", src, torch.uint8), ("hole", hole, torch.uint8), ("age", age, torch.uint8),
             ("origin", origin, torch.float32))
    ou, sr, ho, ag, og = _device_inputs(named, "out", written=("out",))
    L, H, W = _frames_shape(ou, "out")
    for t, nm, shape in ((sr, "src", (L, H, W, 3)), (ho, "hole", (L, H, W)), (ag, "age", (2, L, H, W)), (og, "origin", (2, L, H, W, 2))):
        if tuple(t.shape) != shape:
            raise ValueError("%s must be %s for out %s, got %s" % (nm, list(shape), tuple(ou.shape), tuple(t.shape)))
    if sr.data_ptr() == ou.data_ptr() and sr.numel():
        raise ValueError("src and out must be different buffers: out is written while src is read")
    with torch.cuda.device(ou.device):
        source = torch.empty((L, H, W), dtype=torch.uint8, device=ou.device) if return_source else None
        _L.check(lib.e2fgvi_pixel_fill(_ptr(sr), _ptr(ho), _ptr(ag), _ptr(og), _ptr(ou), _ptr(source) if return_source else None,
                                       L, H, W, _stream()), "pixel_fill")
    return (ou, source) if return_source else ou


GRAIN_MIN_BLOCKS = 32                      # measured blocks a scene, and a band of it, needs for a level of its own
GRAIN_SCALE_MAX = (1 << 22) - 1            # csrc/grain.hip GR_SCALE_MAX: 510 * scale + 2^15 stays below 2^31
GRAIN_STRENGTH_Q8_MAX = 1024               # strength 4 in 1 / 256


def grain_blocks(frames, hole=None):
    """The block sums the grain is measured from, one launch over all frames (csrc/grain.hip grain_blocks_kernel;
    include/e2fgvi_hip.h has the definition; video.match_grain is the caller): frames uint8 [L,H,W,3]; hole uint8 [L,H,W] or None
    (any non-zero byte is hole) -> (energy int32 [L,Hb,Wb,3], band uint8 [L,Hb,Wb]) on the device, Hb = max(0, (H - 2) // 8), Wb
    likewise: per 8 x 8 block of the frame's interior and channel the sum of the squared 5-point Laplacian, and the block's luma
    band 0..7 -- 255 (not measured) when a byte of the block is 0 or 255 or a pixel of its 10 x 10 footprint is hole.  Every entry
    is written; no host read; exact integers, the same in every run.  Device tensors, or anything torch.as_tensor accepts (uploaded
    first); wrong dtypes, shapes that do not fit, non-contiguous inputs and tensors on different devices raise ValueError."""
    lib = _L.load()
    named = [("frames", frames, torch.uint8)]
    if hole is not None:
        named.append(("hole", hole, torch.uint8))
    up = _device_inputs(named, "frames")
    fr = up[0]
    L, H, W = _frames_shape(fr, "frames")
    if hole is not None and tuple(up[1].shape) != (L, H, W):
        raise ValueError("hole must be [%d,%d,%d] for frames %s, got %s" % (L, H, W, tuple(fr.shape), tuple(up[1].shape)))
    Hb, Wb = max(0, (H - 2) // 8), max(0, (W - 2) // 8)
    with torch.cuda.device(fr.device):
        energy = torch.empty((L, Hb, Wb, 3), dtype=torch.int32, device=fr.device)
        band = torch.empty((L, Hb, Wb), dtype=torch.uint8, device=fr.device)
        _L.check(lib.e2fgvi_grain_blocks(_ptr(fr), _ptr(up[1]) if hole is not None else None, L, H, W, _ptr(energy), _ptr(band),
                                         _stream()), "grain_blocks")
    return energy, band


def _grain_q8(strength_q8):
    return _int_arg("strength_q8", strength_q8, 0, GRAIN_STRENGTH_Q8_MAX)


def grain_lut_from_scale(scale, strength_q8=256):
    """The table grain_apply reads, from the strengths at the eight band centres (include/e2fgvi_hip.h, "lut"): scale integer
    [S,8,3] on the device, entries >= 0 -> int32 [S,256,3]: linear between the centres 16 + 32 k of the luma bands, flat outside
    them, times strength_q8 / 256 (an integer in [0, 1024]) rounded, at most GRAIN_SCALE_MAX.  Integer torch ops, no host read."""
    q8 = _grain_q8(strength_q8)
    if not (isinstance(scale, torch.Tensor) and scale.is_cuda) or scale.dim() != 3 or tuple(scale.shape[1:]) != (8, 3) \
            or scale.dtype not in (torch.int32, torch.int64):
        raise ValueError("scale must be a device tensor int32 / int64 [S,8,3], got %s"
                         % ((tuple(scale.shape), scale.dtype) if isinstance(scale, torch.Tensor) else type(scale).__name__,))
    return _grain_table(scale, q8)


def _grain_table(scale, q8):
    """grain_lut_from_scale after the checks"""
    sc = scale.to(torch.int64)
    u = torch.arange(256, device=sc.device, dtype=torch.int64) - 16
    k, f = (u >> 5).clamp(0, 6), (u & 31).view(1, 256, 1)
    mid = (sc[:, k] * (32 - f) + sc[:, k + 1] * f + 16) >> 5
    lut = torch.where((u < 0).view(1, 256, 1), sc[:, :1], torch.where((u >= 224).view(1, 256, 1), sc[:, 7:], mid))
    return ((lut * q8 + 128) >> 8).clamp(max=GRAIN_SCALE_MAX).to(torch.int32)


def grain_lut(energy, band, scene_of, n_scenes, strength_q8=256):
    """The grain levels of every scene from grain_blocks' sums, and the table grain_apply reads (include/e2fgvi_hip.h, "Levels"):
    energy int32 [L,Hb,Wb,3], band uint8 [L,Hb,Wb], scene_of int32 [L] (a frame whose entry is outside [0, n_scenes) is in no
    scene) -> (lut int32 [S,256,3], scale int32 [S,8,3]) on the device, S = n_scenes.  Per scene and channel the lower quartile --
    the element at index (n - 1) // 4 of the ascending energies -- of the measured blocks of every band that has
    GRAIN_MIN_BLOCKS of them, and of all the scene's measured blocks (the scene's level; fewer than GRAIN_MIN_BLOCKS: all zeros);
    a band without its blocks borrows from the nearest band that has them (a tie: the darker; none: the scene's level); clamp to
    [level >> 2, level << 2]; scale = isqrt(E * 196611 * 19 // 20480).
    Everything on the device with no host read: ONE sort of int64 keys (group << 27 | energy -- an energy is below 2^27 -- with
    the groups (scene, band, channel), then (scene, channel) for the scene's level, then one group for what is not measured),
    searchsorted for the ends of the groups, a gather at each group's quartile position, and float64 sqrt with an integer +-1
    correction for the isqrt (its argument stays below 2^53).  strength_q8: an integer in [0, 1024].  The checks of grain_blocks."""
    q8 = _grain_q8(strength_q8)
    S = _int_arg("n_scenes", n_scenes, 0, 1 << 20)
    en, bd, so = _device_inputs((("energy", energy, torch.int32), ("band", band, torch.uint8), ("scene_of", scene_of, torch.int32)),
                                "energy")
    if en.dim() != 4 or en.shape[3] != 3:
        raise ValueError("energy must be [L,Hb,Wb,3], got %s" % (tuple(en.shape),))
    L = en.shape[0]
    if tuple(bd.shape) != tuple(en.shape[:3]):
        raise ValueError("band must be %s for energy %s, got %s" % (list(en.shape[:3]), tuple(en.shape), tuple(bd.shape)))
    _scene_table(so, "scene_of", L)
    with torch.cuda.device(en.device):
        scale = _grain_levels(en, bd, so, S)
        return _grain_table(scale, q8), scale


def _grain_levels(en, bd, so, S):
    """grain_lut after the checks: the scale int32 [S,8,3]; integer torch ops on the tensors' device"""
    L, dev, i64 = en.shape[0], en.device, torch.int64
    if S == 0 or en.numel() == 0:                    # known from the shapes: nothing is measured
        return torch.zeros((S, 8, 3), dtype=torch.int32, device=dev)
    s = so.to(i64).view(L, 1, 1, 1)
    k = bd.to(i64).unsqueeze(-1)
    c = torch.arange(3, device=dev, dtype=i64).view(1, 1, 1, 3)
    ok = (k < 8) & (s >= 0) & (s < S)
    n_band, n_all = S * 24, S * 27                   # the first group of the scenes' levels; the group of the rest
    e = en.to(i64).clamp(0, (1 << 27) - 1)
    g_band = torch.where(ok, (s * 8 + k) * 3 + c, n_all)
    g_scene = torch.where(ok, n_band + s * 3 + c, n_all)
    keys = torch.cat([((g_band << 27) | e).reshape(-1), ((g_scene << 27) | e).reshape(-1)]).sort().values
    ends = torch.searchsorted(keys, torch.arange(n_all + 1, device=dev, dtype=i64) << 27)
    start, n = ends[:-1], ends[1:] - ends[:-1]
    at = (start + (n - 1).clamp(min=0) // 4).clamp(max=keys.numel() - 1)
    q = torch.where(n >= GRAIN_MIN_BLOCKS, keys[at] & ((1 << 27) - 1), torch.zeros_like(n))
    have = (n >= GRAIN_MIN_BLOCKS)
    E, has = q[:n_band].view(S, 8, 3), have[:n_band].view(S, 8, 3)
    G, scene_has = q[n_band:].view(S, 1, 3), have[n_band:].view(S, 1, 3)
    # the band to read: the nearest that has its blocks, the darker of two equally near (cost 2 |j - k| + (j > k))
    j = torch.arange(8, device=dev, dtype=i64)
    cost = 2 * (j.view(1, 8) - j.view(8, 1)).abs() + (j.view(1, 8) > j.view(8, 1)).to(i64)               # [k, j]
    cost = torch.where(has[:, :, 0].reshape(S, 1, 8), cost.view(1, 8, 8), torch.full_like(cost, 1000).view(1, 8, 8))
    pick = cost.argmin(dim=2)                                                                          # [S, k]
    E = torch.where(has.any(dim=1, keepdim=True), torch.gather(E, 1, pick.view(S, 8, 1).expand(S, 8, 3)), G.expand(S, 8, 3))
    E = torch.minimum(torch.maximum(E, G >> 2), G << 2)
    E = torch.where(scene_has, E, torch.zeros_like(E))
    v = E * (196611 * 19) // (1280 * 16)
    r = v.to(torch.float64).sqrt().floor().to(i64)
    r = torch.where(r * r > v, r - 1, r)
    r = torch.where((r + 1) * (r + 1) <= v, r + 1, r)
    return r.to(torch.int32)


def grain_apply(filled, where, lut, scene_of, seed, out=None):
    """Synthetic grain over the pixels of ``where``, one launch over all frames (csrc/grain.hip grain_apply_kernel;
    include/e2fgvi_hip.h has the definition): filled uint8 [L,H,W,3]; where uint8 [L,H,W] (any non-zero byte is set); lut int32
    [S,256,3] as grain_lut made it; scene_of int32 [L]; seed an integer in [0, 2^32) -> device uint8 [L,H,W,3]: at a pixel of
    ``where`` in a frame with 0 <= scene_of[t] < S every channel gets the counter-based noise n (zero mean, variance 21845) of
    (seed, t, x, y, c) times lut[scene_of[t], luma of the filled pixel, c] / 65536, rounded, and is clamped to a byte; every other
    byte is filled's.  ``out``: a device uint8 [L,H,W,3] to write, which may be ``filled`` itself (in place); without it a new
    buffer.  The checks of grain_blocks; no host read; no atomics: the same arguments give the same bytes in every run."""
    lib = _L.load()
    seed = _int_arg("seed", seed, 0, (1 << 32) - 1)
    named = [("filled", filled, torch.uint8), ("where", where, torch.uint8), ("lut", lut, torch.int32), ("scene_of", scene_of, torch.int32)]
    if out is not None:
        named.insert(0, ("out", out, torch.uint8))
    up = _device_inputs(named, "out" if out is not None else "filled", written=("out",))
    fl, wh, lu, so = up[-4:]
    L, H, W = _frames_shape(fl, "filled")
    if tuple(wh.shape) != (L, H, W):
        raise ValueError("where must be [%d,%d,%d] for filled %s, got %s" % (L, H, W, tuple(fl.shape), tuple(wh.shape)))
    if lu.dim() != 3 or tuple(lu.shape[1:]) != (256, 3):
        raise ValueError("lut must be int32 [S,256,3], got %s" % (tuple(lu.shape),))
    _scene_table(so, "scene_of", L)
    if out is not None and tuple(up[0].shape) != (L, H, W, 3):
        raise ValueError("out must be [%d,%d,%d,3], got %s" % (L, H, W, tuple(up[0].shape)))
    with torch.cuda.device(fl.device):
        ou = up[0] if out is not None else torch.empty_like(fl)
        _L.check(lib.e2fgvi_grain_apply(_ptr(fl), _ptr(wh), _ptr(lu) if lu.numel() else None, _ptr(so), lu.shape[0], seed, L, H, W,
                                        _ptr(ou), _stream()), "grain_apply")
    return ou


LINE_ROWS_MIN, LINE_ROWS_MAX = 4, 64       # csrc/line_scratch.hip: parameters outside these ranges are E2FGVI_EINVAL
LINE_TAU_MAX = 254
LINE_GAP_MAX = 4
LINE_SIDE_MAX = 8
LINE_DRIFT_MAX = 2
LINE_SPAN_MAX = 4
LINE_RADIUS_MAX = 16                       # csrc/line_scratch.hip LN_RMAX: the largest paint radius line_paint keeps in LDS


def line_sums(frames, rows):
    """The band sums of the line-scratch detector, one launch over all frames (csrc/line_scratch.hip line_sums_kernel;
    include/e2fgvi_hip.h has the definition; video.detect_line_scratches is the caller): frames uint8 [L,H,W,3] -> device int32
    [L, H // rows, W]: the scene detector's integer luma summed over each band of ``rows`` rows; the H mod rows rows at the bottom
    are in no band.  rows in [LINE_ROWS_MIN, LINE_ROWS_MAX]: an integer, no bool.  Device tensors, or anything torch.as_tensor
    accepts (uploaded first); a wrong dtype or shape and a non-contiguous input raise ValueError.  There is no CPU path and no
    host read; the same input gives the same bits in every run."""
    lib = _L.load()
    rows = _int_arg("rows", rows, LINE_ROWS_MIN, LINE_ROWS_MAX)
    fr, = _device_inputs([("frames", frames, torch.uint8)], "frames")
    L, H, W = _frames_shape(fr, "frames")
    with torch.cuda.device(fr.device):
        S = torch.empty((L, H // rows, W), dtype=torch.int32, device=fr.device)
        _L.check(lib.e2fgvi_line_sums(_ptr(fr), L, H, W, rows, _ptr(S), _stream()), "line_sums")
    return S


def line_columns(S, rows, tau, gap, side, drift, coverage):
    """The cross-section test and the height count of the line-scratch detector, one launch (csrc/line_scratch.hip
    line_columns_kernel; include/e2fgvi_hip.h has the definition): S int32 [L,nb,W] as line_sums made it with the same ``rows`` ->
    (cand, cnt, col, b0, b1) on the device.  cand uint8 [L,nb,W]: bit 0 set where S lies more than tau rows above the largest S
    of the ``side`` columns beyond a gap of ``gap`` columns on either side, bit 1 where it lies more than that below the smallest;
    a column with a side column outside the frame has neither.  Per polarity p (0 bright, 1 dark) and column, over the bands in
    which a candidate lies within ``drift`` columns: cnt int32 [L,2,W] their number, col uint8 [L,2,W] = cnt 100 >= coverage nb,
    b0 and b1 int32 [L,2,W] the first and the last of them (nb and -1 without one).  tau in [0, LINE_TAU_MAX], gap in [0,
    LINE_GAP_MAX], side in [1, LINE_SIDE_MAX], drift in [0, LINE_DRIFT_MAX], coverage in [1, 100]: integers, no bools.  The checks
    of line_sums; no host read; exact integers, the same in every run."""
    lib = _L.load()
    rows = _int_arg("rows", rows, LINE_ROWS_MIN, LINE_ROWS_MAX)
    tau = _int_arg("tau", tau, 0, LINE_TAU_MAX)
    gap = _int_arg("gap", gap, 0, LINE_GAP_MAX)
    side = _int_arg("side", side, 1, LINE_SIDE_MAX)
    drift = _int_arg("drift", drift, 0, LINE_DRIFT_MAX)
    coverage = _int_arg("coverage", coverage, 1, 100)
    sm, = _device_inputs([("S", S, torch.int32)], "S")
    if sm.dim() != 3:
        raise ValueError("S must be int32 [L,nb,W], got %s" % (tuple(sm.shape),))
    L, nb, W = sm.shape
    dev = sm.device
    with torch.cuda.device(dev):
        cand = torch.empty((L, nb, W), dtype=torch.uint8, device=dev)
        # with a band the launch writes every entry; without one there is no launch and zeros (b1: -1) are the answer
        cnt, b0 = (_alloc(nb, (L, 2, W), torch.int32, dev) for _ in range(2))
        b1 = torch.empty_like(cnt) if nb else torch.full_like(cnt, -1)
        col = _alloc(nb, (L, 2, W), torch.uint8, dev)
        # the entry takes the frame's height: nb rows gives nb bands and no remainder
        _L.check(lib.e2fgvi_line_columns(_ptr(sm), L, nb * rows, W, rows, tau, gap, side, drift, coverage, _ptr(cand), _ptr(cnt),
                                         _ptr(col), _ptr(b0), _ptr(b1), _stream()), "line_columns")
    return cand, cnt, col, b0, b1


def line_paint(col, b0, b1, scene, H, rows, drift, span, persist, radius, out=None):
    """The persistence test and the painting of the line-scratch detector (csrc/line_scratch.hip line_keep_kernel and
    line_paint_kernel, two launches; include/e2fgvi_hip.h has the definition): col uint8 [L,2,W], b0 and b1 int32 [L,2,W] as
    line_columns made them; scene int32 [L], equal entries = one scene; H the frames' height -> (keep, counts, masks) on the
    device.  keep uint8 [L,2,W]: a column of ``col`` stays when, of the frames within ``span`` of its own in its scene, at least
    min(persist, their number) have a column of ``col`` within ``drift`` columns; counts int32 [L] the kept columns per frame,
    both polarities added; masks uint8 [L,H,W]: 255 in the rows of the bands b0 .. b1 of a kept column (the H mod rows rows at
    the bottom go with the last band) and the columns within ``radius`` of it, 0 elsewhere.  ``out``: a device uint8 [L,H,W] to
    write the masks into; every byte is written.  span in [0, LINE_SPAN_MAX], persist in [1, 2 span + 1], radius in [0,
    LINE_RADIUS_MAX], drift and rows as above: integers, no bools.  The checks of line_sums; no host read; exact integers."""
    lib = _L.load()
    rows = _int_arg("rows", rows, LINE_ROWS_MIN, LINE_ROWS_MAX)
    drift = _int_arg("drift", drift, 0, LINE_DRIFT_MAX)
    span = _int_arg("span", span, 0, LINE_SPAN_MAX)
    persist = _int_arg("persist", persist, 1, 2 * span + 1)
    radius = _int_arg("radius", radius, 0, LINE_RADIUS_MAX)
    H = _int_arg("H", H, 0, (1 << 31) - 1)
    named = [("col", col, torch.uint8), ("b0", b0, torch.int32), ("b1", b1, torch.int32), ("scene", scene, torch.int32)]
    if out is not None:
        named.append(("out", out, torch.uint8))
    up = _device_inputs(named, "col", written=("out",))
    cl, f0, f1, sc = up[:4]
    if cl.dim() != 3 or cl.shape[1] != 2:
        raise ValueError("col must be uint8 [L,2,W], got %s" % (tuple(cl.shape),))
    L, _, W = cl.shape
    for t, nm in ((f0, "b0"), (f1, "b1")):
        if tuple(t.shape) != (L, 2, W):
            raise ValueError("%s must be int32 [%d,2,%d], got %s" % (nm, L, W, tuple(t.shape)))
    _scene_table(sc, "scene", L)
    if out is not None and tuple(up[4].shape) != (L, H, W):
        raise ValueError("out must be [%d,%d,%d], got %s" % (L, H, W, tuple(up[4].shape)))
    dev = cl.device
    with torch.cuda.device(dev):
        work = L > 0 and W > 0 and H // rows > 0
        masks = _alloc(work, (L, H, W), torch.uint8, dev, up[4] if out is not None else None)
        # with work the entry clears counts and writes every entry of keep
        keep = _alloc(work, (L, 2, W), torch.uint8, dev)
        counts = _alloc(work, L, torch.int32, dev)
        _L.check(lib.e2fgvi_line_paint(_ptr(cl), _ptr(f0), _ptr(f1), _ptr(sc), L, H, W, rows, drift, span, persist, radius, _ptr(keep),
                                       _ptr(counts), _ptr(masks), _stream()), "line_paint")
    return keep, counts, masks


FLICKER_SPAN_MAX = 8                       # csrc/flicker.hip: parameters outside these ranges are E2FGVI_EINVAL
FLICKER_SHIFT_MAX = 64
FLICKER_NODES = 32                         # quantile nodes per frame (FL_K)
FLICKER_PIXELS_MAX = 1 << 26               # H W of a frame: a histogram bin is an int32 and the curve's products stay in 64 bits


def _flicker_frames(fr, name="frames"):
    L, H, W = _frames_shape(fr, name)
    if H * W > FLICKER_PIXELS_MAX:
        raise ValueError("%s must have H W <= 2^26, got %d x %d" % (name, H, W))
    return L, H, W


def flicker_hist(frames, out=None):
    """The luma histograms of the deflicker, one launch over all frames (csrc/flicker.hip flicker_hist_kernel; include/e2fgvi_hip.h
    has the definition; video.deflicker is the caller): frames uint8 [L,H,W,3] -> device int32 [L,256], the number of pixels of
    each frame per level of the scene detector's integer luma.  ``out``: a device int32 [L,256] to write into; every word is
    written (the entry clears the rows first).  Device tensors, or anything torch.as_tensor accepts (uploaded first); a wrong
    dtype or shape, more than 2^26 pixels a frame and a non-contiguous input raise ValueError.  There is no CPU path and no host
    read; integer atomics: the same input gives the same bits in every run."""
    lib = _L.load()
    named = [("frames", frames, torch.uint8)] + ([("out", out, torch.int32)] if out is not None else [])
    up = _device_inputs(named, "frames", written=("out",))
    fr = up[0]
    L, H, W = _flicker_frames(fr)
    if out is not None and tuple(up[1].shape) != (L, 256):
        raise ValueError("out must be int32 [%d,256], got %s" % (L, tuple(up[1].shape)))
    with torch.cuda.device(fr.device):
        hist = _alloc(L > 0 and H * W > 0, (L, 256), torch.int32, fr.device, up[1] if out is not None else None)
        _L.check(lib.e2fgvi_flicker_hist(_ptr(fr), _ptr(hist), L, H, W, _stream()), "flicker_hist")
    return hist


def flicker_curves(hist, scene, N, span, max_shift):
    """The nodes and the tone curves of the deflicker, one launch (csrc/flicker.hip flicker_curves_kernel; include/e2fgvi_hip.h has
    the definition): hist int32 [L,256] as flicker_hist made it, every row summing to ``N`` = H W (the contract; it is not
    checked, which would be a host read); scene int32 [L], equal entries = one scene -> (Q, d) on the device.  Q int32
    [L,FLICKER_NODES]: the 32 luma quantiles (2k + 1) / 64 of each frame in 1/16 levels.  d int16 [L,256]: per frame and luma
    level the shift that moves the frame's nodes onto their rounded mean over the frames within ``span`` of it in its scene,
    clamped to +-``max_shift`` levels at the nodes and interpolated between them.  N in [0, 2^26], span in [0,
    FLICKER_SPAN_MAX], max_shift in [1, FLICKER_SHIFT_MAX]: integers, no bools.  The checks of flicker_hist; no host read; exact
    integers, the same in every run."""
    lib = _L.load()
    N = _int_arg("N", N, 0, FLICKER_PIXELS_MAX)
    span = _int_arg("span", span, 0, FLICKER_SPAN_MAX)
    max_shift = _int_arg("max_shift", max_shift, 1, FLICKER_SHIFT_MAX)
    hs, sc = _device_inputs([("hist", hist, torch.int32), ("scene", scene, torch.int32)], "hist")
    if hs.dim() != 2 or hs.shape[1] != 256:
        raise ValueError("hist must be int32 [L,256], got %s" % (tuple(hs.shape),))
    L = int(hs.shape[0])
    _scene_table(sc, "scene", L)
    with torch.cuda.device(hs.device):
        work = L > 0 and N > 0                           # with work the launch writes every entry
        Q = _alloc(work, (L, FLICKER_NODES), torch.int32, hs.device)
        d = _alloc(work, (L, 256), torch.int16, hs.device)
        _L.check(lib.e2fgvi_flicker_curves(_ptr(hs), _ptr(sc), _ptr(Q), _ptr(d), L, N, span, max_shift, _stream()), "flicker_curves")
    return Q, d


def flicker_apply(frames, d, out=None):
    """The tone curves applied, one launch (csrc/flicker.hip flicker_apply_kernel; include/e2fgvi_hip.h has the definition): frames
    uint8 [L,H,W,3], d int16 [L,256] as flicker_curves made it -> device uint8 [L,H,W,3]: every pixel moved by the shift of its
    luma, the same for its three bytes, each clipped to [0, 255].  ``out``: a device uint8 [L,H,W,3] to write into -- ``frames``
    itself for in place, otherwise one that does not overlap it (the entry refuses any other overlap); every byte is written once.
    The checks of flicker_hist; no host read; exact integers."""
    lib = _L.load()
    named = [("frames", frames, torch.uint8), ("d", d, torch.int16)] + ([("out", out, torch.uint8)] if out is not None else [])
    up = _device_inputs(named, "frames", written=("out",))
    fr, dd = up[:2]
    L, H, W = _flicker_frames(fr)
    if tuple(dd.shape) != (L, 256):
        raise ValueError("d must be int16 [%d,256], got %s" % (L, tuple(dd.shape)))
    if out is not None and tuple(up[2].shape) != tuple(fr.shape):
        raise ValueError("out must be %s, got %s" % (list(fr.shape), tuple(up[2].shape)))
    with torch.cuda.device(fr.device):
        ou = up[2] if out is not None else torch.empty_like(fr)
        _L.check(lib.e2fgvi_flicker_apply(_ptr(fr), _ptr(dd), _ptr(ou), L, H, W, _stream()), "flicker_apply")
    return ou


FLICKER_GRID_MAX = 8                       # csrc/flicker_local.hip: cells per axis (FLL_G_MAX)


def _flicker_grid(grid, H=None, W=None):
    """``grid`` as (gy, gx): a tuple or list of two integers in [1, FLICKER_GRID_MAX], no bools, and -- where there are pixels --
    no more cells than pixels along either axis; ValueError that names it otherwise"""
    if not isinstance(grid, (tuple, list)) or len(grid) != 2:
        raise ValueError("grid must be a tuple of two integers in [1, %d], got %r" % (FLICKER_GRID_MAX, grid))
    gy, gx = (_int_arg("grid", g, 1, FLICKER_GRID_MAX) for g in grid)
    if H and W and (H < gy or W < gx):
        raise ValueError("grid %d x %d has more cells than frames of %d x %d have rows or columns" % (gy, gx, H, W))
    return gy, gx


def _flicker_cells(t, name, what, L, last):
    """(gy, gx) of ``t`` as [L,gy,gx,last]; ValueError that names it otherwise"""
    if (t.dim() != 4 or t.shape[3] != last or (L is not None and t.shape[0] != L)
            or not all(1 <= g <= FLICKER_GRID_MAX for g in t.shape[1:3])):
        raise ValueError("%s must be %s [%s,gy,gx,%d] with gy and gx in [1, %d], got %s"
                         % (name, what, "L" if L is None else L, last, FLICKER_GRID_MAX, tuple(t.shape)))
    return int(t.shape[1]), int(t.shape[2])


def flicker_local_hist(frames, grid, out=None):
    """The luma histograms of the local deflicker, one launch over all frames (csrc/flicker_local.hip flicker_local_hist_kernel;
    include/e2fgvi_hip.h has the definition; video.deflicker_local is the caller): frames uint8 [L,H,W,3], grid = (gy, gx) ->
    device int32 [L,gy,gx,256], the number of pixels per luma level of each cell -- rows [(i H) // gy, ((i + 1) H) // gy) x columns
    [(j W) // gx, ((j + 1) W) // gx) -- of each frame; summed over the cells they are flicker_hist's.  ``out``: a device int32
    [L,gy,gx,256] to write into; every word is written (the entry clears them first).  The checks of flicker_hist, and grid: two
    integers in [1, FLICKER_GRID_MAX] with H >= gy and W >= gx.  No CPU path, no host read; integer atomics: the same bits in
    every run."""
    lib = _L.load()
    named = [("frames", frames, torch.uint8)] + ([("out", out, torch.int32)] if out is not None else [])
    up = _device_inputs(named, "frames", written=("out",))
    fr = up[0]
    L, H, W = _flicker_frames(fr)
    gy, gx = _flicker_grid(grid, H, W)
    if out is not None and tuple(up[1].shape) != (L, gy, gx, 256):
        raise ValueError("out must be int32 [%d,%d,%d,256], got %s" % (L, gy, gx, tuple(up[1].shape)))
    with torch.cuda.device(fr.device):
        hist = _alloc(L > 0 and H * W > 0, (L, gy, gx, 256), torch.int32, fr.device, up[1] if out is not None else None)
        _L.check(lib.e2fgvi_flicker_local_hist(_ptr(fr), _ptr(hist), L, H, W, gy, gx, _stream()), "flicker_local_hist")
    return hist


def flicker_local_curves(hist, scene, H, W, span, max_shift):
    """The nodes and the tone curves of the local deflicker, one launch (csrc/flicker_local.hip flicker_local_curves_kernel;
    include/e2fgvi_hip.h has the definition): hist int32 [L,gy,gx,256] as flicker_local_hist made it of frames of ``H`` x ``W``,
    every row summing to its cell's pixels (the contract; it is not checked, which would be a host read); scene int32 [L], equal
    entries = one scene -> (Q, d16) on the device.  Q int32 [L,gy,gx,FLICKER_NODES]: the 32 luma quantiles of each cell in 1/16
    levels.  d16 int16 [L,gy,gx,256]: per cell and luma level flicker_curves' shift of that cell's rows, in 1/16 levels (not rounded
    to whole ones: flicker_local_apply blends first).  H W in [0, 2^26] with H >= gy and W >= gx where there are pixels; span and
    max_shift as flicker_curves takes them.  No host read; exact integers, the same in every run."""
    lib = _L.load()
    H, W = _int_arg("H", H, 0, FLICKER_PIXELS_MAX), _int_arg("W", W, 0, FLICKER_PIXELS_MAX)
    if H * W > FLICKER_PIXELS_MAX:
        raise ValueError("H W must be <= 2^26, got %d x %d" % (H, W))
    span = _int_arg("span", span, 0, FLICKER_SPAN_MAX)
    max_shift = _int_arg("max_shift", max_shift, 1, FLICKER_SHIFT_MAX)
    hs, sc = _device_inputs([("hist", hist, torch.int32), ("scene", scene, torch.int32)], "hist")
    gy, gx = _flicker_cells(hs, "hist", "int32", None, 256)
    _flicker_grid((gy, gx), H, W)
    L = int(hs.shape[0])
    _scene_table(sc, "scene", L)
    with torch.cuda.device(hs.device):
        work = L > 0 and H * W > 0                       # with work the launch writes every entry
        Q = _alloc(work, (L, gy, gx, FLICKER_NODES), torch.int32, hs.device)
        d16 = _alloc(work, (L, gy, gx, 256), torch.int16, hs.device)
        _L.check(lib.e2fgvi_flicker_local_curves(_ptr(hs), _ptr(sc), _ptr(Q), _ptr(d16), L, H, W, gy, gx, span, max_shift, _stream()),
                 "flicker_local_curves")
    return Q, d16


def flicker_local_apply(frames, d16, out=None):
    """The cells' tone curves blended and applied, one launch (csrc/flicker_local.hip flicker_local_apply_kernel;
    include/e2fgvi_hip.h has the definition): frames uint8 [L,H,W,3], d16 int16 [L,gy,gx,256] as flicker_local_curves made it ->
    device uint8 [L,H,W,3]: every pixel moved by the shifts of its luma in the four cells around it, blended by its position between
    their centres and rounded to whole levels once, the same for its three bytes, each clipped to [0, 255].  ``out`` as
    flicker_apply takes it (``frames`` itself for in place); every byte is written once.  The checks of flicker_local_hist; no host
    read; exact integers."""
    lib = _L.load()
    named = [("frames", frames, torch.uint8), ("d16", d16, torch.int16)] + ([("out", out, torch.uint8)] if out is not None else [])
    up = _device_inputs(named, "frames", written=("out",))
    fr, dd = up[:2]
    L, H, W = _flicker_frames(fr)
    gy, gx = _flicker_cells(dd, "d16", "int16", L, 256)
    _flicker_grid((gy, gx), H, W)
    if out is not None and tuple(up[2].shape) != tuple(fr.shape):
        raise ValueError("out must be %s, got %s" % (list(fr.shape), tuple(up[2].shape)))
    with torch.cuda.device(fr.device):
        ou = up[2] if out is not None else torch.empty_like(fr)
        _L.check(lib.e2fgvi_flicker_local_apply(_ptr(fr), _ptr(dd), _ptr(ou), L, H, W, gy, gx, _stream()), "flicker_local_apply")
    return ou


COLOR_NODES = FLICKER_NODES + 2            # csrc/color.hip: 32 quantiles, the black and the white point (COL_Q)
COLOR_CLIP_MAX = 250                       # per mille; parameters outside these ranges are E2FGVI_EINVAL
COLOR_GAIN_MIN, COLOR_GAIN_MAX = 256, 4096
COLOR_KEEP, COLOR_LEVELS, COLOR_MATCH = 0, 1, 2


def color_hist(frames, out=None):
    """The channel histograms of the colour restoration, one launch over all frames (csrc/color.hip color_hist_kernel;
    include/e2fgvi_hip.h has the definition; video.restore_color is the caller): frames uint8 [L,H,W,3] -> device int32 [L,3,256],
    the number of pixels of each frame per channel and byte value.  ``out``: a device int32 [L,3,256] to write into; every word is
    written (the entry clears them first).  Device tensors, or anything torch.as_tensor accepts (uploaded first); a wrong dtype or
    shape, more than 2^26 pixels a frame and a non-contiguous input raise ValueError.  There is no CPU path and no host read;
    integer atomics: the same input gives the same bits in every run."""
    lib = _L.load()
    named = [("frames", frames, torch.uint8)] + ([("out", out, torch.int32)] if out is not None else [])
    up = _device_inputs(named, "frames", written=("out",))
    fr = up[0]
    L, H, W = _flicker_frames(fr)
    if out is not None and tuple(up[1].shape) != (L, 3, 256):
        raise ValueError("out must be int32 [%d,3,256], got %s" % (L, tuple(up[1].shape)))
    with torch.cuda.device(fr.device):
        hist = _alloc(L > 0 and H * W > 0, (L, 3, 256), torch.int32, fr.device, up[1] if out is not None else None)
        _L.check(lib.e2fgvi_color_hist(_ptr(fr), _ptr(hist), L, H, W, _stream()), "color_hist")
    return hist


def color_nodes(hist, starts, ids, clip=(5, 5)):
    """The quantile nodes of groups of frames, one launch (csrc/color.hip color_nodes_kernel; include/e2fgvi_hip.h has the
    definition): hist int32 [L,3,256] as color_hist made it; starts int32 [G+1] and ids int32 [M], the groups in CSR form -- group
    g pools the histograms of the frames ids[starts[g] : starts[g+1]] -> device int32 [G,3,COLOR_NODES]: per group and channel the
    32 quantiles (2k + 1) / 64 of the pooled histogram, then its black point, below which ``clip[0]`` per mille of the pixels
    lie, and its white point, above which ``clip[1]`` per mille lie; all in 1/16 levels.  An id outside [0, L) is skipped, starts
    are read clamped to [0, M], and a group without a pixel gets zeros (range-checked in the kernel, not here: no host read).
    clip: two integers in [0, COLOR_CLIP_MAX], no bools.  The checks of color_hist; exact integers, the same in every run."""
    lib = _L.load()
    if not isinstance(clip, (tuple, list)) or len(clip) != 2:
        raise ValueError("clip must be a tuple of two integers in [0, %d], got %r" % (COLOR_CLIP_MAX, clip))
    lo, hi = (_int_arg("clip", v, 0, COLOR_CLIP_MAX) for v in clip)
    hs, st, ii = _device_inputs([("hist", hist, torch.int32), ("starts", starts, torch.int32), ("ids", ids, torch.int32)], "hist")
    if hs.dim() != 3 or tuple(hs.shape[1:]) != (3, 256):
        raise ValueError("hist must be int32 [L,3,256], got %s" % (tuple(hs.shape),))
    if st.dim() != 1 or st.numel() < 1:
        raise ValueError("starts must be int32 [G+1], got %s" % (tuple(st.shape),))
    if ii.dim() != 1:
        raise ValueError("ids must be int32 [M], got %s" % (tuple(ii.shape),))
    L, G, M = int(hs.shape[0]), int(st.numel()) - 1, int(ii.numel())
    with torch.cuda.device(hs.device):
        Q = _alloc(G > 0, (G, 3, COLOR_NODES), torch.int32, hs.device)        # with a group the launch writes every entry
        _L.check(lib.e2fgvi_color_nodes(_ptr(hs), _ptr(st), _ptr(ii), _ptr(Q), L, G, M, lo, hi, _stream()), "color_nodes")
    return Q


def _color_target(target):
    """``target`` as (lo_t, hi_t): None is the automatic one (-1, -1), else two integers 0 <= lo_t < hi_t <= 255, no bools"""
    if target is None:
        return -1, -1
    if not isinstance(target, (tuple, list)) or len(target) != 2:
        raise ValueError("target must be None or a tuple of two integers 0 <= lo < hi <= 255, got %r" % (target,))
    lo_t, hi_t = (_int_arg("target", v, 0, 255) for v in target)
    if lo_t >= hi_t:
        raise ValueError("target must be None or a tuple of two integers 0 <= lo < hi <= 255, got %r" % (target,))
    return lo_t, hi_t


def color_lut(Q, mode, T=None, target=None, min_range=32, max_gain=768, strength=256):
    """The byte tables of groups of frames, one launch (csrc/color.hip color_lut_kernel; include/e2fgvi_hip.h has the
    definition): Q int32 [G,3,COLOR_NODES] as color_nodes made it, mode int32 [G] -> device uint8 [G,3,256], per group and channel
    the byte every byte value becomes.  mode COLOR_KEEP (and any other value): the identity.  COLOR_LEVELS: the channel's black
    and white point are brought onto ``target`` = (lo, hi) in levels -- None: onto the smallest black and the largest white point
    of the group's usable channels --, a straight line about the centre of the range whose gain is cut at ``max_gain`` / 256; a
    channel whose range is narrower than ``min_range`` levels is not usable and keeps its bytes.  COLOR_MATCH: the channel's 32
    quantiles are moved onto those of ``T`` (int32 [G,3,COLOR_NODES], another color_nodes result; None: Q itself), straight lines
    between them and slope 1 beyond the first and the last.  ``strength`` / 256 of the way from the identity is gone.  min_range in
    [1, 255], max_gain in [COLOR_GAIN_MIN, COLOR_GAIN_MAX], strength in [0, 256]: integers, no bools.  The checks of color_hist;
    no host read; exact integers, the same in every run."""
    lib = _L.load()
    lo_t, hi_t = _color_target(target)
    min_range = _int_arg("min_range", min_range, 1, 255)
    max_gain = _int_arg("max_gain", max_gain, COLOR_GAIN_MIN, COLOR_GAIN_MAX)
    strength = _int_arg("strength", strength, 0, 256)
    named = [("Q", Q, torch.int32), ("mode", mode, torch.int32)] + ([("T", T, torch.int32)] if T is not None else [])
    up = _device_inputs(named, "Q")
    qq, md = up[:2]
    if qq.dim() != 3 or tuple(qq.shape[1:]) != (3, COLOR_NODES):
        raise ValueError("Q must be int32 [G,3,%d], got %s" % (COLOR_NODES, tuple(qq.shape)))
    G = int(qq.shape[0])
    if tuple(md.shape) != (G,):
        raise ValueError("mode must be int32 [%d], got %s" % (G, tuple(md.shape)))
    if T is not None and tuple(up[2].shape) != tuple(qq.shape):
        raise ValueError("T must be int32 %s, got %s" % (list(qq.shape), tuple(up[2].shape)))
    tt = up[2] if T is not None else qq
    with torch.cuda.device(qq.device):
        lut = torch.empty((G, 3, 256), dtype=torch.uint8, device=qq.device)  # with a group the launch writes every entry
        _L.check(lib.e2fgvi_color_lut(_ptr(qq), _ptr(tt), _ptr(md), _ptr(lut), G, lo_t, hi_t, min_range, max_gain, strength, _stream()),
                 "color_lut")
    return lut


def color_apply(frames, lut, group, out=None):
    """The byte tables applied, one launch (csrc/color.hip color_apply_kernel; include/e2fgvi_hip.h has the definition): frames
    uint8 [L,H,W,3], lut uint8 [G,3,256] as color_lut made it (or the caller's own), group int32 [L] -> device uint8 [L,H,W,3]:
    byte c of every pixel of frame t looked up in lut[group[t]][c]; a frame whose group is outside [0, G) is copied (checked in the
    kernel, not here: no host read).  ``out``: a device uint8 [L,H,W,3] to write into -- ``frames`` itself for in place, otherwise
    one that does not overlap it (the entry refuses any other overlap); every byte is written once.  The checks of color_hist; no
    host read; exact integers."""
    lib = _L.load()
    named = [("frames", frames, torch.uint8), ("lut", lut, torch.uint8), ("group", group, torch.int32)]
    named += [("out", out, torch.uint8)] if out is not None else []
    up = _device_inputs(named, "frames", written=("out",))
    fr, lt, gr = up[:3]
    L, H, W = _flicker_frames(fr)
    if lt.dim() != 3 or tuple(lt.shape[1:]) != (3, 256):
        raise ValueError("lut must be uint8 [G,3,256], got %s" % (tuple(lt.shape),))
    if tuple(gr.shape) != (L,):
        raise ValueError("group must be int32 [%d], got %s" % (L, tuple(gr.shape)))
    if out is not None and tuple(up[3].shape) != tuple(fr.shape):
        raise ValueError("out must be %s, got %s" % (list(fr.shape), tuple(up[3].shape)))
    with torch.cuda.device(fr.device):
        ou = up[3] if out is not None else torch.empty_like(fr)
        _L.check(lib.e2fgvi_color_apply(_ptr(fr), _ptr(lt), _ptr(gr), _ptr(ou), L, H, W, int(lt.shape[0]), _stream()), "color_apply")
    return ou


WEAVE_BANDS = 8                            # csrc/weave.hip: bands per axis (WV_NB)
WEAVE_RADIUS_MAX = 32                      # parameters outside these ranges are E2FGVI_EINVAL
WEAVE_SPAN_MAX = 16
WEAVE_SHIFT_MAX = 64
WEAVE_TEX_MAX = 65535
WEAVE_SIDE_MAX = 4096                      # H and W of the profiles and the match: a profile lives in LDS


def _weave_sides(H, W, name="frames"):
    if H > WEAVE_SIDE_MAX or W > WEAVE_SIDE_MAX:
        raise ValueError("%s must have H and W <= %d, got %d x %d" % (name, WEAVE_SIDE_MAX, H, W))


def weave_profiles(frames):
    """The banded luma profiles of the weave stabiliser, one pass over the frames (csrc/weave.hip weave_profiles_kernel;
    include/e2fgvi_hip.h has the definition; video.stabilize is the caller): frames uint8 [L,H,W,3] -> (col, row) on the device,
    col int32 [L,WEAVE_BANDS,W] the sum of the integer luma over the rows of each band per column, row int32 [L,WEAVE_BANDS,H]
    the sum over the columns of each band per row.  Device tensors, or anything torch.as_tensor accepts (uploaded first); a wrong
    dtype or shape, a side above WEAVE_SIDE_MAX and a non-contiguous input raise ValueError.  There is no CPU path and no host
    read; integer atomics: the same input gives the same bits in every run."""
    lib = _L.load()
    fr, = _device_inputs([("frames", frames, torch.uint8)], "frames")
    L, H, W = _frames_shape(fr, "frames")
    _weave_sides(H, W)
    with torch.cuda.device(fr.device):
        work = L > 0 and H > 0 and W > 0                 # with work the entry writes every word
        col = _alloc(work, (L, WEAVE_BANDS, W), torch.int32, fr.device)
        row = _alloc(work, (L, WEAVE_BANDS, H), torch.int32, fr.device)
        _L.check(lib.e2fgvi_weave_profiles(_ptr(fr), _ptr(col), _ptr(row), L, H, W, _stream()), "weave_profiles")
    return col, row


def weave_match(col, row, scene, radius, tex):
    """The motion of every pair of adjacent frames from their profiles, one launch (csrc/weave.hip weave_match_kernel;
    include/e2fgvi_hip.h has the definition): col int32 [L,8,W] and row int32 [L,8,H] as weave_profiles made them, scene int32
    [L], equal entries = one scene -> device int32 [L,4] = (mx, my, nx, ny): the motion of frame t against frame t - 1 in 1/16 px
    per axis -- the lower median over the valid bands, 0 when fewer than half are valid -- and the number of valid bands per axis.
    radius in [1, WEAVE_RADIUS_MAX], tex in [0, WEAVE_TEX_MAX]: integers, no bools.  No host read; exact integers."""
    lib = _L.load()
    radius = _int_arg("radius", radius, 1, WEAVE_RADIUS_MAX)
    tex = _int_arg("tex", tex, 0, WEAVE_TEX_MAX)
    cl, rw, sc = _device_inputs([("col", col, torch.int32), ("row", row, torch.int32), ("scene", scene, torch.int32)], "col")
    if cl.dim() != 3 or cl.shape[1] != WEAVE_BANDS:
        raise ValueError("col must be int32 [L,%d,W], got %s" % (WEAVE_BANDS, tuple(cl.shape)))
    L, _, W = (int(v) for v in cl.shape)
    if rw.dim() != 3 or tuple(rw.shape[:2]) != (L, WEAVE_BANDS):
        raise ValueError("row must be int32 [%d,%d,H], got %s" % (L, WEAVE_BANDS, tuple(rw.shape)))
    H = int(rw.shape[2])
    _weave_sides(H, W, "col and row")
    _scene_table(sc, "scene", L)
    with torch.cuda.device(cl.device):
        motion = _alloc(L > 0 and H > 0 and W > 0, (L, 4), torch.int32, cl.device)
        _L.check(lib.e2fgvi_weave_match(_ptr(cl), _ptr(rw), _ptr(sc), _ptr(motion), L, H, W, radius, tex, _stream()), "weave_match")
    return motion


def weave_path(motion, scene, span, max_shift, subpixel=True):
    """The correction of every frame from the pair motions, one launch (csrc/weave.hip weave_path_kernel; include/e2fgvi_hip.h
    has the definition): motion int32 [L,4] as weave_match made it, scene int32 [L] -> device int32 [L,2] = (cx, cy) in 1/16 px:
    the rounded mean of the path over the symmetric window of up to ``span`` frames either side inside the frame's segment, minus
    the path, clamped to +-``max_shift`` px; whole pixels without ``subpixel``.  span in [0, WEAVE_SPAN_MAX], max_shift in [1,
    WEAVE_SHIFT_MAX]: integers, no bools; subpixel a bool.  No host read; exact integers."""
    lib = _L.load()
    span = _int_arg("span", span, 0, WEAVE_SPAN_MAX)
    max_shift = _int_arg("max_shift", max_shift, 1, WEAVE_SHIFT_MAX)
    if not isinstance(subpixel, bool):
        raise ValueError("subpixel must be a bool, got %r" % (subpixel,))
    mo, sc = _device_inputs([("motion", motion, torch.int32), ("scene", scene, torch.int32)], "motion")
    if mo.dim() != 2 or mo.shape[1] != 4:
        raise ValueError("motion must be int32 [L,4], got %s" % (tuple(mo.shape),))
    L = int(mo.shape[0])
    _scene_table(sc, "scene", L)
    with torch.cuda.device(mo.device):
        shift = _alloc(L > 0, (L, 2), torch.int32, mo.device)
        _L.check(lib.e2fgvi_weave_path(_ptr(mo), _ptr(sc), _ptr(shift), L, span, max_shift, int(subpixel), _stream()), "weave_path")
    return shift


def weave_apply(frames, shift, out=None, mask=None, return_mask=False):
    """Frames moved by a shift per frame, one launch (csrc/weave.hip weave_apply_kernel; include/e2fgvi_hip.h has the definition):
    frames uint8 [L,H,W,3] or [L,H,W], shift int32 [L,2] = (cx, cy) in 1/16 px (entries beyond +-16 WEAVE_SHIFT_MAX are clamped
    to it) -> device uint8 of the same shape: the picture moved by (cx, cy) / 16 px, bilinear in 1/16 px with taps clamped to the
    frame; a whole-pixel shift copies bytes.  With ``return_mask`` (or a ``mask`` to write into) the result is (out, mask), mask
    uint8 [L,H,W], 255 where a tap of non-zero weight lay outside the frame.  ``out`` / ``mask``: device tensors to write into,
    which must not overlap ``frames`` (the entry refuses it: a shifted read is not in order); every byte is written.  A wrong
    dtype or shape, H W > 2^26 and a non-contiguous input raise ValueError.  No host read; exact integers."""
    lib = _L.load()
    named = [("frames", frames, torch.uint8), ("shift", shift, torch.int32)]
    named += [(nm, v, torch.uint8) for nm, v in (("out", out), ("mask", mask)) if v is not None]
    up = dict(zip([n[0] for n in named], _device_inputs(named, "frames", written=("out", "mask"))))
    fr, sh = up["frames"], up["shift"]
    if fr.dim() not in (3, 4) or (fr.dim() == 4 and fr.shape[3] != 3):
        raise ValueError("frames must be [L,H,W,3] or [L,H,W], got %s" % (tuple(fr.shape),))
    L, H, W = (int(v) for v in fr.shape[:3])
    if H * W > FLICKER_PIXELS_MAX:
        raise ValueError("frames must have H W <= 2^26, got %d x %d" % (H, W))
    if tuple(sh.shape) != (L, 2):
        raise ValueError("shift must be int32 [%d,2], got %s" % (L, tuple(sh.shape)))
    if "out" in up and tuple(up["out"].shape) != tuple(fr.shape):
        raise ValueError("out must be %s, got %s" % (list(fr.shape), tuple(up["out"].shape)))
    if "mask" in up and tuple(up["mask"].shape) != (L, H, W):
        raise ValueError("mask must be [%d,%d,%d], got %s" % (L, H, W, tuple(up["mask"].shape)))
    with torch.cuda.device(fr.device):
        ou = up["out"] if "out" in up else torch.empty_like(fr)
        mk = up.get("mask")
        if mk is None and return_mask:
            mk = _alloc(L * H * W > 0, (L, H, W), torch.uint8, fr.device)
        _L.check(lib.e2fgvi_weave_apply(_ptr(fr), _ptr(sh), _ptr(ou), _ptr(mk), L, H, W, 3 if fr.dim() == 4 else 1, _stream()),
                 "weave_apply")
    return (ou, mk) if mk is not None else ou


INTERLACE_EDGES_MAX = 2                    # csrc/interlace.hip: parameters outside these ranges are E2FGVI_EINVAL
INTERLACE_MODES = {"field": 0, "first": 1, "second": 2}    # mode: field rate; frame rate, the first / the second field kept


def interlace_scores(frames, scene):
    """The field-order scores of the deinterlacer, one launch over all frames (csrc/interlace.hip interlace_scores_kernel;
    include/e2fgvi_hip.h has the definition; video.detect_interlace is the caller): frames uint8 [L,H,W,3], scene int32 [L], equal
    entries = one scene -> device int64 [L,2]: D[t][q] sets the rows of parity q of frame t + 1 against their neighbours in frame
    t, 0 for the last frame of a scene and when H < 4.  Device tensors, or anything torch.as_tensor accepts (uploaded first); a
    wrong dtype or shape, more than 2^26 pixels a frame and a non-contiguous input raise ValueError.  There is no CPU path and no
    host read; integer atomics: the same input gives the same bits in every run."""
    lib = _L.load()
    fr, sc = _device_inputs([("frames", frames, torch.uint8), ("scene", scene, torch.int32)], "frames")
    L, H, W = _flicker_frames(fr)
    _scene_table(sc, "scene", L)
    with torch.cuda.device(fr.device):
        D = _alloc(L > 0 and H > 0 and W > 0, (L, 2), torch.int64, fr.device)     # with work the entry clears every word
        _L.check(lib.e2fgvi_interlace_scores(_ptr(fr), _ptr(sc), _ptr(D), L, H, W, _stream()), "interlace_scores")
    return D


def deinterlace(frames, scene, tff, mode, guard, edges, out=None):
    """The two fields of every frame as pictures of their own, one launch (csrc/interlace.hip interlace_fields_kernel;
    include/e2fgvi_hip.h has the definition; video.deinterlace is the caller): frames uint8 [L,H,W,3], scene int32 [L] -> device
    uint8 [2L,H,W,3] (mode 0, field rate) or [L,H,W,3] (mode 1: the first field kept, mode 2: the second).  A kept row is copied;
    a missing row is the line average of the rows around it, along the direction ``edges`` allows, clamped to within diff of the
    mean of the two fields of its own parity nearest in time.  tff and guard bools, mode in [0, 2], edges in [0,
    INTERLACE_EDGES_MAX]: integers, no bools.  ``out``: a device tensor of the result's shape to write into, which must not
    overlap ``frames`` (the entry refuses it); every byte is written once.  The checks of interlace_scores; no host read; exact
    integers."""
    lib = _L.load()
    for nm, v in (("tff", tff), ("guard", guard)):
        if not isinstance(v, bool):
            raise ValueError("%s must be a bool, got %r" % (nm, v))
    mode = _int_arg("mode", mode, 0, 2)
    edges = _int_arg("edges", edges, 0, INTERLACE_EDGES_MAX)
    named = [("frames", frames, torch.uint8), ("scene", scene, torch.int32)] + ([("out", out, torch.uint8)] if out is not None else [])
    up = _device_inputs(named, "frames", written=("out",))
    fr, sc = up[:2]
    L, H, W = _flicker_frames(fr)
    _scene_table(sc, "scene", L)
    shape = (2 * L if mode == 0 else L, H, W, 3)
    if out is not None and tuple(up[2].shape) != shape:
        raise ValueError("out must be %s, got %s" % (list(shape), tuple(up[2].shape)))
    with torch.cuda.device(fr.device):
        ou = up[2] if out is not None else torch.empty(shape, dtype=torch.uint8, device=fr.device)
        _L.check(lib.e2fgvi_deinterlace(_ptr(fr), _ptr(sc), _ptr(ou), L, H, W, int(tff), mode, int(guard), edges, _stream()),
                 "deinterlace")
    return ou


def telecine_scores(frames, scene):
    """The field-matching scores of the inverse telecine, one launch over all frames (csrc/telecine.hip telecine_scores_kernel;
    include/e2fgvi_hip.h has the definition; video.telecine_scores is the caller): frames uint8 [L,H,W,3], scene int32 [L], equal
    entries = one scene -> device int64 [L,2,3,16]: M[t][q][j][cell] sets the rows of parity q of frame t - 1, t or t + 1 (j = 0,
    1, 2; a frame outside the video or the scene is t itself) against their neighbours in frame t, cell by cell of the scene
    detector's 4 x 4 grid; 0 when H < 4.  The inputs and the checks of interlace_scores.  There is no CPU path and no host read;
    integer atomics: the same input gives the same bits in every run."""
    lib = _L.load()
    fr, sc = _device_inputs([("frames", frames, torch.uint8), ("scene", scene, torch.int32)], "frames")
    L, H, W = _flicker_frames(fr)
    _scene_table(sc, "scene", L)
    with torch.cuda.device(fr.device):
        M = _alloc(L > 0 and H > 0 and W > 0, (L, 2, 3, 16), torch.int64, fr.device)     # with work the entry clears every word
        _L.check(lib.e2fgvi_telecine_scores(_ptr(fr), _ptr(sc), _ptr(M), L, H, W, _stream()), "telecine_scores")
    return M


def field_weave(frames, jobs, keep, out=None):
    """Frames put together from the fields of two frames each, one launch (csrc/telecine.hip telecine_weave_kernel;
    include/e2fgvi_hip.h has the definition; video.inverse_telecine is the caller): frames uint8 [L,H,W,3], ``jobs`` [n][2] = (a, b)
    on the HOST (a list or an integer array) -> device uint8 [n,H,W,3]: the rows of parity ``keep`` (0 or 1, an integer, no bool) of
    out[i] are the rows of frames[a_i], the others those of frames[b_i].  An id outside [0, L) is a ValueError, raised in front of
    the upload of the jobs (the kernel clamps ids all the same).  ``out``: a device tensor of the result's shape to write into,
    which must not overlap ``frames`` (the entry refuses it); every byte is written once.  The checks of interlace_scores; no host
    read; no job or no pixel: no launch."""
    lib = _L.load()
    keep = _int_arg("keep", keep, 0, 1)
    if isinstance(jobs, torch.Tensor) and jobs.is_cuda:
        raise ValueError("jobs must be on the host (a list or an integer array [n][2]), got a device tensor")
    jb = torch.as_tensor(jobs)
    if jb.numel() == 0:
        jb = torch.zeros((0, 2), dtype=torch.int64)
    if jb.dim() != 2 or jb.shape[1] != 2 or jb.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise ValueError("jobs must be integers [n][2], got %s %s" % (jb.dtype, tuple(jb.shape)))
    named = [("frames", frames, torch.uint8)] + ([("out", out, torch.uint8)] if out is not None else [])
    up = _device_inputs(named, "frames", written=("out",))
    fr = up[0]
    L, H, W = _flicker_frames(fr)
    n = int(jb.shape[0])
    if n and (int(jb.min()) < 0 or int(jb.max()) >= L):
        raise ValueError("jobs must name frames in [0, %d), got %d .. %d" % (L, int(jb.min()), int(jb.max())))
    shape = (n, H, W, 3)
    if out is not None and tuple(up[1].shape) != shape:
        raise ValueError("out must be %s, got %s" % (list(shape), tuple(up[1].shape)))
    with torch.cuda.device(fr.device):
        ou = up[1] if out is not None else torch.empty(shape, dtype=torch.uint8, device=fr.device)
        if n and H * W:
            jd = jb.to(torch.int32).contiguous().to(fr.device)
            _L.check(lib.e2fgvi_field_weave(_ptr(fr), _ptr(jd), _ptr(ou), L, n, H, W, keep, _stream()), "field_weave")
    return ou


DENOISE_STRENGTH_MAX = 64                  # csrc/denoise.hip: parameters outside these ranges are E2FGVI_EINVAL
DENOISE_SEARCH_MAX = 2
DENOISE_PIXELS_MAX = 2 ** 31 - 256 - 1


def denoise_work_bytes(L, H, W):
    """the bytes of the luma workspace e2fgvi_denoise asks for (include/e2fgvi_hip.h): a plane a frame with a ring of four pixels
    and rows padded to a dword plus one"""
    return L * (H + 8) * (((W + 11) & ~3) + 4)


def denoise(frames, fwd, bwd, scene, strength, search, max_change, out=None):
    """The motion-compensated temporal denoiser (csrc/denoise.hip; include/e2fgvi_hip.h has the definition; video.denoise is the
    caller): frames uint8 [L,H,W,3]; fwd, bwd fp32 [L-1,H,W,2] in metrics.warp_error's convention; scene int32 [L], equal entries
    = one scene -> device uint8 [L,H,W,3]: every pixel the mean of itself (weight 256) and of the (2 search + 1)^2 pixels around
    the place its flow points at in the frame before and in the frame after, each weighted by max(0, 256 - SAD / (9 strength)
    256) of the 3 x 3 luma patches, and moved by ``max_change`` levels at the most.  One call of the entry: a luma pass into a
    workspace allocated here (denoise_work_bytes: about a byte a pixel) and the filter pass, no host read.  strength in [1, 64], search in [0, 2], max_change in [0, 255]:
    integers, no bools.  ``out``: a device tensor of the frames' shape to write into, which must not overlap ``frames`` (the entry
    refuses it); every byte is written once.  Device tensors, or anything torch.as_tensor accepts (uploaded first); wrong dtypes,
    shapes that do not fit, non-contiguous inputs and tensors on different devices raise ValueError.  There is no CPU path.
    Exact integers: the same inputs give the same bytes in every run."""
    lib = _L.load()
    strength = _int_arg("strength", strength, 1, DENOISE_STRENGTH_MAX)
    search = _int_arg("search", search, 0, DENOISE_SEARCH_MAX)
    max_change = _int_arg("max_change", max_change, 0, 255)
    named = [("frames", frames, torch.uint8), ("fwd", fwd, torch.float32), ("bwd", bwd, torch.float32), ("scene", scene, torch.int32)]
    if out is not None:
        named.append(("out", out, torch.uint8))
    up = _device_inputs(named, "frames", written=("out",))
    fr, fw, bw, sc = up[:4]
    L, H, W = _frames_shape(fr, "frames")
    if H * W > DENOISE_PIXELS_MAX:
        raise ValueError("frames must have H W < 2^31 - 256, got %d x %d" % (H, W))
    _scene_table(sc, "scene", L)
    for t, nm in ((fw, "fwd"), (bw, "bwd")):
        if L >= 1 and tuple(t.shape) != (L - 1, H, W, 2):
            raise ValueError("%s must be [%d,%d,%d,2] for frames %s, got %s" % (nm, L - 1, H, W, tuple(fr.shape), tuple(t.shape)))
    if out is not None and tuple(up[4].shape) != (L, H, W, 3):
        raise ValueError("out must be [%d,%d,%d,3], got %s" % (L, H, W, tuple(up[4].shape)))
    with torch.cuda.device(fr.device):
        ou = up[4] if out is not None else torch.empty_like(fr)
        nwork = denoise_work_bytes(L, H, W) if L >= 2 and H * W > 0 else 0
        work = torch.empty(nwork, dtype=torch.uint8, device=fr.device)
        _L.check(lib.e2fgvi_denoise(_ptr(fr), _ptr(fw), _ptr(bw), _ptr(sc), _ptr(ou), _ptr(work), nwork, L, H, W, strength, search,
                                    max_change, _stream()), "denoise")
    return ou


INTERPOLATE_ITERATIONS_MAX = 8             # csrc/interpolate.hip: parameters outside these ranges are E2FGVI_EINVAL
INTERPOLATE_TOLERANCE_MAX = 255
INTERPOLATE_MATCH_MAX = 765
INTERPOLATE_D_MAX = 64
INTERPOLATE_PIXELS_MAX = DENOISE_PIXELS_MAX


def interpolate_jobs_ok(jobs, L, P):
    """whether every row (ia, ib, fi, k, d) of a host job table lies in its ranges for L frames and P flow pairs (rows that do
    not are skipped by the kernel: csrc/interpolate.hip)"""
    return all(0 <= ia < L and 0 <= ib < L and 0 <= fi < P and 1 <= d <= INTERPOLATE_D_MAX and 0 <= k <= d
               for ia, ib, fi, k, d in jobs)


def interpolate(frames, fwd, bwd, jobs, iterations, tolerance, match, out=None, source=None):
    """Frames at fractional times between frames, gathered along the flows (csrc/interpolate.hip; include/e2fgvi_hip.h has the
    definition; video.retime and video.replace_frames are the callers): frames uint8 [L,H,W,3]; fwd, bwd fp32 [P,H,W,2], P flow
    pairs in metrics.warp_error's convention; jobs int32 [n,5] of (ia, ib, fi, k, d): output frame j is the picture at time k / d
    between frames[ia] and frames[ib], with fwd[fi] the motion ia -> ib on ia's grid and bwd[fi] the motion back on ib's grid
    -> device uint8 [n,H,W,3], and with ``source`` (True, or a device uint8 [n,H,W] to write into) the pair (out, source):
    5 = a copy (k == 0 or k == d), 1 / 2 = both ends seen and matched, found from ia's / ib's side, 3 / 4 = seen in ia / ib alone,
    0 = no trajectory reached the pixel and it is the cross-fade.  One call of the entry, all jobs in one launch per 65535, no host
    read.  iterations in [0, 8] fixed-point steps, tolerance in [0, 255] sixteenths of a pixel, match in [0, 765] grey levels summed
    over the channels: integers, no bools.  A job outside its ranges (d in [1, 64], k in [0, d]) writes nothing on the device; a job
    table that is given on the host is checked here and refused (ValueError).  ``out``: a device tensor [n,H,W,3] to write into,
    which must not overlap ``frames`` (the entry refuses it).  Device tensors, or anything torch.as_tensor accepts (uploaded first);
    wrong dtypes, shapes that do not fit, non-contiguous inputs and tensors on different devices raise ValueError.  There is no CPU
    path.  No atomics: the same inputs give the same bytes in every run."""
    lib = _L.load()
    iterations = _int_arg("iterations", iterations, 0, INTERPOLATE_ITERATIONS_MAX)
    tolerance = _int_arg("tolerance", tolerance, 0, INTERPOLATE_TOLERANCE_MAX)
    match = _int_arg("match", match, 0, INTERPOLATE_MATCH_MAX)
    want_source = source is not None and source is not False
    host_jobs = None
    if not (isinstance(jobs, torch.Tensor) and jobs.is_cuda):          # a table on the host: its ranges are checked below
        host_jobs = torch.as_tensor(jobs)
        if not hasattr(jobs, "dtype") and host_jobs.dtype == torch.int64:
            jobs = host_jobs.to(torch.int32)                            # rows of Python ints; the ranges are checked on host_jobs
    named = [("frames", frames, torch.uint8), ("fwd", fwd, torch.float32), ("bwd", bwd, torch.float32), ("jobs", jobs, torch.int32)]
    if out is not None:
        named.append(("out", out, torch.uint8))
    if want_source and source is not True:
        named.append(("source", source, torch.uint8))
    up = _device_inputs(named, "frames", written=("out", "source"))
    fr, fw, bw, jb = up[:4]
    L, H, W = _frames_shape(fr, "frames")
    if H * W > INTERPOLATE_PIXELS_MAX:
        raise ValueError("frames must have H W < 2^31 - 256, got %d x %d" % (H, W))
    if fw.dim() != 4 or tuple(fw.shape[1:]) != (H, W, 2):
        raise ValueError("fwd must be [P,%d,%d,2] for frames %s, got %s" % (H, W, tuple(fr.shape), tuple(fw.shape)))
    P = fw.shape[0]
    if tuple(bw.shape) != (P, H, W, 2):
        raise ValueError("bwd must be [%d,%d,%d,2] like fwd, got %s" % (P, H, W, tuple(bw.shape)))
    if jb.dim() != 2 or jb.shape[1] != 5:
        raise ValueError("jobs must be int32 [n,5] of (ia, ib, fi, k, d), got %s" % (tuple(jb.shape),))
    n = jb.shape[0]
    if host_jobs is not None and not interpolate_jobs_ok(host_jobs.tolist(), L, P):
        raise ValueError("jobs: every row (ia, ib, fi, k, d) needs ia, ib in [0, %d), fi in [0, %d), d in [1, %d] and k in [0, d]"
                         % (L, P, INTERPOLATE_D_MAX))
    rest = up[4:]
    if out is not None and tuple(rest[0].shape) != (n, H, W, 3):
        raise ValueError("out must be [%d,%d,%d,3], got %s" % (n, H, W, tuple(rest[0].shape)))
    if want_source and source is not True and tuple(rest[-1].shape) != (n, H, W):
        raise ValueError("source must be [%d,%d,%d], got %s" % (n, H, W, tuple(rest[-1].shape)))
    with torch.cuda.device(fr.device):
        ou = rest[0] if out is not None else torch.empty((n, H, W, 3), dtype=torch.uint8, device=fr.device)
        so = None
        if want_source:
            so = rest[-1] if source is not True else torch.empty((n, H, W), dtype=torch.uint8, device=fr.device)
        _L.check(lib.e2fgvi_interpolate(_ptr(fr), _ptr(fw), _ptr(bw), _ptr(jb), _ptr(ou), _ptr(so), n, L, P, H, W, iterations,
                                        tolerance, match, _stream()), "interpolate")
    return (ou, so) if want_source else ou


YUV_LAYOUTS ={"nv12": 0, "i420": 1}     # E2FGVI_YUV_*/ E2FGVI_CHROMA_* of include/e2fgvi_hip.h
YUV_CHROMA = {"left": 0, "nearest": 1}


def yuv_frame_hw(shape):
    """(H, W) of 4:2:0 frames [L,3H/2,W]; ValueError unless the rows divide by 3 and H and W are even (from the shape alone)"""
    if len(shape) != 3:
        raise ValueError("4:2:0 frames must be [L,3H/2,W], got %s" % (tuple(shape),))
    rows, W = int(shape[1]), int(shape[2])
    if rows % 3:
        raise ValueError("4:2:0 frames [L,3H/2,W] need a row count divisible by 3, got %d" % rows)
    H = rows // 3 * 2
    if H % 2 or W % 2:
        raise ValueError("4:2:0 frames need even H and W, got %d x %d" % (H, W))
    return H, W


def _yuv_args(layout, coef, n):
    if layout not in YUV_LAYOUTS:
        raise ValueError('layout must be "nv12" or "i420", got %r' % (layout,))
    vals = [int(v) for v in coef]
    if len(vals) != n or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in coef):
        raise ValueError("coef must be %d integers, got %r" % (n, coef))
    return YUV_LAYOUTS[layout], (C.c_int32 * n)(*vals)


def yuv420_to_rgb(x, layout, chroma, coef):
    """x uint8 [L,3H/2,W] on the device, ``layout`` "nv12" / "i420", ``chroma`` "left" / "nearest", ``coef`` the six integers
    (cy, crv, cgu, cgv, cbu, yo) -> uint8 [L,H,W,3] RGB on the device: one launch on the caller's stream (csrc/yuv.hip
    yuv420_to_rgb_kernel; include/e2fgvi_hip.h has the definition), no host read."""
    lib = _L.load()
    _u8(x, "frames")
    H, W = yuv_frame_hw(x.shape)
    lay, cf = _yuv_args(layout, coef, 6)
    if chroma not in YUV_CHROMA:
        raise ValueError('chroma must be "left" or "nearest", got %r' % (chroma,))
    L = x.shape[0]
    with torch.cuda.device(x.device):
        out = torch.empty((L, H, W, 3), dtype=torch.uint8, device=x.device)
        _L.check(lib.e2fgvi_yuv420_to_rgb(_ptr(x), _ptr(out), L, H, W, lay, YUV_CHROMA[chroma], cf, _stream()), "yuv420_to_rgb")
    return out


def rgb_to_yuv420(rgb, layout, coef, like=None, like_rgb=None):
    """rgb uint8 [L,H,W,3] on the device, H and W even, ``coef`` the ten integers (yr, yg, yb, ur, ug, ub, vr, vg, vb, yo) -> uint8
    [L,3H/2,W] in ``layout`` on the device.  With ``like`` [L,3H/2,W] and ``like_rgb`` [L,H,W,3] (both or neither) the paste form:
    the luma byte of a pixel whose three bytes equal like_rgb's and the chroma pair of a block of four such pixels are like's, the
    rest is encoded.  One launch either way (csrc/yuv.hip rgb_to_yuv420_kernel), every output byte written once, no host read."""
    lib = _L.load()
    _u8(rgb, "rgb")
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise ValueError("rgb must be [L,H,W,3], got %s" % (tuple(rgb.shape),))
    L, H, W, _ = rgb.shape
    if H % 2 or W % 2:
        raise ValueError("4:2:0 frames need even H and W, got %d x %d" % (H, W))
    lay, cf = _yuv_args(layout, coef, 10)
    if (like is None) != (like_rgb is None):
        raise ValueError("like and like_rgb come together")
    if like is not None:
        _u8(like, "like"); _u8(like_rgb, "like_rgb")
        if tuple(like.shape) != (L, H // 2 * 3, W) or like_rgb.shape != rgb.shape or like.device != rgb.device \
                or like_rgb.device != rgb.device:
            raise ValueError("like must be [L,3H/2,W] and like_rgb [L,H,W,3] on the device of rgb %s, got %s and %s"
                             % (tuple(rgb.shape), tuple(like.shape), tuple(like_rgb.shape)))
    with torch.cuda.device(rgb.device):
        out = torch.empty((L, H // 2 * 3, W), dtype=torch.uint8, device=rgb.device)
        _L.check(lib.e2fgvi_rgb_to_yuv420(_ptr(rgb), _ptr(like_rgb), _ptr(like), _ptr(out), L, H, W, lay, cf, _stream()),
                 "rgb_to_yuv420")
    return out


def _restore_geometry(lo, mask_lo, src, tabs, n, box):
    """the shape checks restore_u8 and restore_blend share -> (h, w, FH, FW, left, upper, Bw, Bh); n: frames of lo / mask_lo"""
    ytab, xtab, bx, cx, by, cy = (t for _, t in tabs)
    if lo.dim() != 4 or lo.shape[3] != 3 or src.dim() != 4 or src.shape[3] != 3 or mask_lo.dim() != 3:
        raise ValueError("lo and src must be [L,.,.,3] and mask_lo [L,.,.], got %s, %s and %s"
                         % (tuple(lo.shape), tuple(src.shape), tuple(mask_lo.shape)))
    h, w = lo.shape[1:3]
    FH, FW = src.shape[1], src.shape[2]
    if box is None:
        left, upper, W, H = 0, 0, FW, FH
    else:
        if len(box) != 4:
            raise ValueError("box must be (left, upper, right, lower), got %r" % (box,))
        left, upper, right, lower = (int(v) for v in box)
        if not (0 <= left < right <= FW and 0 <= upper < lower <= FH):
            raise ValueError("box %r must be non-empty and lie inside the %d x %d frame" % (tuple(box), FW, FH))
        W, H = right - left, lower - upper
    if lo.shape[0] != n or tuple(mask_lo.shape) != (n, h, w) or min(n, src.shape[0], h, w, H, W) < 1:
        raise ValueError("lo %s, mask_lo %s and src %s do not belong to one video" % (tuple(lo.shape), tuple(mask_lo.shape),
                                                                                       tuple(src.shape)))
    if any(t.device != lo.device for t in (mask_lo, src) + tuple(t for _, t in tabs)):
        raise ValueError("lo, mask_lo, src and the tables must be on one device")
    if ytab.dim() != 1 or ytab.numel() != H or xtab.dim() != 1 or xtab.numel() != W:
        raise ValueError("ytab / xtab must have H = %d / W = %d entries" % (H, W))
    for n_in, n_out, b, c, ax in ((w, W, bx, cx, "x"), (h, H, by, cy, "y")):
        if tuple(b.shape) != (n_out, 2) or c.dim() != 2 or c.shape[0] != n_out:
            raise ValueError("b%s must be [%d,2] and c%s [%d,ksize]" % (ax, n_out, ax, n_out))
        if c.shape[1] != 2 * math.ceil(2.0 * max(n_in / n_out, 1.0)) + 1 and not (n_in == n_out and c.shape[1] == 1):
            raise ValueError("c%s of %d taps does not belong to a %d -> %d resize" % (ax, c.shape[1], n_in, n_out))
    return h, w, FH, FW, left, upper, W, H


FEATHER_MAX = 16       # csrc/video.hip RF_MAX: the largest radius the feathered paste keeps in LDS


def _feather(feather):
    """the radius as an int: an integer in [0, FEATHER_MAX], ValueError otherwise"""
    if isinstance(feather, bool) or not isinstance(feather, numbers.Integral) or not 0 <= feather <= FEATHER_MAX:
        raise ValueError("feather must be an integer in [0, %d], got %r" % (FEATHER_MAX, feather))
    return int(feather)


def restore_blend(lo, mask_lo, src, ids, first, acc, ytab, xtab, bx, cx, by, cy, box=None, touch=None, feather=0):
    """restore_u8 for the n frames of one window, blended into a source-size accumulator (csrc/video.hip, the BLEND epilogue of
    restore_u8_kernel): lo [n,h,w,3] / mask_lo [n,h,w] uint8, src [L,H,W,3] uint8, ids int32 [n] (frame i of lo belongs to frame
    ids[i] of src and acc; an id outside [0, L) is skipped), first uint8 [n], acc fp32 [L,H,W,3], updated in place:
        acc[ids[i]] = img if first[i] else acc[ids[i]] * 0.5 + img * 0.5,     img = what restore_u8(box=) writes for that frame
    inside ``box`` (None: the whole frame); the tables are restore_u8's.  Nothing outside the box is read or written and only its
    tiles are launched.  ``touch`` = (left, upper, right, lower), a rectangle inside the frame that contains the box: the update
    covers it instead -- img is src between the box and its rim -- for a frame whose acc may differ from src there (an earlier
    window with another box).  ``feather`` = r in [1, FEATHER_MAX]: img is what restore_u8(feather=r) writes (the FEATHER form of the
    kernel); 0 is the hard edge.  acc must not overlap an input.  Returns acc."""
    feather = _feather(feather)
    lib = _L.load()
    _u8(lo, "lo"); _u8(mask_lo, "mask_lo"); _u8(src, "src"); _chk(ids, "ids", torch.int32); _u8(first, "first"); _chk(acc, "acc")
    tabs = (("ytab", ytab), ("xtab", xtab), ("bx", bx), ("cx", cx), ("by", by), ("cy", cy))
    for name, t in tabs:
        _chk(t, name, torch.int32)
    n = ids.numel()
    if ids.dim() != 1 or first.dim() != 1 or first.numel() != n:
        raise ValueError("ids must be int32 [n] and first uint8 [n], got %s and %s" % (tuple(ids.shape), tuple(first.shape)))
    h, w, FH, FW, left, upper, Bw, Bh = _restore_geometry(lo, mask_lo, src, tabs, n, box)
    if tuple(acc.shape) != tuple(src.shape) or any(t.device != src.device for t in (ids, first, acc)):
        raise ValueError("acc must be fp32 %s, and ids, first and acc on the device of src" % (tuple(src.shape),))
    if touch is None:
        tl, tu, Tw, Th = left, upper, Bw, Bh
    else:
        if len(touch) != 4:
            raise ValueError("touch must be (left, upper, right, lower), got %r" % (touch,))
        tl, tu, tr, tb = (int(v) for v in touch)
        if not (0 <= tl <= left and left + Bw <= tr <= FW and 0 <= tu <= upper and upper + Bh <= tb <= FH):
            raise ValueError("touch %r must lie inside the %d x %d frame and contain the box" % (tuple(touch), FW, FH))
        Tw, Th = tr - tl, tb - tu
    args = (_ptr(lo), _ptr(mask_lo), _ptr(src), _ptr(ids), _ptr(first), _ptr(acc), n, src.shape[0], h, w, FH, FW, left, upper, Bw, Bh,
            tl, tu, Tw, Th, _ptr(ytab), _ptr(xtab), _ptr(bx), _ptr(cx), cx.shape[1], _ptr(by), _ptr(cy), cy.shape[1])
    if feather:
        _L.check(lib.e2fgvi_restore_feather_blend(*args, feather, _stream()), "restore_feather_blend")
    else:
        _L.check(lib.e2fgvi_restore_blend(*args, _stream()), "restore_blend")
    return acc


def restore_u8(lo, mask_lo, src, ytab, xtab, bx, cx, by, cy, out=None, box=None, feather=0):
    """out = where(NEAREST(mask_lo) != 0, BICUBIC(lo), src) at the size of src, one fused launch (csrc/video.hip): lo [L,h,w,3]
    finished frames, mask_lo [L,h,w] of 0 / 1, src [L,H,W,3], all uint8; ytab int32 [H] / xtab int32 [W] from video.nearest_table;
    bx int32 [W,2], cx int32 [W,kx] and by int32 [H,2], cy int32 [H,ky] from video.bicubic_tables, or the one-tap identity for an
    axis that keeps its size.  Returns a fresh uint8 [L,H,W,3] unless `out` is given; out must not overlap the inputs.
    ``box`` = (left, upper, right, lower) inside the frame confines the paste to that box: out is src outside it, the tables are
    those of a resize to the box's size (right - left, lower - upper) and index box-relative pixels.
    ``feather`` = r in [1, FEATHER_MAX] ramps the pasted edge into src over r pixels, in the same launch (the FEATHER form of the
    kernel), in integers: with M = NEAREST(mask_lo) != 0 and up = BICUBIC(lo) inside the box, everything outside it counting as 0,
        D = M dilated by the (2r+1) x (2r+1) square,  c(p) = number of q in the box with |q - p| <= r (Chebyshev) and D(q),
        n(p) = number of q in the box with |q - p| <= r,     out = (c * up + (n - c) * src + n // 2) // n.
    Every pixel of M has c = n and gets up itself, every pixel farther than 2r from M is src, and the ramp is cut at the box's
    edge.  0 is the hard edge above; anything else raises ValueError."""
    feather = _feather(feather)
    lib = _L.load()
    _u8(lo, "lo"); _u8(mask_lo, "mask_lo"); _u8(src, "src")
    tabs = (("ytab", ytab), ("xtab", xtab), ("bx", bx), ("cx", cx), ("by", by), ("cy", cy))
    for name, t in tabs:
        _chk(t, name, torch.int32)
    if lo.dim() == 4 and src.dim() == 4 and src.shape[0] != lo.shape[0]:
        raise ValueError("lo %s and src %s do not hold the same number of frames" % (tuple(lo.shape), tuple(src.shape)))
    L = lo.shape[0]
    h, w, FH, FW, left, upper, W, H = _restore_geometry(lo, mask_lo, src, tabs, L, box)
    if out is None:
        out = torch.empty((L, FH, FW, 3), dtype=torch.uint8, device=src.device)
    else:
        _u8(out, "out")
        if tuple(out.shape) != (L, FH, FW, 3) or out.device != src.device:
            raise ValueError("out must be uint8 %s on the device of src" % ((L, FH, FW, 3),))
    if feather:
        _L.check(lib.e2fgvi_restore_feather_u8(_ptr(lo), _ptr(mask_lo), _ptr(src), _ptr(out), L, h, w, FH, FW, left, upper, W, H,
                                               _ptr(ytab), _ptr(xtab), _ptr(bx), _ptr(cx), cx.shape[1], _ptr(by), _ptr(cy), cy.shape[1],
                                               feather, _stream()), "restore_feather_u8")
    elif box is None:
        _L.check(lib.e2fgvi_restore_u8(_ptr(lo), _ptr(mask_lo), _ptr(src), _ptr(out), L, h, w, H, W, _ptr(ytab), _ptr(xtab), _ptr(bx),
                                       _ptr(cx), cx.shape[1], _ptr(by), _ptr(cy), cy.shape[1], _stream()), "restore_u8")
    else:
        _L.check(lib.e2fgvi_restore_box_u8(_ptr(lo), _ptr(mask_lo), _ptr(src), _ptr(out), L, h, w, FH, FW, left, upper, W, H, _ptr(ytab),
                                           _ptr(xtab), _ptr(bx), _ptr(cx), cx.shape[1], _ptr(by), _ptr(cy), cy.shape[1], _stream()),
                 "restore_box_u8")
    return out


def u8_to_float(x):
    """uint8 -> fp32, any shape (ndarray.astype(float32)): the start of restore_blend's accumulator"""
    lib = _L.load()
    _u8(x, "x")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if x.numel():
        _L.check(lib.e2fgvi_u8_to_float(_ptr(x), _ptr(out), x.numel(), _stream()), "u8_to_float")
    return out


def float_to_u8(x):
    lib = _L.load()
    _chk(x, "x")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _L.check(lib.e2fgvi_float_to_u8(_ptr(x), _ptr(out), x.numel(), _stream()), "float_to_u8")
    return out


def pred_to_u8(pred, H=None, W=None):
    """model output [N,3,Hp,Wp] in (-1,1) -> uint8 NHWC [N,H,W,3] = uint8((pred+1)/2*255), cropped to H x W."""
    lib = _L.load()
    _chk(pred, "pred")
    N, c, Hp, Wp = pred.shape
    if c != 3:
        raise ValueError("pred must be [N,3,H,W]")
    H, W = H or Hp, W or Wp
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=pred.device)
    _L.check(lib.e2fgvi_pred_to_u8(_ptr(pred), _ptr(out), N, H, W, Hp, Wp, _stream()), "pred_to_u8")
    return out


def _slabs(cache, rows, ids, what):
    _chk_any(cache, "cache"); _chk(rows, "rows", cache.dtype); _chk(ids, "ids", torch.int32)
    if cache.dim() < 2 or rows.dim() != cache.dim() or tuple(rows.shape[1:]) != tuple(cache.shape[1:]):
        raise ValueError("%s: cache [slots, ...] and rows [n, ...] must agree past the first dimension, got %s and %s"
                         % (what, tuple(cache.shape), tuple(rows.shape)))
    if ids.dim() != 1 or ids.numel() != rows.shape[0] or rows.shape[0] == 0:
        raise ValueError("%s: ids must be int32 [%d]" % (what, rows.shape[0]))
    if ids.device != cache.device or rows.device != cache.device:
        raise ValueError("%s: cache, rows and ids must be on one device" % what)
    return rows[0].numel() * rows.element_size()


def gather_slabs(cache, ids, out=None):
    """out[i] = cache[ids[i]]: cache [slots, ...] (fp32 / bf16 / fp16), ids device int32 [n] -> [n, ...], a fresh tensor
    unless `out` is given.  test.py:152 on cached per-frame results; no host read, capturable (csrc/video.hip)."""
    lib = _L.load()
    _chk_any(cache, "cache")
    if out is None:
        out = torch.empty((ids.numel(),) + tuple(cache.shape[1:]), dtype=cache.dtype, device=cache.device)
    slab = _slabs(cache, out, ids, "gather_slabs")
    _L.check(lib.e2fgvi_gather_slabs(_ptr(cache), cache.shape[0], _ptr(ids), ids.numel(), slab, _ptr(out), _stream()), "gather_slabs")
    return out


def scatter_slabs(rows, ids, cache):
    """cache[ids[i]] = rows[i] (ids distinct): the mirror of gather_slabs.  Returns cache."""
    lib = _L.load()
    slab = _slabs(cache, rows, ids, "scatter_slabs")
    _L.check(lib.e2fgvi_scatter_slabs(_ptr(rows), _ptr(ids), ids.numel(), slab, _ptr(cache), cache.shape[0], _stream()),
             "scatter_slabs")
    return cache
