"""Second-stream aggressor tests: every Winograd kernel the decision table can select runs
on one stream while plain device copies of 256 MB run on another -- the condition under which round 4's wide-tile kernel returned
wrong 16x16-pixel blocks in 72 of 72 launches (profiles/r04_c4_repro.txt: a memory system slow enough for the weight loads issued
past the end of the K loop to land AFTER the compiler had reused their registers) -- and every launch must return the bits of the
unaccompanied launch.  The static side of the same guarantee is build.verify_exit_reuse() (tests/test_host_logic.py)."""
import pytest
import torch

from tests.util import assert_one_conv_launch, gen, launch_trace

pytestmark = pytest.mark.gpu

LAUNCHES = 200          # per (kernel, shape): a 3 % per-launch event is missed with p < 1 %
PER_ROUND = 8


def _codes():
    from e2fgvi_amd import ops
    w3 = [ops.W3_BASE + c for c in (6064, 5132, 164, 132, 32)]         # split-operand: wide tile, four positions per wave, 8-wave shapes
    return w3 + [2464] + [64, 32, 164, 132]                           # fp32 F(2x4) and the fp32 F(2x2) block shapes


# (name, Cout, cpg, groups, N): the two encoder shapes the fault was found on (one source; two sources in two groups) and the
# one-frame propagation shape (the launches that run under the previous step's all-gather in a sharded job)
SHAPES = [("encoder.layers.8", 384, [256], 1, 10), ("encoder.layers.10", 512, [128, 192], 2, 10), ("conv_offset.2", 128, [128], 1, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_winograd_kernels_beside_device_copies_return_the_bits_of_the_launch_alone(dev, shape):
    from e2fgvi_amd import lib as L, ops
    name, cout, cpg, groups, n = shape
    g = gen(1100 + len(name))
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    layer = ops.PackedConv(rnd(cout, sum(cpg), 3, 3) * 0.05, rnd(cout), cpg, groups=groups, pad=1, algo="winograd")
    srcs = [rnd(n, 60, 108, c * groups) for c in cpg]
    big_a, big_b = torch.empty(64 << 20, device=dev), torch.empty(64 << 20, device=dev)
    big_a.normal_()
    side, main = torch.cuda.Stream(device=dev), torch.cuda.current_stream()
    ran = []
    for code in _codes():
        ref = torch.empty(n, 60, 108, cout, device=dev)
        try:
            with launch_trace() as trace:
                layer(srcs, out=ref, act=ops.ACT_LRELU, slope=0.2, tile=code)
        except L.HipError:
            continue                                    # a block shape this geometry rejects (e.g. F(4x4) needs H % 4 == 0)
        # the kernel the code names, in one launch: a split-operand block shape that the launcher refuses does not raise, the
        # fp32 Winograd kernel runs in its place -- and would be what the 200 launches below exercise
        assert_one_conv_launch(trace, "e2fgvi_conv3x3_winograd_x3" if code >= ops.W3_BASE else "e2fgvi_conv3x3_winograd4"
                               if code in ops.W4_CODES else "e2fgvi_conv3x3_winograd", tile=code, what="%s, tile code %d" % (name, code))
        torch.cuda.synchronize()
        outs = [torch.empty_like(ref) for _ in range(PER_ROUND)]
        bad = 0
        for _ in range(LAUNCHES // PER_ROUND):
            for o in outs:
                o.fill_(float("nan"))
            side.wait_stream(main)
            with torch.cuda.stream(side):
                for _ in range(3 * PER_ROUND if n > 1 else PER_ROUND):
                    big_b.copy_(big_a, non_blocking=True)
            for o in outs:
                layer(srcs, out=o, act=ops.ACT_LRELU, slope=0.2, tile=code)
            main.wait_stream(side)
            torch.cuda.synchronize()
            bad += sum(0 if torch.equal(o, ref) else 1 for o in outs)
        assert bad == 0, "%s, tile code %d: %d of %d launches beside device copies differ from the launch alone" % (name, code, bad, LAUNCHES)
        ran.append(code)
    assert len(ran) >= 8 and ops.W3_BASE + ops.W3_WIDE in ran, ran          # the kernels were really exercised, not skipped


def test_wide_kernel_runs_beside_spynet_in_the_headline_forward(dev):
    """With round 4's per-layer gate gone the table may hand encoder.layers.2 / 6 / 8 -- which overlap the SPyNet stream in every
    forward -- to the wide-tile kernel.  Whatever the table says today, this test FORCES the kernel onto those three layers (so
    that it really runs beside the second stream at T = 10; `test_stream_overlap_is_bit_identical_to_serial` only sees the table's
    choice) and compares 60 overlapped forwards with the serial one, bit for bit."""
    from e2fgvi_amd import lib as L, ops
    from e2fgvi_amd.engine import Engine
    from e2fgvi_amd.synth import synth_clip, synth_state_dict
    if not ops.X3_ENABLED:
        pytest.skip("split-operand kernels switched off")
    sd = synth_state_dict("e2fgvi", "stress", 0)
    x = synth_clip(1, 10, 240, 432, seed=5, moving=True)[0].to(dev)
    eng = Engine(sd, "e2fgvi", dev, precision="fp32")
    wide = ops.W3_BASE + ops.W3_WIDE

    def forced(layer):
        def call(sources, **kw):
            return layer(sources, tile=wide, **kw)
        call.name = layer.name
        return call
    for k in (1, 3, 4):                                  # encoder.layers.2 / .6 / .8
        eng.enc[k] = forced(eng.enc[k])
    eng.overlap_flows = False
    L.TRACE = []
    try:
        base, (bf, bb) = eng.forward(x, 10)
        torch.cuda.synchronize()
        kern = {r["meta"]["layer"]: r["meta"]["kernel"] for r in L.TRACE if r.get("meta") and "kernel" in r["meta"]}
    finally:
        L.TRACE = None
    assert all(kern.get("encoder.layers.%d" % i, "").startswith("conv_wino_x3w") for i in (2, 6, 8)), kern
    eng.overlap_flows = True
    for _ in range(60):
        got, (ff, fb) = eng.forward(x, 10)
        torch.cuda.synchronize()
        assert torch.equal(ff, bf) and torch.equal(fb, bb) and torch.equal(got, base)


def test_forced_gather_soak_of_the_eight_clip_step_is_bit_identical(dev):
    """BASELINE configs[2]'s per-GPU step -- 8 clips of 432x240 T=10 per forward, HIP-graph replay, the uint8 frames all-gathered
    over RCCL under the NEXT forward (world size 1: the gather is a device copy, the aggressor of C4) -- for 50 steps: every
    step's gathered frames must be the bits of the plain forward.  This is the configuration in which the wide-tile kernel runs
    beside RCCL's copy kernels since round 4's last commit; the driver's suite at world size 1 is the only place it can be
    soaked on hardware (VERDICT round 4, item 1 iv)."""
    import importlib
    import os
    import socket
    import torch.distributed as dist
    from e2fgvi_amd import ops, runner
    from e2fgvi_amd.synth import synth_clip, synth_state_dict
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "stress", 0))
    net = net.to(dev).eval()
    x = synth_clip(8, 10, 240, 432, seed=47, moving=True)[0].to(dev)
    want = ops.pred_to_u8(net(x, 10)[0].contiguous()).clone()
    torch.cuda.synchronize()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        step = runner.ShardedStep(net, x, 10, group_world=1, use_graph=True, force_gather=True, pack_u8=True)
        bad = 0
        for k in range(51):
            got = step.run()
            if k:
                bad += 0 if torch.equal(got, want) else 1
        bad += 0 if torch.equal(step.finish(), want) else 1
        assert step.graphed and bad == 0, "%d of 51 pipelined steps differ from the plain forward" % bad
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("model,hw,t,lt,k,precision", [("e2fgvi", (240, 432), 10, 10, 3, "fp32"), ("e2fgvi", (240, 432), 6, 3, 2, "fp32"),
                                                        ("e2fgvi_hq", (120, 216), 4, 3, 3, "bf16")])
def test_forwards_in_flight_return_the_bits_of_the_serial_forward(dev, model, hw, t, lt, k, precision):
    """runner.ShardedStep(in_flight=K), round 6: K HIP graphs of the same forward on K streams, any kernel of one beside any kernel
    of another -- every step must return the bits of the single-stream forward (60 steps), in the order the steps were issued"""
    import importlib
    from e2fgvi_amd import runner
    from e2fgvi_amd.synth import synth_clip, synth_state_dict
    net = importlib.import_module("model." + model).InpaintGenerator()
    net.load_state_dict(synth_state_dict(model, "stress", 0))
    net = net.to(dev).eval()
    net.precision = precision
    x = synth_clip(1, t, hw[0], hw[1], seed=31, moving=True)[0].to(dev)
    net(x, lt)
    with runner.whole_propagation(net):          # the pipelines run conv_offset.0 / backbone.0 whole (no side-stream split)
        ref = net(x, lt)[0].clone()
    step = runner.ShardedStep(net, x, lt, in_flight=k)
    got, none = 0, 0
    for n in range(60):
        out = step.run()
        if out is None:
            none += 1
            continue
        assert torch.equal(out, ref), "step %d of %d in flight differs from the serial forward" % (n, k)
        got += 1
    assert torch.equal(step.finish(), ref)
    assert step.graphed and step.in_flight == k and none <= k and got >= 60 - k - 1


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("model,hw,t,lt,precision", [("e2fgvi", (240, 432), 10, 10, "fp32"), ("e2fgvi_hq", (120, 216), 4, 3, "bf16")])
def test_changing_clips_in_flight_come_back_in_order_from_untorn_inputs(dev, model, hw, t, lt, precision, k):
    """runner.ShardedStep(in_flight=K) as a serving step: six different clips cycle through ``step.x.copy_(clip); step.run()`` for 60
    steps.  The frames that come back, in order, are the serial whole-propagation forwards of c_0, c_1, ... -- none skipped, none
    repeated: the eager first call returns its own step, the next K - 1 calls return None while the pipelines fill, call n returns
    step n - (K - 1), finish() the last one.  x is overwritten (with NaN) as soon as run() returns, as the docstring allows: every
    pipeline reads a private copy taken inside run().  With one input shared by the K graphs that write landed under the steps
    still in flight.
    What this test cannot do: a torn read needs two pipelines in phase, and graph replay offers no seam for a delay, so the test
    does not force the race of a caller who merely refreshes x before the next run() -- that ordering holds by construction (the
    copy into the private input is on the pipeline's stream behind its wait for the caller's stream, and the caller's stream
    waits for the copy); the test pins the contract of which clip a returned frame belongs to."""
    import importlib
    from e2fgvi_amd import runner
    from e2fgvi_amd.synth import synth_clip, synth_state_dict
    net = importlib.import_module("model." + model).InpaintGenerator()
    net.load_state_dict(synth_state_dict(model, "stress", 0))
    net = net.to(dev).eval()
    net.precision = precision
    clips = [synth_clip(1, t, hw[0], hw[1], seed=40 + i, moving=True)[0].to(dev) for i in range(6)]
    net(clips[0], lt)
    with runner.whole_propagation(net):
        refs = [net(c, lt)[0].clone() for c in clips]
    for i in range(6):
        for j in range(i):
            assert not torch.equal(refs[i], refs[j]), "clips %d and %d give the same frames" % (i, j)
    step = runner.ShardedStep(net, clips[0].clone(), lt, in_flight=k)
    got, nones = 0, []
    for n in range(60):
        step.x.copy_(clips[n % 6])
        out = step.run()
        step.x.fill_(float("nan"))
        if out is None:
            nones.append(n)
            continue
        assert torch.equal(out, refs[got % 6]), "call %d, %d in flight: not the frames of step %d (clip %d)" % (n, k, got, got % 6)
        got += 1
    assert torch.equal(step.finish(), refs[59 % 6]), "finish() does not return the last step's frames"
    assert step.graphed and step.in_flight == k and nones == list(range(1, k)) and got == 60 - (k - 1)


@pytest.mark.parametrize("tile,ref_tile", [(107, 7), (108, 8)])
def test_ping_pong_gemm_beside_device_copies_returns_the_bits_of_the_one_barrier_tile(dev, tile, ref_tile):
    """conv_bf16x.hip PP (round 6): LDS-DMA through inline asm, raw s_barrier, the kernel's own vmcnt waits -- the discipline the wide-tile
    Winograd kernel needed C4's guards for.  With 256 MB device copies on a second stream (slow, late operand traffic) every launch
    must return the bits of the one-barrier tile's launch alone: a stage read before its pieces have landed, or overwritten while
    its trailing readers are still on it, shows up here.  Shapes: fc1 (K = 512: 16 steps), the SoftSplit convolution (7x7 stride 3,
    retargets per tap: 196 steps) and a two-source 1x1 layer (the source walk)."""
    from e2fgvi_amd import ops
    g = gen(4100 + tile)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    cases = [("fc1", [rnd(7200, 1, 1, 512)], ops.PackedConvX(rnd(1960, 512, 1, 1) * 0.05, rnd(1960), [512], dtype=torch.float32, x3=True)),
             ("ss", [rnd(10, 60, 108, 128)], ops.PackedConvX(rnd(512, 128, 7, 7) * 0.02, rnd(512), [128], stride=3, pad=3, dtype=torch.float32, x3=True)),
             ("fusion", [rnd(10, 60, 108, 128), rnd(10, 60, 108, 128)], ops.PackedConvX(rnd(256, 256, 1, 1) * 0.06, rnd(256), [128, 128], dtype=torch.float32, x3=True))]
    big_a, big_b = torch.empty(64 << 20, device=dev), torch.empty(64 << 20, device=dev)
    big_a.normal_()
    side, main = torch.cuda.Stream(device=dev), torch.cuda.current_stream()
    for name, srcs, layer in cases:
        ref = layer(srcs, tile=ref_tile).clone()
        torch.cuda.synchronize()
        outs = [torch.empty_like(ref) for _ in range(PER_ROUND)]
        bad = 0
        for _ in range(LAUNCHES // PER_ROUND):
            for o in outs:
                o.fill_(float("nan"))
            side.wait_stream(main)
            with torch.cuda.stream(side):
                for _ in range(3 * PER_ROUND):
                    big_b.copy_(big_a, non_blocking=True)
            for o in outs:
                layer(srcs, out=o, tile=tile)
            main.wait_stream(side)
            torch.cuda.synchronize()
            bad += sum(0 if torch.equal(o, ref) else 1 for o in outs)
        assert bad == 0, "%s, tile %d: %d of %d launches beside device copies differ from tile %d alone" % (name, tile, bad, LAUNCHES, ref_tile)


_C8_SCRIPT = r"""
import importlib, sys, torch
sys.path.insert(0, %r)
from e2fgvi_amd import runner
from e2fgvi_amd.synth import synth_clip, synth_state_dict
dev = torch.device("cuda:0")
x = synth_clip(1, 10, 240, 432, seed=0, smooth=False)[0].to(dev)


def engine():
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(synth_state_dict("e2fgvi", "default", 0))
    net = net.to(dev).eval()
    net(x, 10)
    return net


def graphed_steps(net, n, **kw):                            # what bench.time_local does: capture, replay, drop the graph(s)
    step = runner.ShardedStep(net, x, 10, **kw)
    for _ in range(n):
        step.run()
    out = step.finish().clone()
    torch.cuda.synchronize()
    assert step.graphed
    return out


net = engine()
ref = net(x, 10)[0].clone()
with runner.whole_propagation(net):
    ref_whole = net(x, 10)[0].clone()
assert torch.equal(graphed_steps(net, 5), ref)              # bench.py's order: the sequential graph ...
assert torch.equal(graphed_steps(net, 7, in_flight=2), ref_whole)   # ... two pipelines + the calibration's eleven streams ...
del net
torch.cuda.empty_cache()
from e2fgvi_amd import engine as _engine, ops
for rep in range(2):                                        # ... then NEW engines (new side streams), one graph each -- the first one
    ops.X3_ENABLED, _engine.FC2_CONV = rep == 1, rep == 1   # as bench.py's first secondary line builds it (every product an fp32 MFMA)
    net = engine()
    ref1 = net(x, 10)[0].clone()
    assert torch.equal(graphed_steps(net, 4), ref1)
    del net
print("__C8_OK__")
"""


def test_graph_of_a_new_engine_replays_after_earlier_graphs_were_destroyed(dev):
    """with one side stream per main stream, a graph captured on torch.cuda.graph's default capture stream forked a side
    stream that had never run anything; once earlier graphs of the process had been destroyed its replay died in
    hip::Graph::UpdateStreams (SIGSEGV -- hence a subprocess).  ShardedStep._capture captures on the stream its warm-up ran on.
    This walks bench.py's order of captures and destructions in a few seconds; the invocation that crashed 5 of 5 before the fix is
    tests/test_gpu_bench_lines.py::test_default_line_carries_the_hq_configs (this shorter sequence did not crash with the old capture
    stream either: it is the smoke test of the rule, that one is the reproducer)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", _C8_SCRIPT % root], capture_output=True, text=True, timeout=600, cwd=root)
    assert p.returncode == 0 and "__C8_OK__" in p.stdout, (p.returncode, p.stderr[-1500:])
