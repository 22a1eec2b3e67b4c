"""Windows in flight on a COLD engine (video.inpaint_video(in_flight=K)), and the seam that makes them safe (ops._lazy).

The engine builds device state lazily, on whatever stream is current at its first use: the engine itself, the weight packings of
the kernels a layer runs, the shared zero buffers, SoftComp's folded bias image.  inpaint_video(in_flight=K) runs consecutive
windows on K streams that nothing orders with each other, so window 1 (stream 1) finds on the host what window 0 (stream 0, or
its side stream) has only ENQUEUED the producer of.  ops._lazy records an event behind every such producer and makes a fetch on
another stream wait for it.

A test that only ran the cold path would pass by luck: the host takes about as long to enqueue an eager forward as the device
takes to run it.  So the hazard is made deterministic:

* a device-side DELAY of more than one warm forward of the clip's largest window is enqueued in front of every producer (the
  seam is wrapped; the delay sits at the producer, not at the start of the forward, whose host-synchronous index uploads would
  drain it).  A consumer on another stream has then certainly run before the producer unless something orders it;
* the caching allocator's free blocks of every stream torch hands out are POISONED with the 16-bit pattern 0x7FC0 (NaN as fp32,
  bf16 and fp16) beforehand, so that a packing or zero buffer read before its producer is NaN, not a plausible value.

Safety (checked by reading, 720b7bc + this change): everything reachable unordered holds VALUES -- packed weights, zeros, a bias
image.  The index tables (key tables, SPyNet's frame pairs, the driver's window ids) are host-synchronous uploads.  NaN
activations reach only clamped or bounds-tested sampling (misc.hip: fminf / fmaxf clamps and bil_zeros; mdcn.hip: `inside`), so
an unordered read gives wrong bytes, never a wild address.

Negative control (run once by hand on the MI355X): the same harness over a seam WITHOUT the event (the parent
commit's ordering: build on the current stream, fetch from any).  Cold engine, e2fgvi_hq 120x200 L = 23: 47121 of 1656000 bytes
differ (bf16, K = 2), 47542 (fp16, K = 2 and K = 3), 0 (bf16, K = 3).  Cold engine, e2fgvi fp32 240x432 (98 producers): 0 bytes
differ for K = 2 and 3; warm on one shape: 0 bytes in all six cases (fp32: 1 producer, 16-bit: none -- those engines pack at
construction).  So the harness BITES on the 16-bit cold engine (zero buffers and the bias image read before their fill) and
does NOT bite on the fp32 one.  Why: a delay in front of every producer also delays the consumer's stream -- window 1 builds
packings of its own (another size class, other kernels) and falls behind by as many delays as window 0's remaining producers;
window 0's eight key-table uploads are host-synchronous and drain stream 0 up to the last transformer block before window 1 is
enqueued at all; and with four hardware queues two streams may share one, which orders them by submission (the K = 3 bf16 case).
The fp32 cases therefore pin the bytes of the cold path and the completeness of the seam (the CPU test above), not the race.

Every comparison is against a second, separately warmed net with the same state dict running one window at a time.
"""
import ast
import importlib
import os
import time

import numpy as np
import pytest
import torch

from e2fgvi_amd import video

CASES = [("e2fgvi", (240, 432), 36, "fp32"), ("e2fgvi_hq", (120, 200), 23, "bf16"), ("e2fgvi_hq", (120, 200), 23, "fp16")]
# warm on one shape: clip lengths whose window plan puts a shape other than the most common one on a stream other than stream 0
# for K = 2 and for K = 3 (L = 23: the new shapes sit at windows 0, 2, 4 -- all on stream 0 of two; asserted in the test)
CASES_ONE_SHAPE = [("e2fgvi", (240, 432), 36, "fp32"), ("e2fgvi_hq", (120, 200), 27, "bf16"), ("e2fgvi_hq", (120, 200), 27, "fp16")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ CPU: the seam is complete
def _calls(tree, name):
    """(enclosing top-level function / method name, call node) of every call of `name` (a bare name or an attribute)"""
    out = []

    def walk(node, where):
        for ch in ast.iter_child_nodes(node):
            w = where
            if isinstance(ch, (ast.FunctionDef, ast.ClassDef)) and where.count(".") < 1:
                w = (where + "." if where else "") + ch.name
            if isinstance(ch, ast.Call):
                f = ch.func
                if (isinstance(f, ast.Name) and f.id == name) or (isinstance(f, ast.Attribute) and f.attr == name):
                    out.append((w, ch))
            walk(ch, w)
    walk(tree, "")
    return out


def _source(rel):
    with open(os.path.join(ROOT, rel)) as fh:
        return fh.read()


def test_every_lazily_built_device_object_goes_through_the_seam():
    """ops._lazy is the only caller of _no_capture (so a new lazy packing, which must refuse graph capture, cannot be added beside
    the seam), and every accessor of lazily built state returns through it: a later packing built without ordering fails here."""
    ops_src = _source("e2fgvi_amd/ops.py")
    tree = ast.parse(ops_src)
    assert sorted(w for w, _ in _calls(tree, "_no_capture")) == ["_lazy"], "only the seam may call _no_capture"
    through = {w for w, _ in _calls(tree, "_lazy")}
    want = {"PackedConv.wino_packed", "PackedConv.wpacked", "PackedConv._wino4", "PackedConv._alt", "PackedConv._wino_x3",
            "PackedConv._alt3", "PackedConvX.wpacked", "PackedConvX._alt3", "SoftCompGather.bias_image"}
    assert want <= through, sorted(want - through)
    assert {w for w, _ in _calls(ast.parse(_source("e2fgvi_amd/engine.py")), "_lazy")} >= {"Engine._zero"}
    assert {w for w, _ in _calls(ast.parse(_source("e2fgvi_amd/generator.py")), "_lazy")} >= {"_InpaintGeneratorBase.engine"}
    # no pack kernel of a lazily packed layer class and no cached buffer is launched / filled outside a seam build: inside the two
    # conv classes every e2fgvi_pack_* call sits in a function nested in an accessor that returns through _lazy, or in
    # PackedConvX._pack, which only the constructor (host-synchronised by Engine.__init__, or itself inside a seam build of
    # _alt / _alt3) and the wpacked accessor call
    for cls in (n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("PackedConv", "PackedConvX")):
        for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef)):
            packs = [n for n in ast.walk(fn) if isinstance(n, ast.Attribute) and n.attr.startswith("e2fgvi_pack_")]
            if packs and fn.name != "_pack":
                assert cls.name + "." + fn.name in through, "%s.%s packs weights outside the seam" % (cls.name, fn.name)
    pack_callers = {w for w, _ in _calls(tree, "_pack")}
    assert pack_callers == {"PackedConvX.__init__", "PackedConvX.wpacked"}, pack_callers
    eng = ast.parse(_source("e2fgvi_amd/engine.py"))
    zeros = {w for w, c in _calls(eng, "zeros") if getattr(getattr(c.func, "value", None), "id", None) == "torch"}
    assert zeros <= {"Engine.__init__", "Engine._zero"}, zeros


def test_the_seam_builds_once_and_fetches_without_a_device():
    """host behaviour of ops._lazy: one build per key, None counts as absent (attributes that start out as None), the stored
    object comes back on every later fetch, and a wrapper around the seam sees every build (what the GPU tests rely on)"""
    from e2fgvi_amd import ops
    built, store = [], {"alt": None}
    assert ops._lazy(store, "alt", "a", lambda: built.append("alt") or "A") == "A"
    assert ops._lazy(store, "alt", "a", lambda: built.append("alt") or "B") == "A"
    assert ops._lazy(store, (3, 4), "b", lambda: built.append("b") or "C") == "C"
    assert store == {"alt": "A", (3, 4): "C"} and built == ["alt", "b"]


# ------------------------------------------------------------------------------------------------ GPU harness
def _net(model, precision, dev):
    from e2fgvi_amd.synth import synth_state_dict
    net = importlib.import_module("model." + model).InpaintGenerator()
    net.load_state_dict(synth_state_dict(model, "stress", 0))
    net = net.to(dev).eval()
    net.precision = precision
    return net


def _shapes(L):
    windows = video.plan_windows(L, 5, 10, -1)
    return [(len(nb), len(rf)) for nb, rf in windows]


def _warm_forward_ms(net, dev, hw, shape):
    """device time of one warm forward of a window of `shape` = (local frames, reference frames) at the padded size"""
    Hp, Wp = video.padded_size(*hw)
    x = torch.rand(1, shape[0] + shape[1], 3, Hp, Wp, device=dev) * 2 - 1
    net(x, shape[0])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    net(x, shape[0])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


class _Delay:
    """a device-side delay of `ms` on the current stream: torch.cuda._sleep calibrated with a pair of events; a chain of large
    matrix products if _sleep does not scale with its argument here"""

    def __init__(self, dev, forward_ms):
        ms = 1.25 * forward_ms                     # aimed at; what must hold is: no shorter than one warm forward
        def timed(fn):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        self.ms, self.count = ms, 0
        t_small, t_big = timed(lambda: torch.cuda._sleep(2_000_000)), timed(lambda: torch.cuda._sleep(20_000_000))
        if t_big > 1.0 and t_big > 4.0 * t_small:
            self.cycles = int(20_000_000 * ms / t_big) + 1
            self.kind, self.got = "sleep", timed(lambda: torch.cuda._sleep(self.cycles))
        else:
            self.a = torch.randn(4096, 4096, device=dev)
            self.b = torch.empty_like(self.a)
            timed(lambda: torch.mm(self.a, self.a, out=self.b))
            one = timed(lambda: [torch.mm(self.a, self.a, out=self.b) for _ in range(8)]) / 8
            self.n = int(ms / one) + 1
            self.kind, self.got = "mm", timed(lambda: [torch.mm(self.a, self.a, out=self.b) for _ in range(self.n)])
        assert self.got >= forward_ms, "the delay (%s) lasts %.2f ms, one forward %.2f ms" % (self.kind, self.got, forward_ms)

    def __call__(self):
        self.count += 1
        if self.kind == "sleep":
            torch.cuda._sleep(self.cycles)
        else:
            for _ in range(self.n):
                torch.mm(self.a, self.a, out=self.b)


def _delayed_seam(monkeypatch, delay):
    """wrap ops._lazy (looked up as a module global by every accessor, and as ops._lazy by the engine and the generator): the
    delay runs on the producer's stream directly in front of every producer"""
    from e2fgvi_amd import ops
    seam = ops._lazy

    def lazy(store, key, what, build):
        def late():
            delay()
            return build()
        return seam(store, key, what, late)
    monkeypatch.setattr(ops, "_lazy", lazy)


def _poison(dev):
    """NaN (0x7FC0 in every 16 bits) in the caching allocator's free blocks of the current stream and of the 32 streams torch
    hands out in turn -- a block freed on one stream is only handed out again on that stream, and inpaint_video allocates its
    packings on streams of its own.  Large pool: one 192 MB block per stream; small pool: 48 blocks of 1 MB."""
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(device=dev) for _ in range(32)]
    seen = set()
    for st in streams:
        if st.cuda_stream in seen:
            continue
        seen.add(st.cuda_stream)
        with torch.cuda.stream(st):
            big = torch.full((96 << 20,), 0x7FC0, dtype=torch.int16, device=dev)
            small = [torch.full((1 << 19,), 0x7FC0, dtype=torch.int16, device=dev) for _ in range(48)]
            del big, small
    torch.cuda.synchronize()


def _reference(dev, model, hw, L, precision):
    """(frames, masks, reference bytes, warmed reference net, ms of one warm forward of the largest window)"""
    from tests.test_video_driver import _toy_video
    frames, masks = _toy_video(L, hw[0], hw[1], seed=9)
    frames, masks = np.stack(frames), np.stack(masks)
    ref_net = _net(model, precision, dev)
    ref = video.inpaint_video(ref_net, frames, masks, 5, 10, -1)
    ms = _warm_forward_ms(ref_net, dev, hw, max(_shapes(L), key=lambda s: s[0] + s[1]))
    return frames, masks, ref, ref_net, ms


def _check(out, ref, what):
    bad = int((out != ref).sum())
    assert bad == 0, "%s: %d of %d bytes differ from one window at a time" % (what, bad, ref.size)


def cold_engine(dev, monkeypatch, model, hw, L, precision, k, patch=_delayed_seam, stream=None):
    """test 1 / 3: a net that has never run, windows on K streams, the delay in front of every producer"""
    t0 = time.perf_counter()
    shapes = _shapes(L)
    assert len(set(shapes)) >= 3, shapes
    frames, masks, ref, ref_net, ms = _reference(dev, model, hw, L, precision)
    delay = _Delay(dev, ms)
    cold = _net(model, precision, dev)
    _poison(dev)
    patch(monkeypatch, delay)
    if stream is None:
        out = video.inpaint_video(cold, frames, masks, 5, 10, -1, in_flight=k)
    else:
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            out = video.inpaint_video(cold, frames, masks, 5, 10, -1, in_flight=k)
        torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    print("cold %s %s K=%d: forward %.2f ms, delay %.2f ms (%s) x %d producers, %.1f s" % (
        model, precision, k, ms, delay.got, delay.kind, delay.count, time.perf_counter() - t0))
    assert delay.count >= 3 and ref_net is not None            # the engine, a zero buffer, a packing or bias image at least
    return out, ref, delay.count


def warm_on_one_shape(dev, monkeypatch, model, hw, L, precision, k, patch=_delayed_seam):
    """test 2: warm on the clip's most common window shape only; the other shapes first appear in the middle of the in-flight run"""
    t0 = time.perf_counter()
    shapes = _shapes(L)
    common = max(set(shapes), key=lambda v: (shapes.count(v), shapes.index(v)))     # a tie: the shape that appears later
    first = {s: shapes.index(s) for s in set(shapes) if s != common}
    assert len(first) >= 2 and any(i % k for i in first.values()), (shapes, k)     # a new shape on a stream other than stream 0
    frames, masks, ref, ref_net, ms = _reference(dev, model, hw, L, precision)
    delay = _Delay(dev, ms)
    net = _net(model, precision, dev)
    Hp, Wp = video.padded_size(*hw)
    net(torch.rand(1, common[0] + common[1], 3, Hp, Wp, device=dev) * 2 - 1, common[0])
    torch.cuda.synchronize()
    _poison(dev)
    patch(monkeypatch, delay)
    out = video.inpaint_video(net, frames, masks, 5, 10, -1, in_flight=k)
    torch.cuda.synchronize()
    print("one shape warm %s %s K=%d: forward %.2f ms, delay %.2f ms (%s) x %d producers, %.1f s" % (
        model, precision, k, ms, delay.got, delay.kind, delay.count, time.perf_counter() - t0))
    assert ref_net is not None
    return out, ref, delay.count


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("model,hw,L,precision", CASES)
def test_cold_engine_windows_in_flight_return_the_bytes_of_the_sequential_driver(dev, monkeypatch, model, hw, L, precision, k):
    """the first forward this net ever runs is window 0 on stream 0, while window 1 on stream 1 reads what it builds"""
    out, ref, _ = cold_engine(dev, monkeypatch, model, hw, L, precision, k)
    _check(out, ref, "cold engine, in_flight=%d" % k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("model,hw,L,precision", CASES_ONE_SHAPE)
def test_new_window_shapes_in_the_middle_of_a_warm_run_return_the_same_bytes(dev, monkeypatch, model, hw, L, precision, k):
    """warm on one window shape, cold on the next: the shorter windows at the ends of a clip select other kernels and build other
    packings on a stream other than stream 0 while their neighbours are in flight"""
    out, ref, _ = warm_on_one_shape(dev, monkeypatch, model, hw, L, precision, k)
    _check(out, ref, "warm on one shape, in_flight=%d" % k)


@pytest.mark.gpu
@pytest.mark.parametrize("model,hw,L,precision", CASES[:2])
def test_cold_engine_under_a_callers_stream_returns_the_same_bytes(dev, monkeypatch, model, hw, L, precision):
    """the caller's stream is not the default stream: uploads, mask preparation and compositing run on it"""
    out, ref, _ = cold_engine(dev, monkeypatch, model, hw, L, precision, 2, stream=torch.cuda.Stream(device=dev))
    _check(out, ref, "cold engine under torch.cuda.stream(s), in_flight=2")
