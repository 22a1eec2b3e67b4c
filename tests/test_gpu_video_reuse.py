"""video.inpaint_video(reuse=True): every frame through the encoder once, every adjacent pair through SPyNet once, only the local
frames decoded.  The contract is the reference loop around the oracle (not the bytes of reuse=False: launches on a few new
frames may pick other kernels from the size-class table than launches on a whole window)."""
import importlib

import numpy as np
import pytest
import torch

from e2fgvi_amd import ops, video
from oracle import video_ref
from tests.test_video_driver import _toy_video
from tests.util import assert_bound, err

pytestmark = pytest.mark.gpu


def _net(model, dev, precision="fp32"):
    from e2fgvi_amd.synth import synth_state_dict
    sd = synth_state_dict(model, "stress", 0)
    net = importlib.import_module("model." + model).InpaintGenerator()
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    net.precision = precision
    return net, sd


# --------------------------------------------------------------------------- the gather / scatter kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("tail", [(15, 27, 128), (15, 27, 2), (60, 108, 2), (6, 10, 128)])
def test_gather_slabs_is_index_select(dev, dtype, tail):
    """both cache shapes (encoder [slots,h,w,128], flows [slots,h,w,2]; 15 x 27 x 2 fp32 slabs are 8-byte, bf16 ones 4-byte
    multiples: the narrower vector widths), repeated ids, a single id -- bit for bit"""
    g = torch.Generator().manual_seed(7)
    slots = 9
    cache = torch.randn((slots,) + tail, generator=g).to(dtype).to(dev)
    for ids in ([3, 0, 8, 3, 3, 1, 7], [5], list(range(slots))[::-1]):
        idx = torch.tensor(ids, dtype=torch.int32, device=dev)
        got = ops.gather_slabs(cache, idx)
        ref = torch.index_select(cache, 0, idx.long())
        assert got.dtype == dtype and tuple(got.shape) == (len(ids),) + tail
        assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8)), (dtype, tail, ids)
    # the mirror: distinct slots, the rest of the cache untouched
    rows = torch.randn((3,) + tail, generator=g).to(dtype).to(dev)
    idx = torch.tensor([6, 0, 2], dtype=torch.int32, device=dev)
    ref = cache.clone()
    ref[idx.long()] = rows
    ops.scatter_slabs(rows, idx, cache)
    assert torch.equal(cache.view(torch.uint8), ref.view(torch.uint8))


def test_gather_slabs_stays_in_bounds_and_checks_arguments(dev):
    cache = torch.arange(4 * 6, dtype=torch.float32, device=dev).view(4, 6)
    got = ops.gather_slabs(cache, torch.tensor([1, 4, -1, 3], dtype=torch.int32, device=dev))      # ids outside the cache: zeros
    assert torch.equal(got.cpu(), torch.stack([cache[1].cpu(), torch.zeros(6), torch.zeros(6), cache[3].cpu()]))
    with pytest.raises(TypeError):
        ops.gather_slabs(cache, torch.tensor([1], dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.scatter_slabs(torch.zeros((2, 5), device=dev), torch.tensor([0, 1], dtype=torch.int32, device=dev), cache)


# --------------------------------------------------------------------------- the engine's pieces
@pytest.mark.parametrize("model,hw,t,lt", [("e2fgvi", (240, 432), 10, 6), ("e2fgvi_hq", (120, 216), 6, 4)])
def test_engine_pieces_against_the_oracle(dev, model, hw, t, lt):
    """plain forward and the pieced path (encoder on the flat frames, flows of explicit pairs, forward given both, local-only
    decode), each against the ORACLE's first l_t output frames with test_gpu_model.test_end_to_end's bounds: max|d| <= 1e-3 and
    max|d| <= 2e-4 x rms"""
    from e2fgvi_amd.engine import Engine
    from e2fgvi_amd.synth import synth_clip, synth_state_dict
    from oracle import e2fgvi_oracle as O
    sd = synth_state_dict(model, "stress", 0)
    x, _ = synth_clip(1, t, hw[0], hw[1], seed=1, moving=True)
    ref, _ = O.forward(sd, x, lt, model)
    ref = ref[:lt]
    eng = Engine(sd, model, dev)
    xd = x.to(dev)
    with torch.no_grad():
        plain, _ = eng.forward(xd, lt, trace={})
        before = dict(eng.counters)
        enc = eng.encode_frames(xd[0])
        keep = enc.clone()
        fwd, bwd = eng.pair_flows(xd[0, :lt].contiguous(), eng.pair_table([(i, i + 1) for i in range(lt - 1)]))
        h, w = hw[0] // 4, hw[1] // 4
        given = ((fwd.reshape(1, lt - 1, h, w, 2), bwd.reshape(1, lt - 1, h, w, 2)), enc)
        pieced, _ = eng.forward(None, lt, given=given, decode_local=True)
        with pytest.raises(ValueError):
            eng.forward(xd.repeat(2, 1, 1, 1, 1), lt, decode_local=True)
    assert tuple(plain.shape) == (t, 3) + hw and tuple(pieced.shape) == (lt, 3) + hw
    assert {k: eng.counters[k] - before[k] for k in before} == {"encoder_frames": t, "flow_pairs": lt - 1, "decoder_frames": lt}
    # the in-place propagation trap: the given features are consumed (fp32: their local frames now hold propagated features)
    assert torch.equal(enc[lt:], keep[lt:]) and not torch.equal(enc[:lt], keep[:lt])
    for name, got in (("plain", plain[:lt]), ("pieced", pieced)):
        d, r = err(got, ref)
        print("engine pieces %s %s: max abs %.3e (%.2e x rms)" % (model, name, d, r))
        assert torch.isfinite(got).all()
        assert_bound(d, 1e-3, "reuse pieces %s %s output max abs" % (model, name))
        assert_bound(r, 2e-4, "reuse pieces %s %s output max abs / rms" % (model, name))


# --------------------------------------------------------------------------- the whole driver against the reference loop
@pytest.mark.parametrize("L", [11, 23])
def test_reuse_driver_matches_cpu_oracle(dev, L):
    """test_driver_on_gpu_matches_cpu_oracle's setup and condition with reuse=True; L = 23: frames recur in three windows and a
    slot is freed and handed out again (tests/test_video_reuse_plan.py).
    Measured on MI355X (profiles/video_reuse.txt): share of differing bytes with reuse off / on, both with max 1."""
    from oracle import e2fgvi_oracle as O
    frames, masks = _toy_video(L, 60, 100, seed=3)
    net, sd = _net("e2fgvi_hq", dev)
    dil = [video_ref.dilate_cross_np(m > 0, 4) for m in masks]
    ref = video_ref.run(lambda x, n: O.forward(sd, x, n, "e2fgvi_hq")[0], frames, dil, 5, 10, -1)
    for reuse in (False, True):
        out = video.inpaint_video(net, np.stack(frames), np.stack(masks), 5, 10, -1, reuse=reuse)
        d = np.abs(out.astype(int) - ref.astype(int))
        print("driver vs oracle L=%d reuse=%s: max %d, share of differing bytes %.5f" % (L, reuse, d.max(), (d > 0).mean()))
        assert d.max() <= 1 and (d > 0).mean() < 0.02, (reuse, d.max(), (d > 0).mean())


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_reuse_adds_no_error_beyond_the_precisions_own(dev, precision):
    """16-bit paths on the in-flight test's (120, 200), L = 23 input: reuse on against reuse off at the same precision may differ
    by at most what the plain driver at that precision differs from the plain fp32 driver on the same input (largest byte
    difference and share of differing bytes), both measured here."""
    frames, masks = _toy_video(23, 120, 200, seed=9)
    f, m = np.stack(frames), np.stack(masks)
    net, _ = _net("e2fgvi_hq", dev)
    base = video.inpaint_video(net, f, m, 5, 10, -1).astype(int)
    net.precision = precision
    off = video.inpaint_video(net, f, m, 5, 10, -1).astype(int)
    on = video.inpaint_video(net, f, m, 5, 10, -1, reuse=True).astype(int)
    own, added = np.abs(off - base), np.abs(on - off)
    print("%s: plain vs fp32 plain max %d share %.5f; reuse vs plain max %d share %.5f"
          % (precision, own.max(), (own > 0).mean(), added.max(), (added > 0).mean()))
    assert added.max() <= own.max() and (added > 0).mean() <= (own > 0).mean()


# --------------------------------------------------------------------------- the work that is saved, counted
def test_reuse_runs_every_frame_and_pair_once(dev):
    L = 36
    frames, masks = _toy_video(L, 60, 100, seed=4)
    net, _ = _net("e2fgvi_hq", dev)
    eng = net.engine()
    windows = video.plan_windows(L, 5, 10, -1)
    plan = video.plan_reuse(windows)

    def counted(**kw):
        before = dict(eng.counters)
        video.inpaint_video(net, np.stack(frames), np.stack(masks), 5, 10, -1, **kw)
        assert net.engine() is eng
        return {k: eng.counters[k] - before[k] for k in before}
    on = counted(reuse=True)
    assert on["encoder_frames"] == L
    assert on["flow_pairs"] == sum(len(p["pairs"]) for p in plan.windows) == L - 1
    assert on["decoder_frames"] == sum(len(nb) for nb, _ in windows)
    off = counted()
    total = sum(len(nb) + len(rf) for nb, rf in windows)
    assert off["encoder_frames"] == total and off["decoder_frames"] == total
    assert off["flow_pairs"] == sum(len(nb) - 1 for nb, _ in windows)


# --------------------------------------------------------------------------- no state between calls, any stream
def test_repeat_calls_and_a_callers_stream(dev):
    va = [np.stack(v) for v in _toy_video(23, 60, 100, seed=5)]
    vb = [np.stack(v) for v in _toy_video(17, 60, 100, seed=6)]
    fresh = []
    for v in (va, vb):
        net, _ = _net("e2fgvi_hq", dev)
        fresh.append(video.inpaint_video(net, v[0], v[1], 5, 10, -1, reuse=True))
    net, _ = _net("e2fgvi_hq", dev)
    a = video.inpaint_video(net, va[0], va[1], 5, 10, -1, reuse=True)
    b = video.inpaint_video(net, vb[0], vb[1], 5, 10, -1, reuse=True)
    a2 = video.inpaint_video(net, va[0], va[1], 5, 10, -1, reuse=True)
    assert np.array_equal(a, fresh[0]) and np.array_equal(b, fresh[1]) and np.array_equal(a2, fresh[0])
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        c = video.inpaint_video(net, va[0], va[1], 5, 10, -1, reuse=True)
    torch.cuda.current_stream(dev).wait_stream(st)
    assert np.array_equal(c, fresh[0])


def test_one_frame_video_and_options(dev):
    """l_t == 1 on a one-frame video, keep_float, pad and size= go through the reuse path as through the plain one"""
    net, _ = _net("e2fgvi_hq", dev)
    frames, masks = _toy_video(1, 60, 100, seed=2)
    one = video.inpaint_video(net, np.stack(frames), np.stack(masks), reuse=True)
    ref = video.inpaint_video(net, np.stack(frames), np.stack(masks))
    d = np.abs(one.astype(int) - ref.astype(int))
    assert one.shape == (1, 60, 100, 3) and d.max() <= 1 and (d > 0).mean() < 0.02
    frames, masks = _toy_video(7, 80, 130, seed=2)
    kw = dict(neighbor_stride=3, size=(100, 60), dilate=False)
    got = video.inpaint_video(net, np.stack(frames), np.stack(masks), keep_float=True, reuse=True, **kw)
    ref = video.inpaint_video(net, np.stack(frames), np.stack(masks), keep_float=True, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (7, 60, 100, 3)
    d = (got - ref).abs()
    assert d.max().item() <= 1 and (d > 0).float().mean().item() < 0.02


# --------------------------------------------------------------------------- mode combinations
def test_mode_combinations(dev):
    net, _ = _net("e2fgvi_hq", dev)
    frames, masks = _toy_video(12, 60, 100, seed=1)
    f, m = np.stack(frames), np.stack(masks)
    with pytest.raises(ValueError, match="in_flight"):            # refused, as inpaint_video's docstring says
        video.inpaint_video(net, f, m, reuse=True, in_flight=2)
    with pytest.raises(ValueError, match="batch_windows"):
        video.inpaint_video(net, f, m, reuse=True, batch_windows=2)
    with pytest.raises(TypeError):
        video.inpaint_video(lambda x, n: (x.reshape((-1,) + tuple(x.shape[2:])), None), f, m, device=dev, reuse=True)
