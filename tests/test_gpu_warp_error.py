"""E_warp on the device: the kernel (csrc/metrics.hip, e2fgvi_amd.metrics.warp_error) against the float64 reference of
tests/warp_error_cases.py on every case of that module, the flows at the frames' own size it is fed with
(Engine.pair_flows(downscale=1), metrics.video_flows) against the oracle's SPyNet, and metrics.evaluate_video(warp=True)."""
import numpy as np
import pytest
import torch

from tests import warp_error_cases as C
from tests.util import assert_close

pytestmark = pytest.mark.gpu

_CACHE = {}


def _run(dev, frames, c, valid="case"):
    from e2fgvi_amd import metrics
    va = c["valid"] if valid == "case" else valid
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)              # a copy: the cases are read-only
    out = metrics.warp_error(up(frames), up(c["fwd"]), up(c["bwd"]), None if va is None else up(va))
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(frames) - 1, 2) and out.device.type == "cuda"
    return out


def _compare(got, ref, what):
    """n exact, |e - ref| <= 1e-9 max(ref, 1e-12): the bound test_oracle_metrics.py holds the fp64 metrics to"""
    got = got.cpu().numpy()
    for t, r in enumerate(ref):
        print("%s pair %d: n %d (ref %d), e %.17g (ref %.17g)" % (what, t, got[t, 1], r["n"], got[t, 0], r["e"]))
    for t, r in enumerate(ref):
        assert np.isfinite(got[t]).all(), (what, t, got[t])
        assert got[t, 1] == r["n"], (what, t, got[t, 1], r["n"])
        assert abs(got[t, 0] - r["e"]) <= 1e-9 * max(r["e"], 1e-12), (what, t, got[t, 0], r["e"])


@pytest.mark.parametrize("u8", [False, True], ids=["float", "uint8"])
@pytest.mark.parametrize("name", C.NAMES)
def test_kernel_matches_reference(dev, name, u8):
    c = C.case(name)
    _compare(_run(dev, C.frames_u8(name) if u8 else c["frames"], c), C.case_reference(name, u8), "%s %s" % (name, "u8" if u8 else "f32"))


def test_nonfinite_and_huge_flows(dev):
    """finite output, the reference's n, and nothing from an excluded pixel: frame 0 is only ever the A of pair 0, so changing it
    under the pixels pair 0 drops must leave every bit of the result"""
    c = C.case("nonfinite")
    ref = C.case_reference("nonfinite")
    got = _run(dev, c["frames"], c)
    _compare(got, ref, "nonfinite")
    changed = c["frames"].copy()
    drop = ~ref[0]["keep"]
    assert drop.sum() > 20
    changed[0][drop] = 255.0 - changed[0][drop]
    again = _run(dev, changed, c)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    # flows that are non-finite everywhere: nothing is kept, the result is 0 over 0 pixels, not nan
    allbad = dict(c, fwd=np.full_like(c["fwd"], np.nan), bwd=np.full_like(c["bwd"], np.inf))
    assert torch.equal(_run(dev, c["frames"], allbad).cpu(), torch.zeros(2, 2, dtype=torch.float64))
    huge = dict(c, fwd=np.full_like(c["fwd"], -1e30), bwd=np.full_like(c["bwd"], 1e30))
    assert torch.equal(_run(dev, c["frames"], huge).cpu(), torch.zeros(2, 2, dtype=torch.float64))


def test_same_bits_every_run_and_on_a_side_stream(dev):
    for name in ("eval_70x90", "smooth_17x300"):
        c = C.case(name)
        first = _run(dev, c["frames"], c)
        assert torch.equal(first.view(torch.int64), _run(dev, c["frames"], c).view(torch.int64))
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            other = _run(dev, c["frames"], c)
        side.synchronize()
        assert torch.equal(first.view(torch.int64), other.view(torch.int64))


def test_host_inputs_are_uploaded(dev):
    from e2fgvi_amd import metrics
    c = C.case("smooth_7x5")
    out = metrics.warp_error(np.array(c["frames"]), np.array(c["fwd"]), np.array(c["bwd"]))      # copies: the cases are read-only
    _compare(out, C.case_reference("smooth_7x5"), "host inputs")
    assert metrics.warp_score(out) == pytest.approx(np.mean([r["e"] for r in C.case_reference("smooth_7x5")]), rel=1e-9)


def test_argument_errors(dev):
    from e2fgvi_amd import lib, metrics
    c = C.case("smooth_7x5")
    fr, fw, bw = (torch.from_numpy(c[k].copy()).to(dev) for k in ("frames", "fwd", "bwd"))
    with pytest.raises(ValueError):
        metrics.warp_error(fr[:1], fw[:0], bw[:0])                                    # L = 1
    with pytest.raises(ValueError):
        metrics.warp_error(fr, fw[:1], bw)                                            # one flow short
    with pytest.raises(ValueError):
        metrics.warp_error(fr, fw, bw[:, :, :4].contiguous())                         # another width
    with pytest.raises(ValueError):
        metrics.warp_error(fr[..., :2].contiguous(), fw, bw)                          # not 3 channels
    with pytest.raises(ValueError):
        metrics.warp_error(fr, fw, bw, torch.ones((3, 7, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        metrics.warp_error(fr.permute(0, 2, 1, 3), fw.permute(0, 2, 1, 3), bw.permute(0, 2, 1, 3))     # non-contiguous
    with pytest.raises(ValueError):
        metrics.warp_error(fr.double(), fw, bw)
    with pytest.raises(ValueError):
        metrics.warp_error(fr, fw.double(), bw)
    with pytest.raises(ValueError):
        metrics.warp_error(fr, fw, bw.half())
    with pytest.raises(ValueError):
        metrics.warp_error(fr, fw, bw, torch.ones((3, 7, 5), dtype=torch.float32, device=dev))
    # the C entry's own checks
    L = lib.load()
    assert L.e2fgvi_warp_error_workspace(1, 7, 5) < 0 and L.e2fgvi_warp_error_workspace(3, 0, 5) < 0
    assert L.e2fgvi_warp_error_workspace(3, 7, 5) == 2 * 2 * 1 * 8
    work = torch.empty(64, dtype=torch.float64, device=dev)
    out = torch.empty((2, 2), dtype=torch.float64, device=dev)
    p = lambda t: t.data_ptr()
    assert L.e2fgvi_warp_error(p(fr), lib.DT_F32, p(fw), p(bw), None, 1, 7, 5, p(work), p(out), None) == -1
    assert L.e2fgvi_warp_error(p(fr), lib.DT_F32, p(fw), p(bw), None, 3, 7, -5, p(work), p(out), None) == -1
    assert L.e2fgvi_warp_error(None, lib.DT_F32, p(fw), p(bw), None, 3, 7, 5, p(work), p(out), None) == -1
    assert L.e2fgvi_warp_error(p(fr), lib.DT_F32, p(fw), p(bw), None, 3, 7, 5, p(work) + 4, p(out), None) == -1
    assert b"aligned" in L.e2fgvi_last_error()
    assert L.e2fgvi_warp_error(p(fr), lib.DT_BF16, p(fw), p(bw), None, 3, 7, 5, p(work), p(out), None) == -1


# ------------------------------------------------------------------------------------------------ flows at the frames' own size
def _engine(kind, dev):
    if ("eng", kind) not in _CACHE:
        from e2fgvi_amd.engine import Engine
        from e2fgvi_amd.synth import synth_state_dict
        sd = synth_state_dict("e2fgvi", kind, 0)
        _CACHE["eng", kind] = (sd, Engine(sd, "e2fgvi", dev))
    return _CACHE["eng", kind]


@pytest.mark.parametrize("hw", [(40, 72), (64, 96)])           # (40, 72): resized to 64 x 96 inside SPyNet
@pytest.mark.parametrize("kind", ["stress", "peaked"])
def test_pair_flows_at_full_size(dev, kind, hw):
    from e2fgvi_amd.synth import synth_clip
    from oracle import e2fgvi_oracle as O
    sd, eng = _engine(kind, dev)
    x, _ = synth_clip(1, 3, hw[0], hw[1], seed=2, moving=True)
    fr = x[0].contiguous()                                      # [3,3,H,W] in [-1,1]
    pairs = eng.pair_table([(0, 1), (1, 2)])
    with torch.no_grad():
        fwd, bwd = eng.pair_flows(fr.to(dev), pairs, downscale=1)
        f01 = fr * 0.5 + 0.5
        rf = O.spynet(sd, "update_spynet.", f01[:-1], f01[1:])
        rb = O.spynet(sd, "update_spynet.", f01[1:], f01[:-1])
    assert tuple(fwd.shape) == (2,) + hw + (2,) and tuple(bwd.shape) == (2,) + hw + (2,)
    assert_close(fwd.cpu().permute(0, 3, 1, 2), rf, 1e-3, "full-size flow fwd %s %s" % (kind, hw))
    assert_close(bwd.cpu().permute(0, 3, 1, 2), rb, 1e-3, "full-size flow bwd %s %s" % (kind, hw))


def test_pair_flows_downscale_argument(dev):
    from e2fgvi_amd.synth import synth_clip
    _, eng = _engine("stress", dev)
    x, _ = synth_clip(1, 3, 64, 96, seed=2, moving=True)
    fr = x[0].contiguous().to(dev)
    pairs = eng.pair_table([(0, 1), (1, 2)])
    a = eng.pair_flows(fr, pairs)
    b = eng.pair_flows(fr, pairs, downscale=4)
    assert tuple(a[0].shape) == (2, 16, 24, 2)
    for u, v in zip(a, b):
        assert torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))
    for bad in (2, 0, 8, None):
        with pytest.raises(ValueError):
            eng.pair_flows(fr, pairs, downscale=bad)


def test_video_flows(dev):
    import importlib
    from e2fgvi_amd import metrics
    from e2fgvi_amd.synth import synth_clip, synth_state_dict
    from oracle import e2fgvi_oracle as O
    sd = synth_state_dict("e2fgvi", "stress", 0)
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    x, _ = synth_clip(1, 6, 40, 72, seed=4, moving=True)
    frames = ((x[0] * 0.5 + 0.5) * 255).round().clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()      # [6,40,72,3]
    with torch.no_grad():
        f1, b1 = metrics.video_flows(net, frames, chunk=1)
        f4, b4 = metrics.video_flows(net, frames, chunk=4)
        f01 = torch.from_numpy(frames).permute(0, 3, 1, 2).float() / 255
        rf = O.spynet(sd, "update_spynet.", f01[:-1], f01[1:])
    assert tuple(f1.shape) == (5, 40, 72, 2) and f1.dtype == torch.float32 and f1.is_cuda
    assert torch.equal(f1.view(torch.int32), f4.view(torch.int32)) and torch.equal(b1.view(torch.int32), b4.view(torch.int32))
    assert_close(f4.cpu().permute(0, 3, 1, 2), rf, 1e-3, "video_flows fwd")
    with pytest.raises(TypeError):
        metrics.video_flows(lambda x, n: (x, None), frames)


# ------------------------------------------------------------------------------------------------ evaluate_video
def test_evaluate_video_with_warp(dev):
    """test_evaluate_video_matches_reference_loop's video and stand-in model: the default call is unchanged, warp=True adds the
    reference's E_warp rows of the reference loop's blended float frames under the given flows"""
    from e2fgvi_amd import metrics
    from oracle import metrics_ref, video_ref
    rng = np.random.RandomState(5)
    L, h, w = 13, 70, 90
    frames = [np.clip(rng.randint(0, 256, (h, w, 3)) * 0.3 + 90 + 20 * i, 0, 255).astype(np.uint8) for i in range(L)]
    masks = [np.zeros((h, w), np.uint8) for _ in range(L)]
    for i, m in enumerate(masks):
        m[20 + i:45 + i, 30:60] = 1
    fake = lambda x, n: torch.tanh(x.reshape(-1, 3, h, w) * 0.6)
    model = lambda x, n: (fake(x.cpu(), n).to(dev), None)
    ref_comp = video_ref.run(fake, frames, masks, 5, 10, -1, pad=False, as_float=True)
    ref = np.array([metrics_ref.calc_psnr_and_ssim(o, c, 65) for o, c in zip(frames, ref_comp)])
    c = C.case("eval_70x90")
    plain = metrics.evaluate_video(model, np.stack(frames), np.stack(masks))
    assert isinstance(plain, tuple) and len(plain) == 2
    assert np.abs(plain[0] - ref[:, 0]).max() <= 1e-9 * ref[:, 0].max() and np.abs(plain[1] - ref[:, 1]).max() <= 1e-9
    flows = (torch.from_numpy(c["fwd"].copy()).to(dev), torch.from_numpy(c["bwd"].copy()).to(dev))
    psnr, ssim, warp = metrics.evaluate_video(model, np.stack(frames), np.stack(masks), warp=True, flows=flows)
    assert np.array_equal(psnr, plain[0]) and np.array_equal(ssim, plain[1])
    assert isinstance(warp, np.ndarray) and warp.shape == (L - 1, 2) and warp.dtype == np.float64
    comp = np.stack([np.asarray(f, np.float32) for f in ref_comp])
    want = C.reference(comp, c["fwd"], c["bwd"])
    assert min(r["margin"] for r in want) >= 1e-9
    _compare(torch.from_numpy(warp), want, "evaluate_video warp")
    with pytest.raises(TypeError):
        metrics.evaluate_video(model, np.stack(frames), np.stack(masks), warp=True)     # no flows and no engine to make them
