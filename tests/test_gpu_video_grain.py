"""Film grain on the device: ops.grain_blocks, ops.grain_lut and ops.grain_apply (csrc/grain.hip) and video.match_grain against
the numpy restatement of tests/grain_cases.py, every int32 entry and every byte equal, on every named case; buffers 0 and 1 byte
off an allocation's start; outputs pre-filled; in place; reruns; scenes=, hole=, levels= and return_levels; the launches of a
call; and the composition with paste_mask."""
import numpy as np
import pytest
import torch

from e2fgvi_amd import ops, video
from tests import grain_cases as G
from tests.util import launch_trace

pytestmark = pytest.mark.gpu

GRAIN_SYMBOLS = ("e2fgvi_grain_blocks", "e2fgvi_grain_apply")


def _up(a, dev, shift=0):
    """the array on the device, its first byte `shift` bytes behind an allocation's start"""
    a = np.array(a)                                     # a writable copy: the cases are read-only
    buf = torch.zeros(a.nbytes + shift, dtype=torch.uint8, device=dev)
    return buf[shift:].view(torch.from_numpy(a).dtype).view(a.shape).copy_(torch.from_numpy(a))


# ------------------------------------------------------------------------------------------------ the entries
@pytest.mark.parametrize("name", G.NAMES)
def test_entries_are_the_restatement(dev, name):
    c, w = G.case(name), G.want(name)
    L, H, W = c["L"], c["H"], c["W"]
    so = _up(c["scene_of"], dev)
    for shift in (0, 1):
        fr, ho = _up(c["frames"], dev, shift), _up(c["hole"], dev, shift) if c["hole"] is not None else None
        energy, band = ops.grain_blocks(fr, ho)
        assert energy.dtype == torch.int32 and band.dtype == torch.uint8
        assert energy.shape == w["energy"].shape and band.shape == w["band"].shape
        assert np.array_equal(energy.cpu().numpy(), w["energy"]), int((energy.cpu().numpy() != w["energy"]).sum())
        assert np.array_equal(band.cpu().numpy(), w["band"]), int((band.cpu().numpy() != w["band"]).sum())
        lut, scale = ops.grain_lut(energy, band, so, c["n_scenes"], c["strength_q8"])
        assert lut.dtype == scale.dtype == torch.int32 and lut.shape == (c["n_scenes"], 256, 3)
        assert np.array_equal(scale.cpu().numpy(), w["scale"]) and np.array_equal(lut.cpu().numpy(), w["lut"])
        fl, wh = _up(c["filled"], dev, shift), _up(c["where"], dev, shift)
        for table, want in ((lut, w["out"]), (_up(c["alt_lut"], dev), w["alt_out"])):
            # every byte is written: the output starts as 77s
            out = ops.grain_apply(fl, wh, table, so, c["seed"], out=_up(np.full((L, H, W, 3), 77, np.uint8), dev, shift))
            got = out.cpu().numpy()
            assert np.array_equal(got, want), int((got != want).sum())
            assert torch.equal(fl, _up(c["filled"], dev))                                   # filled is only read
            assert torch.equal(ops.grain_apply(fl, wh, table, so, c["seed"]), out)           # a buffer of its own; a rerun
            # in place equals out of place
            same = _up(c["filled"], dev, shift)
            assert ops.grain_apply(same, wh, table, so, c["seed"], out=same) is same and torch.equal(same, out)
    # without a hole plane
    energy, band = ops.grain_blocks(_up(c["frames"], dev))
    want_e, want_b = G.blocks_np(c["frames"])
    assert np.array_equal(energy.cpu().numpy(), want_e) and np.array_equal(band.cpu().numpy(), want_b)
    print(name, "blocks", tuple(band.shape), "measured", int((w["band"] != 255).sum()), "bytes changed", int((w["out"] != c["filled"]).sum()),
          int((w["alt_out"] != c["filled"]).sum()))


@pytest.mark.parametrize("name", G.LEVEL_NAMES)
def test_levels_are_the_restatement(dev, name):
    c = G.level_case(name)
    lut, scale = ops.grain_lut(_up(c["energy"], dev), _up(c["band"], dev), _up(c["scene_of"], dev), c["n_scenes"], c["strength_q8"])
    assert np.array_equal(scale.cpu().numpy(), c["levels"]["scale"]) and np.array_equal(lut.cpu().numpy(), c["lut"])
    assert lut.shape == (c["n_scenes"], 256, 3) and lut.dtype == torch.int32
    for q8 in (0, 1, 255, 1024):
        got = ops.grain_lut_from_scale(scale, q8)
        assert np.array_equal(got.cpu().numpy(), G.lut_np(c["levels"]["scale"], q8))
    # host arrays are uploaded; no scene at all
    lut, scale = ops.grain_lut(np.array(c["energy"]), np.array(c["band"]), np.array(c["scene_of"]), 0)
    assert lut.is_cuda and lut.shape == (0, 256, 3) and scale.shape == (0, 8, 3)


def test_the_table_caps_and_the_isqrt_is_exact(dev):
    big = torch.full((1, 8, 3), 2 ** 21, dtype=torch.int64, device=dev)
    assert (ops.grain_lut_from_scale(big, 1024) == ops.GRAIN_SCALE_MAX).all()
    # one scene of 32 blocks whose energy sweeps values around perfect squares of the scale's argument
    for e in (0, 1, 112, 113, 20479, 20480, 66585600, 12345678):
        energy = torch.full((1, 4, 8, 3), e, dtype=torch.int32, device=dev)
        band = torch.full((1, 4, 8), 3, dtype=torch.uint8, device=dev)
        scale = ops.grain_lut(energy, band, torch.zeros(1, dtype=torch.int32, device=dev), 1)[1]
        want = G.levels_np(energy.cpu().numpy(), band.cpu().numpy(), [0], 1)["scale"]
        assert np.array_equal(scale.cpu().numpy(), want), e


def test_both_clamps_under_strong_grain(dev):
    filled, where, scale, scene_of, seed = G.saturation_case()
    for strength in (0.5, 4):
        q8 = G.q8_of(strength)
        lut = ops.grain_lut_from_scale(_up(scale, dev), q8)
        want = G.apply_np(filled, where, G.lut_np(scale, q8), scene_of, seed)
        assert np.array_equal(lut.cpu().numpy(), G.lut_np(scale, q8)) and (want == 0).any() and (want == 255).any()
        assert np.array_equal(ops.grain_apply(filled, where, lut, scene_of, seed).cpu().numpy(), want)
        assert np.array_equal(video.match_grain(None, filled, where, levels=np.full((8, 3), 40.0), strength=strength, seed=seed, device=dev),
                              want)


def test_runs_are_the_same_bits(dev):
    c, w = G.case("bands_66x70"), G.want("bands_66x70")
    fr, fl, wh, so = (_up(c[k], dev) for k in ("frames", "filled", "where", "scene_of"))
    for _ in range(5):
        energy, band = ops.grain_blocks(fr)
        lut, _ = ops.grain_lut(energy, band, so, 1, c["strength_q8"])
        assert np.array_equal(ops.grain_apply(fl, wh, lut, so, c["seed"]).cpu().numpy(), w["out"])


def test_arguments_are_checked(dev):
    c, w = G.case("odd_19x27"), G.want("odd_19x27")
    fr, ho, fl, wh, so = (_up(c[k], dev) for k in ("frames", "hole", "filled", "where", "scene_of"))
    lut = _up(c["alt_lut"], dev)
    got = ops.grain_blocks(np.array(c["frames"]), np.array(c["hole"]))              # host inputs are uploaded
    assert got[0].is_cuda and np.array_equal(got[1].cpu().numpy(), w["band"])
    for kw, what in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[0]), "frames"), (dict(frames=fr[..., :2]), "contiguous"),
                     (dict(hole=ho.int()), "hole"), (dict(hole=ho[:1]), "hole"), (dict(hole=ho[:, :, ::2]), "contiguous")):
        with pytest.raises(ValueError, match=what):
            ops.grain_blocks(**dict(dict(frames=fr, hole=ho), **kw))
    energy, band = _up(w["energy"], dev), _up(w["band"], dev)
    for kw, what in ((dict(energy=energy.long()), "energy"), (dict(energy=energy[0]), "energy"), (dict(band=band.int()), "band"),
                     (dict(band=band[:1]), "band"), (dict(scene_of=so.long()), "scene_of"), (dict(scene_of=so[:1]), "scene_of"),
                     (dict(n_scenes=-1), "n_scenes"), (dict(n_scenes=1.5), "n_scenes"), (dict(strength_q8=1025), "strength_q8"),
                     (dict(strength_q8=-1), "strength_q8"), (dict(strength_q8=True), "strength_q8")):
        with pytest.raises(ValueError, match=what):
            ops.grain_lut(**dict(dict(energy=energy, band=band, scene_of=so, n_scenes=1), **kw))
    for bad in (lut.float(), lut[0], lut.cpu(), np.zeros((1, 8, 3))):
        with pytest.raises(ValueError, match="scale"):
            ops.grain_lut_from_scale(bad)
    for kw, what in ((dict(filled=fl.float()), "filled"), (dict(filled=fl[0]), "filled"), (dict(where=wh.int()), "where"),
                     (dict(where=wh[:, :, :5]), "contiguous"), (dict(where=wh[:1]), "where"), (dict(lut=lut.long()), "lut"),
                     (dict(lut=lut[:, :255].contiguous()), "lut"), (dict(scene_of=so.float()), "scene_of"), (dict(scene_of=so[:1]), "scene_of"),
                     (dict(seed=-1), "seed"), (dict(seed=2 ** 32), "seed"), (dict(seed=1.0), "seed"), (dict(seed=False), "seed"),
                     (dict(out=np.zeros(c["filled"].shape, np.uint8)), "out"), (dict(out=fl[:1].clone()), "out"),
                     (dict(out=torch.zeros(fl.shape, dtype=torch.int32, device=dev)), "out")):
        with pytest.raises(ValueError, match=what):
            ops.grain_apply(**dict(dict(filled=fl, where=wh, lut=lut, scene_of=so, seed=0), **kw))
    # a table without a scene: every frame is outside, the bytes are filled's
    none = torch.zeros((0, 256, 3), dtype=torch.int32, device=dev)
    assert torch.equal(ops.grain_apply(fl, wh, none, so, 0), fl)


# ------------------------------------------------------------------------------------------------ match_grain
def _grainy(L, H, W, seed, sigmas):
    """a grey ramp with Gaussian noise, the sigma of frame t is sigmas[t]; and the grainless ramp"""
    rng = np.random.RandomState(seed)
    base = G.ramp(L, H, W)
    s = np.asarray(sigmas, np.float64)[:, None, None, None]
    return (np.clip(np.rint(base + s * rng.randn(L, H, W, 3)), 1, 254).astype(np.uint8), np.clip(np.rint(base), 0, 255).astype(np.uint8))


def test_match_grain_is_the_restatement(dev):
    L, H, W = 4, 66, 78
    fr, fl = _grainy(L, H, W, 1, [3, 3, 8, 8])
    where = np.zeros((L, H, W), np.uint8)
    where[:, 20:50, 11:60] = 1
    hole = np.zeros_like(where)
    hole[:, 24:40, 30:50] = 255
    lv = np.linspace(0.5, 9, 24).reshape(8, 3)
    for kw in (dict(hole=hole), dict(hole=hole, scenes=[2]), dict(scenes=[2], strength=2.5, seed=2 ** 32 - 1), dict(hole=where.astype(bool)),
               dict(levels=lv), dict(levels=np.stack([lv, 2 * lv]), scenes=[1], strength=0.5), dict(hole=hole, scenes=[1, 2, 3])):
        want, want_sigma = G.match_np(fr, fl, where, **kw)
        with launch_trace() as trace:
            got = video.match_grain(fr, fl, where, device=dev, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want), (kw.keys(), int((got != want).sum()))
        n = [sum(r["symbol"] == s for r in trace) for s in GRAIN_SYMBOLS]
        assert n == ([0, 1] if "levels" in kw else [1, 1]) and len(trace) == sum(n), [r["symbol"] for r in trace]
        out, sigma = video.match_grain(fr, fl, where, device=dev, return_levels=True, **kw)
        assert np.array_equal(out, want) and sigma.dtype == np.float64 and np.array_equal(sigma, want_sigma)
        assert np.array_equal(got[where == 0], fl[where == 0])
        print(sorted(kw), "changed", int((got != fl).sum()), "sigma green", np.round(sigma[:, :, 1], 2).tolist())
    # frames may be None with levels=; where may be a bool plane
    want = G.match_np(None, fl, where, levels=lv, seed=3)[0]
    assert np.array_equal(video.match_grain(None, fl, where.astype(bool), levels=lv, seed=3, device=dev), want) and (want != fl).any()
    # hole=None means where: the scene with every block in the hole's footprint is returned unchanged
    everywhere = np.ones((L, H, W), np.uint8)
    assert np.array_equal(video.match_grain(fr, fl, everywhere, device=dev), fl)
    # tensor in, tensor out: filled is not written, sigma comes back on the device
    fl_d, fr_d, wh_d = (torch.from_numpy(a).to(dev) for a in (fl, fr, where))
    want, want_sigma = G.match_np(fr, fl, where, hole=hole, scenes=[2], seed=9)
    out, sigma = video.match_grain(fr_d, fl_d, wh_d != 0, hole=torch.from_numpy(hole).to(dev), scenes=[2], seed=9, return_levels=True)
    assert out.is_cuda and sigma.is_cuda and sigma.dtype == torch.float64 and out.data_ptr() != fl_d.data_ptr()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(sigma.cpu().numpy(), want_sigma)
    assert np.array_equal(fl_d.cpu().numpy(), fl)
    assert torch.equal(video.match_grain(fr_d, fl_d, wh_d, hole=torch.from_numpy(hole).to(dev), scenes=[2], seed=9), out)


def test_a_plain_call_is_two_launches_and_an_idle_one_none(dev):
    L, H, W = 3, 34, 42
    fr, fl = _grainy(L, H, W, 2, [4, 4, 4])
    where = np.zeros((L, H, W), np.uint8)
    where[1, 5:9, 7:30] = 1
    hole = np.zeros_like(where)
    with launch_trace() as trace:
        got = video.match_grain(fr, fl, where, hole=hole, device=dev)
    assert [r["symbol"] for r in trace] == list(GRAIN_SYMBOLS)
    assert np.array_equal(got, G.match_np(fr, fl, where, hole=hole)[0]) and (got != fl).any()
    for kw, f, m in ((dict(strength=0), fl, where), (dict(), fl, hole), (dict(), fl[:0], where[:0])):
        with launch_trace() as trace:
            got = video.match_grain(fr[:f.shape[0]], f, m, hole=hole[:f.shape[0]], device=dev, **kw)
        assert not trace and got.shape == f.shape and np.array_equal(got, f)
    # with return_levels the measurement still runs, and only that
    with launch_trace() as trace:
        got, sigma = video.match_grain(fr, fl, where, hole=hole, strength=0, return_levels=True, device=dev)
    assert [r["symbol"] for r in trace] == list(GRAIN_SYMBOLS[:1]) and np.array_equal(got, fl)
    assert np.array_equal(sigma, G.match_np(fr, fl, where, hole=hole)[1]) and (np.abs(sigma[0, 1:6] - 4) < 1).all()


def test_composition_with_the_paste_mask(dev):
    """where = paste_mask(...) from real masks: no byte outside the paste changes, some unsaturated byte inside it does"""
    L, H, W = 3, 64, 96
    fr, fl = _grainy(L, H, W, 3, [5, 5, 5])
    fl = fl.copy()
    fl[:, 28:34, 40:50] = 255                           # a saturated patch inside the paste
    masks = np.zeros((L, 32, 48), np.uint8)
    masks[:, 12:20, 16:30] = 255
    paste = video.paste_mask(masks, (H, W), (48, 32), device=dev)
    p = paste.cpu().numpy() != 0
    assert 0 < p.mean() < 0.5 and p[:, 28:34, 40:50].all()
    out = video.match_grain(fr, fl, paste, device=dev)
    assert np.array_equal(out, G.match_np(fr, fl, p.astype(np.uint8))[0])
    assert np.array_equal(out[~p], fl[~p])
    inside = p[..., None] & (fl > 0) & (fl < 255)
    assert (out[inside] != fl[inside]).any()
    print("paste pixels", int(p.sum()), "bytes changed", int((out != fl).sum()), "of", int(inside.sum()))
