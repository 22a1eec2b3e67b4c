"""Film grain, host side: the numpy restatement (tests/grain_cases.py) against what the feature is for -- the level it reads is the
sigma that was put in, and a grainless fill regrained by it reads like its surroundings --, the statistics of the counter-based
noise, every rule of the levels on the named cases, the argument checks of video.match_grain that need no device, and the header,
the binding and the C entries' error paths on the loaded library.  The kernels and the driver are compared with the restatement in
tests/test_gpu_video_grain.py."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import grain_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ what the feature is for
@pytest.mark.parametrize("sigma", [3, 6, 10])
def test_the_level_read_is_the_sigma_put_in(sigma):
    """flat grey plus Gaussian noise: the band's level is sigma within 5 % (the raw quartile reads 0.91-0.94 sigma; 19 / 16 undoes it)"""
    for seed in (0, 1, 2):
        fr = G.noisy_flat(sigma, seed)
        energy, band = G.blocks_np(fr)
        lv = G.levels_np(energy, band, np.zeros(fr.shape[0], np.int32), 1)
        k = int(np.argmax(lv["count"][0]))
        got = G.sigma_of(lv["scale"][0, k])
        print("sigma", sigma, "seed", seed, "band", k, "blocks", int(lv["count"][0, k]), "reads", np.round(got / sigma, 4).tolist())
        assert lv["count"][0, k] >= G.MIN_BLOCKS and (np.abs(got / sigma - 1) < 0.05).all()


@pytest.mark.parametrize("sigma", [3, 6])
def test_a_regrained_fill_reads_like_its_source(sigma):
    """closure: a smooth ramp with Gaussian noise is the source, the grainless ramp the fill, ``where`` everywhere; the regrained
    fill, measured the same way, reads the source's level in every band that has its 32 blocks, within 5 %"""
    L, H, W = 4, 120, 216
    base = G.ramp(L, H, W)
    src = np.clip(np.rint(base + sigma * np.random.RandomState(5).randn(L, H, W, 3)), 0, 255).astype(np.uint8)
    fill = np.clip(np.rint(base), 0, 255).astype(np.uint8)
    out, _ = G.match_np(src, fill, np.ones((L, H, W), np.uint8), hole=np.zeros((L, H, W), np.uint8), seed=11)
    scene = np.zeros(L, np.int32)
    raw = [G.levels_np(*G.blocks_np(v), scene, 1, borrow=False, clamp=False) for v in (src, out)]
    assert np.array_equal(raw[0]["count"], raw[1]["count"])
    bands = [k for k in range(8) if raw[0]["count"][0, k] >= G.MIN_BLOCKS]
    ratio = G.sigma_of(raw[1]["scale"][0, bands]) / G.sigma_of(raw[0]["scale"][0, bands])
    print("sigma", sigma, "bands", bands, "regrained / source", np.round(ratio, 4).tolist())
    assert len(bands) >= 5 and (np.abs(ratio - 1) < 0.05).all()
    # the fill itself has no grain to speak of: the closure is the synthesis' doing
    flat = G.levels_np(*G.blocks_np(fill), scene, 1, borrow=False, clamp=False)
    assert (G.sigma_of(flat["scale"][0, bands]) < 0.5).all()


def test_the_noise_is_white_and_has_the_stated_variance():
    n = G.noise_np(0, 0, 240, 432).astype(np.float64)
    lag_x = np.corrcoef(n[:, :-1].ravel(), n[:, 1:].ravel())[0, 1]
    lag_y = np.corrcoef(n[:-1].ravel(), n[1:].ravel())[0, 1]
    lag_c = np.corrcoef(n[..., :-1].ravel(), n[..., 1:].ravel())[0, 1]
    print("mean %.3f  sd %.2f  lag-1 x %.4f y %.4f channel %.4f" % (n.mean(), n.std(), lag_x, lag_y, lag_c))
    assert abs(n.mean()) < 1 and abs(n.var() / G.NOISE_VAR - 1) < 0.01 and max(abs(lag_x), abs(lag_y), abs(lag_c)) < 0.01
    assert n.min() >= -510 and n.max() <= 510
    # the variance of the sum of four independent bytes, exactly
    assert 4 * (256 ** 2 - 1) // 12 == G.NOISE_VAR and (2 ** 32 - 1) // G.NOISE_VAR == 196611
    small = G.noise_np(7, 3, 9, 11)
    assert np.array_equal(small, G.noise_np(7, 3, 9, 11))                                       # the same seed repeats
    assert (small != G.noise_np(7, 4, 9, 11)).mean() > 0.9 and (small != G.noise_np(8, 3, 9, 11)).mean() > 0.9
    assert (small[..., 0] != small[..., 1]).mean() > 0.9                                         # channels differ
    # the finaliser, by hand for one value: x = 1
    x = 1
    x ^= x >> 16; x = x * 0x7feb352d & G.M32; x ^= x >> 15; x = x * 0x846ca68b & G.M32; x ^= x >> 16
    assert int(G.mix(1)) == x
    # the pixel counter wraps at 2^32 like the device's unsigned arithmetic
    h = int(G.mix(int(G.mix((5 + 0x9E3779B9 * 2) & G.M32)) ^ (((3 * 7 + 4) * 3 + 1) & G.M32)))
    assert G.noise_np(5, 2, 4, 7)[3, 4, 1] == sum((h >> s) & 255 for s in (0, 8, 16, 24)) - 510


# ------------------------------------------------------------------------------------------------ the blocks
def test_blocks_by_hand():
    """one block, every sum written out pixel by pixel"""
    c = G.case("one_10x10")
    f = c["frames"][0].astype(np.int64)
    e = np.zeros(3, np.int64)
    ysum, clipped = 0, False
    for y in range(1, 9):
        for x in range(1, 9):
            for ch in range(3):
                r = 4 * f[y, x, ch] - f[y, x - 1, ch] - f[y, x + 1, ch] - f[y - 1, x, ch] - f[y + 1, x, ch]
                e[ch] += r * r
                clipped |= f[y, x, ch] in (0, 255)
            ysum += (77 * f[y, x, 0] + 150 * f[y, x, 1] + 29 * f[y, x, 2] + 128) >> 8
    energy, band = G.blocks_np(c["frames"])
    assert energy.shape == (1, 1, 1, 3) and band.shape == (1, 1, 1) and energy.dtype == np.int32 and band.dtype == np.uint8
    assert np.array_equal(energy[0, 0, 0], e) and band[0, 0, 0] == (255 if clipped else (ysum >> 6) >> 5)
    for shape, want in (((2, 9, 30, 3), (2, 0, 3)), ((1, 10, 9, 3), (1, 1, 0)), ((0, 20, 20, 3), (0, 2, 2)), ((1, 2, 1, 3), (1, 0, 0))):
        energy, band = G.blocks_np(np.zeros(shape, np.uint8))
        assert band.shape == want and energy.shape == want + (3,)
    # the largest energy there is fits int32
    worst = np.zeros((1, 10, 10, 3), np.uint8)
    worst[0, (np.arange(10)[:, None] + np.arange(10)[None]) % 2 == 0] = 255
    assert G.blocks_np(worst)[0].max() == 64 * 1020 ** 2 < 2 ** 31


def test_block_validity():
    c = G.case("validity_26x34")
    energy, band = G.blocks_np(c["frames"], c["hole"])
    bad = {(int(a), int(b)) for a, b in zip(*np.nonzero(band[0] == 255))}
    assert bad == G.VALIDITY_WANT_BAD
    # without the hole plane only the clipped bytes inside a block count; the ring's 0 and 255 never do
    _, plain = G.blocks_np(c["frames"])
    assert {(int(a), int(b)) for a, b in zip(*np.nonzero(plain[0] == 255))} == {(0, 3), (2, 0)}
    # one pixel outside a block is in its footprint, two pixels are not: walk a hole pixel away from block (1,2) = y 9..16, x 17..24
    for (y, x), out in (((16, 24), True), ((17, 25), True), ((18, 25), False), ((17, 26), False), ((8, 16), True), ((7, 16), False),
                        ((8, 15), False)):
        hole = np.zeros((1, 26, 34), np.uint8)
        hole[0, y, x] = 3
        assert (G.blocks_np(c["frames"], hole)[1][0, 1, 2] == 255) == out, (y, x)
    # the energy does not depend on the validity
    assert np.array_equal(energy, G.blocks_np(c["frames"])[0])


def test_band_boundaries():
    assert tuple(G.want("edges_10x42")["band"][0, 0]) == G.EDGES_WANT_BAND
    w = G.want("bands_66x70")
    assert set(np.unique(w["band"]).tolist()) == {0, 2, 5}


# ------------------------------------------------------------------------------------------------ the levels
def test_rules_of_the_levels():
    c = G.level_case("rules")
    lv = c["levels"]
    assert lv["count"][0].tolist() == [0, 31, 32, 0, 0, 0, 40, 33] and lv["total"].tolist() == [136, 50, 0]
    energy, band = c["energy"].astype(np.int64), c["band"]
    for ch in range(3):
        mine = lambda k: G.quartile(energy[:3][band[:3] == k][:, ch])
        g = G.quartile(energy[:3][band[:3] != 255][:, ch])
        assert lv["G"][0, ch] == g
        e2 = mine(2)
        assert g >> 2 <= e2 <= g << 2
        # 31 blocks are not enough: band 1 reads band 2's, not its own; so do 0 and 3; 4 has 2 and 6 equally near: the darker
        assert mine(1) != e2 and lv["E"][0, :5, ch].tolist() == [e2] * 5
        # band 6 reads more than 4 G, band 7 less than G / 4: both end on the clamp; 5 borrows from 6
        assert mine(6) > g << 2 and mine(7) < g >> 2
        assert lv["E"][0, 5:, ch].tolist() == [g << 2, g << 2, g >> 2]
        # another scene, another grain; all of its bands borrow from its only one
        e3 = G.quartile(energy[3].reshape(-1, 3)[:, ch])
        assert lv["G"][1, ch] == e3 and lv["E"][1, :, ch].tolist() == [e3] * 8 and e3 > 10 * g
    # nothing measured: nothing; the frames without a scene (energies of 1e7 and more) show nowhere
    assert not lv["scale"][2].any() and lv["E"].max() < 10 ** 6
    # the scale, by hand
    assert lv["scale"][0, 2, 0] == math.isqrt(int(lv["E"][0, 2, 0]) * 196611 * 19 // 20480)
    lv = G.level_case("spread")["levels"]
    assert lv["total"][0] == 40 and lv["count"][0].max() == 5 and (lv["E"][0] == lv["G"][0][None]).all() and lv["G"][0].min() > 0
    lv = G.level_case("thresholds")["levels"]
    assert lv["total"].tolist() == [31, 32] and not lv["scale"][0].any() and (lv["scale"][1] == 110206).all()
    assert 64 * 1020 ** 2 * 4 * 196611 * 19 < 2 ** 53             # the product at the largest clamped energy
    assert not G.level_case("empty")["levels"]["scale"].any()


def test_the_quartile_position():
    for n, at in ((1, 0), (4, 0), (5, 1), (8, 1), (9, 2), (32, 7), (33, 8)):
        assert G.quartile(range(100, 100 + n)) == 100 + at


def test_the_table():
    scale = np.zeros((2, 8, 3), np.int64)
    scale[0] = (np.arange(8) * 1000)[:, None] + np.arange(3)[None] * 7
    scale[1, :, :] = 2 ** 21
    lut = G.lut_np(scale)
    assert lut.dtype == np.int32 and lut.shape == (2, 256, 3)
    assert (lut[0, :17] == scale[0, 0]).all() and (lut[0, 240:] == scale[0, 7]).all()                # flat beyond the outer centres
    assert all((lut[0, 16 + 32 * k] == scale[0, k]).all() for k in range(8))                         # the centres themselves
    assert lut[0, 16 + 32 * 3 + 8, 1] == (3007 * 24 + 4007 * 8 + 16) >> 5 and lut[0, 239, 0] == (6000 * 1 + 7000 * 31 + 16) >> 5
    assert (np.diff(lut[0].astype(np.int64), axis=0) >= 0).all()
    # strength: rounded in 1 / 256, capped
    assert np.array_equal(G.lut_np(scale, 128)[0], (lut[0].astype(np.int64) * 128 + 128) >> 8) and not G.lut_np(scale, 0).any()
    assert (G.lut_np(scale, 1024)[1] == G.SCALE_MAX).all() and (G.lut_np(scale, 511)[1] == (2 ** 21 * 511 + 128) >> 8).all()
    assert [G.q8_of(s) for s in (0, 0.5, 1, 1.001, 1.002, 4)] == [0, 128, 256, 256, 257, 1024]
    assert 510 * G.SCALE_MAX + 32768 < 2 ** 31 and ops.GRAIN_SCALE_MAX == G.SCALE_MAX and ops.GRAIN_MIN_BLOCKS == G.MIN_BLOCKS
    # sigma <-> scale
    assert G.scale_of(G.sigma_of(np.arange(0, 70000, 13))).tolist() == list(range(0, 70000, 13))
    assert abs(G.sigma_of(G.scale_of(6.0)) - 6.0) < 0.002


# ------------------------------------------------------------------------------------------------ the synthesis
def test_apply_guarantees_and_saturation():
    for name in G.NAMES:
        c, w = G.case(name), G.want(name)
        on = c["where"] != 0
        for out in (w["out"], w["alt_out"]):
            assert out.dtype == np.uint8 and np.array_equal(out[~on], c["filled"][~on])
        for t in range(c["L"]):
            if not 0 <= c["scene_of"][t] < c["n_scenes"]:
                assert np.array_equal(w["alt_out"][t], c["filled"][t])
    c, w = G.case("out_of_range_10x18"), G.want("out_of_range_10x18")
    assert (w["alt_out"][1] != c["filled"][1]).any() and np.array_equal(w["alt_out"][[0, 2, 3]], c["filled"][[0, 2, 3]])
    # strong grain on bytes at both ends of the range, strength 0.5 and 4: both clamps, and by hand
    filled, where, scale, scene_of, seed = G.saturation_case()
    for strength in (0.5, 4):
        lut = G.lut_np(scale, G.q8_of(strength))
        out = G.apply_np(filled, where, lut, scene_of, seed)
        for t in range(2):
            n = G.noise_np(seed, t, 12, 16)
            g = lut[0][G.luma(filled[t])]
            raw = filled[t].astype(np.int64) + ((n * g + 32768) // 65536)
            assert np.array_equal(out[t], np.clip(raw, 0, 255)) and (raw < 0).any() and (raw > 255).any()
        assert (out == 0).any() and (out == 255).any() and (out != filled).mean() > 0.3
    # an entry past the cap is read as the cap, a negative one as 0
    big = np.full((1, 256, 3), G.SCALE_MAX + 12345, np.int32)
    assert np.array_equal(G.apply_np(filled, where, big, np.zeros(2, np.int32), 1),
                          G.apply_np(filled, where, np.full((1, 256, 3), G.SCALE_MAX, np.int32), np.zeros(2, np.int32), 1))
    assert np.array_equal(G.apply_np(filled, where, -big, np.zeros(2, np.int32), 1), filled)


def test_match_np_scenes_and_levels():
    c = G.case("scenes_34x42")
    fr, fl = np.array(c["frames"][:4]), np.array(c["filled"][:4])
    where = np.ones((4, 34, 42), np.uint8)
    no_hole = np.zeros_like(where)
    out, sigma = G.match_np(fr, fl, where, hole=no_hole, scenes=[2], seed=5)
    assert sigma.shape == (2, 8, 3) and sigma.dtype == np.float64
    print("two scenes, sigma put in 2 and 9, read", sigma[:, 3].round(2).tolist())
    assert (np.abs(sigma[0] - 2) < 0.4).all() and (np.abs(sigma[1] - 9) < 1.0).all()                 # each scene its own grain
    pooled = G.match_np(fr, fl, where, hole=no_hole, seed=5)[1]
    assert pooled.shape == (1, 8, 3) and (pooled[0] > sigma[0]).all() and (pooled[0] < sigma[1]).all()
    # hole=None means where: everything is hole, nothing is measured, nothing changes
    same, zero = G.match_np(fr, fl, where, seed=5)
    assert np.array_equal(same, fl) and not zero.any()
    # levels= in place of the measurement: [8,3] for every scene, or one per scene
    lv = np.linspace(1, 12, 24).reshape(8, 3)
    a, sa = G.match_np(None, fl, where, scenes=[2], levels=lv, seed=5)
    b, sb = G.match_np(None, fl, where, scenes=[2], levels=np.stack([lv, lv]), seed=5)
    assert np.array_equal(a, b) and np.array_equal(sa, sb) and np.abs(sa[1] - lv).max() < 0.002 and (a != fl).any()
    assert np.array_equal(G.match_np(fr, fl, where, hole=no_hole, strength=0)[0], fl)


def test_tennis_numbers():
    """DESIGN.md 3r's table, recomputed: a spatial estimator reads fine texture as grain where a band has no flat block"""
    rows = {}
    for sigma in (0, 3, 6):
        s, n, g = G.tennis_sigmas(ROOT, sigma)
        clamped = G.tennis_sigmas(ROOT, sigma, clamp=True)[0]
        rows[sigma] = (s, n, g, clamped)
        print("tennis + sigma %d: green sigma per band 0..6 %s blocks %s scene %.2f clamped %s"
              % (sigma, np.round(s, 2).tolist(), n.tolist(), g, np.round(clamped, 2).tolist()))
    s, n, g, clamped = rows[0]
    bulk = [k for k in range(1, 5) if n[k] >= G.MIN_BLOCKS]
    assert len(bulk) == 4 and (s[bulk] < 3).all() and (s[bulk] > 0.5).all()
    for s, n, g, clamped in rows.values():
        assert (clamped <= 2 * g + 0.01).all() and (clamped >= g / 2 - 0.01).all()
    assert rows[6][0][2] > rows[3][0][2] > rows[0][0][2]


# ------------------------------------------------------------------------------------------------ the arguments of match_grain
def test_match_grain_checks_its_arguments():
    sig = inspect.signature(video.match_grain)
    assert list(sig.parameters) == ["frames_u8", "filled_u8", "where", "hole", "scenes", "strength", "seed", "levels", "return_levels",
                                    "device"]
    assert [p.default for p in sig.parameters.values()][3:] == [None, None, 1.0, 0, None, False, None]
    L, H, W = 4, 10, 12
    f = np.zeros((L, H, W, 3), np.uint8)
    m = np.ones((L, H, W), np.uint8)

    def call(frames=f, filled=f, where=m, **kw):
        return video.match_grain(frames, filled, where, **kw)

    for filled in (f[0], f[..., :2], f.astype(np.float32), None, 7):
        with pytest.raises(ValueError, match="filled_u8"):
            call(filled=filled)
    for frames in (f[:3], f[:, :9], f.astype(np.int32), None):
        with pytest.raises(ValueError, match="frames_u8"):
            call(frames=frames)
    for name in ("where", "hole"):
        for bad in (m[:3], m[:, :, :11], m.astype(np.float32), f, 3) + ((None,) if name == "where" else ()):
            with pytest.raises(ValueError, match=name):
                call(**{name: bad})
    for scenes in ([0], [4], [2, 2], [3, 1], "auto", [1.5], 2):
        with pytest.raises(ValueError, match="scenes"):
            call(scenes=scenes)
    for strength in (-0.1, 4.01, True, "1", None, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="strength"):
            call(strength=strength)
    for seed in (-1, 2 ** 32, 1.0, True, None, "0"):
        with pytest.raises(ValueError, match="seed"):
            call(seed=seed)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="return_levels"):
            call(return_levels=bad)
    lv = np.ones((8, 3))
    for levels in (np.ones((3, 8)), np.ones((2, 8, 3)), np.ones(24), -lv, lv * 256, lv * np.nan, "strong", np.ones((1, 1, 8, 3))):
        with pytest.raises(ValueError, match="levels"):
            call(levels=levels)
    with pytest.raises(ValueError, match="levels"):
        call(levels=np.ones((3, 8, 3)), scenes=[2])         # two scenes, three sets of levels
    # good arguments pass the checks: on a host without a device the call gets as far as the refusal of the CPU device
    for kw in ({}, dict(hole=m), dict(where=m.astype(bool), hole=m.astype(bool)), dict(scenes=[1, 3]), dict(scenes=[]), dict(strength=0),
               dict(strength=4, seed=2 ** 32 - 1), dict(levels=lv, frames=None), dict(levels=np.ones((2, 8, 3)), scenes=[2]),
               dict(levels=lv.tolist(), return_levels=True), dict(seed=np.int64(5))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(device="cpu", **kw)
    assert video.match_grain.__doc__ and all(s in video.match_grain.__doc__ for s in
                                             ("outside ``where`` is filled_u8's byte", "across a cut", "returned unchanged"))


def test_the_checks_return_the_tables():
    f = np.zeros((5, 10, 12, 3), np.uint8)
    m = np.ones((5, 10, 12), np.uint8)
    scene_of, S, q8, scale = video._check_grain_args(f, f, m, None, [2, 3], 0.5, 1, None, False)
    assert scene_of.tolist() == [0, 0, 1, 2, 2] == G.scene_table(5, [2, 3])[0].tolist() and S == 3 and q8 == 128 and scale is None
    lv = np.linspace(0, 255, 24).reshape(8, 3)
    scale = video._check_grain_args(None, f, m, None, [2, 3], 1.0, 1, lv, False)[3]
    assert scale.shape == (3, 8, 3) and scale.dtype == np.int64 and np.array_equal(scale[2], G.scale_of(lv))
    assert video._GRAIN_SIGMA_PER_SCALE == G.SIGMA_PER_SCALE and video._GRAIN_SCALE_PER_SIGMA == G.SCALE_PER_SIGMA


# ------------------------------------------------------------------------------------------------ header, binding, C entries
def test_header_and_binding_declare_the_entries():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    names = {}
    for entry in ("e2fgvi_grain_blocks", "e2fgvi_grain_apply"):
        decl = re.search(r"int %s\(([^;]*)\);" % entry, header)
        assert decl, entry
        names[entry] = [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")]
    assert names["e2fgvi_grain_blocks"] == ["frames", "hole", "L", "H", "W", "energy", "band", "stream"]
    assert names["e2fgvi_grain_apply"] == ["filled", "where", "lut", "scene_of", "n_scenes", "seed", "L", "H", "W", "out", "stream"]
    res, args = lib.SYMBOLS["e2fgvi_grain_blocks"]
    assert len(args) == 8 and args[-1] is lib._fp and args[:2] == [lib._fp] * 2 and args[2:5] == [lib._i32] * 3 and args[5:7] == [lib._fp] * 2
    res, args = lib.SYMBOLS["e2fgvi_grain_apply"]
    assert len(args) == 11 and args[-1] is lib._fp and args[:4] == [lib._fp] * 4 and args[4] is lib._i32 and args[6:9] == [lib._i32] * 3
    assert args[5] is lib.C.c_uint32 and args[9] is lib._fp
    assert lib.ABI_VERSION == 9                          # symbols were only added
    assert all(callable(getattr(ops, n)) for n in ("grain_blocks", "grain_lut", "grain_lut_from_scale", "grain_apply"))
    assert callable(video.match_grain)
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "grain.hip"]
    assert len(unit) == 1 and unit[0][1] == "grain.o" and unit[0][2] == build.NOPK and unit[0][1] in build.NOPK_OBJECTS
    # the constants of the definition stand in the header as the restatement has them
    for text in ("0x7feb352d", "0x846ca68b", "0x9E3779B9", "196611", "21845", "(1280 * 16)"):
        assert text in header, text


def test_entries_refuse_bad_arguments_and_return_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    ptrs = ("frames", "hole", "energy", "band")
    good = dict({k: base + (i << 16) for i, k in enumerate(ptrs)}, L=3, H=20, W=30)

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_grain_blocks(a["frames"], a["hole"], a["L"], a["H"], a["W"], a["energy"], a["band"], None)

    for k in ("frames", "energy", "band"):
        assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
    for k in ("L", "H", "W"):
        assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error(), k
    assert rc(H=46341, W=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
    assert rc(H=1, W=2147483647 - 256) == -1 and rc(H=0x7fffffff, W=0x7fffffff) == -1
    for off in (1, 2, 3):
        assert rc(energy=good["energy"] + off) == -1 and b"aligned" in so.e2fgvi_last_error()
    null = {k: None for k in ptrs}
    # no frame, or no block row / column: nothing to write
    assert rc(L=0) == 0 and rc(H=9) == 0 and rc(W=9) == 0 and rc(H=0) == 0 and rc(W=1) == 0
    assert rc(L=0, **null) == 0 and rc(H=9, **null) == 0 and rc(W=9, H=9, L=0, **null) == 0

    aptrs = ("filled", "where", "lut", "scene_of", "out")
    agood = dict({k: base + (i << 16) for i, k in enumerate(aptrs)}, n_scenes=2, seed=7, L=3, H=7, W=5)
    order = ("filled", "where", "lut", "scene_of", "n_scenes", "seed", "L", "H", "W", "out")

    def arc(**kw):
        a = dict(agood, **kw)
        return so.e2fgvi_grain_apply(*[a[k] for k in order], None)

    for k in aptrs:
        assert arc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
    for k in ("L", "H", "W", "n_scenes"):
        assert arc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error(), k
    assert arc(H=46341, W=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
    for k in ("lut", "scene_of"):
        assert arc(**{k: agood[k] + 2}) == -1 and b"aligned" in so.e2fgvi_last_error(), k
    anull = {k: None for k in aptrs}
    assert arc(L=0) == 0 and arc(H=0) == 0 and arc(W=0) == 0 and arc(L=0, seed=2 ** 32 - 1) == 0
    assert arc(L=0, **anull) == 0 and arc(H=0, **anull) == 0 and arc(W=0, H=0, L=0, n_scenes=0, **anull) == 0
    assert so.e2fgvi_abi_version() == 9


def test_the_object_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "grain.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("grain.o not built here (python -m e2fgvi_amd.build)")
    assert build.verify_no_scratch(obj="grain.o", marker="grain_", what="film grain") == 2
