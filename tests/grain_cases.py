"""Film grain restated in numpy (video.match_grain, ops.grain_blocks, ops.grain_lut, ops.grain_apply; the definition is in
include/e2fgvi_hip.h) and the named cases the device code is compared with, entry for entry and byte for byte.

The restatement goes about it another way than the device: the block sums come from array slices where the kernel shuffles
sixteen lanes, the levels from Python loops over sorted lists where ops.grain_lut sorts one array of keys, the square root from
math.isqrt where the device corrects a float64 root.  Everything is an integer, so there is no tolerance anywhere."""
import math

import numpy as np

MIN_BLOCKS = 32
SCALE_MAX = (1 << 22) - 1
NOISE_VAR = 21845                                       # the variance of the sum of four independent bytes, exactly
SIGMA_PER_SCALE = math.sqrt(21845.0) / 65536.0          # grey levels of sigma per unit of scale
SCALE_PER_SIGMA = 65536.0 / math.sqrt(21845.0)
M32 = 0xFFFFFFFF


def luma(frames):
    f = np.asarray(frames).astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def blocks_np(frames, hole=None):
    """(energy int32 [L,Hb,Wb,3], band uint8 [L,Hb,Wb]); band 255 = not measured"""
    f = np.asarray(frames).astype(np.int64)
    L, H, W = f.shape[:3]
    Hb, Wb = max(0, (H - 2) // 8), max(0, (W - 2) // 8)
    if L == 0 or Hb == 0 or Wb == 0:
        return np.zeros((L, Hb, Wb, 3), np.int32), np.zeros((L, Hb, Wb), np.uint8)
    r = 4 * f[:, 1:-1, 1:-1] - f[:, 1:-1, :-2] - f[:, 1:-1, 2:] - f[:, :-2, 1:-1] - f[:, 2:, 1:-1]

    def per_block(a):                                   # [L, H-2, W-2, ...] on the interior -> [L, Hb, 8, Wb, 8, ...]
        a = a[:, :8 * Hb, :8 * Wb]
        return a.reshape((L, Hb, 8, Wb, 8) + a.shape[3:])

    energy = per_block(r * r).sum(axis=(2, 4))
    ysum = per_block(luma(f)[:, 1:-1, 1:-1]).sum(axis=(2, 4))
    inner = f[:, 1:-1, 1:-1]
    bad = per_block(((inner == 0) | (inner == 255)).any(-1)).any(axis=(2, 4))
    if hole is not None:
        h = np.asarray(hole) != 0
        for dy in range(10):
            for dx in range(10):
                bad = bad | h[:, dy:dy + 8 * Hb:8, dx:dx + 8 * Wb:8]
    band = np.where(bad, 255, (ysum >> 6) >> 5)
    return energy.astype(np.int32), band.astype(np.uint8)


def quartile(values):
    v = sorted(int(x) for x in values)
    return v[(len(v) - 1) // 4]


def levels_np(energy, band, scene_of, n_scenes, borrow=True, clamp=True):
    """dict(scale int64 [S,8,3], E [S,8,3] after borrowing and clamp, G [S,3], count [S,8], total [S]); borrow / clamp False: the
    raw quartile of every band that has its blocks (0 elsewhere), for the measurements"""
    energy, band = np.asarray(energy).astype(np.int64), np.asarray(band)
    S = int(n_scenes)
    out = dict(scale=np.zeros((S, 8, 3), np.int64), E=np.zeros((S, 8, 3), np.int64), G=np.zeros((S, 3), np.int64),
               count=np.zeros((S, 8), np.int64), total=np.zeros(S, np.int64))
    for s in range(S):
        frames = [t for t in range(energy.shape[0]) if int(scene_of[t]) == s]
        per = [[] for _ in range(8)]                     # band -> the energies [3] of its measured blocks
        for t in frames:
            for k in range(8):
                per[k] += list(energy[t][band[t] == k])
        out["count"][s] = [len(p) for p in per]
        everything = [e for p in per for e in p]
        out["total"][s] = len(everything)
        if len(everything) < MIN_BLOCKS:
            continue
        has = [k for k in range(8) if len(per[k]) >= MIN_BLOCKS]
        for c in range(3):
            G = quartile(e[c] for e in everything)
            out["G"][s, c] = G
            for k in range(8):
                if k in has:
                    E = quartile(e[c] for e in per[k])
                elif not borrow:
                    continue
                elif has:
                    j = min(has, key=lambda j: (abs(j - k), j))         # the nearest; a tie: the darker
                    E = quartile(e[c] for e in per[j])
                else:
                    E = G
                if clamp:
                    E = min(max(E, G >> 2), G << 2)
                out["E"][s, k, c] = E
                out["scale"][s, k, c] = math.isqrt(E * 196611 * 19 // (1280 * 16))
    return out


def sigma_of(scale):
    """the standard deviation, in grey levels, of the grain a scale lays down"""
    return np.asarray(scale).astype(np.float64) * SIGMA_PER_SCALE


def scale_of(sigma):
    return np.floor(np.asarray(sigma, np.float64) * SCALE_PER_SIGMA + 0.5).astype(np.int64)


def q8_of(strength):
    return int(math.floor(256.0 * float(strength) + 0.5))


def lut_np(scale, strength_q8=256):
    """int32 [S,256,3]"""
    scale = np.asarray(scale).astype(np.int64)
    lut = np.zeros((scale.shape[0], 256, 3), np.int64)
    for y in range(256):
        u = y - 16
        if u < 0:
            v = scale[:, 0]
        elif u >= 224:
            v = scale[:, 7]
        else:
            k, f = u >> 5, u & 31
            v = (scale[:, k] * (32 - f) + scale[:, k + 1] * f + 16) >> 5
        lut[:, y] = np.minimum((v * int(strength_q8) + 128) >> 8, SCALE_MAX)
    return lut.astype(np.int32)


def mix(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def noise_np(seed, t, H, W):
    """n int64 [H,W,3] of frame t: the sum of the hash's four bytes - 510"""
    key = mix(np.uint64((int(seed) + 0x9E3779B9 * int(t)) & M32))
    ys, xs, cs = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), np.arange(3, dtype=np.uint64), indexing="ij")
    h = mix(key ^ (((ys * np.uint64(W) + xs) * 3 + cs) & M32))
    return ((h & 255) + ((h >> 8) & 255) + ((h >> 16) & 255) + ((h >> 24) & 255)).astype(np.int64) - 510


def apply_np(filled, where, lut, scene_of, seed):
    filled = np.asarray(filled)
    L, H, W = filled.shape[:3]
    lut = np.clip(np.asarray(lut).astype(np.int64), 0, SCALE_MAX)
    out = filled.copy()
    Y = luma(filled)
    for t in range(L):
        s = int(scene_of[t])
        if not 0 <= s < lut.shape[0]:
            continue
        g = lut[s][Y[t]]                                            # [H,W,3]
        v = filled[t].astype(np.int64) + ((noise_np(seed, t, H, W) * g + 32768) >> 16)
        on = np.asarray(where[t]) != 0
        out[t][on] = np.clip(v, 0, 255).astype(np.uint8)[on]
    return out


def scene_table(length, scenes=None):
    cuts = [int(c) for c in (scenes or [])]
    return np.array([sum(c <= t for c in cuts) for t in range(length)], np.int32), len(cuts) + 1


def match_np(frames, filled, where, hole=None, scenes=None, strength=1.0, seed=0, levels=None):
    """(out, sigma float64 [S,8,3]) of video.match_grain"""
    filled = np.asarray(filled)
    L = filled.shape[0]
    scene_of, S = scene_table(L, scenes)
    if levels is not None:
        scale = scale_of(levels)
        scale = np.broadcast_to(scale, (S, 8, 3)) if scale.ndim == 2 else scale
    else:
        energy, band = blocks_np(frames, where if hole is None else hole)
        scale = levels_np(energy, band, scene_of, S)["scale"]
    out = apply_np(filled, where, lut_np(scale, q8_of(strength)), scene_of, seed)
    return out, sigma_of(scale)


# ------------------------------------------------------------------------------------------------ the cases
def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _alt_lut(rng, S):
    """a table no measurement would give: every luma its own strength, some entries negative and some past SCALE_MAX"""
    lut = rng.randint(0, 60000, (max(S, 1), 256, 3)).astype(np.int32)
    lut[:, 5::17] = rng.randint(SCALE_MAX - 5, SCALE_MAX + 90000, lut[:, 5::17].shape)
    lut[:, 3::29] = -rng.randint(1, 70000, lut[:, 3::29].shape)
    return lut


def _case(frames, seed, rng, hole=None, scene_of=None, n_scenes=1, strength_q8=256, filled=None, where=None):
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    L, H, W = frames.shape[:3]
    if filled is None:
        filled = rng.randint(0, 256, frames.shape).astype(np.uint8)
        filled[:, ::3, ::5] = rng.choice([0, 1, 254, 255], filled[:, ::3, ::5].shape)       # both clamps
    if where is None:
        where = rng.choice([0, 0, 1, 7, 255], (L, H, W)).astype(np.uint8)
    if scene_of is None:
        scene_of = np.zeros(L, np.int32)
    return _freeze(dict(frames=frames, hole=None if hole is None else np.ascontiguousarray(hole, dtype=np.uint8),
                        filled=np.ascontiguousarray(filled, dtype=np.uint8), where=np.ascontiguousarray(where, dtype=np.uint8),
                        scene_of=np.asarray(scene_of, np.int32), n_scenes=int(n_scenes), strength_q8=int(strength_q8), seed=int(seed),
                        alt_lut=_alt_lut(rng, n_scenes), L=L, H=H, W=W))


def _random(L, H, W, seed, key, **kw):
    rng = np.random.RandomState(key)
    fr = rng.randint(1, 255, (L, H, W, 3)).astype(np.uint8)
    # a clipped byte here and there, a hole pixel in the last block row and one in the frame's last corner: some blocks are out for
    # one reason, some for the other, some are measured
    fr[:, 5::18, 12::22, 1] = rng.choice([0, 255], fr[:, 5::18, 12::22, 1].shape)
    hole = np.zeros((L, H, W), np.uint8)
    hole[:, H - 3, 2], hole[-1, H - 1, W - 1] = 1, 200
    return _case(fr, seed, rng, hole=hole, **kw)


# validity_26x34: Hb = 3, Wb = 4; block (by, bx) covers y in [1 + 8 by, 9 + 8 by), x in [1 + 8 bx, 9 + 8 bx)
VALIDITY_WANT_BAD = {(0, 1), (1, 1), (2, 2), (0, 3), (2, 0)}


def _validity_26x34():
    rng = np.random.RandomState(31)
    fr = rng.randint(60, 190, (1, 26, 34, 3)).astype(np.uint8)
    hole = np.zeros((1, 26, 34), np.uint8)
    hole[0, 8, 12] = 1          # the last row of block (0,1), and one pixel above block (1,1): both are out
    hole[0, 18, 20] = 9         # inside block (2,2); two rows under block (1,2), whose footprint ends at row 17: (1,2) stays
    fr[0, 0, 5] = 0           # in the ring of block (0,0) only: the ring does not invalidate
    fr[0, 12, 0, 2] = 255       # the ring of block (1,0)
    fr[0, 4, 30, 1] = 255       # inside block (0,3)
    fr[0, 20, 3, 0] = 0         # inside block (2,0)
    return _case(fr, 7, rng, hole=hole)


def _edges_10x42():
    """five blocks whose mean luma lands on 31 | 32 and 223 | 224, and one pixel short of 32"""
    rng = np.random.RandomState(32)
    fr = np.zeros((1, 10, 42, 3), np.uint8)
    for bx, v in enumerate((31, 32, 223, 224, 32)):
        fr[0, :, 1 + 8 * bx:9 + 8 * bx] = v
    fr[0, :, 0], fr[0, :, 41] = 31, 32
    fr[0, 4, 1 + 8 * 4 + 3] = 31                        # sum Y = 64 * 32 - 1: the mean is 31 after the shift
    return _case(fr, 0, rng)


EDGES_WANT_BAND = (0, 1, 6, 7, 0)


def _bands_66x70():
    """Hb = Wb = 8, L = 3: 192 blocks; the left half grey 80 (band 2) with noise of sigma 3, the right half grey 176 (band 5) with
    sigma 7, and a dark strip (band 0) of a single block column with sigma 1: a band that has to borrow"""
    rng = np.random.RandomState(33)
    L, H, W = 3, 66, 70
    base = np.empty((L, H, W, 3))
    base[:, :, :33], base[:, :, 33:] = 80, 176
    sig = np.where(np.arange(W) < 33, 3.0, 7.0)[None, None, :, None]
    base[:, :, :9], sig = 10, np.where(np.arange(W)[None, None, :, None] < 9, 1.0, sig)
    fr = np.clip(np.rint(base + sig * rng.randn(L, H, W, 3)), 1, 254)
    filled = np.clip(np.rint(base), 0, 255)
    filled[:, ::6, ::4] = rng.choice([0, 255], filled[:, ::6, ::4].shape)
    return _case(fr, 0xDEADBEEF, rng, filled=filled, where=np.ones((L, H, W), np.uint8))


def _scenes_34x42():
    """Hb = 4, Wb = 5, L = 6: scene 0 = frames 0..1 (sigma 2, 40 blocks), scene 1 = frames 2..3 (sigma 9), frame 4 in scene 2 with
    every block clipped, frame 5 with a scene number out of range"""
    rng = np.random.RandomState(34)
    L, H, W = 6, 34, 42
    sig = np.array([2, 2, 9, 9, 5, 5], np.float64)[:, None, None, None]
    fr = np.clip(np.rint(120 + sig * rng.randn(L, H, W, 3)), 1, 254)
    fr[4, 3::8, 3::8, 0] = 255
    return _case(fr, 0xFFFFFFFF, rng, scene_of=[0, 0, 1, 1, 2, 3], n_scenes=3, strength_q8=384)


def _out_of_range_10x18():
    rng = np.random.RandomState(35)
    fr = rng.randint(1, 255, (4, 10, 18, 3)).astype(np.uint8)
    return _case(fr, 1, rng, scene_of=[-1, 0, 2, -2 ** 31], n_scenes=2)


_BUILDERS = {"noblock_9x30": lambda: _random(2, 9, 30, 3, 21), "one_10x10": lambda: _random(1, 10, 10, 4, 22),
             "odd_19x27": lambda: _random(2, 19, 27, 5, 23), "odd_27x19": lambda: _random(2, 27, 19, 2 ** 32 - 1, 24),
             "row_3x11": lambda: _random(3, 3, 11, 6, 25), "validity_26x34": _validity_26x34, "edges_10x42": _edges_10x42,
             "bands_66x70": _bands_66x70, "scenes_34x42": _scenes_34x42, "out_of_range_10x18": _out_of_range_10x18}
NAMES = tuple(_BUILDERS)
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def want(name):
    """dict(energy, band, levels, lut, out, alt_out) of a frame case under the definition; computed once, read-only"""
    if name not in _WANT:
        c = case(name)
        energy, band = blocks_np(c["frames"], c["hole"])
        lv = levels_np(energy, band, c["scene_of"], c["n_scenes"])
        lut = lut_np(lv["scale"], c["strength_q8"])
        w = dict(energy=energy, band=band, levels=lv, scale=lv["scale"], lut=lut,
                 out=apply_np(c["filled"], c["where"], lut, c["scene_of"], c["seed"]),
                 alt_out=apply_np(c["filled"], c["where"], c["alt_lut"], c["scene_of"], c["seed"]))
        _WANT[name] = _freeze(w)
    return _WANT[name]


# ------------------------------------------------------------------------------------------------ the level cases
# energy / band tables written down directly: what no small frame can be made to hold
def _fill(energy, band, t, k, n, lo, hi, rng, at):
    """n blocks of frame t, from flat position at[0] on, in band k with energies in [lo, hi)"""
    e, b = energy[t].reshape(-1, 3), band[t].reshape(-1)
    e[at[0]:at[0] + n] = rng.randint(lo, hi, (n, 3))
    b[at[0]:at[0] + n] = k
    at[0] += n


def _rules():
    """scene 0 (frames 0-2, 150 blocks): band 1 has 31 blocks, band 2 has 32, band 6 has 40 with energies far above 4 G, band 7
    has 33 far below G / 4, the other bands none: 0, 1 and 3 borrow from 2, 4 has 2 and 6 equally near (the darker: 2), 5 borrows
    from 6.  Scene 1 (frame 3): 50 blocks of band 3, another grain.  Scene 2 (frame 4): nothing measured.  Frames 5 and 6 carry
    scene numbers out of range and energies that would show."""
    rng = np.random.RandomState(41)
    L, Hb, Wb = 7, 5, 10
    energy = rng.randint(0, 5000, (L, Hb, Wb, 3)).astype(np.int32)
    band = np.full((L, Hb, Wb), 255, np.uint8)
    flat_e, flat_b = energy[:3].reshape(1, -1, 3), band[:3].reshape(1, -1)
    at = [0]
    for k, n, lo, hi in ((1, 31, 900, 1100), (2, 32, 1100, 1400), (6, 40, 90000, 120000), (7, 33, 5, 30)):
        _fill(flat_e, flat_b, 0, k, n, lo, hi, rng, at)
    order = rng.permutation(150)                         # spread over the three frames
    energy[:3] = flat_e[0][order].reshape(3, Hb, Wb, 3)
    band[:3] = flat_b[0][order].reshape(3, Hb, Wb)
    band[3], energy[3] = 3, rng.randint(40000, 60000, (Hb, Wb, 3))
    band[5:], energy[5:] = 2, rng.randint(10 ** 7, 6 * 10 ** 7, (2, Hb, Wb, 3))
    return dict(energy=energy, band=band, scene_of=np.array([0, 0, 0, 1, 2, -1, 3], np.int32), n_scenes=3, strength_q8=256)


def _spread():
    """40 measured blocks, five in every band: the scene has a level, no band has one of its own"""
    rng = np.random.RandomState(42)
    energy = rng.randint(100, 4000, (1, 5, 8, 3)).astype(np.int32)
    band = np.repeat(np.arange(8, dtype=np.uint8)[None], 5, 0)[None]
    return dict(energy=energy, band=np.ascontiguousarray(band), scene_of=np.zeros(1, np.int32), n_scenes=1, strength_q8=1024)


def _thresholds():
    """scene 0 has 31 measured blocks in all (nothing), scene 1 has 32 in one band (a level), with the largest energy there is"""
    rng = np.random.RandomState(43)
    energy = np.full((2, 4, 8, 3), 66585600, np.int32)       # 64 * 1020^2
    band = np.full((2, 4, 8), 4, np.uint8)
    band[0, 0, 0] = 255
    energy[0] = rng.randint(0, 9000, (4, 8, 3))
    return dict(energy=energy, band=band, scene_of=np.array([0, 1], np.int32), n_scenes=2, strength_q8=1024)


def _empty():
    return dict(energy=np.zeros((3, 0, 4, 3), np.int32), band=np.zeros((3, 0, 4), np.uint8), scene_of=np.array([0, 1, 1], np.int32),
                n_scenes=2, strength_q8=256)


_LEVEL_BUILDERS = {"rules": _rules, "spread": _spread, "thresholds": _thresholds, "empty": _empty}
LEVEL_NAMES = tuple(_LEVEL_BUILDERS)
_LEVEL_CASES = {}


def level_case(name):
    if name not in _LEVEL_CASES:
        c = _freeze(_LEVEL_BUILDERS[name]())
        c["levels"] = levels_np(c["energy"], c["band"], c["scene_of"], c["n_scenes"])
        c["lut"] = lut_np(c["levels"]["scale"], c["strength_q8"])
        _LEVEL_CASES[name] = c
    return _LEVEL_CASES[name]


def saturation_case():
    """bytes at both ends of the range under grain of sigma 40: (filled, where, scale [1,8,3], scene_of, seed); with strength 0.5
    and 4 both clamps are hit"""
    rng = np.random.RandomState(3)
    filled = rng.choice([0, 1, 254, 255], (2, 12, 16, 3)).astype(np.uint8)
    return filled, np.ones((2, 12, 16), np.uint8), np.broadcast_to(scale_of(40.0), (1, 8, 3)).copy(), np.zeros(2, np.int32), 99


# ------------------------------------------------------------------------------------------------ the measurements
def noisy_flat(sigma, seed, L=4, H=120, W=216, grey=128):
    rng = np.random.RandomState(seed)
    return np.clip(np.rint(grey + sigma * rng.randn(L, H, W, 3)), 0, 255).astype(np.uint8)


def ramp(L, H, W):
    return np.broadcast_to((40 + 170.0 * np.arange(W) / W)[None, None, :, None], (L, H, W, 3))


def tennis_sigmas(root, sigma=0.0, seed=0, frames=6, clamp=False):
    """green-channel sigma per band 0..6 of frames 0-5 of tests/golden/tennis25.npz with Gaussian noise of ``sigma`` on top:
    (sigma per band [7], 0 where the band has no 32 blocks; counts [7]; the scene's level G as a sigma)"""
    import os
    with np.load(os.path.join(root, "tests", "golden", "tennis25.npz")) as z:
        fr = np.asarray(z[[k for k in z.files if z[k].ndim == 4][0]][:frames], np.float64)
    if sigma:
        fr = fr + sigma * np.random.RandomState(seed).randn(*fr.shape)
    fr = np.clip(np.rint(fr), 0, 255).astype(np.uint8)
    energy, band = blocks_np(fr)
    lv = levels_np(energy, band, np.zeros(fr.shape[0], np.int32), 1, borrow=clamp, clamp=clamp)
    g = math.isqrt(int(lv["G"][0, 1]) * 196611 * 19 // (1280 * 16))
    return sigma_of(lv["scale"][0, :7, 1]), lv["count"][0, :7], float(sigma_of(g))
