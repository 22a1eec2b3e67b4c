"""The local deflicker restated in numpy (video.deflicker_local, ops.flicker_local_hist, ops.flicker_local_curves,
ops.flicker_local_apply; the definition is in include/e2fgvi_hip.h), the named cases the device code is compared with word for word
and byte for byte, mutated restatements (VARIANTS) that must each differ from the definition on some case, and the planted flicker
and the measure the grids are judged on.  Integers throughout: there is no tolerance anywhere.  Luma, nodes and windows are those
of tests/flicker_cases.py; the rest is written unlike the kernels on purpose: slices and np.bincount for the cells' counts, whole
rows at once for the shifts per level, one fancy index over the whole video for the blend."""
import numpy as np

from tests import flicker_cases as C

DEFAULTS = dict(grid=(2, 2), span=4, max_shift=32)
NODES = C.NODES
FLAGS = ("ceil_bounds", "frame_N", "no_half", "nearest", "round_first", "swap_f", "across_cut")
VARIANTS = tuple((name, {name: True}) for name in FLAGS)
#   ceil_bounds    cell i starts at ceil(i H / gy), not at its floor
#   frame_N        the nodes and the quantiles of a cell are taken with N = H W in place of its own pixel count
#   no_half        positions are those of the pixels' upper left corners: 2 r in place of 2 r + 1
#   nearest        every pixel gets the curve of its own cell alone, no blend
#   round_first    the cells' shifts are rounded to whole levels in front of the blend
#   swap_f         fx weighs the rows and fy the columns
#   across_cut     frames of another scene are averaged (flicker_cases' flag)
KEYS = ("hist", "Q", "d16", "out")


def bounds(n, g, **f):
    """the g + 1 cell bounds along an axis of n pixels"""
    return [-((-i * n) // g) if f.get("ceil_bounds") else (i * n) // g for i in range(g + 1)]


def cell_of(n, g, **f):
    """int64 [n]: the cell every pixel of an axis lies in"""
    b = bounds(n, g, **f)
    return np.repeat(np.arange(g, dtype=np.int64), np.diff(b))


def hist_np(frames, grid, **f):
    """int32 [L,gy,gx,256]: the pixels of each cell of each frame per luma level"""
    gy, gx = grid
    Y = C.luma(frames)
    L, H, W = Y.shape
    rb, cb = bounds(H, gy, **f), bounds(W, gx, **f)
    hist = np.zeros((L, gy, gx, 256), np.int32)
    for t in range(L):
        for i in range(gy):
            for j in range(gx):
                hist[t, i, j] = np.bincount(Y[t, rb[i]:rb[i + 1], cb[j]:cb[j + 1]].ravel(), minlength=256)
    return hist


def _nodes_of(rows, N):
    """the nodes of rows that need not sum to N (frame_N): the walk stops at level 255 and an empty bin there divides by 1, as the
    header says of a row that breaks the contract"""
    Q = np.zeros((len(rows), NODES), np.int32)
    for t, row in enumerate(np.asarray(rows)):
        cum = np.cumsum(row.astype(np.int64))
        for k in range(NODES):
            r = ((2 * k + 1) * N) // (2 * NODES)
            v = min(int(np.searchsorted(cum, r, "right")), 255)
            below = int(cum[v - 1]) if v else 0
            Q[t, k] = 16 * v + max(0, min(15, (16 * (r - below)) // max(int(row[v]), 1)))
    return Q


def cell_curves_np(rows, N, scene_of, span, max_shift, **f):
    """(Q int32 [L,32], d16 int16 [L,256]) of one cell's rows over the frames"""
    rows = np.asarray(rows).astype(np.int64)
    L, K = len(rows), NODES
    Q = _nodes_of(rows, N) if f.get("frame_N") else C.nodes_np(rows)
    d16 = np.zeros((L, 256), np.int16)
    for t, us in enumerate(C.windows_np(scene_of, span, **f)):
        total = Q[us].astype(np.int64).sum(axis=0)
        T = (2 * total + len(us)) // (2 * len(us))
        s = np.clip(T - Q[t], -16 * max_shift, 16 * max_shift)
        cum = np.cumsum(rows[t])
        c2 = 2 * (cum - rows[t]) + rows[t]
        phi = np.clip((c2 * K * 128) // N - 128, 0, (K - 1) * 256)
        k0, fr = phi >> 8, phi & 255
        k1 = np.minimum(k0 + 1, K - 1)
        d16[t] = (s[k0] * (256 - fr) + s[k1] * fr + 128) >> 8
    return Q, d16


def curves_np(hist, scene_of, H, W, span, max_shift, **f):
    """(Q int32 [L,gy,gx,32], d16 int16 [L,gy,gx,256]) of the cells' histograms of frames of H x W"""
    hist = np.asarray(hist)
    L, gy, gx = hist.shape[:3]
    rb, cb = bounds(H, gy, **f), bounds(W, gx, **f)
    Q, d16 = np.zeros((L, gy, gx, NODES), np.int32), np.zeros((L, gy, gx, 256), np.int16)
    for i in range(gy):
        for j in range(gx):
            n = H * W if f.get("frame_N") else (rb[i + 1] - rb[i]) * (cb[j + 1] - cb[j])
            Q[:, i, j], d16[:, i, j] = cell_curves_np(hist[:, i, j], n, scene_of, span, max_shift, **f)
    return Q, d16


def positions(n, g, **f):
    """(i0, f, i1) int64 [n] of every pixel of an axis: the cell in front, the position behind its centre in 1/256, the cell behind"""
    if f.get("nearest"):
        i0 = cell_of(n, g, **f)
        return i0, np.zeros(n, np.int64), i0
    i = np.arange(n, dtype=np.int64)
    v = np.clip(((2 * i if f.get("no_half") else 2 * i + 1) * g * 128) // n - 128, 0, (g - 1) * 256)
    return v >> 8, v & 255, np.minimum((v >> 8) + 1, g - 1)


def apply_np(frames, d16, **f):
    """uint8 [L,H,W,3]: every pixel moved by the blend of its luma's shifts in the four cells around it, clipped"""
    a = np.asarray(frames).astype(np.int64)
    d16 = np.asarray(d16).astype(np.int64)
    L, H, W = a.shape[:3]
    if L * H * W == 0:
        return np.asarray(frames).astype(np.uint8).copy()
    gy, gx = d16.shape[1:3]
    if f.get("round_first"):
        d16 = ((d16 + 8) >> 4) * 16
    (i0, fy, i1), (j0, fx, j1) = positions(H, gy, **f), positions(W, gx, **f)
    Y = C.luma(a)
    tt = np.arange(L)[:, None, None]
    r0, r1, c0, c1 = i0[None, :, None], i1[None, :, None], j0[None, None, :], j1[None, None, :]
    FY, FX = fy[None, :, None], fx[None, None, :]
    if f.get("swap_f"):
        FY, FX = FX, FY
    top = d16[tt, r0, c0, Y] * (256 - FX) + d16[tt, r0, c1, Y] * FX
    bot = d16[tt, r1, c0, Y] * (256 - FX) + d16[tt, r1, c1, Y] * FX
    D = (top * (256 - FY) + bot * FY + 32768) >> 16
    return np.clip(a + ((D + 8) >> 4)[..., None], 0, 255).astype(np.uint8)


def deflicker_local_np(frames, scenes=None, grid=(2, 2), span=4, max_shift=32, **f):
    """every stage of the definition (or of a variant, by its flags) as a dict of KEYS"""
    frames = np.asarray(frames)
    L, H, W = frames.shape[:3]
    gy, gx = grid
    if H * W == 0:
        hist = np.zeros((L, gy, gx, 256), np.int32)
        Q, d16 = np.zeros((L, gy, gx, NODES), np.int32), np.zeros((L, gy, gx, 256), np.int16)
    else:
        hist = hist_np(frames, grid, **f)
        Q, d16 = curves_np(hist, C.scene_of_np(L, scenes), H, W, span, max_shift, **f)
    return dict(hist=hist, Q=Q, d16=d16, out=apply_np(frames, d16, **f))


# ------------------------------------------------------------------------------------------------ the cases
GAINS, OFFSETS = (256, 282, 231, 270, 240), (0, -7, 6, 3, -5)
TILT_X, TILT_Y = (0, 44, -38, 22, -46), (0, -30, 42, -48, 26)


def _tilted(L, H, W, seed, gains=GAINS, offsets=OFFSETS, tilt_x=TILT_X, tilt_y=TILT_Y):
    """flicker_cases' image moving two pixels a frame, frame t at a gain (in 1/256) that tilts across the frame by tilt_x[t] from
    the left edge to the right and by tilt_y[t] from the top to the bottom, plus offsets[t]: flicker that differs between cells"""
    base = C._image(H, W, seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for t in range(L):
        g = (gains[t % len(gains)] + (tilt_x[t % len(tilt_x)] * (2 * xx - (W - 1))) // (2 * max(W - 1, 1))
             + (tilt_y[t % len(tilt_y)] * (2 * yy - (H - 1))) // (2 * max(H - 1, 1)))
        out.append(np.clip((np.roll(base, 2 * t, axis=1) * g[..., None]) // 256 + offsets[t % len(offsets)], 0, 255))
    return np.stack(out)


def _case(frames, grid, scenes=None, **kw):
    frames = np.ascontiguousarray(np.asarray(frames).astype(np.uint8))
    frames.setflags(write=False)
    c = dict(DEFAULTS, frames=frames, L=frames.shape[0], H=frames.shape[1], W=frames.shape[2], scenes=scenes, grid=tuple(grid))
    c.update(kw)
    return c


def _flat():
    """two flat frames of 260 x 520 at (1, 2): 67 600 pixels in one bin of one cell -- more than 16 bits -- and the two halves
    flicker against each other"""
    fr = np.zeros((2, 260, 520, 3))
    fr[0, :, :260], fr[0, :, 260:], fr[1, :, :260], fr[1, :, 260:] = 90, 130, 130, 90
    return _case(fr, (1, 2))


def _clip():
    """saturated colours -- channels at 0 and 255 beside mid-grey lumas -- under strong tilted flicker: the sums leave [0, 255] at
    both ends"""
    rng = np.random.RandomState(41)
    fr = _tilted(4, 19, 22, 40, (256, 330, 190, 300), (0, 20, -25, 10), (0, 90, -80, 60), (0, -70, 85, -60))
    for t in range(4):
        for c in range(3):
            m = rng.rand(19, 22)
            fr[t, :, :, c] = np.where(m < 0.15, 0, np.where(m > 0.85, 255, fr[t, :, :, c]))
    return _case(fr, (2, 2))


def _rolled():
    """moving scenery alone: no flicker, but the cells' histograms change"""
    base = C._image(16, 18, 42)
    return _case(np.stack([np.roll(base, (3 * t, 5 * t), axis=(0, 1)) for t in range(5)]), (2, 2))


def _big_n(grid):
    """curves alone for frames of 8192 x 8192, n = 2^26 a cell at (1, 1) and 2^25 at (1, 2): a flat row, an even row, and a
    two-level row with odd counts"""
    def build():
        gy, gx = grid
        n = (1 << 26) // (gy * gx)
        hist = np.zeros((3, gy, gx, 256), np.int32)
        for j in range(gx):
            hist[0, 0, j, 200 - 90 * j] = n
            hist[1, 0, j, :] = n // 256
            hist[2, 0, j, 3 + j], hist[2, 0, j, 250 - j] = n - 12345677 - 2 * j, 12345677 + 2 * j
        hist.setflags(write=False)
        return dict(DEFAULTS, frames=None, hist=hist, L=3, H=8192, W=8192, n=n, scenes=None, grid=tuple(grid), max_shift=64)
    return build


_BUILDERS = {
    "5x7_g11": lambda: _case(_tilted(3, 5, 7, 50), (1, 1)),                      # 35 pixels: fewer than a wave
    "5x7_g22": lambda: _case(_tilted(3, 5, 7, 50), (2, 2)),                      # cells of 2 / 3 rows and 3 / 4 columns
    "w1_33x41_g23": lambda: _case(_tilted(4, 33, 41, 51), (2, 3)),               # W mod 4 = 1, column bounds 13 and 27, frames 1 .. 3 off a dword
    "w2_30x42_g34": lambda: _case(_tilted(4, 30, 42, 52), (3, 4)),               # W mod 4 = 2
    "8x8_g88": lambda: _case(_tilted(3, 8, 8, 53), (8, 8)),                      # every cell one pixel
    "9x300_g18": lambda: _case(_tilted(3, 9, 300, 54), (1, 8)),                  # one axis only
    "300x9_g81": lambda: _case(_tilted(3, 300, 9, 55), (8, 1)),
    "3x70x300_g34": lambda: _case(_tilted(3, 70, 300, 56), (3, 4)),              # several workgroups per frame and per cell row
    "3x90x301_g23": lambda: _case(_tilted(3, 90, 301, 59), (2, 3)),              # a cell row of 13 545 pixels: more than a workgroup's, off a group of four
    "flat_260x520_g12": _flat,
    "cuts_g23": lambda: _case(_tilted(6, 12, 14, 57), (2, 3), scenes=[1, 5]),
    "nondefault_g32": lambda: _case(_tilted(9, 20, 23, 58, (256, 320, 200, 290), (0, 12, -14)), (3, 2), scenes=[4], span=2, max_shift=5),
    "clip_g22": _clip,
    "rolled_g22": _rolled,
    "big_n_g11": _big_n((1, 1)),
    "big_n_g12": _big_n((1, 2)),
}
NAMES = tuple(_BUILDERS)
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def settings(c):
    return {k: c[k] for k in ("scenes",) + tuple(DEFAULTS)}


def keys(name):
    """the KEYS a case has: a case without frames (curves alone) has Q and d16"""
    return KEYS if case(name)["frames"] is not None else ("Q", "d16")


def want(name, **f):
    """the dict of keys(name) of a case under the definition (or a variant's flags); computed once, read-only"""
    key = (name,) + tuple(sorted(f))
    if key not in _WANT:
        c = case(name)
        if c["frames"] is None:
            Q, d16 = curves_np(c["hist"], C.scene_of_np(c["L"], c["scenes"]), c["H"], c["W"], c["span"], c["max_shift"], **f)
            w = dict(Q=Q, d16=d16)
        else:
            w = deflicker_local_np(c["frames"], **dict(settings(c), **f))
        for a in w.values():
            a.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ planted flicker and the measure
def plant_tilted(frames, seed, amp=0.1, off=8.0):
    rng = np.random.RandomState(seed); L, H, W = frames.shape[:3]
    yy, xx = np.mgrid[0:H, 0:W]; yy = yy / (H - 1) - 0.5; xx = xx / (W - 1) - 0.5
    out = np.empty_like(frames)
    for t in range(L):
        a, b, c = rng.uniform(-amp, amp, 3); o, p, q = rng.uniform(-off, off, 3)
        gain = 1 + a + 2 * b * xx + 2 * c * yy; offs = o + 2 * p * xx + 2 * q * yy
        out[t] = np.clip(np.rint(frames[t] * gain[..., None] + offs[..., None]), 0, 255)
    return out

def block_roughness(frames, bh=48, bw=54):   # blocks that do not line up with any grid
    Y = luma(frames).astype(np.float64); L, H, W = Y.shape
    m = Y[:, :H // bh * bh, :W // bw * bw].reshape(L, H // bh, bh, W // bw, bw).mean((2, 4))
    return float(np.abs(m[2:] - 2 * m[1:-1] + m[:-2]).mean())


luma = C.luma
_TENNIS = {}


def tennis(root, key):
    """tennis25 (key None), its planted version of a seed (key an int), and for a key (None or seed, "global" or grid) the
    restatement's output of that video at the defaults without a cut -- the global deflicker's or the grid's; computed once,
    read-only"""
    if key not in _TENNIS:
        if key is None or isinstance(key, int):
            a = C.tennis25(root) if key is None else plant_tilted(tennis(root, None), key)
        elif key[1] == "global":
            a = C.deflicker_np(tennis(root, key[0]), **C.DEFAULTS)["out"]
        else:
            a = deflicker_local_np(tennis(root, key[0]), **dict(DEFAULTS, grid=key[1]))["out"]
        a.setflags(write=False)
        _TENNIS[key] = a
    return _TENNIS[key]
