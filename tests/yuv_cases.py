"""The 4:2:0 pixel formats of e2fgvi_amd.video restated in numpy, on planes: Y [L,H,W], U and V [L,H/2,W/2] are cut out of the
frames first (split / join) and every formula of include/e2fgvi_hip.h is then written on whole planes, so the restatement cannot
share an addressing mistake with the kernels of csrc/yuv.hip, which walk strips of the interleaved bytes.  All arithmetic is int32,
``>>`` of a numpy signed integer is the floor shift.  Plus the content the tests run both through."""
import functools

import numpy as np

LAYOUTS = ("nv12", "i420")
CHROMAS = ("left", "nearest")
CONTENTS = ("random", "constant", "checker_luma", "checker_chroma", "hot")


def split(x, layout):
    """frames uint8 [L,3H/2,W] -> (Y [L,H,W], U [L,H/2,W/2], V [L,H/2,W/2])"""
    L, rows, W = x.shape
    H = rows // 3 * 2
    Y = x[:, :H]
    c = x[:, H:].reshape(L, -1)
    if layout == "nv12":
        c = c.reshape(L, H // 2, W // 2, 2)
        return Y, c[..., 0], c[..., 1]
    c = c.reshape(L, 2, H // 2, W // 2)
    return Y, c[:, 0], c[:, 1]


def join(Y, U, V, layout):
    L, H, W = Y.shape
    c = np.stack([U, V], -1) if layout == "nv12" else np.stack([U, V], 1)
    return np.ascontiguousarray(np.concatenate([Y.reshape(L, -1), c.reshape(L, -1)], 1).reshape(L, H // 2 * 3, W).astype(np.uint8))


def _left(C):
    """chroma plane [L,Hc,Wc] -> [L,2Hc,2Wc]: the taps of "left" siting, one rounding"""
    C = C.astype(np.int32)
    right = np.concatenate([C[:, :, 1:], C[:, :, -1:]], 2)
    Hh = np.empty(C.shape[:2] + (2 * C.shape[2],), np.int32)
    Hh[:, :, 0::2] = 2 * C
    Hh[:, :, 1::2] = C + right
    above = np.concatenate([Hh[:, :1], Hh[:, :-1]], 1)
    below = np.concatenate([Hh[:, 1:], Hh[:, -1:]], 1)
    out = np.empty((C.shape[0], 2 * C.shape[1], Hh.shape[2]), np.int32)
    out[:, 0::2] = above + 3 * Hh
    out[:, 1::2] = 3 * Hh + below
    return (out + 4) >> 3


def decode_np(x, layout, chroma, dec, yo):
    """frames [L,3H/2,W], dec = (cy, crv, cgu, cgv, cbu) -> uint8 [L,H,W,3]"""
    cy, crv, cgu, cgv, cbu = (int(v) for v in dec)
    Y, U, V = split(x, layout)
    if chroma == "left":
        u, v = _left(U) - 128, _left(V) - 128
    else:
        u = np.repeat(np.repeat(U.astype(np.int32), 2, 1), 2, 2) - 128
        v = np.repeat(np.repeat(V.astype(np.int32), 2, 1), 2, 2) - 128
    yy = cy * (Y.astype(np.int32) - yo)
    rgb = np.stack([(yy + crv * v + 8192) >> 14, (yy - cgu * u - cgv * v + 8192) >> 14, (yy + cbu * u + 8192) >> 14], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def _encode_planes(rgb, enc, yo):
    yr, yg, yb, ur, ug, ub, vr, vg, vb = (int(v) for v in enc)
    p = rgb.astype(np.int32)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = np.clip(yo + ((yr * R + yg * G + yb * B + 8192) >> 14), 0, 255)
    box = lambda a: a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
    SR, SG, SB = box(R), box(G), box(B)
    U = np.clip(128 + ((ur * SR + ug * SG + ub * SB + 32768) >> 16), 0, 255)
    V = np.clip(128 + ((vr * SR + vg * SG + vb * SB + 32768) >> 16), 0, 255)
    return Y, U, V


def encode_np(rgb, layout, enc, yo):
    """uint8 [L,H,W,3], enc = (yr, yg, yb, ur, ug, ub, vr, vg, vb) -> frames [L,3H/2,W]"""
    return join(*_encode_planes(rgb, enc, yo), layout)


def encode_paste_np(rgb, like_rgb, like, layout, enc, yo):
    Y, U, V = _encode_planes(rgb, enc, yo)
    lY, lU, lV = split(like, layout)
    same = (rgb == like_rgb).all(-1)
    block = same[:, 0::2, 0::2] & same[:, 0::2, 1::2] & same[:, 1::2, 0::2] & same[:, 1::2, 1::2]
    return join(np.where(same, lY, Y), np.where(block, lU, U), np.where(block, lV, V), layout)


def planes(kind, L, H, W, seed=0):
    """(Y, U, V) of the content ``kind``: random bytes (out-of-range levels included), a constant colour per frame, a one-pixel
    checkerboard in luma, one in chroma, and single hot samples at every corner and edge of both planes (the clamped taps)"""
    rng = np.random.RandomState(1000 * seed + 7 * L + 3 * H + W)
    Hc, Wc = H // 2, W // 2
    if kind == "random":
        return tuple(rng.randint(0, 256, s).astype(np.uint8) for s in ((L, H, W), (L, Hc, Wc), (L, Hc, Wc)))
    if kind == "constant":
        c = rng.randint(0, 256, (L, 3, 1, 1)).astype(np.uint8)
        return (np.broadcast_to(c[:, 0], (L, H, W)).copy(), np.broadcast_to(c[:, 1], (L, Hc, Wc)).copy(),
                np.broadcast_to(c[:, 2], (L, Hc, Wc)).copy())
    grid = lambda h, w: (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(np.uint8)
    if kind == "checker_luma":
        Y = np.stack([np.where(grid(H, W) ^ (l & 1), 235, 16) for l in range(L)]).astype(np.uint8)
        return Y, np.full((L, Hc, Wc), 128, np.uint8), np.full((L, Hc, Wc), 128, np.uint8)
    if kind == "checker_chroma":
        g = np.stack([grid(Hc, Wc) ^ (l & 1) for l in range(L)])
        return (np.full((L, H, W), 126, np.uint8), np.where(g, 240, 16).astype(np.uint8), np.where(g, 16, 240).astype(np.uint8))
    if kind == "hot":
        Y, U, V = np.full((L, H, W), 60, np.uint8), np.full((L, Hc, Wc), 128, np.uint8), np.full((L, Hc, Wc), 128, np.uint8)
        for l in range(L):
            for k, (fy, fx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1), (0, .5), (.5, 0), (1, .5), (.5, 1)]):
                if l == 0 or k == l % 8:                # frame 0: all eight; the others one each
                    Y[l, int(fy * (H - 1)), int(fx * (W - 1))] = 255
                    U[l, int(fy * (Hc - 1)), int(fx * (Wc - 1))] = 255 if k & 1 else 0
                    V[l, int(fy * (Hc - 1)), int(fx * (Wc - 1))] = 0 if k & 2 else 255
        return Y, U, V
    raise ValueError(kind)


def frames(kind, L, H, W, layout, seed=0):
    return join(*planes(kind, L, H, W, seed), layout)


def rgb_frames(kind, L, H, W, seed=0):
    """RGB content of the same kinds: the three planes at full size as R, G and B"""
    Y, U, V = planes(kind, L, 2 * H, 2 * W, seed)
    return np.ascontiguousarray(np.stack([Y[:, :H, :W], U[:, :H, :W], V[:, :H, :W]], -1))


@functools.lru_cache(maxsize=None)
def all_triples_yuv(layout):
    """one 4096 x 4096 frame that holds every (Y, U, V) triple once: block b = 2048 bj + bi has the chroma pair (b >> 14, (b >> 6) &
    255) and the four luma values 4 (b & 63) + (0, 1, 2, 3)"""
    b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    U, V = (b >> 14).astype(np.uint8), ((b >> 6) & 255).astype(np.uint8)
    Y = np.empty((4096, 4096), np.uint8)
    for k, (dy, dx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        Y[dy::2, dx::2] = 4 * (b & 63) + k
    x = join(Y[None], U[None], V[None], layout)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def all_triples_rgb():
    """one 4096 x 4096 frame that holds every (R, G, B) triple once: pixel p = 4096 y + x is (p >> 16, (p >> 8) & 255, p & 255)"""
    p = np.arange(4096 * 4096, dtype=np.int64).reshape(1, 4096, 4096)
    x = np.stack([p >> 16, (p >> 8) & 255, p & 255], -1).astype(np.uint8)
    x.setflags(write=False)
    return x


def decode_float(x, layout, matrix, full_range):
    """the rounded, clipped float64 formula with nearest chroma: what the Q14 integers approximate"""
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
    kg = 1.0 - kr - kb
    ys, cs, yo = (1.0, 1.0, 0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16)
    Y, U, V = split(x, layout)
    u = (np.repeat(np.repeat(U, 2, 1), 2, 2).astype(np.float64) - 128.0) * cs
    v = (np.repeat(np.repeat(V, 2, 1), 2, 2).astype(np.float64) - 128.0) * cs
    yy = (Y.astype(np.float64) - yo) * ys
    rgb = np.stack([yy + 2 * (1 - kr) * v, yy - 2 * kb * (1 - kb) / kg * u - 2 * kr * (1 - kr) / kg * v, yy + 2 * (1 - kb) * u], -1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)
