"""Frame interpolation restated in numpy (ops.interpolate, video.retime, video.replace_frames; the definition is in
include/e2fgvi_hip.h), the named cases the device code is compared with byte for byte, mutated restatements (VARIANTS) that must
each differ from the definition on a case named for them -- which is what shows that the cases can see such a mistake -- and the
planted clip the definition is judged on.  fp64 in the order written, then integers: there is no tolerance anywhere.  Written
unlike the kernel on purpose: a job's whole frame at once, a side's state as planes and masks, flows read through flat indices."""
import numpy as np

DEFAULTS = dict(iterations=3, tolerance=8, match=96)
DEFAULT = (3, 8, 96)
# (flag, the case that must see it, the (iterations, tolerance, match) it is seen at)
CAUGHT_BY = (
    ("tap_no_half", "pan_33x70", (3, 8, 96)),               # tap16: Q = floor(16 q), without the half
    ("later_strict", "unmatched_17x23", (3, 8, 96)),        # one-ended: A's side while 2 k < d, not 2 k <= d
    ("tie_strict", "smooth_33x70", (3, 8, 96)),             # both matched: A's side while cost_A < cost_B, not <=
    ("sum_first", "thirds_33x70", (3, 0, 765)),             # the residual as q + (lambda hq - x), not (q + lambda hq) - x
    ("inside_after_trunc", "edges_17x23", (3, 8, 765)),     # inside tested on the coordinates truncated to integers
    # a corner of bil outside the image read all the same, from the address behind it (its weight is 0: only a non-finite flow
    # there can show).  The clamp of tap16's corner indices cannot be seen in a byte: the weight there is 0 and bytes are finite.
    ("corner_unguarded", "lastcol_7x9", (3, 8, 765)),
    ("round_d", "pan_33x70", (3, 8, 96)),                   # the matched colour without the + d / 2
    ("landing_strict", "halves_17x23", (3, 0, 96)),         # landed when |r|^2 < the bound, not <=
)
VARIANTS = tuple((name, {name: True}) for name, _, _ in CAUGHT_BY)


def _inside(qx, qy, H, W, f):
    with np.errstate(invalid="ignore"):
        if f.get("inside_after_trunc"):
            fin = np.isfinite(qx) & np.isfinite(qy)
            tx, ty = np.trunc(np.where(fin, qx, -9.0)), np.trunc(np.where(fin, qy, -9.0))
            return fin & (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
        return np.isfinite(qx) & np.isfinite(qy) & (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)


def _bil(hflat, base, qx, qy, ok, H, W, f):
    """the four-corner sample at q where ``ok`` (elsewhere: anything); hflat float64 [P H W, 2], base the pair's first pixel"""
    qx, qy = np.where(ok, qx, 0.0), np.where(ok, qy, 0.0)
    x0, y0 = np.floor(qx), np.floor(qy)
    wx1, wy1 = qx - x0, qy - y0
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    hx, hy = x0 + 1 < W, y0 + 1 < H
    if f.get("corner_unguarded"):
        hx, hy = np.ones_like(hx), np.ones_like(hy)
    o00 = base + np.clip(y0, 0, H - 1) * W + np.clip(x0, 0, W - 1)
    last = hflat.shape[0] - 1
    with np.errstate(invalid="ignore", over="ignore"):
        c = (wy0 * wx0)[..., None] * hflat[o00]
        for on, w, o in ((hx, wy0 * wx1, o00 + 1), (hy, wy1 * wx0, o00 + W), (hx & hy, wy1 * wx1, o00 + W + 1)):
            c = np.where(on[..., None], c + w[..., None] * hflat[np.minimum(o, last)], c)
    return c[..., 0], c[..., 1]


def _tap16(T, qx, qy, ok, f):
    """T int64 [H,W,3] at q on the 1/16 px grid where ``ok`` (elsewhere: anything)"""
    H, W = T.shape[:2]
    half = 0.0 if f.get("tap_no_half") else 0.5
    Qx = np.floor(np.where(ok, qx, 0.0) * 16.0 + half).astype(np.int64)
    Qy = np.floor(np.where(ok, qy, 0.0) * 16.0 + half).astype(np.int64)
    Qx, Qy = np.clip(Qx, 0, 16 * (W - 1)), np.clip(Qy, 0, 16 * (H - 1))        # a no-op under the definition
    xi, fx, yi, fy = Qx >> 4, (Qx & 15)[..., None], Qy >> 4, (Qy & 15)[..., None]
    x1, y1 = np.minimum(xi + 1, W - 1), np.minimum(yi + 1, H - 1)
    return ((16 - fy) * ((16 - fx) * T[yi, xi] + fx * T[yi, x1]) + fy * ((16 - fx) * T[y1, xi] + fx * T[y1, x1]) + 128) >> 8


def _side(S, E, hflat, base, lam, iterations, bound, f):
    H, W = S.shape[:2]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    h0 = hflat[base:base + H * W].reshape(H, W, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = xx - lam * h0[..., 0], yy - lam * h0[..., 1]
        alive = np.ones((H, W), bool)
        for _ in range(iterations):
            alive = alive & _inside(qx, qy, H, W, f)
            cx, cy = _bil(hflat, base, qx, qy, alive, H, W, f)
            alive = alive & np.isfinite(cx) & np.isfinite(cy)
            qx, qy = np.where(alive, xx - lam * cx, qx), np.where(alive, yy - lam * cy, qy)
        alive = alive & _inside(qx, qy, H, W, f)
        cx, cy = _bil(hflat, base, qx, qy, alive, H, W, f)
        alive = alive & np.isfinite(cx) & np.isfinite(cy)
        cx, cy = np.where(alive, cx, 0.0), np.where(alive, cy, 0.0)
        qx, qy = np.where(alive, qx, 0.0), np.where(alive, qy, 0.0)
        if f.get("sum_first"):
            rx, ry = qx + (lam * cx - xx), qy + (lam * cy - yy)
        else:
            rx, ry = (qx + lam * cx) - xx, (qy + lam * cy) - yy
        rr = rx * rx + ry * ry
        landed = alive & ((rr < bound) if f.get("landing_strict") else (rr <= bound))
        ex, ey = qx + cx, qy + cy
        two = landed & _inside(ex, ey, H, W, f)
    s = _tap16(S, qx, qy, landed, f)
    t = _tap16(E, ex, ey, two, f)
    cost = np.abs(s - t).sum(-1)
    return landed, two, s, t, cost


def reference(frames, fwd, bwd, jobs, iterations, tolerance, match, out=None, source=None, **f):
    """the definition: frames uint8 [L,H,W,3]; fwd, bwd fp32 [P,H,W,2]; jobs int [n,5] -> (out uint8 [n,H,W,3], source uint8
    [n,H,W]); a job outside its ranges leaves its frames of ``out`` / ``source`` (zeros without them) as they are"""
    fr = np.asarray(frames).astype(np.int64)
    L, H, W = fr.shape[:3]
    P = np.asarray(fwd).shape[0]
    jobs = np.asarray(jobs, np.int64).reshape(-1, 5)
    n = len(jobs)
    out = np.zeros((n, H, W, 3), np.uint8) if out is None else np.array(out, np.uint8)
    source = np.zeros((n, H, W), np.uint8) if source is None else np.array(source, np.uint8)
    if H * W == 0:
        return out, source
    flat = [np.asarray(a, np.float32).astype(np.float64).reshape(-1, 2) for a in (fwd, bwd)]
    bound = float(tolerance * tolerance) / 256.0
    for j, (ia, ib, fi, k, d) in enumerate(jobs.tolist()):
        if not (0 <= ia < L and 0 <= ib < L and 0 <= fi < P and 1 <= d <= 64 and 0 <= k <= d):
            continue
        A, B = fr[ia], fr[ib]
        if k == 0 or k == d:
            out[j], source[j] = (A if k == 0 else B), 5
            continue
        tau, sigma = float(k) / float(d), float(d - k) / float(d)
        base = fi * H * W
        la, twa, sa, ta, ca = _side(A, B, flat[0], base, tau, iterations, bound, f)
        lb, twb, sb, tb, cb = _side(B, A, flat[1], base, sigma, iterations, bound, f)
        ma, mb = twa & (ca <= match), twb & (cb <= match)
        half = 0 if f.get("round_d") else d // 2
        col_a = ((d - k) * sa + k * ta + half) // d
        col_b = ((d - k) * tb + k * sb + half) // d
        fade = ((d - k) * A + k * B + half) // d
        first = ma & (~mb | ((ca < cb) if f.get("tie_strict") else (ca <= cb)))
        second = ~first & mb
        none = ~first & ~second
        early = (2 * k < d) if f.get("later_strict") else (2 * k <= d)
        third = none & la & (~lb | early)
        fourth = none & ~third & lb
        code = np.select([first, second, third, fourth], [1, 2, 3, 4], 0)
        col = np.select([m[..., None] for m in (first, second, third, fourth)], [col_a, col_b, sa, sb], fade)
        out[j], source[j] = col.astype(np.uint8), code.astype(np.uint8)
    return out, source


def crossfade(A, B, k, d):
    A, B = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
    return (((d - k) * A + k * B + d // 2) // d).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ named cases
FRACTIONS = ((0, 1), (1, 1), (1, 2), (1, 3), (2, 3), (1, 64), (63, 64), (32, 64))


def noise(L, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (L, H, W, 3)).astype(np.uint8)


def soft(L, H, W, seed, sigma=2.0):
    """one smooth picture, the same in every frame up to noise of a few levels: the two ends of a short trajectory match"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (H + 4, W + 4, 3)).astype(np.float64)
    base = sum(a[j:j + H, k:k + W] for j in range(5) for k in range(5)) / 25.0
    base = 128 + (base - 128) * 3
    return np.clip(np.rint(base[None] + sigma * rng.standard_normal((L, H, W, 3))), 0, 255).astype(np.uint8)


def const_flows(P, H, W, fx, fy):
    """fwd = (fx, fy) everywhere, bwd = its negative"""
    fwd = np.zeros((P, H, W, 2), np.float32)
    fwd[..., 0], fwd[..., 1] = fx, fy
    return fwd, -fwd


def random_flows(P, H, W, seed, amp=6.0):
    rng = np.random.RandomState(seed)
    return tuple((amp * (2 * rng.random_sample((P, H, W, 2)) - 1)).astype(np.float32) for _ in range(2))


def all_jobs(L, P, fractions=FRACTIONS):
    """every fraction, over adjacent and non-adjacent frames in both directions and over a frame with itself, the pairs in turn"""
    pairs = [(a, b) for a in range(L) for b in range(L)]
    return [(pairs[(3 * i + 1) % len(pairs)] + (i % P, k, d)) for i, (k, d) in enumerate(fractions)]


def _case(frames, flows, jobs):
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    fwd, bwd = (np.ascontiguousarray(a, dtype=np.float32) for a in flows)
    jobs = np.ascontiguousarray(np.asarray(jobs, np.int32).reshape(-1, 5))
    for a in (frames, fwd, bwd, jobs):
        a.setflags(write=False)
    L, H, W = frames.shape[:3]
    return dict(frames=frames, fwd=fwd, bwd=bwd, jobs=jobs, L=L, H=H, W=W, P=fwd.shape[0])


def _edges(P, H, W):
    """at the fraction 1/2: per column and row a start q = p - h / 2 exactly on the last column / row, just outside them, on -0.5,
    on 0, 0.4 outside on either side and half a pixel outside"""
    fwd, bwd = np.zeros((P, H, W, 2), np.float32), np.zeros((P, H, W, 2), np.float32)
    kinds = (lambda n: n - 1, lambda n: np.nextafter(np.float32(n - 1), np.float32(n)), lambda n: -0.5, lambda n: 0.0,
             lambda n: n - 1 + 0.4, lambda n: -0.4, lambda n: n - 0.5)
    for x in range(W):
        fwd[:, :, x, 0] = 2.0 * (x - kinds[x % len(kinds)](W))
        bwd[:, :, x, 0] = 2.0 * (x - kinds[(x + 3) % len(kinds)](W))
    for y in range(H):
        fwd[:, y, :, 1] = 2.0 * (y - kinds[(y + 1) % len(kinds)](H))
        bwd[:, y, :, 1] = 2.0 * (y - kinds[(y + 4) % len(kinds)](H))
    return fwd, bwd


def _ends(P, H, W):
    """constant flows whose far end q + h falls on the last row and column for the first rows and columns, and outside for others"""
    return const_flows(P, H, W, 2.0 * ((W - 1) // 4), 2.0 * ((H - 1) // 4))      # even: at the fraction 1/2 the ends are pixels


def _nonfinite(P, H, W, seed, bad=(np.nan, np.inf, -np.inf, 1e30, -1e30)):
    fwd, bwd = (a.copy() for a in const_flows(P, H, W, 0.75, -0.5))
    rng = np.random.RandomState(seed)
    for a in (fwd, bwd):
        hit = rng.randint(0, 8, a.shape)
        which = rng.randint(0, len(bad), a.shape)
        a[hit == 0] = np.asarray(bad, np.float32)[which[hit == 0]]
    return fwd, bwd


def _lastcol(P, H, W):
    """flows of two rows straight down, so that at the fraction 1/2 the last column starts on itself one row up, and NaN flows in
    column 0: what lies at the address behind that start's"""
    fwd, bwd = const_flows(P, H, W, 0.0, 2.0)
    fwd, bwd = fwd.copy(), bwd.copy()
    fwd[:, :, 0], bwd[:, :, 0] = np.nan, np.nan
    return fwd, bwd


def _occlusion(H, W, v=(6.0, -1.0)):
    """two frames: a textured still background and an object of another texture over the middle third that moves by v; exact flows.
    What the object uncovers and covers is seen in one frame only."""
    bg, ob = soft(1, H, W, 50)[0], soft(1, H + 8, W + 8, 51)[0]
    y0, y1, x0, x1 = H // 4, H - H // 4, W // 3, W // 3 + max(W // 4, 1)
    A, B = bg.copy(), bg.copy()
    fwd, bwd = np.zeros((1, H, W, 2), np.float32), np.zeros((1, H, W, 2), np.float32)
    dx, dy = int(v[0]), int(v[1])
    A[y0:y1, x0:x1] = ob[y0:y1, x0:x1]
    fwd[0, y0:y1, x0:x1] = v
    by0, by1, bx0, bx1 = max(y0 + dy, 0), min(y1 + dy, H), max(x0 + dx, 0), min(x1 + dx, W)
    B[by0:by1, bx0:bx1] = ob[by0 - dy:by1 - dy, bx0 - dx:bx1 - dx]
    bwd[0, by0:by1, bx0:bx1] = (-v[0], -v[1])
    return np.stack([A, B]), (fwd, bwd)


def _pan(L, H, W, seed, v):
    """frames that show one smooth picture (the far ends match) under constant flows v: every pixel lands, most are two-ended"""
    return soft(L, H, W, seed), const_flows(L - 1, H, W, *v)


SIZES = ((1, 1), (1, 9), (7, 1), (17, 23), (33, 70), (64, 128))
_BUILDERS = {}
for _H, _W in SIZES:
    # random bytes along random flows of +-6 px, three frames and two pairs: few trajectories land
    _BUILDERS["random_%dx%d" % (_H, _W)] = lambda H=_H, W=_W: _case(noise(3, H, W, 10 * H + W), random_flows(2, H, W, H + W),
                                                                     all_jobs(3, 2))
    # a smooth picture under a constant flow off the 1/16 px grid, four frames and three pairs: most pixels match
    _BUILDERS["pan_%dx%d" % (_H, _W)] = lambda H=_H, W=_W: _case(*_pan(4, H, W, 11 * H + W, (1.3, -0.7)), all_jobs(4, 3))
_MID = ((0, 1, 0, 1, 2), (1, 0, 0, 1, 2), (0, 1, 0, 32, 64), (0, 0, 0, 1, 2))
_BUILDERS.update({
    "zero_17x23": lambda: _case(soft(2, 17, 23, 20), const_flows(1, 17, 23, 0, 0), all_jobs(2, 1)),
    "zero_64x128": lambda: _case(soft(5, 64, 128, 21), const_flows(4, 64, 128, 0, 0), all_jobs(5, 4)),
    "halves_17x23": lambda: _case(soft(3, 17, 23, 22), const_flows(2, 17, 23, 2.5, -1.5), all_jobs(3, 2)),
    "sixteenths_17x23": lambda: _case(soft(3, 17, 23, 23), const_flows(2, 17, 23, 0.5625, -2.1875), all_jobs(3, 2)),
    "thirds_33x70": lambda: _case(soft(2, 33, 70, 24), const_flows(1, 33, 70, 1.0 / 3.0, -0.7), all_jobs(2, 1)),
    "edges_17x23": lambda: _case(soft(2, 17, 23, 25), _edges(1, 17, 23), _MID),
    "edges_7x1": lambda: _case(soft(2, 7, 1, 26), _edges(1, 7, 1), _MID),
    "edges_1x9": lambda: _case(soft(2, 1, 9, 27), _edges(1, 1, 9), _MID),
    "ends_17x23": lambda: _case(soft(2, 17, 23, 28), _ends(1, 17, 23), _MID + ((0, 1, 0, 1, 3), (0, 1, 0, 63, 64))),
    "minus_half_17x23": lambda: _case(soft(2, 17, 23, 29), const_flows(1, 17, 23, -0.5, -0.5), all_jobs(2, 1)),
    "nonfinite_17x23": lambda: _case(soft(3, 17, 23, 30), _nonfinite(2, 17, 23, 31), all_jobs(3, 2)),
    "huge_17x23": lambda: _case(soft(2, 17, 23, 32), _nonfinite(1, 17, 23, 33, (1e30, -1e30, 3e38)), all_jobs(2, 1)),
    "lastcol_7x9": lambda: _case(soft(2, 7, 9, 34), _lastcol(1, 7, 9), _MID),
    "occlusion_33x70": lambda: _case(*_occlusion(33, 70), jobs=((0, 1, 0, 1, 2), (0, 1, 0, 1, 3), (0, 1, 0, 2, 3), (0, 1, 0, 63, 64),
                                                              (0, 1, 0, 1, 64))),
    "occlusion_64x128": lambda: _case(*_occlusion(64, 128, (7.0, 2.0)), jobs=((0, 1, 0, 1, 2), (0, 1, 0, 2, 3), (0, 1, 0, 1, 3))),
    # random bytes under a constant flow: everything lands, nothing matches unless match is 765
    "unmatched_17x23": lambda: _case(noise(3, 17, 23, 35), const_flows(2, 17, 23, 1.25, 0.5), all_jobs(3, 2)),
    # 0 and 255 alone: |s - t| is 0 or 255 and the taps reach both ends of a byte
    "extremes_17x23": lambda: _case(255 * np.random.RandomState(36).randint(0, 2, (3, 17, 23, 3)), const_flows(2, 17, 23, 0.75, 1.5),
                                    all_jobs(3, 2)),
    "extremes_64x128": lambda: _case(255 * (np.random.RandomState(37).randint(0, 8, (2, 64, 128, 1)) > 0) + np.zeros((1, 1, 1, 3)),
                                     random_flows(1, 64, 128, 38, 0.5), all_jobs(2, 1)),
    "five_33x70": lambda: _case(*_pan(5, 33, 70, 39, (-2.0625, 0.4)), all_jobs(5, 4)),
    # flows that vary smoothly: the fixed point has something to do
    "smooth_33x70": lambda: _case(soft(2, 33, 70, 40), _smooth_flows(33, 70), all_jobs(2, 1)),
})


def _smooth_flows(H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    fx, fy = 3.0 + 2.0 * np.sin(xx / 9.0 + yy / 13.0), -1.0 + 1.5 * np.cos(xx / 11.0 - yy / 7.0)
    fwd = np.stack([fx, fy], -1)[None].astype(np.float32)
    return fwd, (-fwd).astype(np.float32)


NAMES = tuple(_BUILDERS)
# every setting a case is run with on the device: (iterations, tolerance, match)
SETTINGS = ((3, 8, 96), (0, 8, 96), (1, 0, 0), (8, 255, 765), (3, 0, 765), (0, 255, 0), (8, 8, 0), (1, 8, 765), (3, 0, 96))
_CASES, _WANT = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


def want(name, setting=DEFAULT, **f):
    """(out, source) of a case at (iterations, tolerance, match) under the definition (or a variant's flags); computed once,
    read-only"""
    key = (name, tuple(setting)) + tuple(sorted(f))
    if key not in _WANT:
        c = case(name)
        w = reference(c["frames"], c["fwd"], c["bwd"], c["jobs"], *setting, **f)
        for a in w:
            a.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ the planted clip
CLIP_H, CLIP_W = 96, 160
CLIP_PAN, CLIP_OBJ_V, CLIP_OBJ_HW, CLIP_OBJ_AT = (1.5, 0.5), (7.0, -1.0), (24, 30), (40.0, 36.0)


def _texture(x, y, seed):
    """a band-limited picture that can be drawn at any real position: a sum of sinusoids per channel, float64 [...,3] in 0..255"""
    rng = np.random.RandomState(seed)
    out = np.zeros(x.shape + (3,))
    for ch in range(3):
        v = np.zeros(x.shape)
        for _ in range(12):
            fx, fy = rng.uniform(-0.45, 0.45, 2)
            v += rng.uniform(0.3, 1.0) * np.sin(fx * x + fy * y + rng.uniform(0, 2 * np.pi))
        out[..., ch] = 128 + 40 * v / 2.5
    return out


def clip_frame(t):
    """the planted clip at the real time t: a 96 x 160 textured pan of (1.5, 0.5) px a frame with a 24 x 30 object of another texture
    on top that moves by (7, -1) px a frame -> (uint8 [H,W,3], the object's mask)"""
    yy, xx = np.mgrid[0:CLIP_H, 0:CLIP_W].astype(np.float64)
    img = _texture(xx + CLIP_PAN[0] * t, yy + CLIP_PAN[1] * t, 60)
    ox, oy = CLIP_OBJ_AT[0] + CLIP_OBJ_V[0] * t, CLIP_OBJ_AT[1] + CLIP_OBJ_V[1] * t
    obj = (xx >= ox) & (xx < ox + CLIP_OBJ_HW[1]) & (yy >= oy) & (yy < oy + CLIP_OBJ_HW[0])
    img[obj] = _texture(xx - ox, yy - oy, 61)[obj] * 0.6 + 90
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), obj


def clip_pair(noise_px=0.0, seed=7):
    """(frames uint8 [2,H,W,3], fwd, bwd fp32 [1,H,W,2]): the clip at t = 0 and t = 1 with its exact flows, plus Gaussian flow noise
    of ``noise_px`` px"""
    (A, ma), (B, mb) = clip_frame(0.0), clip_frame(1.0)
    fwd = np.zeros((1, CLIP_H, CLIP_W, 2)) + (-CLIP_PAN[0], -CLIP_PAN[1])
    bwd = np.zeros((1, CLIP_H, CLIP_W, 2)) + (CLIP_PAN[0], CLIP_PAN[1])
    fwd[0][ma] = CLIP_OBJ_V
    bwd[0][mb] = (-CLIP_OBJ_V[0], -CLIP_OBJ_V[1])
    if noise_px:
        rng = np.random.RandomState(seed)
        fwd, bwd = fwd + noise_px * rng.standard_normal(fwd.shape), bwd + noise_px * rng.standard_normal(bwd.shape)
    return np.stack([A, B]), fwd.astype(np.float32), bwd.astype(np.float32)


def psnr(a, b):
    err = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(10 * np.log10(255.0 ** 2 / np.mean(err ** 2)))
