"""Real pixels for restored holes (e2fgvi_amd.video.propagate_pixels, ops.pixel_track_step, ops.pixel_fill, csrc/pixel_track.hip):
the float64 numpy restatement of the step, of the chains and of the fill, written from the definition in include/e2fgvi_hip.h, and
the named cases both test files run.  It has a sampler of its own (indices clipped into the image, corners outside it selected
away) and walks one chain after the other, scene by scene -- neither the kernels' addressing nor the planner's lockstep order.

The step, for a destination pixel p = (x, y) of frame d with hole[d](p) == 1, the source frame s of the same plane, pull flow g and
check flow c (fp64 on the fp32 / uint8 inputs, in the order written):
    q = (x + g_x(p), y + g_y(p));  inside = g(p) finite and 0 <= q_x <= W-1 and 0 <= q_y <= H-1
    c* = (floor(q_x + 0.5), floor(q_y + 0.5));  a = age[s](c*)
    c_w = bil(c, q): four corners, those outside the image contribute 0, added in the order (y0,x0), (y0,x0+1), (y0+1,x0),
        (y0+1,x0+1);  inconsistent = c_w not finite, or  sx sx + sy sy > 0.01 ((g_x g_x + g_y g_y) + (c_wx c_wx + c_wy c_wy)) + 0.5,
        s. = g + c_w
    reached = inside and a != 255 and a + 1 <= reach and (not check or not inconsistent)
    reached: age[d](p) = a + 1, origin[d](p) = fp32(O_c + (q - c*)), O_c = c* if a == 0 else origin[s](c*);  else age[d](p) = 255
The fill, for a pixel p of frame t with hole[t](p) == 1: the planes in the order of their ages (a tie: plane 0; 255: no candidate);
a candidate of age a names f = t - a (plane 0) or t + a (plane 1) and O = origin(p); it holds iff f is a frame, O is finite and in
the image and every bilinear corner of O with a non-zero weight is in the image and no hole pixel of f; the first that holds gives
min(255, floor(bil(src[f], O) + 0.5)) per channel and source 1 + plane; none: the byte stays, source 3.

VARIANTS are deliberately wrong readings of the text; the CPU tests require each of them to change the result of some case."""
import numpy as np

from tests import mask_key_cases as K

VARIANTS = ("nearest_floor", "no_subpixel", "age_not_incremented", "tie_plane1", "hole_corners_ok", "border_clamp", "check_at_p",
            "swap_channels", "carry_colours")
REACH_MAX = 254


def _bil(T, qx, qy, clamp=False):
    """T [H,W,C] float64 sampled at (qx, qy) (arrays of one shape, 0 <= q <= size - 1): the four corners in the order (y0,x0),
    (y0,x0+1), (y0+1,x0), (y0+1,x0+1), a corner outside the image contributing 0 (``clamp``: the border pixel instead)"""
    H, W = T.shape[:2]
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    wx1, wy1 = qx - x0, qy - y0
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    out = None
    for dy, dx, w in ((0, 0, wy0 * wx0), (0, 1, wy0 * wx1), (1, 0, wy1 * wx0), (1, 1, wy1 * wx1)):
        xc, yc = x0 + dx, y0 + dy
        there = (xc < W) & (yc < H)
        v = T[np.minimum(yc, H - 1), np.minimum(xc, W - 1)]
        term = w[..., None] * v
        if not clamp:
            term = np.where(there[..., None], term, 0.0)
        out = term if out is None else out + term
    return out


def step_np(hole_d, age_s, org_s, age_d, org_d, g, c, reach=REACH_MAX, check=True, variant=None, col_s=None, col_d=None):
    """one job: hole_d uint8 [H,W]; age_s, org_s the source frame of the plane; age_d [H,W] and org_d [H,W,2] are written at the
    hole pixels of the destination; g, c fp32 [H,W,2].  col_s / col_d (variant carry_colours): the colours [H,W,3] float64 that
    variant drags along, resampled at every step."""
    H, W = hole_d.shape
    g64, c64 = g.astype(np.float64), c.astype(np.float64)
    if variant == "swap_channels":
        g64, c64 = g64[..., ::-1], c64[..., ::-1]
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        gx, gy = g64[..., 0], g64[..., 1]
        qx, qy = xs.astype(np.float64) + gx, ys.astype(np.float64) + gy
        finite = np.isfinite(gx) & np.isfinite(gy)
        if variant == "border_clamp":
            inside = finite
            qx, qy = np.clip(qx, 0.0, float(W - 1)), np.clip(qy, 0.0, float(H - 1))
        else:
            inside = finite & (qx >= 0.0) & (qx <= float(W - 1)) & (qy >= 0.0) & (qy <= float(H - 1))
        qx, qy = np.where(inside, qx, 0.0), np.where(inside, qy, 0.0)       # excluded pixels read pixel (0, 0) and are dropped below
        if variant == "nearest_floor":
            nx, ny = np.floor(qx), np.floor(qy)
        else:
            nx, ny = np.floor(qx + 0.5), np.floor(qy + 0.5)
        ix, iy = nx.astype(np.int64), ny.astype(np.int64)
        a = age_s[iy, ix].astype(np.int64)
        cw = c64 if variant == "check_at_p" else _bil(c64, qx, qy, clamp=variant == "border_clamp")
        cx, cy = cw[..., 0], cw[..., 1]
        sx, sy = gx + cx, gy + cy
        lhs = sx * sx + sy * sy
        rhs = 0.01 * ((gx * gx + gy * gy) + (cx * cx + cy * cy)) + 0.5
        bad = ~(np.isfinite(cx) & np.isfinite(cy)) | (lhs > rhs)
        reached = inside & (a != 255) & (a + 1 <= reach)
        if check:
            reached &= ~bad
        ocx = np.where(a == 0, nx, org_s[iy, ix, 0].astype(np.float64))
        ocy = np.where(a == 0, ny, org_s[iy, ix, 1].astype(np.float64))
        if variant == "no_subpixel":
            ox, oy = ocx, ocy
        else:
            ox, oy = ocx + (qx - nx), ocy + (qy - ny)
        new_age = a if variant == "age_not_incremented" else a + 1
        if col_s is not None:                           # the blurred colour: a bilinear sample of the colours carried so far
            known = (age_s != 255).astype(np.float64)[..., None]
            num, den = _bil(col_s * known, qx, qy), _bil(known, qx, qy)
            col = np.where(den > 0, num / np.where(den > 0, den, 1.0), col_s[iy, ix])
    sel = hole_d == 1
    age_d[sel] = np.where(reached, new_age, 255)[sel].astype(np.uint8)
    put = sel & reached
    org_d[put, 0], org_d[put, 1] = ox[put].astype(np.float32), oy[put].astype(np.float32)
    if col_s is not None:
        col_d[put] = col[put]


def chains_np(length, scenes=None):
    """the chains, one list of (pair, dir) per scene and direction, each in the order its jobs must run"""
    cuts = sorted(scenes or ())
    out = []
    for a, b in zip([0] + cuts, cuts + [length]):
        out.append([(t, 0) for t in range(a, b - 1)])
        out.append([(t, 1) for t in range(b - 2, a - 1, -1)])
    return out


def planes_np(case, check=True, variant=None):
    """both planes after all chains of a case -> (age uint8 [2,L,H,W], origin fp32 [2,L,H,W,2], colours or None): origin holds NaN
    where nothing was stored"""
    L, H, W = case["L"], case["H"], case["W"]
    hole, fwd, bwd = case["hole"], case["fwd"], case["bwd"]
    age = np.stack([hole * 255, hole * 255]).astype(np.uint8)
    origin = np.full((2, L, H, W, 2), np.nan, np.float32)
    col = None
    if variant == "carry_colours":
        col = np.stack([case["src"].astype(np.float64)] * 2)
    for chain in chains_np(L, case.get("scenes")):
        for t, d in chain:
            s, dst = (t, t + 1) if d == 0 else (t + 1, t)
            g, c = (bwd[t], fwd[t]) if d == 0 else (fwd[t], bwd[t])
            step_np(hole[dst], age[d, s], origin[d, s], age[d, dst], origin[d, dst], g, c, case.get("reach") or REACH_MAX, check, variant,
                    None if col is None else col[d, s], None if col is None else col[d, dst])
    return age, origin, col


def fill_np(case, age, origin, variant=None, col=None):
    """the fill over all frames -> (out uint8 [L,H,W,3], source uint8 [L,H,W])"""
    L, H, W = case["L"], case["H"], case["W"]
    hole, src = case["hole"], case["src"].astype(np.float64)
    out, source = np.array(case["filled"]), np.zeros((L, H, W), np.uint8)
    for t in range(L):
        ys, xs = np.nonzero(hole[t] == 1)
        if not len(ys):
            continue
        a = age[:, t, ys, xs].astype(np.int64)                     # [2, n]
        first = np.where(a[0] < a[1], 0, 1) if variant == "tie_plane1" else np.where(a[0] <= a[1], 0, 1)
        done = np.zeros(len(ys), bool)
        code = np.full(len(ys), 3, np.uint8)
        rgb = out[t, ys, xs].astype(np.float64)
        for k in (0, 1):
            for pl in (0, 1):
                m = ~done & ((first if k == 0 else 1 - first) == pl) & (a[pl] != 255)
                if not m.any():
                    continue
                am = a[pl][m]
                f = t + am if pl else t - am
                ox = np.where(am == 0, xs[m], origin[pl, t, ys[m], xs[m], 0].astype(np.float64))
                oy = np.where(am == 0, ys[m], origin[pl, t, ys[m], xs[m], 1].astype(np.float64))
                if col is not None:                                 # the colour that was dragged along, whatever its origin
                    ok, val = np.ones(len(am), bool), np.minimum(255.0, np.floor(col[pl, t, ys[m], xs[m]] + 0.5))
                else:
                    ok, val = _candidate(src, hole, f, ox, oy, variant)
                at = np.nonzero(m)[0][ok]
                rgb[at], code[at], done[at] = val[ok], pl + 1, True
        out[t, ys, xs] = rgb.astype(np.uint8)
        source[t, ys, xs] = code
    return out, source


def _candidate(src, hole, f, ox, oy, variant=None):
    """candidates as lists: frame f, origin (ox, oy) -> (holds, rgb float64 [n,3])"""
    L, H, W = hole.shape
    with np.errstate(all="ignore"):
        ok = (f >= 0) & (f < L) & np.isfinite(ox) & np.isfinite(oy) & (ox >= 0.0) & (ox <= float(W - 1)) & (oy >= 0.0) & (oy <= float(H - 1))
        ox, oy, f = np.where(ok, ox, 0.0), np.where(ok, oy, 0.0), np.where(ok, f, 0)
        x0, y0 = np.floor(ox).astype(np.int64), np.floor(oy).astype(np.int64)
        wx1, wy1 = ox - x0, oy - y0
        wx0, wy0 = 1.0 - wx1, 1.0 - wy1
        s = None
        for dy, dx, w in ((0, 0, wy0 * wx0), (0, 1, wy0 * wx1), (1, 0, wy1 * wx0), (1, 1, wy1 * wx1)):
            xc, yc = x0 + dx, y0 + dy
            there = (xc < W) & (yc < H)
            xi, yi = np.minimum(xc, W - 1), np.minimum(yc, H - 1)
            used = w != 0.0
            ok &= ~used | there
            if variant != "hole_corners_ok":
                ok &= ~used | ~there | (hole[f, yi, xi] == 0)
            term = np.where(there[:, None], w[:, None] * src[f, yi, xi], 0.0)
            s = term if s is None else s + term
        return ok, np.minimum(255.0, np.floor(s + 0.5))


def propagate_np(case, check=True, variant=None):
    """the whole propagation of a case -> (out, source, age, origin)"""
    age, origin, col = planes_np(case, check, variant)
    out, source = fill_np(case, age, origin, variant, col)
    return out, source, age, origin


# ---------------------------------------------------------------------------------------------------------------- the cases
def _finish(c, seed, obj=None):
    """src = the truth with the hole painted over (the unwanted object: ``obj``, or noise), filled = the truth with a prediction
    in the hole that no frame holds"""
    rng = np.random.RandomState(seed)
    hole = c["hole"].astype(bool)
    truth = c["truth"]
    paint = rng.randint(0, 256, truth.shape).astype(np.uint8) if obj is None else np.full(truth.shape, obj, np.uint8)
    c["src"] = np.where(hole[..., None], paint, truth)
    c["filled"] = np.where(hole[..., None], rng.randint(0, 256, truth.shape).astype(np.uint8), truth)
    return c


def _static_hole(L, H, W, y0, y1, x0, x1):
    hole = np.zeros((L, H, W), np.uint8)
    hole[:, y0:y1, x0:x1] = 1
    return hole


def _zero_7x5():
    L, H, W = 3, 7, 5
    rng = np.random.RandomState(7)
    fwd, bwd = K._uniform(L, H, W, 0.0, 0.0)
    hole = np.repeat((rng.rand(1, H, W) < 0.4).astype(np.uint8), L, 0)
    return _finish(dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, hole=hole, truth=rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)), 70)


INT_SHIFT = (2, 1)


def _int_shift_24x61():
    """a random texture that moves by exactly (2, 1) pixels per frame behind a static 12 x 9 hole: whatever is fetched is the
    truth to the byte"""
    L, H, W = 16, 24, 61
    vx, vy = INT_SHIFT
    rng = np.random.RandomState(61)
    fwd, bwd = K._uniform(L, H, W, float(vx), float(vy))
    T = rng.randint(0, 256, (H + vy * L, W + vx * L, 3)).astype(np.uint8)
    # frame t at p shows the texture at p - t v
    truth = np.stack([T[vy * (L - t):vy * (L - t) + H, vx * (L - t):vx * (L - t) + W] for t in range(L)])
    return _finish(dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, hole=_static_hole(L, H, W, 8, 17, 24, 36), truth=truth), 610)


# half_shift_40x60's texture: sum_i A_i sin(kx_i x + ky_i y + phase_i + channel) + 128.  One bilinear sample of it is off by at
# most sum_i A_i (kx_i^2 + ky_i^2) / 8 = 4.5 + 3.0 grey levels; a colour dragged along for six steps of (1.5, 0.5) has gone
# through six 2 x 2 box averages, which leave cos(kx / 2)^6 cos(ky / 2)^6 = 0.50 of the first component: 20 grey levels are missing.
HALF_SHIFT = (1.5, 0.5)
HALF_WAVES = ((40.0, 0.9, 0.3, 0.4), (30.0, -0.4, 0.8, 1.9))       # (A, kx, ky, phase)
HALF_BOUND = sum(A * (kx * kx + ky * ky) for A, kx, ky, _ in HALF_WAVES) / 8.0 + 1.0


def half_texture(xs, ys):
    """the analytic texture at the positions (xs, ys) -> float64 [..., 3]"""
    return np.stack([sum(A * np.sin(kx * xs + ky * ys + ph + 0.7 * ch) for A, kx, ky, ph in HALF_WAVES) + 128.0 for ch in range(3)], -1)


def half_truth(t, H=40, W=60):
    """frame t of half_shift_40x60 before rounding: the texture at p - t v"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    return half_texture(xs - HALF_SHIFT[0] * t, ys - HALF_SHIFT[1] * t)


def _half_shift_40x60():
    L, H, W = 12, 40, 60
    fwd, bwd = K._uniform(L, H, W, *HALF_SHIFT)
    truth = np.stack([np.floor(half_truth(t) + 0.5) for t in range(L)]).astype(np.uint8)
    return _finish(dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, hole=_static_hole(L, H, W, 14, 24, 22, 36), truth=truth), 400, obj=0)


def _smooth_70x90():
    """the wavy flows with the two patches where forward and backward disagree, a cut, reach 2 and three holes that drift: one over
    each patch's edge, one against the right and the lower border"""
    k = K.case("smooth_70x90")
    L, H, W = k["L"], k["H"], k["W"]
    rng = np.random.RandomState(900)
    hole = np.zeros((L, H, W), np.uint8)
    for t in range(L):
        hole[t, 10 + t:26 + t, 12 + 2 * t:31 + 2 * t] = 1
        hole[t, 36:50, 44 + t:63 + t] = 1
        hole[t, 56 - t:H, 73 - 2 * t:W] = 1
    return _finish(dict(L=L, H=H, W=W, fwd=k["fwd"], bwd=k["bwd"], hole=hole, scenes=[5], reach=2,
                        truth=rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)), 901)


def _nonfinite_33x64():
    k = K.case("nonfinite_33x64")
    L, H, W = k["L"], k["H"], k["W"]
    rng = np.random.RandomState(640)
    hole = np.zeros((L, H, W), np.uint8)
    for t in range(L):
        hole[t, 4 + t:20 + t, 6 + 5 * t:40 + 5 * t] = 1
    return _finish(dict(L=L, H=H, W=W, fwd=k["fwd"], bwd=k["bwd"], hole=hole, truth=rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)), 641)


def _ragged(L):
    """W % 4 != 0, q on halves in both directions (the nearest pixel is decided by "a half goes up"), and frame 1 all hole"""
    H, W = 9, 13
    rng = np.random.RandomState(13 + L)
    fwd, bwd = K._uniform(L, H, W, -0.5, -0.5)
    hole = (rng.rand(L, H, W) < 0.4).astype(np.uint8)
    hole[1] = 1
    return _finish(dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, hole=hole, truth=rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8)), 130 + L)


def _square_40x60():
    """a hole that moves over a still background: mask_key_cases' square.  The completed frames are still, so the flows are zero,
    and every pixel is reached from the nearest frame in which the square is off it."""
    k = K.square_case()
    L, H, W = k["L"], k["H"], k["W"]
    rng = np.random.RandomState(4060)
    hole = np.stack([K.square_truth(t) for t in range(L)]).astype(np.uint8)
    fwd, bwd = K._uniform(L, H, W, 0.0, 0.0)
    truth = np.repeat(rng.randint(0, 256, (1, H, W, 3)).astype(np.uint8), L, 0)
    return _finish(dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, hole=hole, truth=truth), 4061)


_BUILDERS = {"zero_7x5": _zero_7x5, "int_shift_24x61": _int_shift_24x61, "half_shift_40x60": _half_shift_40x60,
             "smooth_70x90": _smooth_70x90, "nonfinite_33x64": _nonfinite_33x64, "ragged_9x13": lambda: _ragged(3),
             "ragged_2f_9x13": lambda: _ragged(2), "square_40x60": _square_40x60}
NAMES = tuple(_BUILDERS)
_CACHE = {}


def case(name):
    """the named case (built once; nobody writes to it)"""
    if name not in _CACHE:
        c = _BUILDERS[name]()
        for k in ("fwd", "bwd", "hole", "truth", "src", "filled"):
            c[k] = np.ascontiguousarray(c[k])
            c[k].setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


_REF = {}


def reference(name, check=True):
    """(out, source, age, origin) of propagate_np for the named case, computed once"""
    if (name, check) not in _REF:
        res = propagate_np(case(name), check)
        for a in res:
            a.setflags(write=False)
        _REF[(name, check)] = res
    return _REF[(name, check)]


def masks_of(c):
    """masks for a call of propagate_pixels(dilate=False) without size=: paste_mask then returns the case's hole"""
    return c["hole"] * np.uint8(255)
