"""Masks from keyframes (e2fgvi_amd.video.propagate_masks, ops.mask_track_step, csrc/mask_track.hip): the float64 numpy restatement
of the step and of the whole propagation, written from the definition in include/e2fgvi_hip.h, and the named cases both test files
run.  It has a sampler of its own (a zero-padded table read at four shifted positions) and walks its chains key by key, one chain
after the other -- neither the kernel's addressing nor the planner's lockstep order.

The step, for a destination pixel p = (x, y), source mask M, pull flow g and check flow c (fp64 on the fp32 / uint8 inputs, in the
order written):
    q = (x + g_x(p), y + g_y(p));  inside = g(p) finite and 0 <= q_x <= W-1 and 0 <= q_y <= H-1
    s = bil(M, q), c_w = bil(c, q): four corners, those outside the image contribute 0, added in the order (y0,x0), (y0,x0+1),
        (y0+1,x0), (y0+1,x0+1)
    inconsistent = c_w not finite, or  sx sx + sy sy > 0.01 ((g_x g_x + g_y g_y) + (c_wx c_wx + c_wy c_wy)) + 0.5,  s. = g + c_w
    dst(p) = inside and s >= 0.5 and (not check or not inconsistent)
`margin` is the smallest |lhs - rhs| of that comparison over the candidate pixels (inside, s >= 0.5, c_w finite) of a step.

VARIANTS are deliberately wrong readings of the text; the CPU tests require each of them to change the masks of some case."""
import numpy as np

VARIANTS = ("swap_channels", "wrong_pull_flow", "check_at_p", "border_clamp", "strict_greater", "no_check", "cross_key", "intersection")


def _corners(T, x0, y0):
    """T [H,W,C] float64 -> its values at (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1); one row and one column of zeros stand for
    the corners outside the image (x0 in [0, W-1], y0 in [0, H-1])"""
    P = np.zeros((T.shape[0] + 1, T.shape[1] + 1, T.shape[2]), np.float64)
    P[:-1, :-1] = T
    return P[y0, x0], P[y0, x0 + 1], P[y0 + 1, x0], P[y0 + 1, x0 + 1]


def _corners_clamped(T, x0, y0):
    H, W = T.shape[:2]
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    return T[y0, x0], T[y0, x1], T[y1, x0], T[y1, x1]


def step_np(M, g, c, check=True, variant=None):
    """M uint8 [H,W] of 0 / 1, g and c fp32 [H,W,2] -> (dst uint8 [H,W], margin, candidates): the definition above"""
    H, W = M.shape
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
        qx, qy = np.where(inside, qx, 0.0), np.where(inside, qy, 0.0)       # excluded pixels read corner (0, 0) and are dropped below
        x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
        wx1, wy1 = qx - x0, qy - y0
        wx0, wy0 = 1.0 - wx1, 1.0 - wy1
        w = (wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1)
        corners = _corners_clamped if variant == "border_clamp" else _corners
        m = corners(M.astype(np.float64)[..., None], x0, y0)
        s = w[0] * m[0][..., 0]
        for k in (1, 2, 3):
            s = s + w[k] * m[k][..., 0]
        cand = inside & ((s > 0.5) if variant == "strict_greater" else (s >= 0.5))
        if variant == "check_at_p":
            cw = c64
        else:
            v = corners(c64, x0, y0)
            cw = w[0][..., None] * v[0]
            for k in (1, 2, 3):
                cw = cw + w[k][..., None] * v[k]
        cx, cy = cw[..., 0], cw[..., 1]
        cfin = np.isfinite(cx) & np.isfinite(cy)
        sx, sy = gx + cx, gy + cy
        lhs = sx * sx + sy * sy
        rhs = 0.01 * ((gx * gx + gy * gy) + (cx * cx + cy * cy)) + 0.5
        bad = ~cfin | (lhs > rhs)
        tested = cand & cfin
        margin = float(np.abs(lhs - rhs)[tested].min()) if tested.any() else float("inf")
    keep = cand if (not check or variant == "no_check") else cand & ~bad
    return keep.astype(np.uint8), margin, int(cand.sum())


def job_flows(fwd, bwd, t, d, variant=None):
    """(g, c) of the job (pair t, dir d)"""
    g, c = (bwd[t], fwd[t]) if d == 0 else (fwd[t], bwd[t])
    return (c, g) if variant == "wrong_pull_flow" else (g, c)


def run_job(planes, fwd, bwd, t, d, check=True, variant=None):
    """one job on planes [2,L,H,W] in place -> (margin, candidates)"""
    src, dst = (t, t + 1) if d == 0 else (t + 1, t)
    g, c = job_flows(fwd, bwd, t, d, variant)
    planes[d, dst], margin, cand = step_np(planes[d, src], g, c, check, variant)
    return margin, cand


def chains_np(length, keys, scenes=None, reach=None, variant=None):
    """the chains, one list of (pair, dir) per key and direction, each in the order its jobs must run"""
    cuts, keyset = set(scenes or ()), set(keys)
    stop_at_key = variant != "cross_key"
    out = []
    for k in keys:
        for d in (0, 1):
            chain, f = [], k
            while True:
                nxt = f + 1 if d == 0 else f - 1
                crossing = (nxt if d == 0 else f) in cuts              # a cut c separates c - 1 from c
                if nxt < 0 or nxt >= length or crossing or (stop_at_key and nxt in keyset) or (reach is not None and len(chain) >= reach):
                    break
                chain.append((min(f, nxt), d))
                f = nxt
            out.append(chain)
    return out


def binarise(key_masks):
    return (np.asarray(key_masks) != 0).astype(np.uint8)


def planes_np(case, check=True, variant=None):
    """both planes after all chains of a case -> (planes uint8 [2,L,H,W], records): records holds (pair, dir, number in its chain,
    margin, candidates) of every job, chain after chain"""
    L, H, W = case["L"], case["H"], case["W"]
    planes = np.zeros((2, L, H, W), np.uint8)
    planes[:, list(case["keys"])] = binarise(case["key_masks"])
    records = []
    for chain in chains_np(L, case["keys"], case.get("scenes"), case.get("reach"), variant):
        for i, (t, d) in enumerate(chain):
            margin, cand = run_job(planes, case["fwd"], case["bwd"], t, d, check, variant)
            records.append((t, d, i, margin, cand))
    return planes, records


def propagate_np(case, check=True, variant=None):
    """the whole propagation of a case -> (masks uint8 [L,H,W], records of planes_np): the union of the two planes"""
    planes, records = planes_np(case, check, variant)
    masks = planes[0] & planes[1] if variant == "intersection" else planes[0] | planes[1]
    return masks, records


def case_margin(case):
    return min([r[3] for r in propagate_np(case)[1]] + [float("inf")])


# ---------------------------------------------------------------------------------------------------------------- the cases
def _blob(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


def _uniform(L, H, W, dx, dy):
    f = np.empty((L - 1, H, W, 2), np.float32)
    f[..., 0], f[..., 1] = dx, dy
    return f, -f


def _zero_7x5():
    L, H, W = 3, 7, 5
    rng = np.random.RandomState(7)
    fwd, bwd = _uniform(L, H, W, 0.0, 0.0)
    return dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, keys=[1], key_masks=(rng.rand(1, H, W) < 0.4).astype(np.uint8) * 200)


SHIFT = (90, 2)


def _shift_17x301():
    L, H, W = 5, 17, 301
    fwd, bwd = _uniform(L, H, W, float(SHIFT[0]), float(SHIFT[1]))
    m = _blob(H, W, 3, 10, 40, 130)
    m[5, 60:70] = 0                                     # not a plain rectangle
    m[12:15, 295:301] = 255                             # at the right border: a clamped sampler smears it over frame 0
    return dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, keys=[1], key_masks=m[None])


def _tie_9x13():
    L, H, W = 3, 9, 13
    fwd, bwd = _uniform(L, H, W, -0.5, -0.5)            # the pull flow of a forward job is bwd = (+0.5, +0.5): every s is k / 4
    rng = np.random.RandomState(13)
    masks = (rng.rand(2, H, W) < 0.5).astype(np.uint8)
    return dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, keys=[0, 1], key_masks=masks)


SQUARE = dict(w=12, h=10, x=8.0, y=6.0, vx=1.5, vy=0.5)


def square_truth(t, H=40, W=60):
    """the pixels whose centres the square covers in frame t: 12 x 10 of them at every position"""
    ys, xs = np.mgrid[0:H, 0:W]
    x, y = SQUARE["x"] + SQUARE["vx"] * t, SQUARE["y"] + SQUARE["vy"] * t
    return (xs >= x) & (xs < x + SQUARE["w"]) & (ys >= y) & (ys < y + SQUARE["h"])


def square_case(key=0):
    """the ideal flows of the moving square: the object's pixels carry its velocity, the background stands still"""
    L, H, W = 8, 40, 60
    fwd, bwd = np.zeros((L - 1, H, W, 2), np.float32), np.zeros((L - 1, H, W, 2), np.float32)
    for t in range(L - 1):
        fwd[t][square_truth(t)] = (SQUARE["vx"], SQUARE["vy"])
        bwd[t][square_truth(t + 1)] = (-SQUARE["vx"], -SQUARE["vy"])
    return dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, keys=[key], key_masks=square_truth(key).astype(np.uint8)[None])


def _wave(H, W, t, at=None):
    """a smooth flow field of about two pixels, evaluated at the grid or at the positions `at` = (x, y)"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    if at is not None:
        xs, ys = at
    a = 0.045 * xs + 0.031 * ys + 0.9 * t
    b = 0.027 * xs - 0.052 * ys + 1.7 * t
    return 2.0 * np.sin(a) + 0.7 * np.cos(b), 1.6 * np.cos(a + 0.4) - 0.8 * np.sin(b)


def _smooth_70x90():
    L, H, W = 6, 70, 90
    rng = np.random.RandomState(90)
    fwd, bwd = np.empty((L - 1, H, W, 2), np.float32), np.empty((L - 1, H, W, 2), np.float32)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    for t in range(L - 1):
        ux, uy = _wave(H, W, t)
        fwd[t, ..., 0], fwd[t, ..., 1] = ux, uy
        # the backward flow at p: minus the forward flow at the point that lands on p, to first order p - u(p)
        vx, vy = _wave(H, W, t, (xs - ux, ys - uy))
        bwd[t, ..., 0], bwd[t, ..., 1] = -vx, -vy
    noise = rng.randn(2, L - 1, H, W, 2).astype(np.float32) * 0.02
    fwd, bwd = fwd + noise[0], bwd + noise[1]
    bwd[:, 14:30, 20:36] += np.float32(1.25)            # a patch where the two flows disagree: the test drops what is pulled from it
    fwd[:, 40:52, 50:70, 1] -= np.float32(1.0)
    masks = np.stack([_blob(H, W, 10, 34, 12, 40), _blob(H, W, 30, 60, 41, 77), _blob(H, W, 5, 25, 50, 86)])
    masks[1, 40:46, 50:60] = 0
    return dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, keys=[0, 4, 5], key_masks=masks, scenes=[5], reach=2)


def _nonfinite_33x64():
    L, H, W = 3, 33, 64
    fwd, bwd = _uniform(L, H, W, 1.0, 0.0)
    rng = np.random.RandomState(64)
    for f in (fwd, bwd):
        for value in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            where = rng.rand(*f.shape) < 0.02
            f[where] = value
    return dict(L=L, H=H, W=W, fwd=fwd, bwd=bwd, keys=[1], key_masks=_blob(H, W, 4, 28, 6, 58)[None])


_BUILDERS = {"zero_7x5": _zero_7x5, "shift_17x301": _shift_17x301, "tie_9x13": _tie_9x13, "square_40x60": square_case,
             "smooth_70x90": _smooth_70x90, "nonfinite_33x64": _nonfinite_33x64}
NAMES = tuple(_BUILDERS)
TIE_CASES = ("tie_9x13",)
_CACHE = {}


def case(name):
    """the named case (built once; nobody writes to it)"""
    if name not in _CACHE:
        c = _BUILDERS[name]()
        for k in ("fwd", "bwd", "key_masks"):
            c[k].setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


_REF = {}


def reference(name, check=True):
    """(masks, records) of propagate_np for the named case, computed once"""
    if (name, check) not in _REF:
        masks, rec = propagate_np(case(name), check)
        masks.setflags(write=False)
        _REF[(name, check)] = (masks, rec)
    return _REF[(name, check)]


def frames_of(c):
    """frames for a call that is given its flows: only their shape matters"""
    return np.zeros((c["L"], c["H"], c["W"], 3), np.uint8)
