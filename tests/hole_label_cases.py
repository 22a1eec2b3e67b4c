"""Connected components of the hole's footprint (ops.hole_components, csrc/video.hip label_*_kernel): the mask builders of the
device tests and a numpy / pure-Python restatement of the semantics -- a stack-based flood fill over the 8 neighbours, then the
components renumbered by their first pixel in raster order.  tests/test_video_holes.py pins the restatement to
scipy.ndimage.label; tests/test_gpu_video_holes.py compares the kernels with it, every integer equal."""
import numpy as np

NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def footprint_np(masks):
    """uint8 [L,Hm,Wm] -> bool [Hm,Wm]: some frame's byte is non-zero"""
    return (np.asarray(masks) != 0).any(0) if len(masks) else np.zeros(np.asarray(masks).shape[1:], bool)


def components_np(U):
    """bool [Hm,Wm] -> (labels int32 [Hm,Wm], boxes int32 [K,5]): labels 0 outside U, else 1 .. K by the component's smallest
    y * Wm + x; boxes[k-1] = (x0, y0, x1, y1, area), upper ends exclusive"""
    U = np.asarray(U, bool)
    Hm, Wm = U.shape
    raw = np.zeros((Hm, Wm), np.int64)
    n = 0
    ys, xs = np.nonzero(U)
    for y, x in zip(ys.tolist()[::-1], xs.tolist()[::-1]):          # seeds from the LAST pixel: the fill's own order is not the answer
        if raw[y, x]:
            continue
        n += 1
        raw[y, x] = n
        stack = [(y, x)]
        while stack:
            cy, cx = stack.pop()
            for dy, dx in NEIGHBOURS:
                yy, xx = cy + dy, cx + dx
                if 0 <= yy < Hm and 0 <= xx < Wm and U[yy, xx] and not raw[yy, xx]:
                    raw[yy, xx] = n
                    stack.append((yy, xx))
    # renumber by first pixel: np.unique's first indices are raster positions
    labels = np.zeros((Hm, Wm), np.int32)
    boxes = np.zeros((n, 5), np.int32)
    if n:
        vals, first = np.unique(raw.ravel(), return_index=True)
        order = [int(v) for v, _ in sorted(zip(vals.tolist(), first.tolist()), key=lambda t: t[1]) if v]
        for k, v in enumerate(order, 1):
            sel = raw == v
            labels[sel] = k
            yy, xx = np.nonzero(sel)
            boxes[k - 1] = (xx.min(), yy.min(), xx.max() + 1, yy.max() + 1, sel.sum())
    return labels, boxes


def spiral(Hm, Wm):
    """a one-pixel-wide spiral from the first pixel inwards, one pixel of background between its arms: a single chain"""
    U = np.zeros((Hm, Wm), bool)
    inb = lambda y, x: 0 <= y < Hm and 0 <= x < Wm
    y, x, dy, dx = 0, 0, 0, 1
    U[0, 0] = True
    while True:
        for _ in range(2):                              # straight on, else one turn to the right
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            ok = inb(ny, nx) and not U[ny, nx] and not (inb(fy, fx) and U[fy, fx])
            if ok:
                break
            dy, dx = dx, -dy
        if not ok:
            return U
        y, x = ny, nx
        U[y, x] = True


def comb(Hm, Wm, joined_at_bottom):
    """teeth on every other column, joined only by the last (or the first) row"""
    U = np.zeros((Hm, Wm), bool)
    U[:, ::2] = True
    U[-1 if joined_at_bottom else 0, :] = True
    return U


def two_combs(Hm, Wm):
    """teeth from the first row on columns 0, 6, 12 ... and from the last row on columns 3, 9, 15 ..., two background pixels between
    neighbouring teeth and between a tooth's end and the other comb's row: exactly 2 components from 5 x 4 on"""
    U = np.zeros((Hm, Wm), bool)
    U[0, :] = True
    U[-1, :] = True
    U[:max(Hm - 2, 0), ::6] = True
    U[2:, 3::6] = True
    return U


def corner_cases(Hm, Wm, TH, TW):
    """pixel pairs around the corner where four tiles meet, (TH, TW): name -> (U, number of components)"""
    out = {}
    if Hm > TH + 1 and Wm > TW + 1:
        for name, pix, k in (("corner_diag", [(TH - 1, TW - 1), (TH, TW)], 1), ("corner_anti", [(TH - 1, TW), (TH, TW - 1)], 1),
                             ("corner_apart", [(TH - 1, TW - 1), (TH + 1, TW + 1)], 2)):
            U = np.zeros((Hm, Wm), bool)
            for y, x in pix:
                U[y, x] = True
            out[name] = (U, k)
    return out


def footprints(Hm, Wm, TH, TW):
    """name -> bool [Hm,Wm]: the smallest masks that can break each stage of the labelling (tests/test_gpu_video_holes.py)"""
    out = {"empty": np.zeros((Hm, Wm), bool), "full": np.ones((Hm, Wm), bool)}
    c = np.zeros((Hm, Wm), bool)
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = True
    out["corners"] = c
    yy, xx = np.mgrid[0:Hm, 0:Wm]
    out["checkerboard"] = (yy + xx) % 2 == 0                       # ONE component under 8-connectivity
    out["isolated"] = (yy % 2 == 0) & (xx % 2 == 0)                # the largest K there is: every component has area 1
    out["spiral"] = spiral(Hm, Wm)
    out["comb_bottom"] = comb(Hm, Wm, True)
    out["comb_top"] = comb(Hm, Wm, False)
    out["two_combs"] = two_combs(Hm, Wm)
    for name, (U, _) in corner_cases(Hm, Wm, TH, TW).items():
        out[name] = U
    bar = np.zeros((Hm, Wm), bool)
    bar[Hm // 2, :] = True
    out["bar"] = bar
    for d in (0.3, 0.41, 0.6):                                      # 0.41: about the 8-connectivity percolation threshold
        out["noise%g" % d] = np.random.RandomState(int(d * 100) + 7 * Hm + Wm).rand(Hm, Wm) < d
    return out


def video_of(U, name="", L=3, seed=0):
    """a footprint spread over L frames: every pixel of U is set in a random non-empty choice of frames, with the values 1 and 255;
    the bar has its left half in the first frame and its right half in the last"""
    U = np.asarray(U, bool)
    Hm, Wm = U.shape
    rng = np.random.RandomState(seed)
    if name == "bar":
        m = np.zeros((L, Hm, Wm), np.uint8)
        m[0, :, :Wm // 2] = U[:, :Wm // 2]
        m[L - 1, :, Wm // 2:] = U[:, Wm // 2:] * 255
        return m
    pick = rng.rand(L, Hm, Wm) < 0.4
    own = rng.randint(0, L, (Hm, Wm))
    pick[own, np.arange(Hm)[:, None], np.arange(Wm)[None, :]] = True
    vals = np.where(rng.rand(L, Hm, Wm) < 0.5, 1, 255).astype(np.uint8)
    return (pick & U[None]) * vals
