"""The measurements behind detect_defects' defaults (video.DEFECT_*), on the numpy restatement of tests/defect_cases.py -- no device
is needed: ``python tools/defects_stats.py > profiles/defects_stats.txt``.

The video is frame 0 of tests/golden/tennis25.npz translated 1.5 / 0.5 px per frame (PIL BICUBIC), 7 frames, ideal flows, a
12-pixel border left out.  "clean" is the share of the judged pixels a video without a defect keeps after the support test and
before the dilation (false alarms); "covered" is the share of the planted pixels (30 grey rectangles per centre frame, luma 20 or
235, sides 2-7 px) under the dilated masks.  One setting moves at a time around the defaults.  The last table is what failed motion
compensation looks like: the fixture's real, moving frames judged with flows of zero -- the share of each frame that is set."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import defect_cases as D      # noqa: E402

DEFAULTS = dict(threshold=16, slack=0, support=3, radius=1)


def judged(a):
    b = D.STATS_BORDER
    return a[1:-1, b:-b, b:-b]


def measure(clean, planted, marks, **kw):
    s = dict(DEFAULTS, **kw)
    ids = D.plan_np(clean[0].shape[0])
    out = []
    for fr, fwd, bwd in (clean, planted):
        cand = D.candidates_np(fr, fwd, bwd, ids, s["threshold"], s["slack"])
        kept, _ = D.clean_np(cand, ids, s["support"], 0)
        full, _ = D.clean_np(cand, ids, s["support"], s["radius"])
        out.append((cand, kept, full))
    (cand, kept, _), (_, _, full) = out
    n = judged(kept).size
    m = judged(marks)
    return (int(judged(cand).sum()), int((judged(kept) > 0).sum()), 100.0 * (judged(kept) > 0).sum() / n,
            int(((judged(full) > 0) & m).sum()), int(m.sum()), 100.0 * ((judged(full) > 0) & m).sum() / m.sum())


def main():
    c = D.tennis_video(ROOT)
    p = D.tennis_video(ROOT, planted=True)
    clean, planted, marks = c[:3], p[:3], p[3]
    print("judged pixels: %d" % judged(marks).size)
    print("%-22s %10s %8s %9s %18s" % ("setting", "candidates", "kept", "clean %", "covered"))
    rows = [dict()] + [dict(threshold=v) for v in (8, 12, 20, 24, 32)] + [dict(slack=v) for v in (1, 2)] + \
           [dict(support=v) for v in (1, 2, 4, 5)] + [dict(radius=v) for v in (0, 2)]
    for kw in rows:
        a = measure(clean, planted, marks, **kw)
        name = ", ".join("%s=%d" % kv for kv in kw.items()) or "defaults (16, 0, 3, 1)"
        print("%-22s %10d %8d %9.4f %8d / %d = %5.1f %%" % ((name,) + a))
    # failed compensation: the real frames, flows of zero
    with np.load(os.path.join(ROOT, "tests", "golden", "tennis25.npz")) as z:
        fr = np.asarray(z["frames"][:9], np.uint8)
    zero = np.zeros((fr.shape[0] - 1,) + fr.shape[1:3] + (2,), np.float32)
    _, counts = D.detect_np(fr, zero, zero, max_fraction=1.0)
    share = 100.0 * counts[1:-1] / float(fr.shape[1] * fr.shape[2])
    print("flows of zero on the moving frames 1..7, defaults: %% of the frame set: %s" % " ".join("%.2f" % v for v in share))
    _, counts = D.detect_np(planted[0], planted[1], planted[2], max_fraction=1.0)
    share = 100.0 * counts[1:-1] / float(fr.shape[1] * fr.shape[2])
    print("the planted video, ideal flows, defaults:          %% of the frame set: %s" % " ".join("%.2f" % v for v in share))


if __name__ == "__main__":
    main()
