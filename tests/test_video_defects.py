"""The host side of the dust-and-dirt detector (video.detect_defects, inpaint_video(masks_u8="defects")) without a device: the
numpy restatement's cases can see every mutated restatement, the plan of eligible frames, every refusal before the device, the
header and the binding, the C entries' refusals, and the conditions the defaults were chosen under."""
import itertools
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import defect_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Gen:
    """what the checks take for the generator: an object with engine()"""
    def engine(self):
        raise AssertionError("the engine was asked for")


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_detect_defects_device", touched)


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name,flags", D.VARIANTS, ids=[v[0] for v in D.VARIANTS])
def test_every_variant_differs_from_the_definition_on_some_case(name, flags):
    seen = [n for n in D.NAMES if any(not np.array_equal(a, b) for a, b in zip(D.want(n), D.want(n, **flags)))]
    print(name, seen)
    assert seen


def test_cases_hold_what_they_are_named_for():
    assert len(D.VARIANTS) == 10 and set(D.NAMES) >= {"zero_7x5", "shift_17x301", "half_9x13", "wave_70x90", "nonfinite_33x64",
                                                      "cuts_L7", "corner_slack2", "radius16_20x20", "support9"}
    # exact ties are not flagged, one level further is
    cand = D.want("zero_7x5")[0]
    assert (cand[1, 1, 1], cand[1, 4, 3], cand[1, 4, 1], cand[1, 1, 3]) == (0, 0, 1, 1)
    c = D.case("shift_17x301")
    cand = D.want("shift_17x301")[0]
    assert c["W"] % 4 == 1 and cand[1, :, 90:211].any() and not cand[1, :, :90].any() and not cand[1, :, 211:].any()
    assert not cand[1, 15:].any()                       # y + 2 > H - 1
    c = D.case("wave_70x90")
    assert not np.array_equal(c["bwd"], -c["fwd"])
    cand, raw, masks, counts = D.want("wave_70x90")
    limit = int(c["max_fraction"] * c["H"] * c["W"])
    assert counts[4] > limit and raw[4].any() and not masks[4].any() and masks[1].any() and masks[2].any()
    assert D.plan_np(7, [3]) == [1, 4, 5] and [t for t in range(7) if D.want("cuts_L7")[3][t]] == [1, 4, 5]
    c = D.case("nonfinite_33x64")
    assert all(np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any() and (f == np.float32(1e30)).any()
               for f in (c["fwd"], c["bwd"]))
    assert D.want("radius16_20x20")[2][1].all() and D.case("radius16_20x20")["radius"] == 16
    assert D.case("support9")["support"] == 9 and 0 < (D.want("support9")[1] > 0).sum() < D.want("support9")[0].sum()
    assert D.case("corner_slack2")["slack"] == 2
    for n in ("short_L1", "short_L2"):
        assert not D.want(n)[2].any() and not D.want(n)[3].any()


def test_plan_defect_frames_is_the_restatement():
    for length in range(10):
        cuts = [[]] + [list(c) for k in (1, 2) for c in itertools.combinations(range(1, length), k)]
        for sc in cuts:
            assert video.plan_defect_frames(length, sc) == D.plan_np(length, sc), (length, sc)
        assert video.plan_defect_frames(length) == D.plan_np(length) == list(range(1, length - 1))
    assert video.plan_defect_frames(np.int64(7), (3,)) == [1, 4, 5]
    for scenes in ([0], [7], [3, 3], [4, 2], "auto", [True], 3):
        with pytest.raises(ValueError, match="scenes"):
            video.plan_defect_frames(7, scenes)
    for length in (-1, 2.0, True, None):
        with pytest.raises(ValueError, match="length"):
            video.plan_defect_frames(length)


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_detect_defects_checks_before_the_device(no_device):
    f = np.zeros((5, 6, 8, 3), np.uint8)
    fl = (np.zeros((4, 6, 8, 2), np.float32),) * 2
    call = lambda frames, **kw: video.detect_defects(None, frames, **dict(dict(flows=fl), **kw))
    for bad in (f[0], f[..., :2], np.zeros((5, 6, 8), np.uint8)):
        with pytest.raises(ValueError, match="frames"):
            call(bad)
    for name, values in (("threshold", (-1, 255, 1.5, True, None, "16")), ("slack", (-1, 3, 0.5, False)),
                         ("support", (0, 10, 2.5, True)), ("radius", (-1, 17, 1.5, True)),
                         ("max_fraction", (0, -0.1, 1.5, True, None, "x")), ("return_counts", (1, 0, None, "yes"))):
        for v in values:
            with pytest.raises(ValueError, match=name):
                call(f, **{name: v})
    for flows in ((fl[0],), fl + fl[:1], (fl[0], fl[1][:3]), (fl[0][..., :1], fl[1]), 7, (None, None)):
        with pytest.raises(ValueError, match="flows"):
            call(f, flows=flows)
    with pytest.raises(ValueError, match="flows"):      # the flows must have the size the frames are resized to
        call(f, size=(16, 12))
    for size in ((0, 4), (8,), (8.5, 6), 8, (8, 6, 3), (True, 4)):
        with pytest.raises(ValueError, match="size"):
            call(f, size=size)
    for scenes in ([0], [5], [2, 2], "auto", [True]):
        with pytest.raises(ValueError, match="scenes"):
            call(f, scenes=scenes)
    for model in (None, lambda x, n: (x, None)):
        with pytest.raises(TypeError, match="InpaintGenerator"):
            video.detect_defects(model, f)
    # nothing to judge: empty masks, no launch and no flows -- the generator's engine is never asked for
    for L, kw in ((0, {}), (1, {}), (2, {}), (3, dict(scenes=[1])), (4, dict(scenes=[2])), (2, dict(size=(4, 3)))):
        m, n = video.detect_defects(_Gen(), np.ones((L, 6, 8, 3), np.uint8), return_counts=True, **kw)
        h, w = (3, 4) if "size" in kw else (6, 8)
        assert m.shape == (L, h, w) and m.dtype == np.uint8 and not m.any() and n.shape == (L,) and not n.any()
        assert video.detect_defects(_Gen(), np.ones((L, 6, 8, 3), np.uint8), **kw).shape == (L, h, w)


def test_inpaint_video_defects_checks_before_the_device(no_device):
    f = np.zeros((12, 8, 8, 3), np.uint8)
    gen = _Gen()
    for model in (None, lambda x, n: (x, None)):
        with pytest.raises(TypeError, match="InpaintGenerator"):
            video.inpaint_video(model, f, "defects", device="cpu")
    with pytest.raises(ValueError, match="mask_keys"):
        video.inpaint_video(gen, f, "defects", mask_keys=[2, 9], device="cpu")
    with pytest.raises(ValueError, match="mask_keys"):   # the string's own rule comes before the model's
        video.inpaint_video(None, f, "defects", mask_keys=[2, 9], device="cpu")
    with pytest.raises(ValueError, match="scenes"):
        video.inpaint_video(gen, f, "defects", scenes=[12], device="cpu")
    with pytest.raises(ValueError, match="no seam"):
        video.inpaint_video(gen, f, "defects", feather=2, device="cpu")
    for s in ("bogus", "", "Overlay", "auto", "logo", "Defects", "defect"):
        with pytest.raises(ValueError, match="overlay"):
            video.inpaint_video(gen, f, s, device="cpu")
    # good arguments pass the checks: on a host without a device the call gets as far as the refusal of the CPU device
    for kw in ({}, dict(scenes="auto"), dict(scenes=[4]), dict(size=(108, 60), restore=True, region="holes"), dict(reuse=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            video.inpaint_video(gen, f, "defects", device="cpu", **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        video.inpaint_video(gen, np.zeros((12, 12, 8), np.uint8), "defects", pixel_format="nv12", device="cpu")


def test_check_call_with_defects(no_device):
    import inspect
    defaults = {k: p.default for k, p in inspect.signature(video.inpaint_video).parameters.items()
                if p.default is not inspect.Parameter.empty and k != "device"}
    assert "defects" not in defaults                     # the driver got no new parameter
    c = video._check_call((12, 60, 108, 3), "defects", _Gen(), **defaults)
    assert c.defects is True and c.overlay is False and video._Call._fields[-1] == "defects" and len(video._Call._fields) == 21
    assert video._check_call((12, 60, 108, 3), np.zeros((12, 60, 108), np.uint8), None, **defaults).defects is False
    assert video._check_call((12, 60, 108, 3), "overlay", None, **defaults).defects is False
    assert video._Call(*range(20)).defects is False      # today's 20 fields still build the record
    c = video._check_call((12, 60, 108, 3), "defects", _Gen(), **dict(defaults, scenes="auto", size=(54, 30), restore=True))
    assert c.defects and c.scenes == "auto" and c.restore
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video._check_call((12, 60, 108, 3), "defects", None, **defaults)
    with pytest.raises(ValueError, match="mask_keys"):
        video._check_call((12, 60, 108, 3), "defects", _Gen(), **dict(defaults, mask_keys=[1]))
    assert (video.DEFECT_THRESHOLD, video.DEFECT_SLACK, video.DEFECT_SUPPORT, video.DEFECT_RADIUS, video.DEFECT_MAX_FRACTION) == \
        (16, 0, 3, 1, 0.02)
    sig = inspect.signature(video.detect_defects).parameters
    assert [sig[k].default for k in ("threshold", "slack", "support", "radius", "max_fraction", "return_counts")] == \
        [16, 0, 3, 1, 0.02, False]


# ------------------------------------------------------------------------------------------------ header, binding, C entries
def _declared(header, name):
    decl = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert decl, name
    return [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")]


def test_header_and_binding_declare_the_entries():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    assert _declared(header, "e2fgvi_defect_candidates") == ["frames", "fwd", "bwd", "ids", "n", "L", "H", "W", "tau", "slack", "cand",
                                                             "stream"]
    assert _declared(header, "e2fgvi_defect_clean") == ["cand", "ids", "n", "L", "H", "W", "support", "radius", "out", "counts", "stream"]
    res, args = lib.SYMBOLS["e2fgvi_defect_candidates"]
    assert len(args) == 12 and args[:4] == [lib._fp] * 4 and args[4:10] == [lib._i32] * 6 and args[10:] == [lib._fp] * 2
    res, args = lib.SYMBOLS["e2fgvi_defect_clean"]
    assert len(args) == 11 and args[:2] == [lib._fp] * 2 and args[2:8] == [lib._i32] * 6 and args[8:] == [lib._fp] * 3
    assert lib.ABI_VERSION == 9                          # symbols were only added
    assert callable(ops.defect_candidates) and callable(ops.defect_clean) and callable(video.detect_defects)
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "defects.hip"]
    assert len(unit) == 1 and unit[0][1] == "defects.o" and unit[0][1] in build.NOPK_OBJECTS and unit[0][2] == build.NOPK


def test_built_object_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "defects.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("object or llvm-objdump not present (python -m e2fgvi_amd.build)")
    # three candidate kernels (one per slack) and the cleaning kernel
    assert build.verify_no_scratch(obj="defects.o", marker="defect_", what="dust and dirt") == 4


def test_entries_refuse_bad_arguments_and_return_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    good = dict(frames=base + 1, fwd=base + (1 << 16), bwd=base + (1 << 17), ids=base + (1 << 18), n=2, L=4, H=7, W=5, tau=16, slack=0,
                cand=base + (1 << 19) + 3)
    order = ("frames", "fwd", "bwd", "ids", "n", "L", "H", "W", "tau", "slack", "cand")
    ptrs = ("frames", "fwd", "bwd", "ids", "cand")

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_defect_candidates(*[a[k] for k in order], None)

    def common(rc, ptrs, who):
        for k in ptrs:
            assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error(), k
        for L in (2, 1, 0):
            assert rc(L=L) == -1 and b"L >= 3" in so.e2fgvi_last_error() and who in so.e2fgvi_last_error()
            assert rc(L=L, n=0) == 0                    # nothing listed: no work, whatever L is
        for k in ("n", "L", "H", "W"):
            assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error(), k
        assert rc(H=46341, W=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
        assert rc(H=1, W=2147483647 - 256) == -1 and rc(H=0x7fffffff, W=0x7fffffff) == -1
        assert rc(ids=good["ids"] + 2) == -1 and b"aligned" in so.e2fgvi_last_error()
        null = {k: None for k in ptrs}
        assert rc(n=0) == 0 and rc(H=0) == 0 and rc(W=0) == 0
        assert rc(n=0, **null) == 0 and rc(H=0, **null) == 0 and rc(W=0, H=0, n=0, **null) == 0

    common(rc, ptrs, b"defect_candidates")
    for v in (-1, 255, 1 << 20):
        assert rc(tau=v) == -1 and b"tau" in so.e2fgvi_last_error()
        assert rc(tau=v, n=0) == -1
    for v in (-1, 3):
        assert rc(slack=v) == -1 and b"slack" in so.e2fgvi_last_error()
    assert rc(fwd=good["fwd"] + 4) == -1 and b"aligned" in so.e2fgvi_last_error()
    assert rc(bwd=good["bwd"] + 4) == -1 and b"aligned" in so.e2fgvi_last_error()

    good2 = dict(cand=base + 1, ids=good["ids"], n=2, L=4, H=7, W=5, support=3, radius=1, out=base + (1 << 19) + 3, counts=base + (1 << 20))
    order2 = ("cand", "ids", "n", "L", "H", "W", "support", "radius", "out", "counts")

    def rc2(**kw):
        a = dict(good2, **kw)
        return so.e2fgvi_defect_clean(*[a[k] for k in order2], None)

    common(rc2, ("cand", "ids", "out", "counts"), b"defect_clean")
    for v in (0, 10, -3):
        assert rc2(support=v) == -1 and b"support" in so.e2fgvi_last_error()
    for v in (-1, 17):
        assert rc2(radius=v) == -1 and b"radius" in so.e2fgvi_last_error()
        assert rc2(radius=v, H=0) == -1
    assert rc2(counts=good2["counts"] + 2) == -1 and b"aligned" in so.e2fgvi_last_error()
    assert so.e2fgvi_abi_version() == 9


# ------------------------------------------------------------------------------------------------ the conditions on the defaults
def test_defaults_hold_their_conditions_on_the_translated_video():
    """The restatement with video's DEFECT_* defaults on the 7-frame translated-tennis video (1.5 / 0.5 px per frame, PIL BICUBIC,
    ideal flows, a 12-pixel border left out): a clean video keeps at most 0.05 % of the judged pixels before the dilation, and the
    dilated masks of the planted video (30 grey rectangles per centre frame, luma 20 or 235, sides 2-7 px, seed 0) cover at least
    95 % of the planted pixels.  Measured: 52 of 440640 = 0.0118 % and 2918 of 2955 = 98.7 % (profiles/defects_stats.txt)."""
    s = dict(threshold=video.DEFECT_THRESHOLD, slack=video.DEFECT_SLACK, support=video.DEFECT_SUPPORT, radius=video.DEFECT_RADIUS)
    b = D.STATS_BORDER
    fr, fwd, bwd, _ = D.tennis_video(ROOT)
    assert fr.shape == (7, 240, 432, 3)
    ids = D.plan_np(7)
    assert ids == [1, 2, 3, 4, 5]
    cand = D.candidates_np(fr, fwd, bwd, ids, s["threshold"], s["slack"])
    kept, _ = D.clean_np(cand, ids, s["support"], 0)
    judged = kept[1:-1, b:-b, b:-b]
    print("clean: %d candidates, %d kept of %d judged = %.4f %%" % (cand[1:-1, b:-b, b:-b].sum(), (judged > 0).sum(), judged.size,
                                                                     100.0 * (judged > 0).sum() / judged.size))
    assert judged.size == 440640 and (judged > 0).sum() <= 0.0005 * judged.size
    fr, fwd, bwd, marks = D.tennis_video(ROOT, planted=True)
    masks, counts = D.detect_np(fr, fwd, bwd, max_fraction=video.DEFECT_MAX_FRACTION, **s)
    hit, n = int(((masks > 0) & marks).sum()), int(marks.sum())
    print("planted: %d of %d covered = %.1f %%; set per frame %s of %d" % (hit, n, 100.0 * hit / n, counts.tolist(), 240 * 432))
    assert hit >= 0.95 * n
    assert counts.max() <= int(video.DEFECT_MAX_FRACTION * 240 * 432)      # heavy dirt stays under the frame guard
