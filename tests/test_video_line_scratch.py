"""The host side of the line-scratch detector (video.detect_line_scratches) without a device: the numpy restatement holds its named
cases and every mutated restatement moves one of them, the conditions the defaults were chosen under, every refusal before the
device, the header and the binding, and the C entries' refusals."""
import inspect
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import line_scratch_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"e2fgvi_line_sums": ["frames", "L", "H", "W", "rows", "S", "stream"],
           "e2fgvi_line_columns": ["S", "L", "H", "W", "rows", "tau", "gap", "side", "drift", "coverage", "cand", "cnt", "col", "b0", "b1",
                                   "stream"],
           "e2fgvi_line_paint": ["col", "b0", "b1", "scene", "L", "H", "W", "rows", "drift", "span", "persist", "radius", "keep", "counts",
                                 "masks", "stream"]}


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_detect_line_scratches_device", touched)


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name,flags", C.VARIANTS, ids=[v[0] for v in C.VARIANTS])
def test_every_variant_differs_from_the_definition_on_some_case(name, flags):
    seen = [n for n in C.NAMES if any(not np.array_equal(C.want(n)[k], C.want(n, **flags)[k]) for k in C.KEYS)]
    print(name, seen)
    assert seen


def _painted_columns(w, t=0):
    return sorted(set(np.nonzero(w["masks"][t])[1].tolist()))


def test_cases_hold_what_they_are_named_for():
    assert len(C.VARIANTS) >= 8 and C.DEFAULTS == dict(rows=16, tau=6, gap=2, side=3, drift=1, coverage=50, span=2, persist=3, radius=2)
    for n in C.NAMES:
        c, w = C.case(n), C.want(n)
        L, H, W = c["L"], c["H"], c["W"]
        assert L <= 12 and H <= 75 and W <= 110 or n == "wide_20x300"
        nb = H // c["rows"]
        assert [w[k].shape for k in C.KEYS] == [(L, nb, W), (L, nb, W)] + [(L, 2, W)] * 5 + [(L,), (L, H, W)]
        assert set(np.unique(w["masks"]).tolist()) <= {0, 255} and np.array_equal(w["counts"], w["keep"].reshape(L, -1).sum(1))
    # bright, dark, both; widths 1, 2 and 3: the centre columns, `drift` more that share their height, `radius` more painted
    w = C.want("bright_w1")
    assert w["keep"][:, 0, 19:22].all() and w["counts"].tolist() == [3] * 5 and not w["keep"][:, 1].any()
    assert _painted_columns(w) == list(range(17, 24)) and w["masks"][:, :, 17:24].all()
    w = C.want("dark_w2")
    assert w["keep"][:, 1, 26:30].all() and w["counts"].tolist() == [4] * 5 and not w["keep"][:, 0].any()
    w = C.want("both_w3")
    assert w["keep"][:, 0, 10:15].all() and w["keep"][:, 1, 34:37].all() and w["counts"].tolist() == [8] * 5
    assert (w["cand"][:, :, 11:14] == 1).all() and (w["cand"][:, :, 35] == 2).all()
    # the first and the last column with all its side columns in the frame, and one column outside each
    w, c = C.want("edges_in"), C.case("edges_in")
    assert (w["cand"][:, :, 5] == 1).all() and (w["cand"][:, :, c["W"] - 6] == 2).all() and w["counts"].tolist() == [6] * 3
    assert _painted_columns(w) == list(range(2, 9)) + list(range(c["W"] - 9, c["W"] - 2))
    assert all(not C.want("edges_out")[k].any() for k in ("cand", "col", "keep", "counts", "masks"))
    # 75 rows: four bands, and the 11 rows below them are painted with the last
    w = C.want("remainder_75")
    assert w["S"].shape[1] == 4 and w["masks"][:, 64:, 19:26].all() and not w["masks"][:, 64:, :19].any()
    # nothing to judge
    for n in ("short_H", "narrow_W"):
        assert not C.want(n)["masks"].any() and not C.want(n)["counts"].any() and not C.want(n)["cand"].any()
    assert C.want("short_H")["S"].shape[1] == 0 and C.case("narrow_W")["W"] == 2 * (2 + 3)
    # the polarities never mix; 40 % of the height is not enough and 60 % is, painted over its own bands only
    w = C.want("mixed_column")
    assert w["cnt"][:, :, 18].tolist() == [[2, 2]] * 4 and not w["col"].any()
    assert C.want("partial_40")["cnt"][:, 0, 15].tolist() == [2] * 4 and not C.want("partial_40")["masks"].any()
    w = C.want("partial_60")
    assert w["keep"][:, 0, 15].all() and (w["b0"][:, 0, 15] == 0).all() and (w["b1"][:, 0, 15] == 2).all()
    assert w["masks"][:, :24, 13:18].all() and not w["masks"][:, 24:].any()
    # a scratch that wanders by `drift` between the bands is one column; by drift + 2 per band it is none
    w = C.want("wander_drift")
    assert (w["cnt"][:, 0, 20] == 9).all() and w["keep"][:, 0, 20].all() and (w["cnt"][:, 0, 19] == 6).all()
    assert (C.want("wander_far")["cand"] == 1).sum() == 36 and not C.want("wander_far")["col"].any()
    # persistence
    w = C.want("two_of_five")
    assert w["col"][[1, 3], 0, 17].all() and not w["col"][[0, 2, 4]].any() and not w["keep"].any() and not w["masks"].any()
    w = C.want("cut_L8")
    assert w["col"][1:6, 0, 17].all() and w["keep"][:, 0, 17].tolist() == [0, 1, 1, 1, 0, 0, 0, 0]
    assert C.want("single_L1")["keep"][0, 0, 17] == 1 and C.want("single_L1")["masks"].any()
    assert C.want("jitter2")["keep"][:, 0, 17].tolist() == [1, 0, 1, 0, 1]
    # texture: candidates, and no column with the height
    w = C.want("strokes")
    assert (w["cand"] == 1).any() and (w["cand"] == 2).any() and w["cnt"].max() == 1 and not w["col"].any() and not w["masks"].any()
    # exact ties are no candidates, one level further is
    w = C.want("ties")
    assert [int(w["cand"][0, 0, x]) for x in (10, 22, 36, 48)] == [0, 1, 0, 2]
    c = C.case("nondefault_12x75x110")
    assert all(c[k] != v for k, v in C.DEFAULTS.items()) and c["W"] % 4 == 2 and c["H"] % c["rows"] and c["scenes"] == [5, 9]
    w = C.want("nondefault_12x75x110")
    assert w["keep"][:, 0].any() and w["keep"][:, 1].any() and len(set(w["counts"].tolist())) > 1
    assert C.case("small_9x13")["H"] * C.case("small_9x13")["W"] < 256 and C.want("small_9x13")["masks"].all()
    assert _painted_columns(C.want("wide_20x300")) == list(range(137, 144)) + list(range(247, 262))


# ------------------------------------------------------------------------------------------------ the conditions on the defaults
@pytest.mark.parametrize("which", ["translated", "raw"])
def test_defaults_hold_their_conditions(which):
    """The restatement with video's LINE_* defaults on the two clean videos of the measurement (frame 0 of tests/golden/tennis25.npz
    moved (1.5, 0.5) px per frame, 12 frames; the 25 raw frames): not one set pixel on the clean video, and with three planted
    full-height scratches (line_scratch_cases.plant, seeds 0 to 5) at least 95 % of the planted pixels are set and no set pixel
    lies farther than 4 columns from a planted one.  Measured: recall 0.951 ... 1.000 (translated), 0.969 ... 0.996 (raw), no
    stray pixel in any of the 12 runs (profiles/line_scratch.txt)."""
    s = dict(rows=video.LINE_ROWS, tau=video.LINE_TAU, gap=video.LINE_GAP, side=video.LINE_SIDE, drift=video.LINE_DRIFT,
             coverage=video.LINE_COVERAGE, span=video.LINE_SPAN, persist=video.LINE_PERSIST, radius=video.LINE_RADIUS)
    assert s == C.DEFAULTS
    fr = C.stats_video(ROOT, which)
    assert fr.shape == ((12 if which == "translated" else 25), 240, 432, 3)
    w = C.detect_np(fr, **s)
    print(which, "clean: set", int((w["masks"] > 0).sum()), "kept", int(w["counts"].sum()), "columns", int(w["col"].sum()),
          "candidates", int((w["cand"] > 0).sum()))
    assert not w["masks"].any() and not w["counts"].any()
    for seed in range(6):
        planted, marks = C.plant(fr, seed)
        recall, strays = C.recall_and_strays(C.detect_np(planted, **s)["masks"], marks)
        print(which, "seed", seed, "recall %.4f" % recall, "strays", strays)
        assert recall >= 0.95 and strays == 0


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_detect_line_scratches_checks_before_the_device(no_device):
    f = np.zeros((5, 32, 40, 3), np.uint8)
    call = video.detect_line_scratches
    for bad in (f[0], f[..., :2], np.zeros((5, 32, 40), np.uint8), f.astype(np.float32), f.astype(np.int32), [[1, 2, 3]], None):
        with pytest.raises(ValueError, match="frames"):
            call(bad)
    ranges = dict(rows=(4, 64), tau=(0, 254), gap=(0, 4), side=(1, 8), drift=(0, 2), coverage=(1, 100), span=(0, 4), persist=(1, 5),
                  radius=(0, 16))
    for name, (lo, hi) in ranges.items():
        for v in (lo - 1, hi + 1, lo + 0.5, True, False, None, str(lo), np.bool_(True)):
            with pytest.raises(ValueError, match=name):
                call(f, **{name: v})
    # persist is bounded by the frames that can vote: 2 span + 1
    for span, persist in ((0, 2), (1, 4), (4, 10)):
        with pytest.raises(ValueError, match="persist"):
            call(f, span=span, persist=persist)
    for scenes in ([0], [5], [2, 2], [3, 1], "auto", "", [True], 3):
        with pytest.raises(ValueError, match="scenes"):
            call(f, scenes=scenes)
    for v in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="return_counts"):
            call(f, return_counts=v)
    # good arguments pass the checks and reach the device layer, which the fixture has taken away; a CPU device is refused
    for kw in ({}, dict(scenes=[2]), dict(scenes=[]), dict(span=0, persist=1), dict(span=4, persist=9), dict(rows=4, radius=16),
               dict(rows=np.int64(64), tau=254, gap=4, side=8, drift=2, coverage=100)):
        with pytest.raises(AssertionError, match="device work"):
            call(f, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(f, device="cpu", **kw)
    scene_of, params = video._check_line_args(np.zeros((7, 32, 40, 3), np.uint8), [2, 5], 16, 6, 2, 3, 1, 50, 2, 3, 2, False)
    assert scene_of.dtype == np.int32 and scene_of.tolist() == [0, 0, 1, 1, 1, 2, 2] == C.scene_of_np(7, [2, 5]).tolist()
    assert params == (16, 6, 2, 3, 1, 50, 2, 3, 2)


def test_defaults_and_signature():
    sig = inspect.signature(video.detect_line_scratches).parameters
    assert list(sig) == ["frames_u8", "scenes"] + list(C.DEFAULTS) + ["return_counts", "device"]
    assert {k: sig[k].default for k in C.DEFAULTS} == C.DEFAULTS and sig["return_counts"].default is False
    assert {k: getattr(video, "LINE_" + k.upper()) for k in C.DEFAULTS} == C.DEFAULTS
    assert (ops.LINE_ROWS_MIN, ops.LINE_ROWS_MAX, ops.LINE_TAU_MAX, ops.LINE_GAP_MAX, ops.LINE_SIDE_MAX, ops.LINE_DRIFT_MAX,
            ops.LINE_SPAN_MAX, ops.LINE_RADIUS_MAX) == (4, 64, 254, 4, 8, 2, 4, 16)
    # the driver is untouched: no new parameter, no new mask string, the record as it was
    assert len(video._Call._fields) == 21 and video._Call._fields[-1] == "defects"
    assert not any("line" in k or "scratch" in k for k in inspect.signature(video.inpaint_video).parameters)


# ------------------------------------------------------------------------------------------------ header, binding, C entries
def _declared(header, name):
    decl = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert decl, name
    return [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")]


def test_header_and_binding_declare_the_entries():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    for name, args in ENTRIES.items():
        decl = _declared(header, name)
        assert decl == args, name
        res, types = lib.SYMBOLS[name]
        assert res is lib.C.c_int and len(types) == len(args)
        ints = {"L", "H", "W", "rows", "tau", "gap", "side", "drift", "coverage", "span", "persist", "radius"}
        assert [t is lib._i32 for t in types] == [a in ints for a in args] and all(t in (lib._i32, lib._fp) for t in types), name
    assert lib.ABI_VERSION == 9                          # symbols were only added
    assert all(callable(f) for f in (ops.line_sums, ops.line_columns, ops.line_paint, video.detect_line_scratches,
                                     video._check_line_args))
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "line_scratch.hip"]
    assert len(unit) == 1 and unit[0][1] == "line_scratch.o" and unit[0][1] in build.NOPK_OBJECTS and unit[0][2] == build.NOPK


def test_source_has_no_floating_point():
    src = open(os.path.join(ROOT, "e2fgvi_amd", "csrc", "line_scratch.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double|half)\b", code) and not re.search(r"\d\.\d*f?\b", code)
    assert len(re.findall(r"\batomic\w+\(", code)) == 1 and "atomicAdd(counts" in code


def test_built_object_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "line_scratch.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("object or llvm-objdump not present (python -m e2fgvi_amd.build)")
    # the sums, the columns, the keep and the paint kernel
    assert build.verify_no_scratch(obj="line_scratch.o", marker="line_", what="line scratch") == 4
    assert build.verify_no_pk_u8() == len(build.UNITS)


def test_entries_refuse_bad_arguments_and_return_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    ptrs = dict(frames=base + 1, S=base + (1 << 16), cand=base + (2 << 16) + 1, cnt=base + (3 << 16), col=base + (4 << 16) + 3,
                b0=base + (5 << 16), b1=base + (6 << 16), scene=base + (7 << 16), keep=base + (8 << 16) + 1, counts=base + (9 << 16),
                masks=base + (10 << 16) + 3)
    good = dict(ptrs, L=4, H=40, W=30, rows=16, tau=6, gap=2, side=3, drift=1, coverage=50, span=2, persist=3, radius=2)
    words = {"S", "cnt", "b0", "b1", "scene", "counts"}
    ranges = dict(rows=(4, 64), tau=(0, 254), gap=(0, 4), side=(1, 8), drift=(0, 2), coverage=(1, 100), span=(0, 4), radius=(0, 16))
    for name, args in ENTRIES.items():
        who = name[len("e2fgvi_"):].encode()

        def rc(**kw):
            a = dict(good, **kw)
            return getattr(so, name)(*[a[k] for k in args[:-1]], None)

        mine = [k for k in args if k in ptrs]
        null = {k: None for k in mine}
        for k in mine:
            assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), (name, k)
            if k in words:
                assert rc(**{k: ptrs[k] + 2}) == -1 and b"aligned" in so.e2fgvi_last_error(), (name, k)
        for k in ("L", "H", "W"):
            assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error(), (name, k)
        assert rc(H=46341, W=46341) == -1 and b"2^31" in so.e2fgvi_last_error()
        assert rc(H=1, W=2147483647 - 256) == -1 and rc(H=0x7fffffff, W=0x7fffffff) == -1
        for k, (lo, hi) in ranges.items():
            if k in args:
                for v in (lo - 1, hi + 1, -(1 << 30), 1 << 30):
                    assert rc(**{k: v}) == -1 and k.encode() in so.e2fgvi_last_error(), (name, k, v)
                    assert rc(**dict(null, **{k: v, "L": 0})) == -1          # decided from the arguments alone, work or not
        if "persist" in args:
            for span, persist in ((0, 2), (2, 6), (4, 10), (2, 0)):
                assert rc(span=span, persist=persist) == -1 and b"persist" in so.e2fgvi_last_error()
        # no work: no frame, no pixel, or no band -- nothing is launched and the pointers are not looked at
        for kw in (dict(L=0), dict(H=0), dict(W=0), dict(H=15), dict(H=3, rows=4), dict(L=0, H=0, W=0)):
            assert rc(**kw) == 0 and rc(**dict(null, **kw)) == 0, (name, kw)
    assert so.e2fgvi_abi_version() == 9
