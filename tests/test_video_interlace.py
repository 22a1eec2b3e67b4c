"""The host side of the deinterlacer (video.deinterlace, video.detect_interlace, video.field_order_from_scores) without a device:
the numpy restatement holds its named cases and every mutated restatement moves the case named for it, the guarantees that follow
from the definition, the planted clips the definition is judged on, every refusal before the device, the header and the binding,
and the C entries' refusals."""
import inspect
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import interlace_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"e2fgvi_interlace_scores": ["frames", "scene", "D", "L", "H", "W", "stream"],
           "e2fgvi_deinterlace": ["frames", "scene", "out", "L", "H", "W", "tff", "mode", "guard", "edges", "stream"]}


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_deinterlace_device", touched)


@pytest.fixture(scope="module")
def tennis():
    return C.tennis25(ROOT)


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name,case,setting", C.CAUGHT_BY, ids=[v[0] for v in C.CAUGHT_BY])
def test_every_variant_differs_from_the_definition_on_its_case(name, case, setting):
    if setting is None:
        a, b = C.want_scores(case), C.want_scores(case, **{name: True})
    else:
        a, b = C.want(case, setting), C.want(case, setting, **{name: True})
    print(name, case, setting, int((a != b).sum()))
    assert a.shape == b.shape and not np.array_equal(a, b)


def test_cases_hold_what_they_are_named_for():
    flags = dict((v[0], v[1]) for v in C.CAUGHT_BY)
    for flag in ("t0_not_halved", "guard_clamped", "two_without_one", "plus_vs_zero", "no_minus_one", "second_field_pair", "missing_zero",
                 "across_cut", "wrap_columns", "per_channel", "updn_border", "round_up", "score_rows_odd"):
        assert flags[flag] in C.NAMES, flag
    assert len(C.SETTINGS) == 36 and {s[0] for s in C.SETTINGS} == {0, 1} and {s[1] for s in C.SETTINGS} == {0, 1, 2}
    assert {s[2] for s in C.SETTINGS} == {0, 1} and {s[3] for s in C.SETTINGS} == {0, 1, 2}
    shapes = {(C.case(n)["H"], C.case(n)["W"]) for n in C.NAMES}
    assert {(H, W) for H in range(1, 7) for W in (1, 2, 3, 4, 5, 7)} <= shapes and {(37, 53), (9, 1100), (300, 20)} <= shapes
    assert {C.case(n)["L"] for n in C.NAMES} >= {1, 2, 3, 4}
    assert [C.case(n)["scenes"] for n in ("cut1_6x7", "cut2_6x7", "cut3_6x7", "cuts_6x7")] == [[1], [2], [3], [1, 2, 3]]
    assert all(C.case(n)["H"] * C.case(n)["W"] <= 10000 for n in C.NAMES)
    for n in ("extremes_12x13", "extremes_40x52"):
        assert set(np.unique(C.case(n)["frames"]).tolist()) == {0, 255}
        # both ends of the clamp are reached: bytes of the result that are neither the line average nor the temporal mean
        got = C.want(n, (1, 0, 1, 0))
        assert set(np.unique(got).tolist()) >= {0, 127, 255}
    # a flat video comes back flat at every setting: every score ties and J stays 0
    for s in C.SETTINGS:
        assert (C.want("flat_8x9", s) == 90).all()
    for n in ("noise_37x53", "tiny_1x1", "tiny_2x3", "cut2_6x7", "single_6x7"):
        c = C.case(n)
        for tff, guard, edges in ((1, 1, 0), (0, 0, 2), (0, 1, 1)):
            full = C.want(n, (tff, 0, guard, edges))
            assert full.shape == (2 * c["L"],) + c["frames"].shape[1:] and full.dtype == np.uint8
            # the kept rows are the caller's bytes
            kept = ~C.missing_rows(len(full), c["H"], bool(tff))
            assert np.array_equal(full[kept], np.repeat(c["frames"], 2, axis=0)[kept])
            # the frame-rate results, computed on their own, are the even and the odd pictures
            for mode in (1, 2):
                own = C.deinterlace_np(c["frames"], c["scenes"], tff, mode, guard, edges)
                assert own.shape == c["frames"].shape and np.array_equal(own, full[mode - 1::2])
    # one row: the missing picture is the temporal mean, the first frame's previous field is its own
    c = C.case("tiny_1x5")
    fr = c["frames"].astype(np.int64)
    full = C.want("tiny_1x5", (1, 0, 1, 2))
    assert np.array_equal(full[0::2], c["frames"]) and np.array_equal(full[1], (fr[0] + fr[1]) >> 1) and np.array_equal(full[5], fr[2])
    full = C.want("tiny_1x5", (0, 0, 1, 0))
    assert np.array_equal(full[1::2], c["frames"]) and np.array_equal(full[2], (fr[0] + fr[1]) >> 1) and np.array_equal(full[0], fr[0])
    # scores: nothing under four rows, nothing on the last frame of a scene, as many even rows as odd ones
    for n in C.NAMES:
        c, D = C.case(n), C.want_scores(n)
        assert D.shape == (c["L"], 2) and D.dtype == np.int64 and not D[-1].any() and (D >= 0).all()
        if c["H"] < 4:
            assert not D.any()
    assert not C.want_scores("cuts_6x7").any() and not C.want_scores("cut2_6x7")[1].any() and C.want_scores("cut2_6x7")[[0, 2]].all()
    Y = C.luma(C.case("tiny_5x4")["frames"])
    assert C.want_scores("tiny_5x4")[0].tolist() == [int(np.abs(2 * Y[1][2] - Y[0][1] - Y[0][3]).sum()), int(np.abs(2 * Y[1][1] - Y[0][0] - Y[0][2]).sum())]


def test_scene_by_scene_is_the_call_with_scenes():
    c = C.case("cut2_40x52")
    for s in ((1, 0, 1, 0), (0, 0, 0, 2), (1, 2, 1, 1)):
        parts = [C.deinterlace_np(c["frames"][a:b], None, *s) for a, b in ((0, 2), (2, 4))]
        assert np.array_equal(np.concatenate(parts), C.want("cut2_40x52", s))
    assert np.array_equal(np.concatenate([C.scores_np(c["frames"][:2]), C.scores_np(c["frames"][2:])]), C.want_scores("cut2_40x52"))


# ------------------------------------------------------------------------------------------------ the field order rule
def test_field_order_from_scores_on_hand_made_tables():
    rule = video.field_order_from_scores
    t = lambda rows: np.array(rows, np.int64).reshape(-1, 2)
    # 100 * 94 < 95 * 100 votes, 100 * 95 < 95 * 100 does not; the last frame never votes
    assert rule(t([[94, 100], [95, 100], [100, 94], [1, 1000]]))[1].tolist() == [1, 0, -1, 0]
    assert rule(t([[94, 100], [95, 100], [100, 94], [1, 1000]]))[0] == "mixed"
    assert rule(t([[89, 100], [90, 100], [0, 0]]), margin=10)[1].tolist() == [1, 0, 0]
    assert rule(t([[50, 100], [51, 100], [0, 0]]), margin=50)[1].tolist() == [0, 0, 0]
    assert rule(t([[49, 100], [100, 49], [0, 0]]), margin=50)[1].tolist() == [1, -1, 0]
    for rows, scenes, verdict in (([[1, 2]] * 9, None, "tff"), ([[2, 1]] * 9, None, "bff"), ([[5, 5]] * 9, None, "progressive"),
                                  ([], None, "progressive"), ([[1, 2]], None, "progressive"), ([[1, 2]] * 4, [1, 2, 3], "progressive"),
                                  # 8 pairs: two votes are a quarter of them; one is not
                                  ([[1, 2]] * 2 + [[5, 5]] * 7, None, "tff"), ([[1, 2]] + [[5, 5]] * 8, None, "progressive"),
                                  # n+ > 2 n-: 5 against 2 is tff, 4 against 2 is mixed, and the mirror
                                  ([[1, 2]] * 5 + [[2, 1]] * 2 + [[0, 0]], None, "tff"), ([[1, 2]] * 4 + [[2, 1]] * 2 + [[0, 0]], None, "mixed"),
                                  ([[2, 1]] * 5 + [[1, 2]] * 2 + [[0, 0]], None, "bff"), ([[2, 1]] * 4 + [[1, 2]] * 2 + [[0, 0]], None, "mixed"),
                                  # a cut takes the pair in front of it out: frames 0 .. 2 say tff, frame 3 would say bff
                                  ([[1, 2]] * 3 + [[2, 1]] + [[1, 2]] * 2, [4], "tff")):
        got, votes = rule(t(rows), scenes)
        assert got == verdict == C.field_order_np(t(rows), scenes)[0], (rows, scenes, got)
        assert votes.dtype == np.int8 and votes.shape == (len(rows),) and np.array_equal(votes, C.field_order_np(t(rows), scenes)[1])
    assert rule(t([[1, 2]] * 3 + [[2, 1]] + [[1, 2]] * 2), [4])[1].tolist() == [1, 1, 1, 0, 1, 0]
    # exact at the size of the scores: 2^36 a word
    k = (1 << 36) // 100
    assert rule(t([[95 * k - 1, 100 * k], [0, 0]]))[1].tolist() == [1, 0] and rule(t([[95 * k, 100 * k], [0, 0]]))[1].tolist() == [0, 0]
    assert rule(t([[100 * k, 95 * k - 1], [0, 0]]))[1].tolist() == [-1, 0] and rule(t([[100 * k, 95 * k], [0, 0]]))[1].tolist() == [0, 0]
    for bad in (np.zeros((3, 2), np.int32), np.zeros((3, 2), np.float64), np.zeros((3, 3), np.int64), np.zeros(6, np.int64), [[1, 2]], None):
        with pytest.raises(ValueError, match="D must"):
            rule(bad)
    for margin in (0, 51, 5.5, True, None, "5"):
        with pytest.raises(ValueError, match="margin"):
            rule(t([[1, 2]] * 3), margin=margin)
    for scenes in ([0], [3], "auto", [2, 1]):
        with pytest.raises(ValueError, match="scenes"):
            rule(t([[1, 2]] * 3), scenes)
    assert video.INTERLACE_MARGIN == 5 and inspect.signature(rule).parameters["margin"].default == 5


# ------------------------------------------------------------------------------------------------ the planted clips
def test_locked_off_clip_beats_line_averaging_and_the_pan_is_close_to_it(tennis):
    """conditions 1 to 3: with the defaults the locked-off clip beats line averaging by at least 3 dB and the pan is within 2 dB of
    it; the kept rows are the source's bytes.  The restatement's figures: locked-off 36.16 dB against 27.88 for
    line averaging and 34.20 for weaving, pan 29.04 against 29.53 and 19.47."""
    for name, (clip, src), lo in (("locked-off", C.locked_off_clip(tennis), 3.0), ("pan", C.pan_clip(tennis), -2.0)):
        got = C.deinterlace_np(clip, None, 1, 0, 1, 0)
        ours, avg, weave = C.psnr_missing(got, src), C.psnr_missing(C.line_average(clip), src), C.psnr_missing(C.weave_fields(clip), src)
        print(name, "ours %.2f line averaging %.2f weaving %.2f" % (ours, avg, weave))
        assert ours >= avg + lo, name
        kept = ~C.missing_rows(len(got), got.shape[1])
        assert got.shape == src.shape and np.array_equal(got[kept], src[kept])
    assert C.DEFAULTS == dict(order="tff", rate="field", keep="first", guard=True, edges=0)


def test_still_video_comes_back_doubled_without_the_guard_and_changed_with_it(tennis):
    """condition 4: four copies of a frame come back as eight, byte for byte, with guard=False; with guard=True they do not, which
    is what the docstring warns of (the restatement changes 302 276 bytes of 2 488 320)"""
    still = np.repeat(tennis[:1], 4, axis=0)
    assert np.array_equal(C.deinterlace_np(still, None, 1, 0, 0, 0), np.repeat(tennis[:1], 8, axis=0))
    changed = int((C.deinterlace_np(still, None, 1, 0, 1, 0) != np.repeat(tennis[:1], 8, axis=0)).sum())
    print("bytes changed by the guard on a still video", changed)
    assert changed > 0
    doc = " ".join(video.deinterlace.__doc__.split())
    assert "``guard=True`` changes static detail" in doc and "does not come back byte for byte" in doc


def test_verdicts_on_the_planted_clips(tennis):
    """condition 5: "tff", "bff", "progressive", "tff" for the pan in either order, the progressive frames and the locked-off clip"""
    for name, clip, verdict in (("pan tff", C.pan_clip(tennis, True)[0], "tff"), ("pan bff", C.pan_clip(tennis, False)[0], "bff"),
                                ("progressive", tennis[:12], "progressive"), ("locked-off", C.locked_off_clip(tennis)[0], "tff")):
        D = C.scores_np(clip)
        ratio = D[:-1, 0] / D[:-1, 1]
        got, votes = video.field_order_from_scores(D)
        print(name, "D0 / D1 %.3f .. %.3f" % (ratio.min(), ratio.max()), got, votes.tolist())
        assert got == verdict == C.field_order_np(D)[0], name


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_deinterlace_checks_before_the_device(no_device):
    f = np.zeros((5, 32, 40, 3), np.uint8)
    call = video.deinterlace
    for bad in (f[0], f[..., :2], np.zeros((5, 32, 40), np.uint8), f.astype(np.float32), f.astype(np.int32), [[1, 2, 3]], None):
        with pytest.raises(ValueError, match="frames"):
            call(bad)
    for name, values in dict(order=("TFF", "", "progressive", None, 1, True), rate=("fields", "", None, 2, True),
                             keep=("both", "", None, 0, False)).items():
        for v in values:
            with pytest.raises(ValueError, match=name):
                call(f, **dict(dict(rate="frame"), **{name: v}))
    with pytest.raises(ValueError, match="keep"):
        call(f, rate="field", keep="second")
    with pytest.raises(ValueError, match="keep"):
        call(f, keep="second")
    for v in (-1, 3, 0.5, True, False, None, "1", np.bool_(True)):
        with pytest.raises(ValueError, match="edges"):
            call(f, edges=v)
    for v in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="guard"):
            call(f, guard=v)
    for scenes in ([0], [5], [2, 2], [3, 1], "auto", "", [True], 3):
        with pytest.raises(ValueError, match="scenes"):
            call(f, scenes=scenes)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(1, 8193, 8192, 3), strides=(0, 0, 0, 0))
    with pytest.raises(ValueError, match="frames"):
        call(big)
    for kw in ({}, dict(scenes=[2]), dict(scenes=[]), dict(order="bff"), dict(order="auto"), dict(rate="frame"), dict(rate="frame", keep="second"),
               dict(guard=False, edges=2), dict(edges=np.int64(1)), dict(guard=np.bool_(False))):
        with pytest.raises(AssertionError, match="device work"):
            call(f, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(f, device="cpu", **kw)
    scene_of, cuts, mode, edges = video._check_deinterlace_args(np.zeros((7, 32, 40, 3), np.uint8), "bff", "frame", "second", [2, 5], True, 2)
    assert scene_of.dtype == np.int32 and scene_of.tolist() == [0, 0, 1, 1, 1, 2, 2] == C.scene_of_np(7, [2, 5]).tolist()
    assert (cuts, mode, edges) == ([2, 5], 2, 2)
    assert [video._check_deinterlace_args(f, "tff", r, k, None, True, 0)[2] for r, k in (("field", "first"), ("frame", "first"), ("frame", "second"))] == [0, 1, 2]


def test_detect_interlace_checks_before_the_device(no_device):
    f = np.zeros((5, 32, 40, 3), np.uint8)
    call = video.detect_interlace
    for bad in (f[0], f[..., :2], f.astype(np.float32), None):
        with pytest.raises(ValueError, match="frames"):
            call(bad)
    for v in (0, 51, 2.5, True, False, None, "5", np.bool_(True)):
        with pytest.raises(ValueError, match="margin"):
            call(f, margin=v)
    for v in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="return_scores"):
            call(f, return_scores=v)
    for scenes in ([0], [5], [2, 2], "auto", "", [True], 3):
        with pytest.raises(ValueError, match="scenes"):
            call(f, scenes=scenes)
    for kw in ({}, dict(scenes=[2]), dict(margin=1), dict(margin=50, return_scores=True), dict(margin=np.int64(7))):
        with pytest.raises(AssertionError, match="device work"):
            call(f, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(f, device="cpu", **kw)


def test_defaults_and_signature():
    sig = inspect.signature(video.deinterlace).parameters
    assert list(sig) == ["frames_u8", "order", "rate", "keep", "scenes", "guard", "edges", "device"]
    assert {k: sig[k].default for k in C.DEFAULTS} == C.DEFAULTS and sig["scenes"].default is None and sig["device"].default is None
    sig = inspect.signature(video.detect_interlace).parameters
    assert list(sig) == ["frames_u8", "scenes", "margin", "return_scores", "device"]
    assert sig["margin"].default == 5 and sig["return_scores"].default is False and sig["scenes"].default is None
    assert list(inspect.signature(video.field_order_from_scores).parameters) == ["D", "scenes", "margin"]
    assert list(inspect.signature(ops.deinterlace).parameters) == ["frames", "scene", "tff", "mode", "guard", "edges", "out"]
    assert list(inspect.signature(ops.interlace_scores).parameters) == ["frames", "scene"]
    assert ops.INTERLACE_EDGES_MAX == 2 and ops.INTERLACE_MODES == {"field": 0, "first": 1, "second": 2}
    # the driver is untouched: no new parameter, the record as it was
    assert len(video._Call._fields) == 21 and video._Call._fields[-1] == "defects"
    assert not any("interlace" in k or "field" in k for k in inspect.signature(video.inpaint_video).parameters)
    for word in ("in front of deflicker", "[2 c for c in cuts]", "3:2 pulldown is not undone", "are not converted", "no better than line averaging",
                 "``guard=True`` changes static detail", 'order="auto"', "runs detect_interlace first", "kept rows are the caller's bytes"):
        assert word in " ".join(video.deinterlace.__doc__.split()), word


# ------------------------------------------------------------------------------------------------ header, binding, C entries
def _declared(header, name):
    decl = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert decl, name
    return [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")]


def test_header_and_binding_declare_the_entries():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    ints = {"L", "H", "W", "tff", "mode", "guard", "edges"}
    for name, args in ENTRIES.items():
        assert _declared(header, name) == args, name
        res, types = lib.SYMBOLS[name]
        assert res is lib.C.c_int and len(types) == len(args)
        assert [t is lib._i32 for t in types] == [a in ints for a in args] and all(t in (lib._i32, lib._fp) for t in types), name
    assert lib.ABI_VERSION == 9                          # symbols were only added
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "interlace.hip"]
    assert len(unit) == 1 and unit[0][1] == "interlace.o" and unit[0][1] in build.NOPK_OBJECTS and unit[0][2] == build.NOPK
    # the row of the table build() walks: verify_no_scratch over the unit's kernels on every build
    assert ("interlace.o", "interlace_", "deinterlacer", False) in build.KERNEL_CHECKS and "for obj, marker, what, _ in KERNEL_CHECKS" in inspect.getsource(build.build)


def test_source_has_no_floating_point():
    src = open(os.path.join(ROOT, "e2fgvi_amd", "csrc", "interlace.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double|half)\b", code) and not re.search(r"\d\.\d*f?\b", code)


def test_built_object_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "interlace.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("object or llvm-objdump not present (python -m e2fgvi_amd.build)")
    # the scores kernel and the fields kernel without and with the direction search, for either field order
    assert build.verify_no_scratch(obj="interlace.o", marker="interlace_", what="deinterlacer") == 5


def test_entries_refuse_bad_arguments_and_return_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    ptrs = dict(frames=base + 1, scene=base + (1 << 16), D=base + (2 << 16), out=base + (8 << 16) + 3)
    good = dict(ptrs, L=4, H=40, W=30, tff=1, mode=0, guard=1, edges=0)
    ranges = dict(tff=(0, 1), mode=(0, 2), guard=(0, 1), edges=(0, 2))
    for name, args in ENTRIES.items():
        who = name[len("e2fgvi_"):].encode()

        def rc(**kw):
            a = dict(good, **kw)
            return getattr(so, name)(*[a[k] for k in args[:-1]], None)

        mine = [k for k in args if k in ptrs]
        null = {k: None for k in mine}
        for k in mine:
            assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), (name, k)
        assert rc(scene=ptrs["scene"] + 2) == -1 and b"aligned" in so.e2fgvi_last_error()
        if "D" in args:
            assert rc(D=ptrs["D"] + 4) == -1 and b"aligned" in so.e2fgvi_last_error()
        for k in ("L", "H", "W"):
            assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), (name, k)
        assert rc(**dict(null, H=8193, W=8192)) == -1 and b"2^26" in so.e2fgvi_last_error()
        assert rc(**dict(null, H=0x7fffffff, W=0x7fffffff)) == -1
        assert rc(**dict(null, H=8192, W=8192)) == -1 and b"null" in so.e2fgvi_last_error()
        for k, (lo, hi) in ranges.items():
            if k in args:
                for v in (lo - 1, hi + 1, -(1 << 30), 1 << 30):
                    assert rc(**{k: v}) == -1 and k.encode() in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), (name, k, v)
                    assert rc(**dict(null, **{k: v, "L": 0})) == -1          # decided from the arguments alone, work or not
        # no work: no frame or no pixel -- nothing is launched and the pointers are not looked at
        for kw in (dict(L=0), dict(H=0), dict(W=0), dict(L=0, H=0, W=0)):
            assert rc(**kw) == 0 and rc(**dict(null, **kw)) == 0, (name, kw)
    # any overlap of out with frames is refused, out == frames too; the field-rate result is twice as long
    run = lambda frames, out, mode: so.e2fgvi_deinterlace(frames, ptrs["scene"], out, 4, 40, 30, 1, mode, 1, 0, None)
    size = 3 * 4 * 40 * 30
    for frames, out in ((base, base), (base, base + 1), (base, base + size - 1), (base + size - 1, base), (base + 5, base)):
        for mode in (0, 1, 2):
            assert run(frames, out, mode) == -1 and b"overlap" in so.e2fgvi_last_error(), (frames, out, mode)
    assert run(base + 2 * size - 1, base, 0) == -1 and b"overlap" in so.e2fgvi_last_error()
    assert so.e2fgvi_abi_version() == 9
