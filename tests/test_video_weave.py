"""The host side of the weave stabiliser (video.stabilize, video.apply_shifts) without a device: the numpy restatement holds its
named cases and every mutated restatement moves the case named for it, the guarantees that follow from the definition, planted
weave on a static camera and on the tennis clip, every refusal before the device, the header and the binding, and the C
entries' refusals."""
import inspect
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import weave_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"e2fgvi_weave_profiles": ["frames", "col", "row", "L", "H", "W", "stream"],
           "e2fgvi_weave_match": ["col", "row", "scene", "motion", "L", "H", "W", "radius", "tex", "stream"],
           "e2fgvi_weave_path": ["motion", "scene", "shift", "L", "span", "max_shift", "subpixel", "stream"],
           "e2fgvi_weave_apply": ["frames", "shift", "out", "mask", "L", "H", "W", "C", "stream"]}


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_stabilize_device", touched)


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name,case", C.CAUGHT_BY, ids=[v[0] for v in C.CAUGHT_BY])
def test_every_variant_differs_from_the_definition_on_its_case(name, case):
    seen = [k for k in C.KEYS if not np.array_equal(C.want(case)[k], C.want(case, **{name: True})[k])]
    print(name, case, seen)
    assert seen


def test_cases_hold_what_they_are_named_for():
    assert len(C.VARIANTS) >= 8 and C.DEFAULTS == dict(span=4, radius=16, max_shift=16, tex=2, subpixel=True)
    for flag in ("shift_sign", "tie_positive", "no_c0_rule", "upper_median", "asym_window", "across_cut", "across_untrusted",
                 "mask_clamped", "trunc_q"):
        assert flag in dict(C.CAUGHT_BY)
    for n in C.NAMES:
        c, w = C.case(n), C.want(n)
        L, H, W = c["L"], c["H"], c["W"]
        assert H * W <= 10000, n
        assert [(w[k].shape, w[k].dtype) for k in C.KEYS] == [((L, 8, W), np.int32), ((L, 8, H), np.int32), ((L, 4), np.int32),
                                                             ((L, 2), np.int32), ((L, H, W, 3), np.uint8), ((L, H, W), np.uint8)]
        # either set of profiles adds up to the frame's luma
        total = C.luma(c["frames"]).reshape(L, -1).sum(axis=1)
        assert np.array_equal(w["col"].sum(axis=(1, 2)), total) and np.array_equal(w["row"].sum(axis=(1, 2)), total)
        assert not w["motion"][0].any() and np.abs(w["shift"]).max(initial=0) <= 16 * c["max_shift"]
        assert w["motion"][:, 2:].min() >= 0 and w["motion"][:, 2:].max() <= 8 and set(np.unique(w["mask"]).tolist()) <= {0, 255}
        # an untrusted pair has motion 0; a frame that is not moved has the caller's bytes and no mask
        assert not w["motion"][:, :2][w["motion"][:, 2:] < 4].any()
        still = ~w["shift"].any(axis=1)
        assert np.array_equal(w["out"][still], c["frames"][still]) and not w["mask"][still].any()
        # the first and the last frame of the video end a segment
        assert not w["shift"][[0, -1]].any()
    shapes = {(C.case(n)["H"], C.case(n)["W"]) for n in C.NAMES}
    assert {(40, 52), (37, 53), (7, 64), (1, 1), (64, 9)} <= shapes and {C.case(n)["L"] for n in C.NAMES} >= {1, 2, 9}
    assert {C.case(n)["radius"] for n in C.NAMES} >= {1, 32} and {C.case(n)["span"] for n in C.NAMES} >= {0, 1, 16}
    # H = 7: row band 0 is empty, seven bands count on x, none on y
    assert C.want("rows_7x64")["motion"][1].tolist() == [32, 0, 7, 0] and not C.want("rows_7x64")["col"][:, 0].any()
    # a window shorter than 2 R: nothing is trusted; one pixel; a flat frame
    for n in ("short_64x9", "one_1x1", "flat"):
        assert not C.want(n)["motion"].any() and C.want(n)["out"].tobytes() == C.case(n)["frames"].tobytes(), n
    assert C.want("r1")["motion"][1:, 2:].min() == 8 and np.abs(C.want("r1")["motion"][:, :2]).max() <= 8
    assert C.want("r32_8x141")["motion"][:, 0].tolist() == [0, 400, -448]
    assert not C.want("span0")["shift"].any() and C.want("span0")["motion"].any()
    c, w = C.case("cut_mid"), C.want("cut_mid")
    assert c["scenes"] == [4] and not w["motion"][4].any() and not w["shift"][[3, 4]].any() and w["shift"][[1, 2, 5, 6, 7]].all()
    w = C.want("flat_mid")
    assert w["motion"][[4, 5], 2:].max() < 4 and not w["shift"][3:6].any() and w["shift"][[1, 2, 6, 7]].any(axis=1).all()
    c, w = C.case("clamp"), C.want("clamp")
    assert np.abs(w["shift"]).max() == 16 * c["max_shift"] == 16 and np.abs(C.want("clamp", no_clamp=True)["shift"]).max() > 16
    assert C.want("periodic_tie")["motion"][1].tolist() == [-32, 0, 8, 8]
    assert C.want("exact_edge")["motion"][1].tolist() == [0, 0, 8, 8] and C.want("exact_edge", no_c0_rule=True)["motion"][1, 0] > 0
    assert C.want("two_motions")["motion"][1:, 0].tolist() == [16, 16] and C.want("two_motions", upper_median=True)["motion"][1, 0] == 48
    # fractions of either sign, and their whole-pixel rounding
    s = C.want("sub_37x53")["shift"]
    assert (s < 0).any() and (s > 0).any() and (s & 15).any()
    assert np.array_equal(C.want("whole_37x53")["shift"], ((s + 8) >> 4) << 4)
    assert C.case("tall_300x20")["H"] > 8 * 32 and C.case("wide_9x1100")["W"] > 1024


# ------------------------------------------------------------------------------------------------ what follows from the definition
def test_whole_pixel_shift_copies_bytes_and_the_mask_is_what_was_exposed():
    fr = C.case("sub_37x53")["frames"][:3]
    out, mask = C.apply_np(fr, np.array([[32, -48], [0, 0], [-16, 0]], np.int32))
    assert np.array_equal(out[0][:-3, 2:], fr[0][3:, :-2]) and mask[0][:-3, 2:].max() == 0 and mask[0][-3:].min() == 255 == mask[0][:, :2].min()
    assert out[1].tobytes() == fr[1].tobytes() and not mask[1].any()
    assert np.array_equal(out[2][:, :-1], fr[2][:, 1:]) and np.array_equal(out[2][:, -1], fr[2][:, -1]) and mask[2][:, :-1].max() == 0
    # a fraction: floor semantics for a negative shift -- X = 16 x + 5: x0 = x, fx = 5
    out, mask = C.apply_np(fr[:1], np.array([[-5, 0]], np.int32))
    a, b = fr[0][:, :-1].astype(np.int64), fr[0][:, 1:].astype(np.int64)
    assert np.array_equal(out[0][:, :-1], (16 * (11 * a + 5 * b) + 128) >> 8) and mask[0][:, :-1].max() == 0 and mask[0][:, -1].min() == 255
    # one plane moves like three
    planes, _ = C.apply_np(fr[..., 1], np.array([[-37, 43]] * 3, np.int32))
    assert np.array_equal(planes, C.apply_np(fr, np.array([[-37, 43]] * 3, np.int32))[0][..., 1])


def test_constant_motion_gets_no_correction():
    """the symmetric mean of a straight path is the path, whatever the speed, the span and the length"""
    for L, span, m in ((9, 4, (37, -5)), (2, 1, (16, 16)), (30, 16, (-100, 3)), (5, 16, (1, 0))):
        motion = np.tile(np.array([m[0], m[1], 8, 8], np.int32), (L, 1))
        motion[0] = 0
        assert not C.path_np(motion, C.scene_of_np(L), span, 16).any()
        # and inside either scene around a cut
        cut = L // 2
        motion[cut] = 0
        assert not C.path_np(motion, C.scene_of_np(L, [cut]), span, 16).any()


def test_constant_pan_comes_back_byte_for_byte():
    """crops of one random-texture image, two columns a frame.  Along the axis of the pan the crops' profiles are equal up to the
    move, so the match is exact: 32 on every pair.  The other axis sees other columns in its bands on every frame and its motion
    is 0 give or take a sixteenth, so the frames are made too low for a window on it here; the case "pan" -- a diagonal pan,
    both axes measured, motion within 3/16 px of the pan -- comes back byte for byte once corrections are whole pixels"""
    fr = C.crops(9, 16, 200, 50, pan=(2, 0))
    w = C.stabilize_np(fr, radius=4)
    assert w["motion"][1:].tolist() == [[32, 0, 8, 0]] * 8 and not w["shift"].any()
    assert w["out"].tobytes() == fr.tobytes() and not w["mask"].any()
    c, w = C.case("pan"), C.want("pan")
    assert np.abs(w["motion"][1:, :2] - np.array([32, -16])).max() <= 3 and w["motion"][1:, 2:].min() == 8
    assert np.abs(w["shift"]).max() <= 1
    whole = C.stabilize_np(c["frames"], **dict(C.settings(c), subpixel=False))
    assert not whole["shift"].any() and whole["out"].tobytes() == c["frames"].tobytes()


@pytest.mark.parametrize("axis", [0, 1])
def test_planted_weave_on_a_static_camera_is_measured_exactly(axis):
    """a static camera with whole-pixel weave along one axis: on that axis the path is 16 times the plant, the corrections the
    hand formula.  (The other axis sees other columns -- or rows -- in its bands on every frame: its match is not exact and its
    motion is 0 give or take a sixteenth; it is printed.)"""
    plant = np.array([0, 2, -1, 3, 0, -3, 1, 1, -2, 2, 0, -1])
    L, span = len(plant), 3
    moves = [None, None]
    moves[axis] = 16 * plant
    fr = C.crops(L, 48, 60, 51 + axis, *moves)
    w = C.stabilize_np(fr, span=span, radius=6)
    print("axis", axis, "the other axis' motion", w["motion"][:, 1 - axis].tolist(), "bands", w["motion"][:, 3 - axis].tolist())
    assert w["motion"][1:, 2 + axis].min() == 8
    path = np.cumsum(w["motion"][:, axis])
    assert np.array_equal(path, 16 * plant)
    hand = []
    for t in range(L):
        k = min(span, t, L - 1 - t)
        window = [16 * int(v) for v in plant[t - k:t + k + 1]]
        hand.append(int(np.floor(sum(window) / len(window) + 0.5)) - 16 * int(plant[t]))
    assert w["shift"][:, axis].tolist() == hand


def test_planted_weave_on_tennis25_is_measured():
    """tests/golden/tennis25.npz (25 frames of 240 x 432, the camera pans, the player moves) under weave_cases.plant(seed 1) --
    whole-pixel weave of +-3 px with replicated borders -- at radius 24: the restatement's pair motion differs from the clean
    video's motion plus the planted difference by at most 8/16 px on at least 22 of the 24 pairs, per axis.  Measured (DESIGN.md
    3v): along x at most 6/16 px on 23 pairs and 198/16 on the pair of frames 20 and 21, where the pan is fast and blurred;
    along y at most 2/16 px on all 24.  The planted weave's rms goes from 2.12 px to 1.55 px over both axes at span 4 -- the one
    wrong pair bends the x path; y alone keeps 0.88 of 1.92 px, the mean of the weave over the window."""
    clean = C.tennis25(ROOT)
    planted, d = C.plant(clean, 1)
    assert np.abs(d).max() == 3 and planted.shape == clean.shape
    so = C.scene_of_np(len(clean))
    mc = C.match_np(*C.profiles_np(clean), so, 24, 2)
    mp = C.match_np(*C.profiles_np(planted), so, 24, 2)
    for axis in range(2):
        err = np.abs(mp[1:, axis] - (mc[1:, axis] + 16 * np.diff(d[:, axis])))
        print("axis", axis, "errors in 1/16 px", err.tolist(), "valid bands", mp[1:, 2 + axis].tolist(), "clean motion", mc[1:, axis].tolist())
        assert (err <= 8).sum() >= 22
    shift = C.path_np(mp, so, 4, 16)
    before, after = C.residual_rms(0 * shift, d), C.residual_rms(shift - C.path_np(mc, so, 4, 16), d)
    print("residual weave rms px", before, "->", after)
    assert after < before


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_stabilize_checks_before_the_device(no_device):
    f = np.zeros((5, 32, 40, 3), np.uint8)
    call = video.stabilize
    for bad in (f[0], f[..., :2], np.zeros((5, 32, 40), np.uint8), f.astype(np.float32), f.astype(np.int32), [[1, 2, 3]], None):
        with pytest.raises(ValueError, match="frames"):
            call(bad)
    for name, (lo, hi) in dict(span=(0, 16), radius=(1, 32), max_shift=(1, 64), tex=(0, 65535)).items():
        for v in (lo - 1, hi + 1, lo + 0.5, True, False, None, str(lo), np.bool_(True)):
            with pytest.raises(ValueError, match=name):
                call(f, **{name: v})
    for scenes in ([0], [5], [2, 2], [3, 1], "auto", "", [True], 3):
        with pytest.raises(ValueError, match="scenes"):
            call(f, scenes=scenes)
    for flag in ("subpixel", "return_shifts", "return_mask"):
        for v in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match=flag):
                call(f, **{flag: v})
    # a side above 4096: from the shape alone (the array is never touched)
    for shape in ((1, 4097, 8, 3), (1, 8, 4097, 3)):
        big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=shape, strides=(0, 0, 0, 0))
        with pytest.raises(ValueError, match="frames"):
            call(big)
    # good arguments pass the checks and reach the device layer, which the fixture has taken away; a CPU device is refused
    for kw in ({}, dict(scenes=[2]), dict(scenes=[]), dict(span=0), dict(span=16, radius=32, max_shift=64, tex=0), dict(radius=np.int64(1)),
               dict(subpixel=False, return_shifts=True, return_mask=True)):
        with pytest.raises(AssertionError, match="device work"):
            call(f, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(f, device="cpu", **kw)
    scene_of, *rest = video._check_stabilize_args(np.zeros((7, 32, 40, 3), np.uint8), [2, 5], 4, 16, 16, 2, True, False, False)
    assert scene_of.dtype == np.int32 and scene_of.tolist() == [0, 0, 1, 1, 1, 2, 2] == C.scene_of_np(7, [2, 5]).tolist()
    assert rest == [4, 16, 16, 2]


def test_apply_shifts_checks_before_the_device(no_device):
    f, s = np.zeros((5, 32, 40, 3), np.uint8), np.zeros((5, 2), np.int32)
    for bad in (f[0, 0], f[..., :2], f.astype(np.float32), None):
        with pytest.raises(ValueError, match="frames"):
            video.apply_shifts(bad, s)
    for bad in (s[:4], s.astype(np.int64), s.astype(np.float32), s[:, :1], None, [[0, 0]] * 5):
        with pytest.raises(ValueError, match="shifts"):
            video.apply_shifts(f, bad)
    for good in (f, f[..., 0]):
        with pytest.raises(AssertionError, match="device work"):
            video.apply_shifts(good, s)
        with pytest.raises(RuntimeError, match="no CPU path"):
            video.apply_shifts(good, s, device="cpu")


def test_defaults_and_signature():
    sig = inspect.signature(video.stabilize).parameters
    assert list(sig) == ["frames_u8", "scenes", "span", "radius", "max_shift", "tex", "subpixel", "return_shifts", "return_mask", "device"]
    assert {k: sig[k].default for k in C.DEFAULTS} == C.DEFAULTS and sig["return_shifts"].default is False
    assert sig["return_mask"].default is False and sig["scenes"].default is None and sig["device"].default is None
    assert dict(span=video.WEAVE_SPAN, radius=video.WEAVE_RADIUS, max_shift=video.WEAVE_MAX_SHIFT, tex=video.WEAVE_TEX, subpixel=True) == C.DEFAULTS
    assert (ops.WEAVE_BANDS, ops.WEAVE_RADIUS_MAX, ops.WEAVE_SPAN_MAX, ops.WEAVE_SHIFT_MAX) == (8, 32, 16, 64) == (C.NB, 32, 16, C.SHIFT_LIMIT // 16)
    assert list(inspect.signature(video.apply_shifts).parameters) == ["frames_u8", "shifts", "device"]
    assert list(inspect.signature(ops.weave_apply).parameters) == ["frames", "shift", "out", "mask", "return_mask"]
    # the driver is untouched: no new parameter, the record as it was
    assert len(video._Call._fields) == 21 and video._Call._fields[-1] == "defects"
    assert not any("weave" in k or "stabil" in k for k in inspect.signature(video.inpaint_video).parameters)
    for word in ("byte for byte", "first and last frame of a segment", "untrusted pair", "translation only", "no rotation", "softens",
                 "subpixel=False", "bends the path", "inpaint_video", "apply_shifts", "after deflicker", "2 span + 1"):
        assert word in video.stabilize.__doc__, word


# ------------------------------------------------------------------------------------------------ header, binding, C entries
def _declared(header, name):
    decl = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert decl, name
    return [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")]


def test_header_and_binding_declare_the_entries():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    ints = {"L", "H", "W", "C", "radius", "tex", "span", "max_shift", "subpixel"}
    for name, args in ENTRIES.items():
        assert _declared(header, name) == args, name
        res, types = lib.SYMBOLS[name]
        assert res is lib.C.c_int and len(types) == len(args)
        assert [t is lib._i32 for t in types] == [a in ints for a in args] and all(t in (lib._i32, lib._fp) for t in types), name
    assert lib.ABI_VERSION == 9                          # symbols were only added
    assert all(callable(f) for f in (ops.weave_profiles, ops.weave_match, ops.weave_path, ops.weave_apply, video.stabilize,
                                     video.apply_shifts, video._check_stabilize_args, video._stabilize_device))
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "weave.hip"]
    assert len(unit) == 1 and unit[0][1] == "weave.o" and unit[0][1] in build.NOPK_OBJECTS and unit[0][2] == build.NOPK


def test_source_has_no_floating_point():
    src = open(os.path.join(ROOT, "e2fgvi_amd", "csrc", "weave.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double|half)\b", code) and not re.search(r"\d\.\d*f?\b", code)


def test_built_object_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "weave.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("object or llvm-objdump not present (python -m e2fgvi_amd.build)")
    # profiles, match, path and the apply kernel for one and for three bytes a pixel
    assert build.verify_no_scratch(obj="weave.o", marker="weave_", what="weave stabiliser") == 5
    assert build.verify_no_pk_u8() == len(build.UNITS)


def test_entries_refuse_bad_arguments_and_return_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    ptrs = dict(frames=base + 1, col=base + (1 << 16), row=base + (2 << 16), scene=base + (3 << 16), motion=base + (4 << 16),
                shift=base + (5 << 16), out=base + (8 << 16) + 3, mask=base + (12 << 16) + 1)
    good = dict(ptrs, L=4, H=40, W=30, C=3, radius=16, tex=2, span=4, max_shift=16, subpixel=1)
    words = {"col", "row", "scene", "motion", "shift"}
    ranges = dict(radius=(1, 32), tex=(0, 65535), span=(0, 16), max_shift=(1, 64), subpixel=(0, 1), C=(1, 3))
    for name, args in ENTRIES.items():
        who = name[len("e2fgvi_"):].encode()

        def rc(**kw):
            a = dict(good, **kw)
            return getattr(so, name)(*[a[k] for k in args[:-1]], None)

        mine = [k for k in args if k in ptrs]
        null = {k: None for k in mine}
        for k in mine:
            if k == "mask":                              # may be null
                continue
            assert rc(**{k: None}) == -1 and b"null" in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), (name, k)
            if k in words:
                assert rc(**{k: ptrs[k] + 2}) == -1 and b"aligned" in so.e2fgvi_last_error(), (name, k)
        for k in ("L", "H", "W"):
            if k in args:
                assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), (name, k)
        if name in ("e2fgvi_weave_profiles", "e2fgvi_weave_match"):
            assert rc(**dict(null, H=4097)) == -1 and b"4096" in so.e2fgvi_last_error() and rc(**dict(null, W=4097)) == -1
            assert rc(**dict(null, H=4096, W=4096)) == -1 and b"null" in so.e2fgvi_last_error()
        if name == "e2fgvi_weave_apply":
            assert rc(**dict(null, H=8193, W=8192)) == -1 and b"2^26" in so.e2fgvi_last_error()
            assert rc(**dict(null, H=0x7fffffff, W=0x7fffffff)) == -1
            assert rc(**dict(null, H=8192, W=8192)) == -1 and b"null" in so.e2fgvi_last_error()
            assert rc(C=2) == -1 and b"C must be" in so.e2fgvi_last_error()
        for k, (lo, hi) in ranges.items():
            if k in args:
                for v in (lo - 1, hi + 1, -(1 << 30), 1 << 30):
                    assert rc(**{k: v}) == -1 and k.encode() in so.e2fgvi_last_error() and who in so.e2fgvi_last_error(), (name, k, v)
                    assert rc(**dict(null, **{k: v, "L": 0})) == -1          # decided from the arguments alone, work or not
        # no work: no frame or no pixel -- nothing is launched and the pointers are not looked at
        for kw in (dict(L=0), dict(H=0), dict(W=0), dict(L=0, H=0, W=0)):
            if all(k in args for k in kw):              # a size the entry does not take would leave it with work
                assert rc(**kw) == 0 and rc(**dict(null, **kw)) == 0, (name, kw)
    # any overlap of out or mask with frames, or of mask with out, is refused -- out == frames too: a shifted read is not in order
    apply = lambda frames, out, mask=None: so.e2fgvi_weave_apply(frames, ptrs["shift"], out, mask, 4, 40, 30, 3, None)
    size = 3 * 4 * 40 * 30
    for frames, out in ((base, base), (base, base + 1), (base, base + size - 1), (base + size - 1, base), (base + 5, base)):
        assert apply(frames, out) == -1 and b"overlap" in so.e2fgvi_last_error(), (frames, out)
    far = base + (64 << 16)
    for mask in (base, base + size - 1, far, far + size - 1, far - size // 3 + 1):
        assert apply(base, far, mask) == -1 and b"overlap" in so.e2fgvi_last_error(), mask
    assert so.e2fgvi_abi_version() == 9
