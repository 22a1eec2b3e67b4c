"""The host side of the deflicker (video.deflicker) without a device: the numpy restatement holds its named cases and every mutated
restatement moves one of them, the guarantees that follow from the definition, the condition the defaults are judged on, every
refusal before the device, the header and the binding, and the C entries' refusals."""
import inspect
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import flicker_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"e2fgvi_flicker_hist": ["frames", "hist", "L", "H", "W", "stream"],
           "e2fgvi_flicker_curves": ["hist", "scene", "Q", "d", "L", "N", "span", "max_shift", "stream"],
           "e2fgvi_flicker_apply": ["frames", "d", "out", "L", "H", "W", "stream"]}
_PLANTED = {}


def _planted(seed):
    """(the planted tennis25 video, the restatement's dict at the defaults), computed once per seed"""
    if seed not in _PLANTED:
        p = C.plant(C.tennis25(ROOT), seed)
        p.setflags(write=False)
        _PLANTED[seed] = (p, C.deflicker_np(p, **C.DEFAULTS))
    return _PLANTED[seed]


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_deflicker_device", touched)


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name,flags", C.VARIANTS, ids=[v[0] for v in C.VARIANTS])
def test_every_variant_differs_from_the_definition_on_some_case(name, flags):
    seen = [n for n in C.NAMES if any(not np.array_equal(C.want(n)[k], C.want(n, **flags)[k]) for k in C.keys(n))]
    print(name, seen)
    assert seen


def test_cases_hold_what_they_are_named_for():
    assert len(C.VARIANTS) >= 9 and C.DEFAULTS == dict(span=4, max_shift=32) and C.KEYS == ("hist", "Q", "d", "out")
    framed = [n for n in C.NAMES if C.case(n)["frames"] is not None]
    assert [n for n in C.NAMES if n not in framed] == ["big_N"]
    for n in framed:
        c, w = C.case(n), C.want(n)
        L, H, W = c["L"], c["H"], c["W"]
        assert H * W <= 2000 or n in ("3x70x300", "flat_260")
        assert [(w[k].shape, w[k].dtype) for k in C.KEYS] == [((L, 256), np.int32), ((L, 32), np.int32), ((L, 256), np.int16),
                                                             ((L, H, W, 3), np.uint8)]
        assert (w["hist"].sum(axis=1) == H * W).all() and w["Q"].min() >= 0 and w["Q"].max() <= 4095
        assert (np.diff(w["Q"].astype(np.int64), axis=1) >= 0).all() and np.abs(w["d"]).max() <= c["max_shift"]
        # the nodes once more, from the sorted lumas and without a histogram
        assert np.array_equal(w["Q"], C.nodes_sorted_np(c["frames"]))
    assert {C.case(n)["W"] % 4 for n in framed} == {0, 1, 2, 3}
    c = C.case("5x7")
    assert (c["H"], c["W"]) == (5, 7) and c["H"] * c["W"] < 256 and (c["H"] * c["W"]) % 64
    c = C.case("3x70x300")
    assert (c["L"], c["H"], c["W"]) == (3, 70, 300) and c["H"] * c["W"] > 2 * 8192
    assert (C.case("w1_33x41")["H"] * C.case("w1_33x41")["W"] * 3) % 4 and C.case("w2_30x42")["H"] * C.case("w2_30x42")["W"] % 4 == 0
    # black beside white: bins 0 and 255 alone, the shifts clamp at max_shift and nothing of one frame is in the other's counts
    w = C.want("black_white")
    assert w["hist"][0].nonzero()[0].tolist() == [0] and w["hist"][1].nonzero()[0].tolist() == [255]
    assert w["d"][0, 0] == 32 and w["d"][1, 255] == -32 and (w["out"][0] == 32).all() and (w["out"][1] == 223).all()
    assert not np.array_equal(w["d"], C.want("black_white", no_clamp=True)["d"])
    # one bin past 16 bits; both flat frames meet in the middle
    w = C.want("flat_260")
    assert w["hist"].max() == 67600 > 65535 and (w["out"] == 110).all()
    w = C.want("two_level")
    assert all(len(set((q // 16).tolist())) == 2 for q in w["Q"]) and set(np.unique(C.case("two_level")["frames"]).tolist()) == {40, 200}
    # alone in its window: one frame, a scene of one frame at either end, span == 0
    assert not C.want("single")["d"].any() and C.want("single")["out"].tobytes() == C.case("single")["frames"].tobytes()
    c, w = C.case("cuts_ends"), C.want("cuts_ends")
    assert c["scenes"] == [1, c["L"] - 1] and not w["d"][[0, -1]].any() and w["d"][1:-1].any(axis=1).all()
    assert np.array_equal(w["out"][[0, -1]], c["frames"][[0, -1]])
    c = C.case("span_gt_L")
    assert c["span"] > c["L"] and C.want("span_gt_L")["d"].any()
    c = C.case("nondefault")
    assert all(c[k] != v for k, v in C.DEFAULTS.items()) and c["scenes"] and np.abs(C.want("nondefault")["d"]).max() == c["max_shift"]
    # shifts that leave [0, 255] at both ends
    c, w = C.case("clip"), C.want("clip")
    total = c["frames"].astype(np.int64) + np.stack([w["d"][t][C.luma(c["frames"][t])] for t in range(c["L"])])[..., None]
    assert (total < 0).any() and (total > 255).any()
    c = C.case("big_N")
    assert c["N"] == 1 << 26 and (c["hist"].sum(axis=1) == c["N"]).all() and c["hist"].max() == c["N"]
    assert C.want("big_N")["d"].any() and 2 * c["N"] * 32 * 128 > 1 << 32


# ------------------------------------------------------------------------------------------------ what follows from the definition
def test_luma_of_the_result_is_luma_plus_shift_where_nothing_clips():
    seen = 0
    for n in C.NAMES:
        c, w = C.case(n), C.want(n)
        if c["frames"] is None:
            continue
        f = c["frames"].astype(np.int64)
        Y = C.luma(f)
        shift = np.stack([w["d"][t].astype(np.int64)[Y[t]] for t in range(c["L"])])
        free = ((f + shift[..., None] >= 0) & (f + shift[..., None] <= 255)).all(axis=-1)
        assert np.array_equal(C.luma(w["out"])[free], (Y + shift)[free]), n
        # a byte at a level that is not moved is the caller's byte
        assert np.array_equal(w["out"][shift == 0], c["frames"][shift == 0]), n
        seen += int(free.sum())
    assert seen > 50000


def test_rolled_video_alone_frames_and_span_zero_come_back_identical():
    c, w = C.case("rolled"), C.want("rolled")
    assert (w["hist"] == w["hist"][0]).all() and not w["d"].any() and w["out"].tobytes() == c["frames"].tobytes()
    fr = C.case("w1_33x41")["frames"]
    # every frame a scene of its own: n == 1 everywhere
    w = C.deflicker_np(fr, scenes=[1, 2, 3])
    assert not w["d"].any() and w["out"].tobytes() == fr.tobytes()
    w = C.deflicker_np(fr, span=0)
    assert not w["d"].any() and w["out"].tobytes() == fr.tobytes()
    assert C.deflicker_np(fr)["d"].any()
    for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
        w = C.deflicker_np(np.zeros(shape, np.uint8))
        assert w["out"].shape == shape and w["d"].shape == (shape[0], 256) and not w["d"].any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_flicker_on_tennis25_is_taken_out(seed):
    """tests/golden/tennis25.npz (25 frames of 240 x 432, the camera pans) under flicker_cases.plant -- a gain of +-10 % and an
    offset of +-8 levels per frame -- through the restatement at the defaults: the roughness of the result (the mean |second
    difference| of the frames' mean luma along time) is at most 0.25 of the flickered video's, and level plus shift does not
    decrease with the level on any frame.  Measured: 0.105, 0.080, 0.089 for seeds 0, 1, 2; the clean video has 0.37, the
    flickered ones 13.3 ... 16.0."""
    planted, w = _planted(seed)
    before, after = C.roughness(planted), C.roughness(w["out"])
    print("seed", seed, "roughness", before, "->", after, "ratio", after / before)
    assert after <= 0.25 * before
    moved = np.arange(256)[None, :] + w["d"].astype(np.int64)
    assert (np.diff(moved, axis=1) >= 0).all()


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_deflicker_checks_before_the_device(no_device):
    f = np.zeros((5, 32, 40, 3), np.uint8)
    call = video.deflicker
    for bad in (f[0], f[..., :2], np.zeros((5, 32, 40), np.uint8), f.astype(np.float32), f.astype(np.int32), [[1, 2, 3]], None):
        with pytest.raises(ValueError, match="frames"):
            call(bad)
    for name, (lo, hi) in dict(span=(0, 8), max_shift=(1, 64)).items():
        for v in (lo - 1, hi + 1, lo + 0.5, True, False, None, str(lo), np.bool_(True)):
            with pytest.raises(ValueError, match=name):
                call(f, **{name: v})
    for scenes in ([0], [5], [2, 2], [3, 1], "auto", "", [True], 3):
        with pytest.raises(ValueError, match="scenes"):
            call(f, scenes=scenes)
    for v in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="return_curves"):
            call(f, return_curves=v)
    # more than 2^26 pixels a frame: from the shape alone (the array is never touched)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(1, 8193, 8192, 3), strides=(0, 0, 0, 0))
    with pytest.raises(ValueError, match="frames"):
        call(big)
    # good arguments pass the checks and reach the device layer, which the fixture has taken away; a CPU device is refused
    for kw in ({}, dict(scenes=[2]), dict(scenes=[]), dict(span=0), dict(span=8, max_shift=64), dict(span=np.int64(1), max_shift=1),
               dict(return_curves=True)):
        with pytest.raises(AssertionError, match="device work"):
            call(f, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(f, device="cpu", **kw)
    scene_of, span, max_shift = video._check_flicker_args(np.zeros((7, 32, 40, 3), np.uint8), [2, 5], 4, 32, False)
    assert scene_of.dtype == np.int32 and scene_of.tolist() == [0, 0, 1, 1, 1, 2, 2] == C.scene_of_np(7, [2, 5]).tolist()
    assert (span, max_shift) == (4, 32)


def test_defaults_and_signature():
    sig = inspect.signature(video.deflicker).parameters
    assert list(sig) == ["frames_u8", "scenes", "span", "max_shift", "return_curves", "device"]
    assert {k: sig[k].default for k in C.DEFAULTS} == C.DEFAULTS and sig["return_curves"].default is False
    assert sig["scenes"].default is None and sig["device"].default is None
    assert dict(span=video.FLICKER_SPAN, max_shift=video.FLICKER_MAX_SHIFT) == C.DEFAULTS
    assert (ops.FLICKER_SPAN_MAX, ops.FLICKER_SHIFT_MAX, ops.FLICKER_NODES) == (8, 64, 32) == (8, 64, C.NODES)
    assert list(inspect.signature(ops.flicker_apply).parameters) == ["frames", "d", "out"]
    # the driver is untouched: no new parameter, the record as it was
    assert len(video._Call._fields) == 21 and video._Call._fields[-1] == "defects"
    assert not any("flicker" in k for k in inspect.signature(video.inpaint_video).parameters)
    for text in (video.deflicker.__doc__,):
        for word in ("saturation", "highlights", "ends of a scene", "clean video", "varies over the frame", "``hole``"):
            assert word in text, word
    assert "deflicker" in video.detect_defects.__doc__ and "deflicker" in video.detect_line_scratches.__doc__


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
        ints = {"L", "H", "W", "N", "span", "max_shift"}
        assert [t is lib._i32 for t in types] == [a in ints for a in args] and all(t in (lib._i32, lib._fp) for t in types), name
    assert lib.ABI_VERSION == 9                          # symbols were only added
    assert all(callable(f) for f in (ops.flicker_hist, ops.flicker_curves, ops.flicker_apply, video.deflicker,
                                     video._check_flicker_args, video._deflicker_device))
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "flicker.hip"]
    assert len(unit) == 1 and unit[0][1] == "flicker.o" and unit[0][1] in build.NOPK_OBJECTS and unit[0][2] == build.NOPK


def test_source_has_no_floating_point():
    src = open(os.path.join(ROOT, "e2fgvi_amd", "csrc", "flicker.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double|half)\b", code) and not re.search(r"\d\.\d*f?\b", code)


def test_built_object_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "flicker.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("object or llvm-objdump not present (python -m e2fgvi_amd.build)")
    # the histogram, the curves and the apply kernel
    assert build.verify_no_scratch(obj="flicker.o", marker="flicker_", what="deflicker") == 3
    assert build.verify_no_pk_u8() == len(build.UNITS)


def test_entries_refuse_bad_arguments_and_return_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    ptrs = dict(frames=base + 1, hist=base + (1 << 16), scene=base + (2 << 16), Q=base + (3 << 16), d=base + (4 << 16) + 2,
                out=base + (8 << 16) + 3)
    good = dict(ptrs, L=4, H=40, W=30, N=1200, span=4, max_shift=32)
    words = {"hist", "scene", "Q"}
    ranges = dict(span=(0, 8), max_shift=(1, 64))
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
            if k == "d":
                assert rc(d=ptrs["d"] + 1) == -1 and b"aligned" in so.e2fgvi_last_error(), (name, k)
        for k in ("L", "H", "W", "N"):
            if k in args:
                assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error(), (name, k)
        if "H" in args:
            assert rc(**dict(null, H=8193, W=8192)) == -1 and b"2^26" in so.e2fgvi_last_error()
            assert rc(**dict(null, H=1, W=(1 << 26) + 1)) == -1 and rc(**dict(null, H=0x7fffffff, W=0x7fffffff)) == -1
            # 2^26 itself passes the size check: with null pointers the refusal is theirs
            assert rc(**dict(null, H=8192, W=8192)) == -1 and b"null" in so.e2fgvi_last_error()
        else:
            assert rc(**dict(null, N=(1 << 26) + 1)) == -1 and b"2^26" in so.e2fgvi_last_error()
            assert rc(**dict(null, N=1 << 26)) == -1 and b"null" in so.e2fgvi_last_error()
        for k, (lo, hi) in ranges.items():
            if k in args:
                for v in (lo - 1, hi + 1, -(1 << 30), 1 << 30):
                    assert rc(**{k: v}) == -1 and k.encode() in so.e2fgvi_last_error(), (name, k, v)
                    assert rc(**dict(null, **{k: v, "L": 0})) == -1          # decided from the arguments alone, work or not
        # no work: no frame or no pixel -- nothing is launched and the pointers are not looked at
        for kw in (dict(L=0), dict(H=0), dict(W=0), dict(N=0), dict(L=0, H=0, W=0, N=0)):
            if all(k in args for k in kw):              # a size the entry does not take would leave it with work
                assert rc(**kw) == 0 and rc(**dict(null, **kw)) == 0, (name, kw)
    # out may be frames itself; any other overlap of the two ranges of 3 L H W bytes is refused
    apply = lambda frames, out: so.e2fgvi_flicker_apply(frames, ptrs["d"], out, 4, 40, 30, None)
    size = 3 * 4 * 40 * 30
    for frames, out in ((base, base + 1), (base, base + size - 1), (base + size - 1, base), (base + 5, base)):
        assert apply(frames, out) == -1 and b"overlap" in so.e2fgvi_last_error(), (frames, out)
    assert so.e2fgvi_abi_version() == 9
