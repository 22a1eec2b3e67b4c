"""The host side of the colour restoration (video.restore_color, video.apply_color) without a device: the numpy restatement holds
its named cases and every mutated restatement moves one of them, the guarantees that follow from the definition, the planted fades
the tool is judged on, every refusal before the device, the header and the binding, and the C entries' refusals."""
import inspect
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import color_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"e2fgvi_color_hist": ["frames", "hist", "L", "H", "W", "stream"],
           "e2fgvi_color_nodes": ["hist", "starts", "ids", "Q", "L", "G", "M", "lo", "hi", "stream"],
           "e2fgvi_color_lut": ["Q", "T", "mode", "lut", "G", "lo_t", "hi_t", "min_range", "max_gain", "strength", "stream"],
           "e2fgvi_color_apply": ["frames", "lut", "group", "out", "L", "H", "W", "G", "stream"]}
VIDEOS = tuple(n for n in C.NAMES if C.case(n)["kind"] == "video")
_PLANTED = {}


def _planted(fade):
    """(the clean tennis25 video, the faded one), computed once per fade"""
    if fade not in _PLANTED:
        clean = C.tennis25(ROOT)
        faded = C.plant_fade(clean, **C.FADES[fade])
        for a in (clean, faded):
            a.setflags(write=False)
        _PLANTED[fade] = (clean, faded)
    return _PLANTED[fade]


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_restore_color_device", touched)


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name,flags", C.VARIANTS, ids=[v[0] for v in C.VARIANTS])
def test_every_variant_differs_from_the_definition_on_some_case(name, flags):
    seen = [n for n in C.NAMES if n != "slabs_65540"
            and any(not np.array_equal(C.want(n)[k], C.want(n, **flags)[k]) for k in C.keys(n))]
    print(name, seen)
    assert seen


def test_the_two_node_derivations_agree():
    seen = 0
    for n in VIDEOS:
        c, w = C.case(n), C.want(n)
        starts, ids = w["starts"].tolist(), w["ids"]
        for src, st, ii, key in ((c["frames"], starts, ids, "Q"),) + (
                ((c["graded"], w["gstarts"].tolist(), w["gids"], "T"),) if c["graded"] is not None else ()):
            for g in range(len(st) - 1)[:3]:
                mine = ii[st[g]:st[g + 1]]
                if not len(mine):
                    continue                             # a scene without a key has no graded frame
                for ch in range(3):
                    assert np.array_equal(w[key][g, ch], C.nodes_sorted_np(src[mine][..., ch], c["clip"])), (n, key, g, ch)
                    seen += 1
    assert seen > 60


def test_cases_hold_what_they_are_named_for():
    assert len(C.VARIANTS) == 11 and C.DEFAULTS == dict(clip=(5, 5), target=None, min_range=32, max_gain=768, strength=256)
    for n in VIDEOS:
        c, w = C.case(n), C.want(n)
        L, H, W = c["frames"].shape[:3]
        S = len(c["scenes"] or []) + 1
        assert H * W <= 2000 or n in ("3x70x300", "flat_260")
        assert [(w[k].shape, w[k].dtype) for k in ("hist", "Q", "lut", "out")] == [
            ((L, 3, 256), np.int32), ((S, 3, 34), np.int32), ((S, 3, 256), np.uint8), ((L, H, W, 3), np.uint8)]
        assert (w["hist"].sum(axis=2) == H * W).all() and w["Q"].min() >= 0 and w["Q"].max() <= 4095
        assert (np.diff(w["Q"][..., :32].astype(np.int64), axis=-1) >= 0).all() and (w["Q"][..., 32] <= w["Q"][..., 33]).all()
    assert {C.case(n)["frames"].shape[2] % 4 for n in VIDEOS} == {0, 1, 2, 3}
    f = C.case("5x7")["frames"]
    assert f.shape[1:3] == (5, 7) and f.shape[1] * f.shape[2] < 256
    f = C.case("3x70x300")["frames"]
    assert f.shape[:3] == (3, 70, 300) and 70 * 300 > 2 * 8192
    assert (33 * 41 * 3) % 4 and C.case("w1_33x41")["frames"].shape[1:3] == (33, 41) and (30 * 42) % 4 == 0
    # one bin per channel past 16 bits; no usable channel: the identity
    w = C.want("flat_260")
    assert w["hist"].max() == 67600 > 65535 and w["out"].tobytes() == C.case("flat_260")["frames"].tobytes()
    w = C.want("black_white")
    assert set(np.unique(w["hist"][0].nonzero()[1]).tolist()) == {0} and set(np.unique(w["hist"][1].nonzero()[1]).tolist()) == {255}
    # tied nodes in Q and in T, in match mode
    w = C.want("two_level")
    assert (w["mode"] == C.MATCH).all() and all((np.diff(w[k][g, ch, :32]) == 0).any() and len(set((w[k][g, ch, :32] // 16).tolist())) == 2 for k in "QT" for g in range(2) for ch in range(3))
    c = C.case("lut_ties")
    assert (np.diff(c["Q"][0, 0, :32]) == 0).sum() >= 10 and (np.diff(c["T"][0, 0, :32]) == 0).sum() >= 10 and (c["Q"][0, 0, :32] % 16 == 0).sum() >= 10
    assert c["T"].min() < 0 and c["T"].max() > 4095 and c["mode"].tolist() == [2, 1, 0, 7]
    w = C.want("lut_ties")["lut"]
    assert np.array_equal(w[2], w[3]) and np.array_equal(w[2, 0], np.arange(256))
    # an unusable channel beside usable ones keeps its bytes
    c, w = C.case("one_flat_channel"), C.want("one_flat_channel")
    assert w["Q"][0, 1, 33] - w["Q"][0, 1, 32] < 16 * 32 and np.array_equal(w["out"][..., 1], c["frames"][..., 1])
    assert not np.array_equal(w["out"][..., 0], c["frames"][..., 0])          # onto the range of the blue channel, the widest
    # clipping at both ends
    c, w = C.case("saturated"), C.want("saturated")
    assert c["target"] == (0, 255) and (c["frames"] == 0).any() and (c["frames"] == 255).any()
    assert all((w["lut"][0, ch, :30] == 0).all() and (w["lut"][0, ch, -30:] == 255).all() for ch in range(3))
    # the gain limit binds on the narrow channel: its slope is max_gain / 256 = 3
    c, w = C.case("narrow_gain"), C.want("narrow_gain")
    den = int(w["Q"][0, 2, 33] - w["Q"][0, 2, 32])
    assert c["min_range"] == 16 and 16 * 16 <= den <= 16 * 21 and int(w["lut"][0, 2, 135]) - int(w["lut"][0, 2, 125]) == 30
    assert not np.array_equal(w["lut"], C.want("narrow_gain", no_gain_limit=True)["lut"])
    assert C.case("clip_0")["clip"] == (0, 0) and C.case("clip_250")["clip"] == (250, 250)
    f, w = C.case("clip_0")["frames"], C.want("clip_0")
    assert all(w["Q"][0, ch, 32] // 16 == f[..., ch].min() and w["Q"][0, ch, 33] // 16 == f[..., ch].max() for ch in range(3))
    assert C.case("strength_128")["strength"] == 128 and C.case("target_16_235")["target"] == (16, 235)
    w = C.want("target_16_235")
    assert all(abs(int(w["lut"][0, ch, int(w["Q"][0, ch, 32]) // 16]) - 16) <= 2 for ch in range(3))
    # two keys pooled, a scene without a key under both values of ``otherwise``, one key
    for n, mode in (("keys_9", [2, 1, 2]), ("keys_9_keep", [2, 0, 2])):
        c, w = C.case(n), C.want(n)
        assert c["frames"].shape[:3] == (9, 20, 23) and c["graded"].shape == (3, 11, 13, 3) and c["scenes"] == [4, 7] and c["keys"] == [1, 2, 8]
        assert w["mode"].tolist() == mode and w["group"].tolist() == [0] * 4 + [1] * 3 + [2] * 2
        assert w["starts"].tolist() == [0, 2, 5, 6] and w["ids"].tolist() == [1, 2, 4, 5, 6, 8]
        assert w["gstarts"].tolist() == [0, 2, 2, 3] and w["gids"].tolist() == [0, 1, 2]
    assert np.array_equal(C.want("keys_9_keep")["out"][4:7], C.case("keys_9_keep")["frames"][4:7])
    assert not np.array_equal(C.want("keys_9")["out"][4:7], C.case("keys_9")["frames"][4:7])
    c, w = C.case("graded_n2"), C.want("graded_n2")
    assert c["keys"] is None and len(c["graded"]) == 2 and (w["mode"] == C.MATCH).all() and np.array_equal(w["T"][0], w["T"][1])
    c = C.case("big_N")
    assert c["hist"].shape == (40, 3, 256) and (c["hist"].sum(axis=2) == 1 << 26).all() and (c["hist"][..., 250] % 2 == 1).all() and ((c["hist"] > 0).sum(axis=2) == 3).all()
    assert 40 * (1 << 26) > 1 << 31 and C.want("big_N")["Q"].shape == (3, 3, 34) and (C.want("big_N")["Q"][:, :, 33] > 16 * 249).all()
    c, w = C.case("bad_ids"), C.want("bad_ids")
    L = len(c["hist"])
    assert {-1, L} <= set(c["ids"].tolist()) and (np.diff(c["starts"]) < 0).any() and c["starts"].max() > len(c["ids"]) and c["starts"].min() < 0
    assert np.array_equal(w["Q"][0], C.nodes_np(c["hist"], [0, 2], [0, 1])[0])          # 0, -1, 1, L: frames 0 and 1
    assert not w["Q"][1].any() and w["Q"][2].any() and not w["Q"][4].any() and not w["Q"][5].any()
    c, w = C.case("group_out"), C.want("group_out")
    G = len(c["lut"])
    assert {-1, G} <= set(c["group"].tolist()) and np.array_equal(w["out"][[1, 3, 4]], c["frames"][[1, 3, 4]])
    assert not np.array_equal(w["out"][0], c["frames"][0])
    c, w = C.case("slabs_65540"), C.want("slabs_65540")
    assert c["frames"].shape == (65540, 2, 3, 3) and c["scenes"] == [65537] and c["keys"] == [5, 65538] and w["hist"].nbytes > 200e6
    assert w["ids"].tolist() == [5, 65538] and (w["mode"] == C.MATCH).all()


# ------------------------------------------------------------------------------------------------ what follows from the definition
def test_every_table_is_monotone_and_a_byte():
    seen = 0
    for n in C.NAMES:
        w = C.want(n)
        if "lut" in w:
            assert w["lut"].dtype == np.uint8 and (np.diff(w["lut"].astype(np.int64), axis=-1) >= 0).all(), n
            seen += w["lut"].shape[0]
    assert seen >= 30
    rng = np.random.RandomState(7)
    G = 200
    Q = np.zeros((G, 3, C.NQ), np.int32)
    T = np.zeros((G, 3, C.NQ), np.int32)
    for a in (Q, T):
        a[..., :32] = np.sort(rng.randint(0, 4096, (G, 3, 32)) // rng.choice([1, 16, 256], (G, 3, 1)) * rng.choice([1, 16], (G, 3, 1)), axis=-1).clip(0, 4095)
        a[..., 32:] = np.sort(rng.randint(0, 4096, (G, 3, 2)), axis=-1)
    mode = rng.randint(0, 3, G).astype(np.int32)
    for kw in (dict(), dict(target=(16, 235), min_range=1, max_gain=4096), dict(strength=77, max_gain=256), dict(target=(0, 255), min_range=255)):
        lut = C.lut_np(Q, mode, T, **kw)
        assert (np.diff(lut.astype(np.int64), axis=-1) >= 0).all(), kw
        assert np.array_equal(lut[mode == 0], np.tile(np.arange(256, dtype=np.uint8), (int((mode == 0).sum()), 3, 1)))


def test_mode_keep_and_strength_zero_are_the_identity():
    ident = np.arange(256, dtype=np.uint8)
    for n in VIDEOS[:4] + ("two_level", "keys_9"):
        c = C.case(n)
        w = C.restore_np(c["frames"], **dict(C.settings(c), strength=0))
        assert (w["lut"] == ident).all() and w["out"].tobytes() == c["frames"].tobytes(), n
        assert (C.lut_np(C.want(n)["Q"], np.zeros(len(C.want(n)["Q"]), np.int32), C.want(n)["T"]) == ident).all()
    for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
        w = C.restore_np(np.zeros(shape, np.uint8), scenes=[1] if shape[0] else None)
        assert w["out"].shape == shape and (w["lut"] == ident).all()


def test_planted_fades_on_tennis25_are_restored():
    """tests/golden/tennis25.npz (25 frames of 240 x 432) under color_cases.plant_fade through the restatement.  Measured, in dB
    against the clean video: the affine fade 19.87 faded, 32.98 after automatic levels, 45.66 (worst frame 44.77) with frame 0 and
    its clean version as the only key, 44.36 with frame 12; the fade with gamma 18.44, 27.88, 45.40 (44.48), 44.29.  The floors
    are those figures less about 2 dB."""
    for fade in ("affine", "gamma"):
        clean, faded = _planted(fade)
        key = C.restore_np(faded, graded=clean[:1], keys=[0])
        levels = C.restore_np(faded)
        print(fade, "faded", C.psnr(faded, clean), "levels", C.psnr(levels["out"], clean), "key 0", C.psnr(key["out"], clean),
              "worst frame", min(C.psnr_frames(key["out"], clean)))
        assert C.psnr(key["out"], clean) >= 42
        assert (np.diff(key["lut"].astype(np.int64), axis=-1) >= 0).all() and (np.diff(levels["lut"].astype(np.int64), axis=-1) >= 0).all()
        if fade == "affine":
            assert C.psnr(levels["out"], clean) >= 31


def test_clean_clip_through_automatic_levels_changes_no_byte_by_more_than_8():
    """measured: 41.68 dB against itself, at most 8 levels, 9.4 % of the bytes by more than 3"""
    clean, _ = _planted("affine")
    out = C.restore_np(clean)["out"]
    d = np.abs(out.astype(np.int64) - clean.astype(np.int64))
    print("clean", C.psnr(out, clean), "max", int(d.max()), "more than 3", float((d > 3).mean()))
    assert d.max() <= 8


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_restore_color_checks_before_the_device(no_device):
    f = np.zeros((5, 32, 40, 3), np.uint8)
    g = np.zeros((2, 8, 9, 3), np.uint8)
    call = video.restore_color
    for bad in (f[0], f[..., :2], np.zeros((5, 32, 40), np.uint8), f.astype(np.float32), f.astype(np.int32), [[1, 2, 3]], None):
        with pytest.raises(ValueError, match="frames"):
            call(bad)
    for name, (lo, hi) in dict(min_range=(1, 255), max_gain=(256, 4096), strength=(0, 256)).items():
        for v in (lo - 1, hi + 1, lo + 0.5, True, False, None, str(lo), np.bool_(True)):
            with pytest.raises(ValueError, match=name):
                call(f, **{name: v})
    for clip in ((-1, 5), (5, 251), (5,), (5, 5, 5), 5, None, (True, 5), (2.5, 5), "55"):
        with pytest.raises(ValueError, match="clip"):
            call(f, clip=clip)
    for target in ((-1, 200), (0, 256), (100, 100), (200, 100), (16,), 16, (True, 200), "ab", (-1, -1)):
        with pytest.raises(ValueError, match="target"):
            call(f, target=target)
    for scenes in ([0], [5], [2, 2], [3, 1], "auto", "", [True], 3):
        with pytest.raises(ValueError, match="scenes"):
            call(f, scenes=scenes)
    for v in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="return_curves"):
            call(f, return_curves=v)
    for v in ("Levels", "", None, 1, "match"):
        with pytest.raises(ValueError, match="otherwise"):
            call(f, otherwise=v)
    for bad in (g[0], g[..., :2], g.astype(np.float32), g[:0], np.zeros((2, 0, 9, 3), np.uint8), [[1, 2, 3]]):
        with pytest.raises(ValueError, match="graded"):
            call(f, graded=bad)
    for keys in ([0], [0, 1, 2], [1, 1], [2, 1], [0, 5], [-1, 2], [], [True, 2], [0.0, 1.0], 3):
        with pytest.raises(ValueError, match="keys"):
            call(f, graded=g, keys=keys)
    with pytest.raises(ValueError, match="keys"):
        call(f, keys=[1])
    # more than 2^26 pixels a frame: from the shape alone (the array is never touched)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(1, 8193, 8192, 3), strides=(0, 0, 0, 0))
    with pytest.raises(ValueError, match="frames"):
        call(big)
    with pytest.raises(ValueError, match="graded"):
        call(f, graded=big)
    # good arguments pass the checks and reach the device layer, which the fixture has taken away; a CPU device is refused
    for kw in ({}, dict(scenes=[2]), dict(scenes=[]), dict(strength=0), dict(clip=[0, 250], target=[0, 255]), dict(graded=g),
               dict(graded=g, keys=[0, 4], otherwise="keep"), dict(graded=g, keys=(np.int64(1), 3), scenes=[2]),
               dict(min_range=np.int64(1), max_gain=4096, target=(16, 235)), dict(return_curves=True)):
        with pytest.raises(AssertionError, match="device work"):
            call(f, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(f, device="cpu", **kw)
    # the plan is the restatement's
    c = C.case("keys_9")
    for name in ("keys_9", "keys_9_keep", "graded_n2", "3x70x300", "w1_33x41"):
        c, w = C.case(name), C.want(name)
        plan = video._check_restore_color_args(c["frames"], c["scenes"], c["graded"], c["keys"], c["otherwise"], c["clip"], c["target"],
                                               c["min_range"], c["max_gain"], c["strength"], False)
        assert plan["scene_of"].dtype == np.int32 and np.array_equal(plan["scene_of"], w["group"]) and plan["S"] == len(w["mode"])
        assert all(plan[k].dtype == np.int32 for k in ("starts", "ids", "mode")) and np.array_equal(plan["mode"], w["mode"])
        assert np.array_equal(plan["starts"], w["starts"]) and np.array_equal(plan["ids"], w["ids"])
        if c["keys"] is not None:
            assert np.array_equal(plan["gstarts"], w["gstarts"]) and np.array_equal(plan["gids"], w["gids"])
        elif c["graded"] is not None:                   # one pool of all graded frames, for every scene
            assert plan["gstarts"].tolist() == [0, len(c["graded"])] and plan["gids"].tolist() == list(range(len(c["graded"])))
        else:
            assert plan["gstarts"] is None and plan["gids"] is None


def test_apply_color_checks_before_the_device(no_device):
    f = np.zeros((5, 32, 40, 3), np.uint8)
    luts = np.zeros((2, 3, 256), np.uint8)
    for bad in (f[0], f.astype(np.float32), None):
        with pytest.raises(ValueError, match="frames"):
            video.apply_color(bad, luts, scenes=[2])
    for bad in (luts[:1], luts[:, :2], luts[..., :255], luts.astype(np.int32), None, [[1]]):
        with pytest.raises(ValueError, match="luts"):
            video.apply_color(f, bad, scenes=[2])
    with pytest.raises(ValueError, match="luts"):
        video.apply_color(f, luts)
    for scenes in ([0], "auto", [3, 1]):
        with pytest.raises(ValueError, match="scenes"):
            video.apply_color(f, luts, scenes=scenes)
    with pytest.raises(AssertionError, match="device work"):
        video.apply_color(f, luts, scenes=[2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        video.apply_color(f, luts, scenes=[2], device="cpu")


def test_defaults_and_signature():
    sig = inspect.signature(video.restore_color).parameters
    assert list(sig) == ["frames_u8", "scenes", "graded", "keys", "otherwise", "clip", "target", "min_range", "max_gain", "strength",
                         "return_curves", "device"]
    assert {k: sig[k].default for k in C.DEFAULTS} == C.DEFAULTS and sig["return_curves"].default is False
    assert all(sig[k].default is None for k in ("scenes", "graded", "keys", "device")) and sig["otherwise"].default == "levels"
    assert list(inspect.signature(video.apply_color).parameters) == ["frames_u8", "luts", "scenes", "device"]
    assert (ops.COLOR_NODES, ops.COLOR_CLIP_MAX, ops.COLOR_GAIN_MIN, ops.COLOR_GAIN_MAX) == (C.NQ, 250, 256, 4096)
    assert (ops.COLOR_KEEP, ops.COLOR_LEVELS, ops.COLOR_MATCH) == (C.KEEP, C.LEVELS, C.MATCH)
    assert list(inspect.signature(ops.color_hist).parameters) == ["frames", "out"]
    assert list(inspect.signature(ops.color_nodes).parameters) == ["hist", "starts", "ids", "clip"]
    assert list(inspect.signature(ops.color_lut).parameters) == ["Q", "mode", "T", "target", "min_range", "max_gain", "strength"]
    assert list(inspect.signature(ops.color_apply).parameters) == ["frames", "lut", "group", "out"]
    d = inspect.signature(ops.color_lut).parameters
    assert (inspect.signature(ops.color_nodes).parameters["clip"].default, d["min_range"].default, d["max_gain"].default,
            d["strength"].default, d["T"].default, d["target"].default) == ((5, 5), 32, 768, 256, None, None)
    # the driver is untouched: no new parameter, the record as it was
    assert len(video._Call._fields) == 21 and video._Call._fields[-1] == "defects"
    assert not any("color" in k for k in inspect.signature(video.inpaint_video).parameters)
    for word in ("one grade per scene", "no drift", "clean video", "41.68 dB", "after deflicker", "detect_defects"):
        assert word in video.restore_color.__doc__, word


# ------------------------------------------------------------------------------------------------ header, binding, C entries
def _declared(header, name):
    decl = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert decl, name
    return [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")]


def test_header_and_binding_declare_the_entries():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    ptrs = {"frames", "hist", "starts", "ids", "Q", "T", "mode", "lut", "group", "out", "stream"}
    for name, args in ENTRIES.items():
        decl = _declared(header, name)
        assert decl == args, name
        res, types = lib.SYMBOLS[name]
        assert res is lib.C.c_int and len(types) == len(args)
        assert [t is lib._fp for t in types] == [a in ptrs for a in args] and all(t in (lib._i32, lib._fp) for t in types), name
    assert lib.ABI_VERSION == 9                          # symbols were only added
    assert all(callable(f) for f in (ops.color_hist, ops.color_nodes, ops.color_lut, ops.color_apply, video.restore_color,
                                     video.apply_color, video._check_restore_color_args, video._restore_color_device))
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "color.hip"]
    assert len(unit) == 1 and unit[0][1] == "color.o" and unit[0][1] in build.NOPK_OBJECTS and unit[0][2] == build.NOPK


def test_source_has_no_floating_point():
    code = {}
    for name in ("color.hip", "frame_bytes.h"):
        src = open(os.path.join(ROOT, "e2fgvi_amd", "csrc", name)).read()
        code[name] = "\n".join(line.split("//")[0] for line in src.splitlines())
        assert not re.search(r"\b(float|double|half)\b", code[name]) and not re.search(r"\d\.\d*f?\b", code[name]), name
    # the group of four pixels comes from the header of the byte-frame kernels, and nothing of the deflicker's is borrowed
    assert '#include "frame_bytes.h"' in code["color.hip"] and "flicker_common.h" not in code["color.hip"]


def test_built_object_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "color.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("object or llvm-objdump not present (python -m e2fgvi_amd.build)")
    # the histogram, the nodes, the table and the apply kernel
    assert build.verify_no_scratch(obj="color.o", marker="color_", what="colour restoration") == 4


def test_entries_refuse_bad_arguments_and_return_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    names = ("frames", "hist", "starts", "ids", "Q", "T", "mode", "lut", "group", "out")
    ptrs = {k: base + ((i + 1) << 16) for i, k in enumerate(names)}
    ptrs.update(frames=ptrs["frames"] + 1, lut=ptrs["lut"] + 3, out=ptrs["out"] + (1 << 20) + 3)
    good = dict(ptrs, L=4, H=40, W=30, G=3, M=7, lo=5, hi=5, lo_t=-1, hi_t=-1, min_range=32, max_gain=768, strength=256)
    words = {"hist", "starts", "ids", "Q", "T", "mode", "group"}
    ranges = dict(lo=(0, 250), hi=(0, 250), min_range=(1, 255), max_gain=(256, 4096), strength=(0, 256))
    no_work = {"e2fgvi_color_hist": (dict(L=0), dict(H=0), dict(W=0), dict(L=0, H=0, W=0)), "e2fgvi_color_nodes": (dict(G=0),),
               "e2fgvi_color_lut": (dict(G=0),), "e2fgvi_color_apply": (dict(L=0), dict(H=0), dict(W=0), dict(L=0, G=0))}
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
        for k in ("L", "H", "W", "G", "M"):
            if k in args:
                assert rc(**{k: -1}) == -1 and b"negative" in so.e2fgvi_last_error(), (name, k)
        if "H" in args:
            assert rc(**dict(null, H=8193, W=8192)) == -1 and b"2^26" in so.e2fgvi_last_error()
            assert rc(**dict(null, H=1, W=(1 << 26) + 1)) == -1 and rc(**dict(null, H=0x7fffffff, W=0x7fffffff)) == -1
            # 2^26 itself passes the size check: with null pointers the refusal is theirs
            assert rc(**dict(null, H=8192, W=8192)) == -1 and b"null" in so.e2fgvi_last_error()
        for k, (lo, hi) in ranges.items():
            if k in args:
                for v in (lo - 1, hi + 1, -(1 << 30), 1 << 30):
                    assert rc(**{k: v}) == -1 and k.encode() in so.e2fgvi_last_error(), (name, k, v)
                    assert rc(**dict(null, **{k: v, "G": 0})) == -1          # decided from the arguments alone, work or not
        if "lo_t" in args:
            for lo_t, hi_t in ((-1, 200), (0, -1), (-2, -2), (100, 100), (200, 100), (0, 256), (-1, 0)):
                assert rc(lo_t=lo_t, hi_t=hi_t) == -1 and b"target" in so.e2fgvi_last_error(), (lo_t, hi_t)
                assert rc(**dict(null, lo_t=lo_t, hi_t=hi_t, G=0)) == -1
            for lo_t, hi_t in ((0, 255), (0, 1), (16, 235)):
                assert rc(**dict(null, lo_t=lo_t, hi_t=hi_t)) == -1 and b"null" in so.e2fgvi_last_error()
        # no work: nothing is launched and the pointers are not looked at
        for kw in no_work[name]:
            assert rc(**kw) == 0 and rc(**dict(null, **kw)) == 0, (name, kw)
    # out may be frames itself; any other overlap of the two ranges of 3 L H W bytes is refused
    apply = lambda frames, out: so.e2fgvi_color_apply(frames, ptrs["lut"], ptrs["group"], out, 4, 40, 30, 3, None)
    size = 3 * 4 * 40 * 30
    for frames, out in ((base, base + 1), (base, base + size - 1), (base + size - 1, base), (base + 5, base)):
        assert apply(frames, out) == -1 and b"overlap" in so.e2fgvi_last_error(), (frames, out)
    assert so.e2fgvi_abi_version() == 9
