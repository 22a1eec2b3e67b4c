"""The temporal denoiser off the device: the numpy restatement of tests/denoise_cases.py and what follows from the definition, the
mutated restatements and the cases that catch them, the planted pan the definition is judged on, every refusal before the device,
the header and the binding, and the C entry's refusals from the arguments alone."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import denoise_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["frames", "fwd", "bwd", "scene", "out", "work", "work_bytes", "L", "H", "W", "strength", "search", "max_change", "stream"]
# PSNR in dB against the clean pan: (noise sigma, flows off by, h, s) -> the restatement's figure; the draft's table reads the same
# to 0.01 dB in every cell
PAN = {(5, 0.0, 8, 1): 39.23, (5, 0.0, 16, 1): 37.59, (5, 0.0, 8, 0): 37.74, (10, 0.0, 8, 1): 30.55, (10, 0.0, 16, 1): 34.43,
       (10, 0.0, 8, 0): 29.23, (5, 0.9, 8, 1): 38.98, (5, 0.9, 8, 0): 35.07}
NOISY = {5: 34.19, 10: 28.20}


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_denoise_device", touched)
    monkeypatch.setattr(video, "_device_flows", touched)


@pytest.fixture(scope="module")
def tennis():
    return C.tennis25(ROOT)


def _ref(c, setting, scenes=None):
    return C.reference(c["frames"], c["fwd"], c["bwd"], C.scene_of_np(c["L"], c["scenes"] if scenes is None else scenes), *setting)


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name,case,setting", C.CAUGHT_BY, ids=[v[0] for v in C.CAUGHT_BY])
def test_every_variant_differs_from_the_definition_on_its_case(name, case, setting):
    a, b = C.want(case, setting), C.want(case, setting, **{name: True})
    print(name, case, setting, int((a != b).sum()))
    assert a.shape == b.shape and a.dtype == np.uint8 and not np.array_equal(a, b)


def test_mutations_asked_for_are_all_there():
    assert len(C.CAUGHT_BY) == 12 and len({v[0] for v in C.CAUGHT_BY}) == 12 and all(v[1] in C.NAMES for v in C.CAUGHT_BY)
    assert all(v[2][0] in (1, 8, 64) and v[2][1] in (0, 1, 2) and v[2][2] in (0, 3, 255) for v in C.CAUGHT_BY)


def test_weight_scale_is_rounded_to_nearest():
    assert [C.weight_scale(h) for h in (1, 2, 8, 16, 64)] == [7282, 3641, 910, 455, 114]
    assert C.weight_scale(64, m_floor=True) == 113
    # the bounds the header states: SAD m < 2^25, Wsum <= 13056, acc < 2^22
    assert 9 * 255 * C.weight_scale(1) < 2 ** 25 and 256 + 2 * 25 * 256 == 13056 and 13056 * 255 + 13056 // 2 < 2 ** 22


def test_cases_hold_what_they_are_named_for():
    c = C.case("halves_17x23")
    assert np.all(c["fwd"] * 2 % 2 == 1) and np.all(c["bwd"] * 2 % 2 == 1)
    c = C.case("edges_17x23")
    qx = np.arange(23)[None, None, :] + c["fwd"][..., 0].astype(np.float64)
    assert (qx == 22).any() and (qx > 22).any() and (qx == -0.5).any() and (qx == 0).any() and ((qx > 22) & (qx < 22.001)).any()
    c = C.case("nonfinite_17x23")
    for bad in (np.isnan, np.isposinf, np.isneginf, lambda a: a == np.float32(1e30)):
        assert bad(c["fwd"]).any() and bad(c["bwd"]).any()
    c = C.case("corners_17x23")
    assert set(np.unique(np.arange(23)[None, None, :] + c["fwd"][..., 0])) == {0, 22}
    assert set(np.unique(C.case("extremes_17x23")["frames"])) == {0, 255}
    assert [C.case(n)["scenes"] for n in ("cut1_17x23", "cut4_17x23", "cuts_17x23")] == [[1], [4], [1, 2, 3, 4]]
    assert sorted({C.case(n)["L"] for n in C.NAMES}) == [1, 2, 3, 5]
    assert {(C.case(n)["H"], C.case(n)["W"]) for n in C.NAMES} >= set(C.SIZES)
    assert {s[0] for s in C.SETTINGS} == {1, 8, 64} and {s[1] for s in C.SETTINGS} == {0, 1, 2} and {s[2] for s in C.SETTINGS} == {0, 3, 255}


# ------------------------------------------------------------------------------------------------ what the definition guarantees
def test_no_change_allowed_or_no_neighbour_returns_the_input():
    for name in ("soft_33x70", "random_17x23", "extremes_17x23"):
        c = C.case(name)
        for h, s in ((8, 1), (64, 2)):
            assert np.array_equal(_ref(c, (h, s, 0)), c["frames"])
            assert np.array_equal(_ref(c, (h, s, 255), scenes=list(range(1, c["L"]))), c["frames"])
    assert np.array_equal(C.want("cuts_17x23", (64, 2, 255)), C.case("cuts_17x23")["frames"])
    assert np.array_equal(C.want("single_17x23", (64, 2, 255)), C.case("single_17x23")["frames"])


def test_no_byte_moves_by_more_than_the_limit():
    for name in ("soft_33x70", "five_33x70", "extremes_64x128"):
        c = C.case(name)
        free = _ref(c, (64, 2, 255)).astype(int)
        assert np.abs(free - c["frames"]).max() > 3
        for limit in (1, 3):
            out = _ref(c, (64, 2, limit)).astype(int)
            assert np.abs(out - c["frames"]).max() == limit
            assert np.array_equal(out, np.clip(free, c["frames"].astype(int) - limit, c["frames"].astype(int) + limit))


def test_scene_by_scene_is_the_call_with_scenes():
    c = C.case("cut2_17x23")
    for setting in ((8, 1, 255), (64, 2, 3)):
        whole = C.want("cut2_17x23", setting)
        parts = [C.reference(c["frames"][a:b], c["fwd"][a:b - 1], c["bwd"][a:b - 1], np.zeros(b - a, np.int32), *setting) for a, b in ((0, 2), (2, 5))]
        assert np.array_equal(whole, np.concatenate(parts))
        assert not np.array_equal(whole, _ref(c, setting, scenes=[]))           # and the cut is seen


def test_still_video_and_a_blotch_on_it_come_back_byte_for_byte(tennis):
    """a noiseless still video comes back as it is wherever the candidates that count carry the pixel's own bytes: at search == 0 on
    any picture, at every search on a flat one.  At search >= 1 a textured still picture does NOT come back byte for byte under
    this definition -- the candidates one pixel beside r match well in smooth texture and carry other bytes (13 740 of 36 000
    bytes change at search 1 on this clip, 18 589 at search 2): the price of the search, stated in DESIGN.md 3x.  The blotch of
    + 80 luma levels on one frame is neither spread nor removed at the default strength, on all frames."""
    zero = (np.zeros((4, 40, 60, 2), np.float32),) * 2
    scene = np.zeros(5, np.int32)
    for blotch in (False, True):
        clip = C.still_clip(tennis, blotch)
        if blotch:
            assert np.all(C.luma(clip)[2, 17:22, 30:35] - C.luma(clip)[1, 17:22, 30:35] == 80)
        assert np.array_equal(C.reference(clip, *zero, scene, 8, 0, 255), clip)
        changed = [int((C.reference(clip, *zero, scene, 8, s, 255) != clip).sum()) for s in (1, 2)]
        print("blotch" if blotch else "still", "bytes changed at search 1, 2:", changed)
        assert all(changed)
    flat = np.full((5, 40, 60, 3), 120, np.uint8)
    flat[2, 17:22, 30:35] += 80
    for s in (0, 1, 2):
        assert np.array_equal(C.reference(flat, *zero, scene, 8, s, 255), flat)
        assert np.array_equal(C.reference(np.full_like(flat, 77), *zero, scene, 64, s, 255), np.full_like(flat, 77))


def test_the_pan_gains_what_the_draft_measured(tennis):
    clean, fwd, bwd = C.pan_clip(tennis)
    scene = np.zeros(8, np.int32)
    got = {}
    for sigma, noisy in zip((5, 10), C.noisy_clips(clean)):
        assert abs(C.psnr(noisy, clean) - NOISY[sigma]) < 0.01
        for h, s in ((8, 1), (16, 1), (8, 0)):
            got[(sigma, 0.0, h, s)] = C.psnr(C.reference(noisy, fwd, bwd, scene, h, s, 255), clean)
        if sigma == 5:
            off = np.float32(0.9)                                               # fwd + 0.9 and bwd - 0.9 on both axes: bwd stays - fwd
            for s in (1, 0):
                got[(5, 0.9, 8, s)] = C.psnr(C.reference(noisy, fwd + off, bwd - off, scene, 8, s, 255), clean)
    for k in sorted(got):
        print("sigma %d, flows off by %.1f, h %d, s %d: %.3f dB (table %.2f)" % (k + (got[k], PAN[k])))
    assert got[(5, 0.0, 8, 1)] - C.psnr(C.noisy_clips(clean)[0], clean) >= 4
    assert got[(10, 0.0, 16, 1)] - C.psnr(C.noisy_clips(clean)[1], clean) >= 4
    assert got[(5, 0.9, 8, 1)] - got[(5, 0.9, 8, 0)] >= 2
    for k, v in PAN.items():
        assert abs(got[k] - v) < 0.01, (k, got[k], v)


# ------------------------------------------------------------------------------------------------ video.denoise in front of the device
def test_denoise_checks_before_the_device(no_device):
    c = C.case("soft_17x23")
    fr, flows = np.array(c["frames"]), (c["fwd"], c["bwd"])
    for bad in (fr.astype(np.float32), fr[0], fr[..., :2], None, [1, 2]):
        with pytest.raises(ValueError, match="frames"):
            video.denoise(None, bad, flows=flows)
    for name, lo, hi in (("strength", 1, 64), ("search", 0, 2), ("max_change", 0, 255)):
        for v in (lo - 1, hi + 1, True, False, 1.5, None, "1"):
            with pytest.raises(ValueError, match=name):
                video.denoise(None, fr, flows=flows, **{name: v})
    for scenes in ("auto", [0], [3], [2, 1], [1.5]):
        with pytest.raises(ValueError, match="scenes"):
            video.denoise(None, fr, flows=flows, scenes=scenes)
    for bad in ((c["fwd"],), (c["fwd"][:1], c["bwd"]), (c["fwd"], c["bwd"][:, :5]), 3, (c["fwd"][..., :1], c["bwd"][..., :1])):
        with pytest.raises(ValueError, match="flows"):
            video.denoise(None, fr, flows=bad)
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.denoise(None, fr)
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.denoise(object(), fr, max_change=0)                               # checked although nothing would run
    with pytest.raises(AssertionError, match="device work"):
        video.denoise(None, fr, flows=flows, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        video.denoise(None, fr, flows=flows, device="cpu")


def test_no_work_returns_the_input_without_the_device(no_device):
    c = C.case("soft_17x23")
    fr, flows = np.array(c["frames"]), (c["fwd"], c["bwd"])
    for kw in (dict(max_change=0), dict(scenes=[1, 2])):
        out = video.denoise(None, fr, flows=flows, **kw)
        assert isinstance(out, np.ndarray) and out is not fr and out.dtype == np.uint8 and np.array_equal(out, fr)
        t = torch.from_numpy(fr)
        on = video.denoise(None, t, flows=flows, **kw)
        assert isinstance(on, torch.Tensor) and on is not t and on.data_ptr() != t.data_ptr() and torch.equal(on, t)
    one = np.array(C.case("single_17x23")["frames"])
    assert np.array_equal(video.denoise(None, one, flows=(C.case("single_17x23")["fwd"], C.case("single_17x23")["bwd"])), one)
    for shape in ((0, 5, 7, 3), (3, 0, 7, 3), (3, 5, 0, 3)):
        e = np.zeros(shape, np.uint8)
        f = np.zeros((max(shape[0] - 1, 0),) + shape[1:3] + (2,), np.float32)
        out = video.denoise(None, e, flows=(f, f))
        assert out.shape == shape and out.dtype == np.uint8


def test_defaults_and_signature():
    sig = inspect.signature(video.denoise).parameters
    assert list(sig) == ["model", "frames_u8", "flows", "scenes", "strength", "search", "max_change", "device"]
    assert {k: sig[k].default for k in C.DEFAULTS} == C.DEFAULTS == dict(strength=8, search=1, max_change=255)
    assert sig["flows"].default is None and sig["scenes"].default is None and sig["device"].default is None
    assert list(inspect.signature(ops.denoise).parameters) == ["frames", "fwd", "bwd", "scene", "strength", "search", "max_change", "out"]
    assert (ops.DENOISE_STRENGTH_MAX, ops.DENOISE_SEARCH_MAX) == (64, 2)
    assert ops.denoise_work_bytes(3, 17, 23) == 3 * 25 * 36 and ops.denoise_work_bytes(2, 1, 1) == 2 * 9 * 16
    # the driver is untouched: no new parameter, the record as it was
    assert len(video._Call._fields) == 21 and video._Call._fields[-1] == "defects"
    assert not any("denoise" in k or "strength" in k for k in inspect.signature(video.inpaint_video).parameters)
    for word in ("about 1.6 times the sigma of the noise", "two neighbours only", "computed on the noisy frames", "has not been measured",
                 "no real noisy tape", "neither spread nor removed", "There is no CPU path"):
        assert word in " ".join(video.denoise.__doc__.split()), word


# ------------------------------------------------------------------------------------------------ header, binding, C entry
def test_header_and_binding_declare_the_entry():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    decl = re.search(r"int e2fgvi_denoise\(([^;]*)\);", header)
    assert decl and [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")] == ARGS
    res, types = lib.SYMBOLS["e2fgvi_denoise"]
    assert res is lib.C.c_int and len(types) == len(ARGS)
    want = [lib._i64 if a == "work_bytes" else lib._i32 if a in ("L", "H", "W", "strength", "search", "max_change") else lib._fp for a in ARGS]
    assert list(types) == want
    assert lib.ABI_VERSION == 9                          # a symbol was only added
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "denoise.hip"]
    assert len(unit) == 1 and unit[0][1] == "denoise.o" and unit[0][1] in build.NOPK_OBJECTS and unit[0][2] == build.NOPK
    # the row of the table build() walks: verify_no_scratch over the unit's kernels on every build
    assert ("denoise.o", "denoise_", "temporal denoiser", False) in build.KERNEL_CHECKS and "for obj, marker, what, _ in KERNEL_CHECKS" in inspect.getsource(build.build)
    for word in ("floor(q + 0.5)", "is dropped, not clamped", "256 + the sum of w(c)", "(Wsum >> 1)", "(65536 + (9 h) / 2) / (9 h)"):
        assert word in " ".join(header.split()), word


def test_built_object_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "denoise.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("object or llvm-objdump not present (python -m e2fgvi_amd.build)")
    # the luma pass and the filter at search 0, 1 and 2
    assert build.verify_no_scratch(obj="denoise.o", marker="denoise_", what="temporal denoiser") == 4
    isa = build.device_isa(obj)
    assert isa.count("v_sad_u8") >= 3 * (1 + 9 + 25) and "v_alignbyte_b32" in isa


def test_entry_refuses_bad_arguments_and_returns_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    base = 1 << 20
    L, H, W = 4, 40, 30
    need = ops.denoise_work_bytes(L, H, W)
    ptrs = dict(frames=base + 1, fwd=base + (1 << 16), bwd=base + (2 << 16), scene=base + (3 << 16), out=base + (4 << 16) + 3, work=base + (5 << 16))
    good = dict(ptrs, work_bytes=need, L=L, H=H, W=W, strength=8, search=1, max_change=255)

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_denoise(*[a[k] for k in ARGS[:-1]], None)

    def err():
        return so.e2fgvi_last_error()

    null = {k: None for k in ptrs}
    for k in ptrs:
        assert rc(**{k: None}) == -1 and b"null" in err() and b"denoise" in err(), k
    for k, off in (("fwd", 4), ("bwd", 4), ("scene", 2), ("work", 2)):
        assert rc(**{k: ptrs[k] + off}) == -1 and b"aligned" in err(), k
    assert rc(work_bytes=need - 1) == -1 and b"work must hold" in err() and str(need).encode() in err()
    for k in ("L", "H", "W"):
        assert rc(**{k: -1}) == -1 and b"negative" in err(), k
    assert rc(**dict(null, H=46341, W=46341)) == -1 and b"2^31" in err()
    assert rc(**dict(null, H=0x7fffffff, W=0x7fffffff)) == -1
    assert rc(**dict(null, H=46340, W=46340)) == -1 and b"null" in err()
    for k, (lo, hi) in dict(strength=(1, 64), search=(0, 2), max_change=(0, 255)).items():
        for v in (lo - 1, hi + 1, -(1 << 30), 1 << 30):
            assert rc(**{k: v}) == -1 and k.encode() in err() and b"denoise" in err(), (k, v)
            assert rc(**dict(null, **{k: v, "L": 0})) == -1          # decided from the arguments alone, work or not
    # no work: no frame or no pixel -- nothing is launched and the pointers are not looked at
    for kw in (dict(L=0), dict(H=0), dict(W=0), dict(L=0, H=0, W=0)):
        assert rc(**kw) == 0 and rc(**dict(null, **kw)) == 0, kw
    # any overlap of out with frames is refused, out == frames too; and so is a workspace that overlaps either
    size = 3 * L * H * W
    for frames, out in ((base, base), (base, base + 1), (base, base + size - 1), (base + size - 1, base), (base + 5, base)):
        assert rc(frames=frames, out=out) == -1 and b"overlap" in err(), (frames, out)
    assert rc(work=ptrs["out"] + 1) == -1 and b"overlap" in err()
    assert rc(work=(ptrs["frames"] + size - 1) & ~3) == -1 and b"overlap" in err()
    assert so.e2fgvi_abi_version() == 9
