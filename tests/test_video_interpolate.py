"""Frame interpolation off the device: the planners of video.retime and video.replace_frames against hand-written tables, every
refusal before the device, the numpy restatement of tests/interpolate_cases.py and what follows from the definition, the mutated
restatements and the cases that catch them, the planted clip the definition is judged on, the header and the binding, and the C
entry's refusals from the arguments alone."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from e2fgvi_amd import lib, ops, video
from tests import interpolate_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["frames", "fwd", "bwd", "jobs", "out", "source", "n", "L", "P", "H", "W", "iterations", "tolerance", "match", "stream"]
# PSNR in dB against the rendered truth of the planted clip: (flow noise in px, k, d, iterations) -> the restatement's figure
QUALITY = {(0.0, 1, 2, 3): 39.51, (0.0, 1, 4, 3): 40.99, (0.0, 3, 4, 3): 37.75, (0.3, 1, 2, 3): 39.50, (0.3, 1, 4, 3): 41.25,
           (0.3, 3, 4, 3): 37.52, (0.3, 1, 2, 0): 38.29, (0.3, 1, 4, 0): 39.51, (0.3, 3, 4, 0): 36.68}
FADE = {(1, 2): 34.41, (1, 4): 35.93, (3, 4): 35.75}
NEARER = {(1, 2): 29.80, (1, 4): 33.82, (3, 4): 33.57}


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("device work in the argument checks")
    monkeypatch.setattr(lib, "load", touched)
    monkeypatch.setattr(video, "_upload", touched)
    monkeypatch.setattr(video, "_interpolate_device", touched)
    monkeypatch.setattr(video, "_device_flows", touched)


# ------------------------------------------------------------------------------------------------ the planners
def test_plan_retime_tables():
    # 16 -> 24 fps: three frames for two; five source frames give (5 - 1) 3 // 2 + 1 = 7
    assert video.plan_retime(5, (3, 2)) == ([(0, 0, 0, 0, 3), (0, 1, 0, 2, 3), (1, 2, 1, 1, 3), (2, 2, 0, 0, 3), (2, 3, 2, 2, 3), (3, 4, 3, 1, 3),
                                             (4, 4, 0, 0, 3)], [0, 1, 2, 3])
    # doubling, as an integer and as a pair
    double = ([(0, 0, 0, 0, 2), (0, 1, 0, 1, 2), (1, 1, 0, 0, 2), (1, 2, 1, 1, 2), (2, 2, 0, 0, 2)], [0, 1])
    assert video.plan_retime(3, 2) == double == video.plan_retime(3, (2, 1))
    # every other frame: copies alone, no pair needs flows
    assert video.plan_retime(6, (1, 2)) == ([(0, 0, 0, 0, 1), (2, 2, 0, 0, 1), (4, 4, 0, 0, 1)], [])
    # slowing down by 3/4: times 0, 4/3, 8/3 of four frames
    assert video.plan_retime(4, (3, 4)) == ([(0, 0, 0, 0, 3), (1, 2, 0, 1, 3), (2, 3, 1, 2, 3)], [1, 2])
    # a cut at 2: the pair (1, 2) is not interpolated; at the half the later frame is the nearer one
    assert video.plan_retime(4, 2, [2]) == ([(0, 0, 0, 0, 2), (0, 1, 0, 1, 2), (1, 1, 0, 0, 2), (2, 2, 0, 0, 2), (2, 2, 0, 0, 2), (2, 3, 1, 1, 2),
                                             (3, 3, 0, 0, 2)], [0, 2])
    # thirds across a cut: 1/3 goes back, 2/3 goes on
    assert video.plan_retime(2, 3, [1]) == ([(0, 0, 0, 0, 3), (0, 0, 0, 0, 3), (1, 1, 0, 0, 3), (1, 1, 0, 0, 3)], [])
    assert video.plan_retime(1, 5) == ([(0, 0, 0, 0, 5)], []) and video.plan_retime(0, 2) == ([], [])
    assert video.plan_retime(3, 1) == ([(0, 0, 0, 0, 1), (1, 1, 0, 0, 1), (2, 2, 0, 0, 1)], [])
    rows, pairs = video.plan_retime(3, 64)
    assert len(rows) == 129 and rows[63] == (0, 1, 0, 63, 64) and rows[64] == (1, 1, 0, 0, 64) and pairs == [0, 1]
    for L in (2, 5, 9):                                                 # every row lies in the ranges the kernel asks for
        for rate in (2, 3, (3, 2), (64, 63), (5, 7), (1, 64)):
            cuts = [1] if L > 2 else []
            rows, pairs = video.plan_retime(L, rate, cuts)
            num, den = (rate, 1) if isinstance(rate, int) else rate
            assert len(rows) == (L - 1) * num // den + 1 and ops.interpolate_jobs_ok(rows, L, max(len(pairs), 1))
            assert all(ib == ia + 1 and pairs[fi] == ia and ib not in cuts and d == num for ia, ib, fi, k, d in rows if k)
            assert all(ia == ib and fi == 0 for ia, ib, fi, k, d in rows if not k)
    for bad in (0, -1, 65, 2.0, True, (3,), (0, 1), (1, 0), (65, 1), (2, 65), (2, 1.0), "2", None, (1, 2, 3)):
        with pytest.raises(ValueError, match="rate"):
            video.plan_retime(5, bad)
    with pytest.raises(ValueError, match="scenes"):
        video.plan_retime(5, 2, [5])
    with pytest.raises(ValueError, match="scenes"):
        video.plan_retime(5, 2, "auto")


def test_plan_replace_tables():
    assert video.plan_replace(5, [2]) == [(1, 3, [2])]
    assert video.plan_replace(6, [3, 1, 2]) == [(0, 4, [1, 2, 3])]
    assert video.plan_replace(8, [1, 3, 4, 6]) == [(0, 2, [1]), (2, 5, [3, 4]), (5, 7, [6])]
    # runs at the ends of the video and of a scene have one good neighbour
    assert video.plan_replace(5, [0, 4]) == [(None, 1, [0]), (3, None, [4])]
    assert video.plan_replace(8, [0, 2, 3, 7], [5]) == [(None, 1, [0]), (1, 4, [2, 3]), (6, None, [7])]
    assert video.plan_replace(8, [3, 4], [4]) == [(2, None, [3]), (None, 5, [4])]        # a run is cut at a cut
    assert video.plan_replace(5, []) == [] and video.plan_replace(0, []) == []
    assert video.plan_replace(66, list(range(1, 64))) == [(0, 64, list(range(1, 64)))]
    # the jobs: frame i of a run between a and c is the time (i - a) / (c - a); r counts the runs with two neighbours
    with pytest.raises(ValueError, match="no good frame"):
        video.plan_replace(8, [0, 2, 3, 5, 7], [7])                     # frame 7 is a scene of its own
    assert video._replace_jobs(8, video.plan_replace(8, [0, 2, 3, 5], [7])) == [
        (1, 1, 0, 0, 1), (1, 1, 0, 0, 1), (1, 4, 0, 1, 3), (1, 4, 0, 2, 3), (4, 4, 0, 0, 1), (4, 6, 1, 1, 2), (6, 6, 0, 0, 1), (7, 7, 0, 0, 1)]
    with pytest.raises(ValueError, match="no good frame"):
        video.plan_replace(3, [0, 1, 2])
    with pytest.raises(ValueError, match="no good frame"):
        video.plan_replace(5, [2, 3], [2, 4])
    with pytest.raises(ValueError, match="more than 63"):
        video.plan_replace(70, list(range(1, 65)))
    for bad in ([5], [-1], [1, 1], [1.5], [True], "12", 3, [None]):
        with pytest.raises(ValueError, match="bad"):
            video.plan_replace(5, bad)
    with pytest.raises(ValueError, match="scenes"):
        video.plan_replace(5, [1], [0])


# ------------------------------------------------------------------------------------------------ every refusal before the device
def test_argument_errors_name_the_argument(no_device):
    c = C.case("pan_17x23")
    fr = np.array(c["frames"])
    L, H, W = fr.shape[:3]
    at = np.arange(L - 1) % c["P"]
    flows = (c["fwd"][at], c["bwd"][at])
    one = [(c["fwd"][0], c["bwd"][0])]
    for kw, what in ((dict(frames_u8=fr[0]), "frames"), (dict(frames_u8=fr[..., :2]), "frames"), (dict(rate=0), "rate"), (dict(rate=(3, 0)), "rate"),
                     (dict(rate=2.5), "rate"), (dict(rate=(1, 2, 3)), "rate"), (dict(flows=(flows[0],)), "flows"), (dict(flows=(flows[0][:1], flows[1])), "flows"),
                     (dict(flows=(flows[0][:, :5], flows[1][:, :5])), "flows"), (dict(flows=3), "flows"), (dict(flows=(flows[0].astype(np.float64), flows[1])), "flows"),
                     (dict(flows=(torch.from_numpy(flows[0].copy()), torch.from_numpy(flows[1].copy()).double())), "flows"), (dict(scenes=[L]), "scenes"),
                     (dict(scenes="auto"), "scenes"), (dict(scenes=[2, 1]), "scenes"), (dict(iterations=9), "iterations"), (dict(iterations=-1), "iterations"),
                     (dict(iterations=True), "iterations"), (dict(iterations=1.5), "iterations"), (dict(tolerance=256), "tolerance"),
                     (dict(tolerance=-1), "tolerance"), (dict(match=766), "match"), (dict(match=-1), "match"), (dict(match=None), "match"),
                     (dict(return_source=1), "return_source")):
        with pytest.raises(ValueError, match=what):
            video.retime(**dict(dict(model=None, frames_u8=fr, rate=2, flows=flows), **kw))
    for kw, what in ((dict(frames_u8=fr[0]), "frames"), (dict(bad=[L]), "bad"), (dict(bad=[1, 1]), "bad"), (dict(bad="1"), "bad"), (dict(bad=[0.5]), "bad"),
                     (dict(bad=list(range(L))), "no good frame"), (dict(flows=[]), "flows"), (dict(flows=one + one), "flows"), (dict(flows=flows), "flows"),
                     (dict(flows=[(c["fwd"][0][:5], c["bwd"][0][:5])]), "flows"), (dict(flows=[(c["fwd"][0],)]), "flows"), (dict(flows=7), "flows"),
                     (dict(flows=[(c["fwd"][0].astype(np.float64), c["bwd"][0])]), "flows"),
                     (dict(flows=[(torch.from_numpy(c["fwd"][0].copy()), torch.from_numpy(c["bwd"][0].copy()).half())]), "flows"),
                     (dict(scenes=[0]), "scenes"), (dict(scenes="auto"), "scenes"), (dict(iterations=9), "iterations"), (dict(tolerance=256), "tolerance"),
                     (dict(tolerance=False), "tolerance"), (dict(match=766), "match"), (dict(return_source=None), "return_source")):
        with pytest.raises(ValueError, match=what):
            video.replace_frames(**dict(dict(model=None, frames_u8=fr, bad=[1], flows=one), **kw))
    # without flows the model must be the generator, where flows are needed at all
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.retime(None, fr)
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.replace_frames(object(), fr, [1])
    # the checks passed: the next thing is the device
    with pytest.raises(AssertionError, match="device work"):
        video.retime(None, fr, 2, flows=flows, device="cuda")
    with pytest.raises(AssertionError, match="device work"):
        video.replace_frames(None, fr, [1], flows=one, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        video.retime(None, fr, 2, flows=flows, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        video.replace_frames(None, fr, [0], device="cpu")              # a copy of frame 1: no flows, and still no CPU path


def test_no_work_returns_a_copy_without_the_device(no_device):
    fr = np.array(C.case("pan_17x23")["frames"])
    for call in (lambda x, **kw: video.retime(None, x, 1, **kw), lambda x, **kw: video.retime(None, x, (5, 5), **kw),
                 lambda x, **kw: video.replace_frames(None, x, [], **kw), lambda x, **kw: video.retime(None, x[:1], 3, **kw),
                 lambda x, **kw: video.retime(None, x[:0], 3, **kw), lambda x, **kw: video.replace_frames(None, x[:0], [], **kw)):
        out = call(fr)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and not np.shares_memory(out, fr) and np.array_equal(out, fr[:len(out)])
        out, src = call(fr, return_source=True)
        assert src.dtype == np.uint8 and src.shape == out.shape[:3] and (src == 5).all()
        # a tensor on the host comes back as the working path returns it (video._like_input): a numpy array, and a copy
        t = torch.from_numpy(fr)
        on = call(t)
        assert isinstance(on, np.ndarray) and on.dtype == np.uint8 and not np.shares_memory(on, fr) and np.array_equal(on, fr[:len(on)])


def test_defaults_and_signatures():
    sig = inspect.signature(video.retime).parameters
    assert list(sig) == ["model", "frames_u8", "rate", "flows", "scenes", "iterations", "tolerance", "match", "return_source", "device"]
    assert sig["rate"].default == 2 and sig["return_source"].default is False
    rep = inspect.signature(video.replace_frames).parameters
    assert list(rep) == ["model", "frames_u8", "bad", "flows", "scenes", "iterations", "tolerance", "match", "return_source", "device"]
    for s in (sig, rep):
        assert {k: s[k].default for k in C.DEFAULTS} == C.DEFAULTS == dict(iterations=3, tolerance=8, match=96)
        assert s["flows"].default is None and s["scenes"].default is None and s["device"].default is None
    assert list(inspect.signature(ops.interpolate).parameters) == ["frames", "fwd", "bwd", "jobs", "iterations", "tolerance", "match", "out", "source"]
    assert (ops.INTERPOLATE_ITERATIONS_MAX, ops.INTERPOLATE_TOLERANCE_MAX, ops.INTERPOLATE_MATCH_MAX, ops.INTERPOLATE_D_MAX) == (8, 255, 765, 64)
    assert ops.INTERPOLATE_PIXELS_MAX == ops.DENOISE_PIXELS_MAX
    assert list(inspect.signature(video.plan_retime).parameters) == ["length", "rate", "scenes"]
    assert list(inspect.signature(video.plan_replace).parameters) == ["length", "bad", "scenes"]
    for fn in (video.retime, video.replace_frames):
        doc = " ".join(fn.__doc__.split())
        for word in ("source == 0 is the mask to hand to inpaint_video", "thin", "damaged neighbours", "There is no CPU path"):
            assert word in doc, (fn.__name__, word)
    assert "bridged linearly in time" in " ".join(video.replace_frames.__doc__.split())
    assert "ranslation" in video.retime.__doc__


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name,case,setting", C.CAUGHT_BY, ids=[v[0] for v in C.CAUGHT_BY])
def test_every_variant_differs_from_the_definition_on_its_case(name, case, setting):
    a, b = C.want(case, setting), C.want(case, setting, **{name: True})
    print(name, case, setting, "out", int((a[0] != b[0]).sum()), "source", int((a[1] != b[1]).sum()))
    assert a[0].shape == b[0].shape and a[0].dtype == np.uint8 and not np.array_equal(a[0], b[0])     # a byte of a frame, not a code alone


def test_mutations_asked_for_are_all_there():
    assert [v[0] for v in C.CAUGHT_BY] == ["tap_no_half", "later_strict", "tie_strict", "sum_first", "inside_after_trunc", "corner_unguarded",
                                           "round_d", "landing_strict"]
    assert all(v[1] in C.NAMES for v in C.CAUGHT_BY)
    assert all(v[2][0] in (0, 1, 3, 8) and v[2][1] in (0, 8, 255) and v[2][2] in (0, 96, 765) for v in C.CAUGHT_BY)


def test_every_source_code_occurs():
    """over the named cases at the default setting every code 0 to 5 is on at least 32 pixels -- a test that compares nothing
    shows nothing"""
    total = np.zeros(6, np.int64)
    for name in C.NAMES:
        out, src = C.want(name)
        assert src.max() <= 5
        total += np.bincount(src.ravel(), minlength=6)
    print("pixels per source code", total.tolist())
    assert (total >= 32).all()


def test_cases_hold_what_they_are_named_for():
    assert {(C.case(n)["H"], C.case(n)["W"]) for n in C.NAMES} >= {(1, 1), (1, 9), (7, 1), (17, 23), (33, 70), (64, 128)}
    assert {C.case(n)["L"] for n in C.NAMES} == {2, 3, 4, 5}
    seen = {(int(k), int(d)) for n in C.NAMES for _, _, _, k, d in C.case(n)["jobs"]}
    assert seen >= {(0, 1), (1, 1), (1, 2), (1, 3), (2, 3), (1, 64), (63, 64), (32, 64)}
    rows = np.concatenate([C.case(n)["jobs"] for n in C.NAMES])
    assert (rows[:, 0] == rows[:, 1]).any() and (np.abs(rows[:, 0] - rows[:, 1]) == 1).any() and (np.abs(rows[:, 0] - rows[:, 1]) > 1).any()
    assert (rows[:, 0] > rows[:, 1]).any() and rows[:, 2].max() >= 3
    assert {s[0] for s in C.SETTINGS} == {0, 1, 3, 8} and {s[1] for s in C.SETTINGS} == {0, 8, 255} and {s[2] for s in C.SETTINGS} == {0, 96, 765}
    assert C.SETTINGS[0] == C.DEFAULT
    assert not C.case("zero_17x23")["fwd"].any() and not C.case("zero_64x128")["bwd"].any()
    assert np.all(C.case("halves_17x23")["fwd"] * 2 % 2 == 1) and np.all(C.case("sixteenths_17x23")["fwd"] * 16 % 2 == 1)
    assert np.all(C.case("minus_half_17x23")["fwd"] == -0.5)
    c = C.case("edges_17x23")                                            # the starts at the fraction 1/2
    qx = np.arange(23)[None, None, :] - 0.5 * c["fwd"][..., 0].astype(np.float64)
    assert (qx == 22).any() and ((qx > 22) & (qx < 22.001)).any() and (qx == -0.5).any() and (qx == 0).any() and (qx == 22.5).any()
    c = C.case("ends_17x23")                                             # the far ends q + h at the fraction 1/2
    ex = np.arange(23)[None, None, :] + 0.5 * c["fwd"][..., 0].astype(np.float64)
    assert (ex == 22).any() and (ex > 22).any()
    c = C.case("nonfinite_17x23")
    for bad in (np.isnan, np.isposinf, np.isneginf, lambda a: a == np.float32(1e30)):
        assert bad(c["fwd"]).any() and bad(c["bwd"]).any()
    assert (np.abs(C.case("huge_17x23")["fwd"]) >= 1e30).any() and np.isfinite(C.case("huge_17x23")["fwd"]).all()
    assert np.abs(C.case("random_33x70")["fwd"]).max() > 5.9 and np.abs(C.case("random_33x70")["fwd"]).max() <= 6
    assert set(np.unique(C.case("extremes_17x23")["frames"])) == {0, 255} == set(np.unique(C.case("extremes_64x128")["frames"]))
    f = C.case("occlusion_33x70")["fwd"][0]
    assert {tuple(v) for v in f.reshape(-1, 2).tolist()} == {(0.0, 0.0), (6.0, -1.0)}     # a step edge
    assert np.isnan(C.case("lastcol_7x9")["fwd"][:, :, 0]).all() and np.isfinite(C.case("lastcol_7x9")["fwd"][:, :, 1:]).all()


# ------------------------------------------------------------------------------------------------ what follows from the definition
def test_the_ends_are_copies():
    for name in ("random_33x70", "nonfinite_17x23", "pan_1x1"):
        c = C.case(name)
        for setting in ((3, 8, 96), (0, 0, 0), (8, 255, 765)):
            rows = [(ia, ib, fi, k, d) for ia in range(c["L"]) for ib in range(c["L"]) for fi in range(c["P"]) for k, d in ((0, 1), (1, 1), (0, 64), (64, 64), (0, 7), (7, 7))]
            out, src = C.reference(c["frames"], c["fwd"], c["bwd"], rows, *setting)
            assert (src == 5).all()
            assert all(np.array_equal(out[j], c["frames"][ia if k == 0 else ib]) for j, (ia, ib, fi, k, d) in enumerate(rows))


def test_a_still_picture_comes_back_at_every_fraction_and_setting():
    """A == B under zero flows: both sides start and end on p, match at cost 0, and the mix of a byte with itself is the byte"""
    fr = C.noise(1, 17, 23, 90)
    zero = np.zeros((1, 17, 23, 2), np.float32)
    rows = [(0, 0, 0, k, d) for k, d in C.FRACTIONS + ((5, 7), (31, 64), (33, 64), (1, 5))]
    for it in (0, 1, 3, 8):
        for tol in (0, 8, 255):
            for match in (0, 96, 765):
                out, src = C.reference(fr, zero, zero, rows, it, tol, match)
                assert all(np.array_equal(o, fr[0]) for o in out), (it, tol, match)
                assert all((s == (5 if k in (0, d) else 1)).all() for s, (_, _, _, k, d) in zip(src, rows))


def test_an_integer_translation_is_reproduced_in_the_interior():
    """B is A moved by v = (4, -2) and the flows say so exactly: at 1/2 the new frame is A moved by (2, -1), byte for byte, wherever both
    ends lie in the frames; at 1/4 it is A moved by (1, -0.5): the rounded mean of two rows, on the 1/16 px grid"""
    big = C.noise(1, 40, 48, 91)[0]
    A, B = big[4:36, 4:44], big[6:38, 0:40]                             # B(p) = A(p - v)
    assert np.array_equal(B[:-2, 4:], A[2:, :-4])
    H, W = A.shape[:2]
    fwd, bwd = C.const_flows(1, H, W, 4.0, -2.0)
    fr = np.stack([A, B])
    for setting in ((3, 8, 96), (0, 0, 0), (8, 255, 765)):
        out, src = C.reference(fr, fwd, bwd, [(0, 1, 0, 1, 2), (0, 1, 0, 1, 4), (1, 0, 0, 1, 2)], *setting)
        # the picture at 1/2: out(p) = A(p - (2, -1)) = big[y + 4 + 1, x + 4 - 2]
        want = big[5:37, 2:42]
        inner = (slice(2, H - 2), slice(4, W - 4))
        assert np.array_equal(out[0][inner], want[inner]) and (src[0][inner] == 1).all(), setting
        # at 1/4: out(p) = A(x - 1, y + 0.5) = (A(x - 1, y) + A(x - 1, y + 1) + 1) >> 1
        a, b = big[4:36, 3:43].astype(int), big[5:37, 3:43].astype(int)
        assert np.array_equal(out[1][inner], ((a + b + 1) >> 1)[inner]) and (src[1][inner] == 1).all(), setting
        # from B to A along the same pair read backwards (fwd = B -> A is bwd): the same middle frame
        back, _ = C.reference(fr, bwd, fwd, [(1, 0, 0, 1, 2)], *setting)
        assert np.array_equal(back[0][inner], want[inner])
    assert not np.array_equal(out[0], C.crossfade(A, B, 1, 2))


# ------------------------------------------------------------------------------------------------ the planted clip
def test_quality_on_the_planted_clip():
    """PSNR against the rendered truth on the planted clip (a 96 x 160 textured pan of (1.5, 0.5) px a frame, a 24 x 30 object moving
    by (7, -1) px a frame, exact flows), the restatement's figures in dB -- the device equals the restatement byte for byte, so
    they are the device's:
        fraction   interpolated   cross-fade   nearer frame
        1/2        39.51          34.41        29.80
        1/4        40.99          35.93        33.82
        3/4        37.75          35.75        33.57
    With Gaussian flow noise of 0.3 px: 39.50, 41.25 and 37.52 at three fixed-point iterations, 38.29, 39.51 and 36.68
    without them.  At 3/4 the object has covered background that the earlier frame still shows: the earlier side lands there alone and
    paints it (source 3), which costs 3 dB against 1/4 -- the definition's one-ended rule cannot tell covered from uncovered, DESIGN.md
    3y.  0.01 to 0.02 % of the pixels fall back to the cross-fade with exact flows, 0.14 to 0.16 % with the noise.  Each
    figure must reach the one written here less 0.5 dB and beat both the cross-fade and the nearer frame."""
    pairs = {noise: C.clip_pair(noise) for noise in (0.0, 0.3)}
    for (noise, k, d, it), figure in QUALITY.items():
        fr, fwd, bwd = pairs[noise]
        truth, _ = C.clip_frame(k / d)
        out, src = C.reference(fr, fwd, bwd, [(0, 1, 0, k, d)], it, 8, 96)
        got = C.psnr(out[0], truth)
        fade, nearer = C.psnr(C.crossfade(fr[0], fr[1], k, d), truth), C.psnr(fr[0] if 2 * k <= d else fr[1], truth)
        print("noise %.1f at %d/%d, %d iterations: %.2f dB, cross-fade %.2f, nearer %.2f, source 0 on %.3f %%"
              % (noise, k, d, it, got, fade, nearer, 100.0 * (src == 0).mean()))
        assert got >= figure - 0.5 and got > fade and got > nearer, (noise, k, d, it, got)
        assert abs(fade - FADE[(k, d)]) < 0.01 and abs(nearer - NEARER[(k, d)]) < 0.01
        assert (src == 0).mean() < 0.01
    # the iterations earn their keep under flow noise
    assert QUALITY[(0.3, 1, 2, 3)] - QUALITY[(0.3, 1, 2, 0)] > 1.0


# ------------------------------------------------------------------------------------------------ header, binding, C entry
def test_header_and_binding_declare_the_entry():
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    decl = re.search(r"int e2fgvi_interpolate\(([^;]*)\);", header)
    assert decl and [a.split()[-1].lstrip("*") for a in " ".join(decl.group(1).split()).split(",")] == ARGS
    res, types = lib.SYMBOLS["e2fgvi_interpolate"]
    assert res is lib.C.c_int and list(types) == [lib._fp] * 6 + [lib._i32] * 8 + [lib._fp]
    assert lib.ABI_VERSION == 9                          # a symbol was only added
    from e2fgvi_amd import build
    unit = [u for u in build.UNITS if u[0] == "interpolate.hip"]
    assert len(unit) == 1 and unit[0][1] == "interpolate.o" and unit[0][1] in build.NOPK_OBJECTS
    assert unit[0][2] == build.NOPK + ["-ffp-contract=off"]
    src = inspect.getsource(build.build)
    # the row of the table build() walks: verify_no_scratch over the unit's kernel and, its last field, verify_no_fma64 over the object
    assert ("interpolate.o", "interpolate_", "frame interpolation", True) in build.KERNEL_CHECKS
    assert "verify_no_scratch(objdir, obj, marker, what)" in src and "verify_no_fma64(objdir, obj)" in src and src.count("in KERNEL_CHECKS") == 2
    for word in ("the product first", "(double)(tol tol) / 256.0", "floor(q 16 + 0.5)", "cost_A <= cost_B", "2 k <= d", "writes nothing"):
        assert word in " ".join(header.split()), word


def test_built_object_rounds_every_operation_and_has_no_scratch():
    from e2fgvi_amd import build
    obj = os.path.join(build.CSRC, "build", "interpolate.o")
    if not (os.path.exists(obj) and os.path.exists(build.OBJDUMP)):
        pytest.skip("object or llvm-objdump not present (python -m e2fgvi_amd.build)")
    assert build.verify_no_scratch(obj="interpolate.o", marker="interpolate_", what="frame interpolation") == 1
    assert build.verify_no_fma64(obj="interpolate.o") > 0
    assert "v_div_scale_f64" not in build.device_isa(obj)               # k / d comes from the table


def test_entry_refuses_bad_arguments_and_returns_on_no_work():
    """E2FGVI_EINVAL from the arguments alone and 0 without a launch when there is no work: no device is needed (the addresses are
    never read)"""
    so = lib.load()                                      # a tree that is not built fails here (HipLibraryMissing); it does not skip
    base = 1 << 20
    n, L, P, H, W = 3, 4, 2, 40, 30
    ptrs = dict(frames=base + 1, fwd=base + (1 << 16), bwd=base + (2 << 16), jobs=base + (3 << 16), out=base + (4 << 16) + 3, source=base + (6 << 16) + 1)
    good = dict(ptrs, n=n, L=L, P=P, H=H, W=W, iterations=3, tolerance=8, match=96)

    def rc(**kw):
        a = dict(good, **kw)
        return so.e2fgvi_interpolate(*[a[k] for k in ARGS[:-1]], None)

    def err():
        return so.e2fgvi_last_error()

    null = {k: None for k in ptrs}
    for k in ("frames", "fwd", "bwd", "jobs", "out"):                    # source may be null
        assert rc(**{k: None}) == -1 and b"null" in err() and b"interpolate" in err(), k
    for k, off in (("fwd", 4), ("bwd", 4), ("jobs", 2)):
        assert rc(**{k: ptrs[k] + off}) == -1 and b"aligned" in err(), k
    for k in ("n", "L", "P", "H", "W"):
        assert rc(**{k: -1}) == -1 and b"negative" in err(), k
    assert rc(**dict(null, H=46341, W=46341)) == -1 and b"2^31" in err()
    assert rc(**dict(null, H=46340, W=46340)) == -1 and b"null" in err()
    for k, (lo, hi) in dict(iterations=(0, 8), tolerance=(0, 255), match=(0, 765)).items():
        for v in (lo - 1, hi + 1, -(1 << 30), 1 << 30):
            assert rc(**{k: v}) == -1 and k.encode() in err() and b"interpolate" in err(), (k, v)
            assert rc(**dict(null, **{k: v, "n": 0})) == -1          # decided from the arguments alone, work or not
    # no work: no job or no pixel -- nothing is launched and the pointers are not looked at
    for kw in (dict(n=0), dict(H=0), dict(W=0), dict(n=0, H=0, W=0)):
        assert rc(**kw) == 0 and rc(**dict(null, **kw)) == 0, kw
    # any overlap of out with frames is refused, out == frames too
    fsize, osize = 3 * L * H * W, 3 * n * H * W
    for frames, out in ((base, base), (base, base + 1), (base, base + fsize - 1), (base + osize - 1, base), (base + 5, base)):
        assert rc(frames=frames, out=out) == -1 and b"overlap" in err(), (frames, out)
    # and so is a source that lies on anything that is read or on out, and an out that lies on the flows or the jobs
    ssize, hsize = n * H * W, 8 * P * H * W
    for k, size in (("frames", fsize), ("fwd", hsize), ("bwd", hsize), ("jobs", 20 * n), ("out", osize)):
        for at in (ptrs[k], ptrs[k] + size - 1, ptrs[k] - ssize + 1):
            assert rc(source=at) == -1 and b"source must not overlap" in err(), (k, at)
    for k, size in (("fwd", hsize), ("bwd", hsize), ("jobs", 20 * n)):
        assert rc(out=ptrs[k] + size - 1) == -1 and b"out must not overlap" in err(), k
    assert so.e2fgvi_abi_version() == 9
