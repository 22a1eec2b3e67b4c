"""The 4:2:0 pixel formats without a device: the Q14 coefficients, the numpy restatement of tests/yuv_cases.py against anchors and
against the float64 formula over every (Y, U, V) triple, the properties of the paste form, and every refusal of the new arguments,
raised from the arguments and the shapes alone."""
import os
import re

import numpy as np
import pytest

from e2fgvi_amd import lib, ops, video
from tests import yuv_cases as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = {
    ("bt601", False): ((19077, 26149, 6419, 13320, 33050), (4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170)),
    ("bt601", True): ((16384, 22970, 5638, 11700, 29032), (4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332)),
    ("bt709", False): ((19077, 29372, 3494, 8731, 34610), (2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660)),
    ("bt709", True): ((16384, 25802, 3069, 7670, 30402), (3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751)),
}


def _coef(matrix, full):
    dec, enc = video.yuv_coefficients(matrix, full)
    return dec, enc, 0 if full else 16


def test_coefficients_are_the_table():
    for (matrix, full), (dec, enc) in TABLE.items():
        got = video.yuv_coefficients(matrix, full)
        assert got == (dec, enc), (matrix, full, got)
        assert all(type(v) is int for t in got for v in t)
        assert sum(enc[:3]) == (16384 if full else 14071)
        assert sum(enc[3:6]) == 0 and sum(enc[6:]) == 0
    with pytest.raises(ValueError, match="matrix"):
        video.yuv_coefficients("bt2020", False)


def _one(rgb=None, yuv=None, matrix="bt601", full=False, chroma="nearest"):
    dec, enc, yo = _coef(matrix, full)
    if rgb is not None:
        x = Y.encode_np(np.broadcast_to(np.array(rgb, np.uint8), (1, 2, 2, 3)), "i420", enc, yo)
        return tuple(int(v) for v in (x[0, 0, 0], x[0, 2, 0], x[0, 2, 1]))
    y, u, v = yuv
    x = Y.join(np.full((1, 2, 2), y, np.uint8), np.full((1, 1, 1), u, np.uint8), np.full((1, 1, 1), v, np.uint8), "i420")
    return tuple(int(c) for c in Y.decode_np(x, "i420", chroma, dec, yo)[0, 1, 1])


def test_anchors():
    for matrix in ("bt601", "bt709"):
        for chroma in Y.CHROMAS:
            assert _one(yuv=(16, 128, 128), matrix=matrix, chroma=chroma) == (0, 0, 0)
            assert _one(yuv=(235, 128, 128), matrix=matrix, chroma=chroma) == (255, 255, 255)
        assert _one(rgb=(0, 0, 0), matrix=matrix) == (16, 128, 128)
        assert _one(rgb=(255, 255, 255), matrix=matrix) == (235, 128, 128)
    assert _one(rgb=(255, 0, 0), matrix="bt601") == (81, 90, 240)
    assert _one(rgb=(255, 0, 0), matrix="bt709") == (63, 102, 240)


@pytest.mark.parametrize("matrix,full", sorted(TABLE), ids=str)
def test_integer_decode_is_within_one_level_of_the_float_formula_on_every_triple(matrix, full):
    dec, _, yo = _coef(matrix, full)
    x = Y.all_triples_yuv("nv12")
    planes = Y.split(x, "nv12")
    seen = (planes[0].astype(np.int64) << 16) | (np.repeat(np.repeat(planes[1], 2, 1), 2, 2).astype(np.int64) << 8) \
        | np.repeat(np.repeat(planes[2], 2, 1), 2, 2)
    assert np.unique(seen).size == 1 << 24                                  # the frame does hold every triple
    got = Y.decode_np(x, "nv12", "nearest", dec, yo).astype(np.int16)
    want = Y.decode_float(x, "nv12", matrix, full).astype(np.int16)
    assert int(np.abs(got - want).max()) <= 1


def test_left_siting_keeps_a_constant_chroma_plane():
    for layout in Y.LAYOUTS:
        for shape in ((1, 2, 2), (2, 6, 10), (1, 34, 66)):
            x = Y.frames("constant", *shape, layout)
            _, U, V = Y.split(x, layout)
            assert np.array_equal(Y._left(U), np.repeat(np.repeat(U, 2, 1), 2, 2))
            dec, _, yo = _coef("bt709", False)
            assert np.array_equal(Y.decode_np(x, layout, "left", dec, yo), Y.decode_np(x, layout, "nearest", dec, yo))


def test_a_constant_colour_round_trips_within_one_level():
    """encode o decode of a constant (Y, U, V) frame that decodes inside the RGB cube (no channel clipped to 0 or 255) gives the
    frame back within one level, with both chroma modes: the three RGB roundings move Y by at most 0.5 (yr + yg + yb) / 2^14 <= 0.5
    and U, V by at most 0.5 (|ur| + |ug| + |ub|) / 2^14 <= 0.5, and the encoder's own rounding adds 0.5.
    The other way round an RGB colour does NOT come back within one level in general, and no converter's does: a limited-range
    chroma step is cbu / 2^14 = 2.1 levels of B, so half a step of U, half a step of Y (0.58) and the last rounding bound the error
    by 0.5 (cbu + cy) / 2^14 + 0.5 < 2.2, that is two levels; that bound is checked as well."""
    rng = np.random.RandomState(5)
    yuv = rng.randint(0, 256, (4000, 3)).astype(np.uint8)
    rgbc = np.concatenate([rng.randint(0, 256, (500, 3)), [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]]])
    rgb = np.broadcast_to(rgbc.astype(np.uint8)[:, None, None, :], (len(rgbc), 4, 6, 3))
    for (matrix, full) in TABLE:
        dec, enc, yo = _coef(matrix, full)
        assert 0.5 * (dec[4] + dec[0]) / 16384 + 0.5 < 2.2
        for layout in Y.LAYOUTS:
            const = lambda c, h, w: np.broadcast_to(c[:, None, None], (len(c), h, w))
            x = Y.join(const(yuv[:, 0], 4, 6), const(yuv[:, 1], 2, 3), const(yuv[:, 2], 2, 3), layout)
            inside = np.all((Y.decode_np(x, layout, "nearest", dec, yo) > 0) & (Y.decode_np(x, layout, "nearest", dec, yo) < 255),
                            axis=(1, 2, 3))
            assert inside.sum() > 400
            for chroma in Y.CHROMAS:
                back = Y.encode_np(Y.decode_np(x, layout, chroma, dec, yo), layout, enc, yo).astype(np.int16)
                assert int(np.abs(back - x)[inside].max()) <= 1, (matrix, full, layout, chroma)
                there = Y.decode_np(Y.encode_np(rgb, layout, enc, yo), layout, chroma, dec, yo).astype(np.int16)
                assert int(np.abs(there - rgb).max()) <= 2, (matrix, full, layout, chroma)


def test_paste_returns_like_for_its_own_decoding():
    dec, enc, yo = _coef("bt709", False)
    for layout in Y.LAYOUTS:
        for chroma in Y.CHROMAS:
            for kind in Y.CONTENTS:
                like = Y.frames(kind, 3, 6, 10, layout)
                like_rgb = Y.decode_np(like, layout, chroma, dec, yo)
                assert np.array_equal(Y.encode_paste_np(like_rgb.copy(), like_rgb, like, layout, enc, yo), like)


def test_paste_changes_only_the_bytes_of_changed_pixels_and_their_blocks():
    dec, enc, yo = _coef("bt601", True)
    L, H, W = 2, 8, 12
    for layout in Y.LAYOUTS:
        like = Y.frames("random", L, H, W, layout)
        like_rgb = Y.decode_np(like, layout, "left", dec, yo)
        rgb = like_rgb.copy()
        changed = [(0, 0, 0), (0, 3, 5), (1, 7, 11), (1, 4, 4)]
        for l, y, x in changed:
            rgb[l, y, x, 1] ^= 0x80
        got = Y.encode_paste_np(rgb, like_rgb, like, layout, enc, yo)
        gY, gU, gV = Y.split(got, layout)
        lY, lU, lV = Y.split(like, layout)
        pix = np.zeros((L, H, W), bool)
        blk = np.zeros((L, H // 2, W // 2), bool)
        for l, y, x in changed:
            pix[l, y, x] = True
            blk[l, y // 2, x // 2] = True
        assert np.array_equal(gY[~pix], lY[~pix]) and np.array_equal(gU[~blk], lU[~blk]) and np.array_equal(gV[~blk], lV[~blk])
        # and what did change is the plain encode of the result
        plain = Y.split(Y.encode_np(rgb, layout, enc, yo), layout)
        assert np.array_equal(gY[pix], plain[0][pix]) and np.array_equal(gU[blk], plain[1][blk]) and np.array_equal(gV[blk], plain[2][blk])


def test_layouts_hold_the_same_planes():
    p = Y.planes("random", 2, 6, 10)
    for layout in Y.LAYOUTS:
        x = Y.join(*p, layout)
        assert x.shape == (2, 9, 10) and all(np.array_equal(a, b) for a, b in zip(Y.split(x, layout), p))
    nv, pl = Y.join(*p, "nv12"), Y.join(*p, "i420")
    assert np.array_equal(nv[:, :6], pl[:, :6]) and not np.array_equal(nv, pl)
    assert nv[0, 6, 0] == p[1][0, 0, 0] and nv[0, 6, 1] == p[2][0, 0, 0] and pl[0, 6, 1] == p[1][0, 0, 1]


def test_every_refusal_comes_before_any_device_work(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(lib, "load", no_library)
    monkeypatch.setattr(video, "_upload", lambda *a, **k: no_library())
    fmt = video.yuv_format()
    assert tuple(fmt) == ("nv12", "bt709", False, "left") and fmt == video.yuv_format("nv12", "bt709", False, "left")
    with pytest.raises(AttributeError):
        fmt.layout = "i420"
    for bad in (dict(layout="nv21"), dict(layout=None), dict(matrix="bt2020"), dict(chroma="center"), dict(chroma=0),
                dict(full_range="yes"), dict(full_range=1)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            video.yuv_format(**bad)
    ok = np.zeros((2, 6, 8), np.uint8)
    # (an odd H would need 3H/2 rows, which is no integer: the rows that do not divide by 3 are that case)
    for x, what in ((np.zeros((2, 7, 8), np.uint8), "divisible by 3"), (np.zeros((2, 8, 8), np.uint8), "divisible by 3"),
                    (np.zeros((2, 6, 7), np.uint8), "even"), (np.zeros((2, 6, 8, 3), np.uint8), "3H/2")):
        with pytest.raises(ValueError, match=what):
            video.yuv420_to_rgb(x)
        with pytest.raises(ValueError, match=what):
            video.inpaint_video(None, x, np.zeros((2, 4, 8), np.uint8), pixel_format="nv12")
    for bad in ("yv12", "NV12", 3, ("nv12",)):
        with pytest.raises(ValueError, match="nv12"):
            video.yuv420_to_rgb(ok, bad)
        with pytest.raises(ValueError, match="nv12"):
            video.rgb_to_yuv420(np.zeros((2, 4, 8, 3), np.uint8), bad)
        with pytest.raises(ValueError, match="nv12"):
            video.inpaint_video(None, ok, np.zeros((2, 4, 8), np.uint8), pixel_format=bad)
    for shape in ((2, 5, 8, 3), (2, 4, 7, 3)):
        with pytest.raises(ValueError, match="even"):
            video.rgb_to_yuv420(np.zeros(shape, np.uint8))
    with pytest.raises(ValueError, match="frames"):
        video.rgb_to_yuv420(ok)
    with pytest.raises(ValueError, match="like"):
        video.rgb_to_yuv420(np.zeros((2, 4, 8, 3), np.uint8), like=np.zeros((2, 6, 6), np.uint8))
    masks = np.zeros((2, 4, 8), np.uint8)
    with pytest.raises(ValueError, match="keep_float"):
        video.inpaint_video(None, ok, masks, pixel_format="i420", keep_float=True)
    for size in ((5, 4), (4, 3)):
        with pytest.raises(ValueError, match="even"):
            video.inpaint_video(None, ok, masks, pixel_format=fmt, size=size)
    # the frame size the other checks speak of is the decoded one: a box inside 8 x 4 passes them, one inside 8 x 6 does not
    with pytest.raises(ValueError):
        video.inpaint_video(None, ok, masks, pixel_format="nv12", size=(4, 2), region=(0, 0, 8, 6))
    with pytest.raises(ValueError):
        video.inpaint_video(None, ok, masks, pixel_format="nv12", scenes=[2])                 # two frames: no frame 2 to cut at
    # everything in order: the call gets as far as the refusal of the CPU device
    for kw in (dict(), dict(size=(4, 2)), dict(size=(5, 3), restore=True), dict(size=(4, 2), region=(0, 0, 8, 4))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            video.inpaint_video(None, ok, masks, pixel_format="nv12", device="cpu", **kw)


def test_c_entries_refuse_bad_geometry_and_launch_nothing_for_empty_frames():
    """the host side of the two entries runs without a device: the refusals set the error text, and L H W = 0 returns before a launch"""
    import ctypes
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = lib.load()
    dec, enc = (ctypes.c_int32 * 6)(*TABLE["bt709", False][0], 16), (ctypes.c_int32 * 10)(*TABLE["bt709", False][1], 16)
    p = ctypes.c_void_p(256)                           # never dereferenced: every call below returns in front of the launch
    for L, H, W, lay, chroma, what in ((1, 3, 4, 0, 0, b"even"), (1, 4, 5, 1, 1, b"even"), (1, 4, 4, 2, 0, b"layout"),
                                      (1, 4, 4, -1, 0, b"layout"), (1, 4, 4, 0, 2, b"chroma")):
        assert so.e2fgvi_yuv420_to_rgb(p, p, L, H, W, lay, chroma, dec, None) == -1 and what in so.e2fgvi_last_error()
        if what != b"chroma":
            assert so.e2fgvi_rgb_to_yuv420(p, None, None, p, L, H, W, lay, enc, None) == -1 and what in so.e2fgvi_last_error()
    assert so.e2fgvi_rgb_to_yuv420(p, p, None, p, 1, 4, 4, 0, enc, None) == -1 and b"like" in so.e2fgvi_last_error()
    for L, H, W in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert so.e2fgvi_yuv420_to_rgb(None, None, L, H, W, 0, 0, dec, None) == 0
        assert so.e2fgvi_rgb_to_yuv420(None, None, None, None, L, H, W, 1, enc, None) == 0


def test_abi_is_still_9_with_the_two_entries_added():
    assert lib.ABI_VERSION == 9
    header = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    for name, nargs in (("e2fgvi_yuv420_to_rgb", 9), ("e2fgvi_rgb_to_yuv420", 10)):
        assert name in lib.SYMBOLS and len(lib.SYMBOLS[name][1]) == nargs
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs
    assert ops.YUV_LAYOUTS == {"nv12": 0, "i420": 1} and ops.YUV_CHROMA == {"left": 0, "nearest": 1}
    for macro, v in (("E2FGVI_YUV_NV12", 0), ("E2FGVI_YUV_I420", 1), ("E2FGVI_CHROMA_LEFT", 0), ("E2FGVI_CHROMA_NEAREST", 1)):
        assert re.search(r"#define %s %d\b" % (macro, v), header)
