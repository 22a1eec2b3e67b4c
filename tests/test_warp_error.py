"""The float64 reference of E_warp (tests/warp_error_cases.py) against what the definition must give on inputs whose answer is
known, and against the wrong readings of the definition it has to tell apart.  The device kernel is held to this reference in
test_gpu_warp_error.py."""
import numpy as np
import pytest
import torch

from tests import warp_error_cases as C


def test_constant_frames_zero_flows():
    """e = 3 ((c1 - c2) / 255)^2 and n = H W"""
    H, W = 6, 11
    frames = np.stack([np.full((H, W, 3), 40.0), np.full((H, W, 3), 190.0), np.full((H, W, 3), 190.0)])
    z = np.zeros((2, H, W, 2))
    r = C.reference(frames, z, z)
    assert r[0]["n"] == H * W and abs(r[0]["e"] - 3 * (150 / 255.0) ** 2) <= 1e-15
    assert r[1]["n"] == H * W and r[1]["e"] == 0.0


def test_scene():
    H, W = C.SCENE_HW
    for u8 in (False, True):
        clean = C.case_reference("scene", u8)
        for r in clean:
            assert r["n"] >= 0.85 * H * W and r["e"] <= 1e-4, (u8, r["n"], r["e"])
            assert r["outside"].any() and r["occluded"].any() and r["boundary"].any()
        flick = C.case_reference("scene_flicker", u8)
        for t in (1, 2):                                  # the pairs that hold frame 2
            assert flick[t]["n"] == clean[t]["n"] and flick[t]["e"] >= 10 * clean[t]["e"], (u8, t, flick[t]["e"], clean[t]["e"])
        for t in (0, 3):
            assert flick[t]["e"] == clean[t]["e"]
        for z, r in zip(C.case_reference("scene_zero_flows", u8), clean):
            assert z["n"] == H * W and z["e"] >= 100 * r["e"], (u8, z["e"], r["e"])


def test_scene_exclusion_classes_of_pair_0():
    """the rectangle's leading edges uncover nothing in frame 1 (occlusion), its outline is a flow discontinuity (motion boundary),
    the background's drift leaves the frame on two sides (outside): disjoint here, and they account for every dropped pixel"""
    r = C.case_reference("scene")[0]
    H, W = C.SCENE_HW
    out, occ, mb = int(r["outside"].sum()), int((r["occluded"] & ~r["boundary"]).sum()), int((r["boundary"] & ~r["occluded"]).sum())
    assert (out, occ, mb) == (166, 78, 79) and not (r["occluded"] & r["boundary"]).any()
    assert r["n"] == H * W - out - occ - mb == 3133


@pytest.mark.parametrize("name", C.NAMES)
def test_threshold_margin(name):
    """a condition on the INPUTS of every case the kernel is compared on: no threshold test is decided by less than 1e-9, so the
    device's fused multiply-adds cannot flip a decision the reference took"""
    for u8 in (False, True):
        for t, r in enumerate(C.case_reference(name, u8)):
            assert r["margin"] >= 1e-9, (name, t, r["margin"])


@pytest.mark.parametrize("name", ["scene", "smooth_33x65", "smooth_1x9", "smooth_9x1"])
def test_warp_equals_oracle_flow_warp(name):
    from oracle import e2fgvi_oracle as O
    c = C.case(name)
    for t, r in enumerate(C.case_reference(name)):
        B = torch.from_numpy(c["frames"][t + 1].astype(np.float64)).permute(2, 0, 1)[None]
        ref = O.flow_warp(B, torch.from_numpy(c["fwd"][t].astype(np.float64))[None], "zeros")[0].permute(1, 2, 0).numpy()
        inside = ~r["outside"]
        assert inside.any()
        assert np.abs(r["warped"] - ref)[inside].max() <= 1e-13 * 255


def test_nonfinite_flows_are_excluded_by_select():
    c = C.case("nonfinite")
    assert not np.isfinite(c["fwd"]).all() and not np.isfinite(c["bwd"]).all()
    for t, r in enumerate(C.case_reference("nonfinite")):
        assert np.isfinite(r["e"]) and 0 < r["n"] < c["fwd"][t][..., 0].size
        f = np.isfinite(c["fwd"][t]).all(-1)
        assert not r["keep"][~f].any()
        assert not r["keep"][:, :-1][~f[:, 1:]].any() and not r["keep"][:-1, :][~f[1:, :]].any()      # the neighbours used


BITE = {"swap_channels": "scene", "border": "scene", "bwd_unwarped": "scene", "no_half": "eval_70x90", "no_rel": "eval_70x90",
        "central_diff": "scene", "ignore_valid": "smooth_valid_40x56", "div_hw": "scene"}


@pytest.mark.parametrize("variant", C.VARIANTS)
def test_reference_tells_wrong_variants_apart(variant):
    """each wrong reading of the definition moves n (any change counts) or e (by at least 1 %) on some pair of some case"""
    assert set(BITE) == set(C.VARIANTS)
    name = BITE[variant]
    good, bad = C.case_reference(name), C.case_reference(name, False, variant)
    moved = [g["n"] != b["n"] or abs(g["e"] - b["e"]) >= 0.01 * g["e"] > 0 for g, b in zip(good, bad)]
    assert any(moved), (variant, [(g["n"], b["n"], g["e"], b["e"]) for g, b in zip(good, bad)])
