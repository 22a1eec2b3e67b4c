"""The static cache plan of video.inpaint_video(reuse=True) (e2fgvi_amd/video.py::plan_reuse): host logic, replayed here."""
import math

import pytest

from e2fgvi_amd import video

CASES = [(100, 5, 10, -1), (23, 5, 10, -1), (12, 5, 10, 2), (7, 3, 10, -1), (1, 5, 10, -1), (41, 5, 10, 4)]


@pytest.mark.parametrize("L,stride,ref_length,num_ref", CASES)
def test_plan_replays(L, stride, ref_length, num_ref):
    windows = video.plan_windows(L, stride, ref_length, num_ref)
    plan = video.plan_reuse(windows)
    assert len(plan.windows) == len(windows)
    held, held_pairs = {}, {}                      # slot -> what it holds right now
    encoded, computed = [], []
    peak = peak_pairs = 0
    for k, ((nb, rf), p) in enumerate(zip(windows, plan.windows)):
        # the neighbour and reference ids are exactly plan_windows's
        assert p["neighbors"] == nb and p["refs"] == rf
        # fills: no slot is reused while live, one slot per new frame / pair
        assert len(p["encode"]) == len(p["new_slots"]) and len(p["pairs"]) == len(p["new_pair_slots"])
        for j, s in zip(p["encode"], p["new_slots"]):
            assert s not in held, "slot %d still holds frame %d" % (s, held.get(s, -1))
            assert 0 <= s < plan.slots
            held[s] = j
            encoded.append(j)
        for pr, s in zip(p["pairs"], p["new_pair_slots"]):
            assert s not in held_pairs and 0 <= s < plan.pair_slots
            held_pairs[s] = pr
            computed.append(pr)
        peak, peak_pairs = max(peak, len(held)), max(peak_pairs, len(held_pairs))
        # the masked frames built now: the new frames first, then what only the new pairs need; pair positions point into them
        assert p["clip"][:len(p["encode"])] == p["encode"] and len(set(p["clip"])) == len(p["clip"])
        assert [(p["clip"][a], p["clip"][b]) for a, b in p["pair_pos"]] == p["pairs"]
        assert set(p["clip"]) == set(p["encode"]) | {j for pr in p["pairs"] for j in pr}
        # every id of the window is resident when the window runs, under the slot the plan names
        assert [held.get(s) for s in p["enc_slots"]] == nb + rf
        assert [held_pairs.get(s) for s in p["flow_slots"]] == list(zip(nb[:-1], nb[1:]))
        # releases: only what no later window lists
        for s in p["free"]:
            j = held.pop(s)
            assert all(j not in a + b for a, b in windows[k + 1:])
        for s in p["free_pairs"]:
            pr = held_pairs.pop(s)
            assert all(pr not in zip(a[:-1], a[1:]) for a, _ in windows[k + 1:])
    assert not held and not held_pairs             # everything is released after its last use
    # each frame of the video is encoded once, each needed pair computed once
    assert sorted(encoded) == list(range(L))
    needed = sorted({pr for nb, _ in windows for pr in zip(nb[:-1], nb[1:])})
    assert sorted(computed) == needed and len(set(computed)) == len(computed)
    # peak slots equal the plan's own report
    assert peak == plan.slots and peak_pairs == plan.pair_slots
    if num_ref == -1:
        assert plan.slots <= math.ceil(L / ref_length) + 2 * stride + 1


def test_first_window_encodes_the_references_of_the_whole_video():
    plan = video.plan_reuse(video.plan_windows(100, 5, 10, -1))
    assert plan.windows[0]["encode"] == [0, 1, 2, 3, 4, 5] + list(range(10, 100, 10))
    assert plan.windows[1]["encode"] == [6, 7, 8, 9] and plan.windows[1]["pairs"] == [(5, 6), (6, 7), (7, 8), (8, 9), (9, 10)]
    assert plan.windows[1]["clip"] == [6, 7, 8, 9, 5, 10]


def test_a_freed_slot_is_handed_out_again():
    plan = video.plan_reuse(video.plan_windows(23, 5, 10, -1))
    freed = set()
    reused = False
    for p in plan.windows:
        reused |= bool(freed & set(p["new_slots"]))
        freed |= set(p["free"])
    assert reused
    assert plan.cache_bytes(15, 27, 4) == plan.slots * 15 * 27 * 128 * 4 + 2 * plan.pair_slots * 15 * 27 * 2 * 4


def test_reuse_refuses_what_it_does_not_support_before_touching_the_device():
    """argument checks come first: no GPU needed"""
    import numpy as np
    f, m = np.zeros((3, 8, 8, 3), np.uint8), np.zeros((3, 8, 8), np.uint8)

    class WithEngine:
        def engine(self):
            raise AssertionError("not reached")
    with pytest.raises(ValueError, match="batch_windows"):
        video.inpaint_video(WithEngine(), f, m, reuse=True, batch_windows=2)
    with pytest.raises(ValueError, match="in_flight"):
        video.inpaint_video(WithEngine(), f, m, reuse=True, in_flight=2)
    with pytest.raises(TypeError, match="InpaintGenerator"):
        video.inpaint_video(lambda x, n: (x, None), f, m, reuse=True)
