"""Pins the CPU oracle (oracle/e2fgvi_oracle.py) against the committed golden fixtures made from the real reference:
sub-sampled outputs at many sizes (tests/golden/make_golden.py) and, for small cases, the reference's flows, a grid and the
edges of its output, the means of every output row, column and 6x6 tile, its batch behaviour and its state_dict key order
(tests/golden/make_pin_golden.py -> pin_reference.npz)."""
import glob
import os

import numpy as np
import pytest
import torch

from e2fgvi_amd.synth import synth_clip, synth_state_dict
from oracle import e2fgvi_oracle as O

PIN = os.path.join(os.path.dirname(__file__), "golden", "pin_reference.npz")
GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "g[0-9]*_*.npz")),
              key=lambda q: int(os.path.basename(q).split("_")[0][1:]))
# minutes each on a CPU (the 1080x1944 clip, the 10-frame 720x1296 clips of round 6): the HIP path is compared with these on the GPU
# box; the oracle is pinned at the 12x12 window grid by g5 and on the peaked weights by g11 / g12
SLOW = ("g1_", "g6_", "g9_", "g10_", "g13_", "g14_")


def load_golden(path):
    z = np.load(path)
    H, W, t, lt, b, seed, so, sf = [int(v) for v in z["meta"]]
    return z, str(z["model"]), str(z["kind"]), (H, W), t, lt, b, seed, so, sf


def test_fixtures_present():
    assert len(GOLD) >= 4


@pytest.mark.parametrize("path", [p for p in GOLD if not os.path.basename(p).startswith(SLOW)], ids=os.path.basename)
def test_oracle_matches_golden(path):
    """(g1, the 5-frame 432x240 clip, is checked on the GPU box and in test_oracle_vs_reference's big case; g6, the
    1080x1944 clip, costs minutes on a CPU: the HIP path is compared with it directly on the GPU box, and the oracle is
    pinned at a 12x12 window grid by g5)"""
    z, model, kind, (H, W), t, lt, b, seed, so, sf = load_golden(path)
    sd = synth_state_dict(model, kind, 0)
    x, _ = synth_clip(b, t, H, W, seed=seed, moving=True)
    out, (ff, fb) = O.forward(sd, x, lt, model)
    assert np.abs(out[:, :, ::so, ::so].numpy() - z["out_sub"]).max() < 2e-5
    assert np.abs(ff[..., ::sf, ::sf].numpy() - z["flow_fwd_sub"]).max() < 1e-4
    assert np.abs(fb[..., ::sf, ::sf].numpy() - z["flow_bwd_sub"]).max() < 1e-4
    assert np.abs(out.double().mean(dim=(1, 2, 3)).numpy() - z["out_frame_mean"]).max() < 1e-6


def pin(key):
    with np.load(PIN) as z:
        return z[key]


def assert_out_matches(prefix, out, bound):
    """`out` [N, 3, H, W] against the reference's stored output (make_pin_golden.out_summary): every element of the grid and of
    the edge rows / columns within `bound`; the mean of every row / column of every plane within bound / sqrt(its length), the
    mean of every tile x tile tile within bound / tile (less the float32 rounding of the stored tile means) -- independent
    per-element differences of up to `bound` average down by about that much, a difference that runs along a whole row or
    column of a tile or of a plane does not"""
    g, tl = int(pin("grid")), int(pin("tile"))
    N, C, H, W = out.shape
    rows, cols = pin(prefix + "out_row_mean"), pin(prefix + "out_col_mean")
    assert rows.shape == (N, C, H) and cols.shape == (N, C, W)
    o = out.numpy()
    assert np.abs(o[:, :, ::g, ::g] - pin(prefix + "out_grid")).max() < bound
    assert np.abs(o[:, :, [0, -1], :] - pin(prefix + "out_edge_rows")).max() < bound
    assert np.abs(o[:, :, :, [0, -1]] - pin(prefix + "out_edge_cols")).max() < bound
    assert np.abs(out.double().mean(3).numpy() - rows).max() < bound / np.sqrt(W)
    assert np.abs(out.double().mean(2).numpy() - cols).max() < bound / np.sqrt(H)
    tiles = pin(prefix + "out_tile_mean")
    assert tiles.shape == (N, C, H // tl, W // tl)
    got = out.double().reshape(N, C, H // tl, tl, W // tl, tl).mean(dim=(3, 5)).numpy()
    assert (np.abs(got - tiles) < bound / tl - np.spacing(np.abs(tiles)) / 2).all()


def reference_state_dict(model, sd):
    """the state_dict of the reference InpaintGenerator after a strict load of `sd`: sd's tensors in the reference's key order"""
    keys = [str(k) for k in pin("keys_" + model)]
    assert sorted(keys) == sorted(sd.keys())
    return {k: sd[k] for k in keys}


@pytest.mark.parametrize("model,kind,hw,t,lt,b", [("e2fgvi_hq", "stress", (60, 108), 3, 2, 2),
                                                  ("e2fgvi_hq", "stress", (60, 108), 2, 1, 1),      # one local frame
                                                  ("e2fgvi_hq", "default", (120, 216), 3, 3, 1),
                                                  ("e2fgvi", "stress", (240, 432), 3, 2, 1),
                                                  ("e2fgvi_hq", "peaked", (120, 216), 3, 2, 1)])
def test_oracle_vs_reference(model, kind, hw, t, lt, b):
    """the oracle against the reference's output and flows on the same clip (pin_reference.npz)"""
    sd = synth_state_dict(model, kind, 0)
    assert [str(k) for k in pin("keys_" + model)] == list(sd.keys())
    key = "%s_%s_%dx%d_t%d_lt%d_b%d/" % (model, kind, hw[0], hw[1], t, lt, b)
    rf, rb = (torch.from_numpy(pin(key + n)) for n in ("flow_fwd", "flow_bwd"))
    x, _ = synth_clip(b, t, hw[0], hw[1], seed=21, moving=True)
    oo, (of, ob) = O.forward(sd, x, lt, model)
    assert tuple(oo.shape) == (b * t, 3, hw[0], hw[1])
    assert_out_matches(key, oo, 2e-5)
    assert tuple(rf.shape) == tuple(of.shape) == (b, lt - 1, 2, hw[0] // 4, hw[1] // 4)
    if lt > 1:
        assert (rf - of).abs().max() < 1e-5 and (rb - ob).abs().max() < 1e-5


def test_reference_batch_is_clip_independent():
    """clips are independent units: b=2 == two b=1 calls -- the sharding premise.  The reference's difference
    (b=2 output) - (b=1 outputs) is stored whole in units of diff_step (pin_reference.npz): its largest value plus the
    rounding half-step bounds the true one.  The oracle reproduces the reference's b=2 output."""
    q, step = pin("batch/halves_diff_q"), float(pin("diff_step"))
    assert q.shape == (6, 3, 60, 108)
    assert np.abs(q.astype(np.float64)).max() * step + step / 2 < 1e-6
    x, _ = synth_clip(2, 3, 60, 108, seed=22, moving=True)
    oo, _ = O.forward(synth_state_dict("e2fgvi_hq", "stress", 0), x, 2, "e2fgvi_hq")
    assert_out_matches("batch/", oo, 2e-5)


def test_checkpoint_files_written_by_the_reference_load(tmp_path):
    """README.md:148-149 / test.py:119-120: a checkpoint FILE written by the reference (torch.save of its state_dict, the
    format of the released E2FGVI-CVPR22.pth / E2FGVI-HQ-CVPR22.pth) loads into the drop-in, also with the mmcv
    {'state_dict': ...} wrapper, DDP 'module.' prefixes, and as a SPyNet-only file (flow_comp.py:59-72).  The file is
    written as the reference writes it: its state_dict's keys in its order (pin_reference.npz)."""
    import importlib
    for model in ("e2fgvi", "e2fgvi_hq"):
        ref = reference_state_dict(model, synth_state_dict(model, "stress", 0))
        path = str(tmp_path / (model + ".pth"))
        torch.save(ref, path)
        net = importlib.import_module("model." + model).InpaintGenerator()
        net.load_checkpoint(path)
        for k, v in ref.items():
            assert torch.equal(net.state_dict()[k], v), k
        torch.save({"state_dict": {"module." + k: v for k, v in ref.items()}, "meta": {}}, path)
        net2 = importlib.import_module("model." + model).InpaintGenerator()
        net2.load_checkpoint(path)
        assert all(torch.equal(net2.state_dict()[k], v) for k, v in ref.items())
        pre = "update_spynet."
        spy = {"state_dict": {k[len(pre):]: v + 1 for k, v in ref.items() if k.startswith(pre)}}
        torch.save(spy, path)
        net2.load_checkpoint(path)
        assert torch.equal(net2.update_spynet.basic_module[3].basic_module[2].conv.weight,
                           ref[pre + "basic_module.3.basic_module.2.conv.weight"] + 1)
