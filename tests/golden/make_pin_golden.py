"""Generate tests/golden/pin_reference.npz from the REAL reference (run in the build container only).

    python tests/golden/make_pin_golden.py

What tests/test_oracle_pin.py compares the oracle with, for every case of PIN_CASES and for the b = 2 clip of the
clip-independence check, in a form that keeps the fixture small (the whole outputs would be megabytes of noise-like floats):
  flow_fwd / flow_bwd   the reference's flows, whole
  out_grid              output frames at every GRID-th row and column (from row / column 0)
  out_edge_rows / _cols the first and last row / column of every output plane, whole
  out_row_mean / _col_mean   the mean of every row / column of every output plane (float64)
  out_tile_mean         the mean of every TILE x TILE tile of every output plane (float32)
For the clip-independence check also batch/halves_diff_q: (b=2 output) - (the two b=1 outputs), whole, as integers in units
of DIFF_STEP.  And the reference's state_dict key order per model (the key order of a checkpoint FILE the reference writes).
The reference is imported read-only through oracle/ref_import.py (mmcv shim), with the synthetic weights of e2fgvi_amd.synth.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from e2fgvi_amd.synth import synth_clip, synth_state_dict  # noqa: E402

OUT = os.path.join(HERE, "pin_reference.npz")
# model, weights kind, (H, W), t, l_t, clips -- clip seed PIN_SEED
PIN_CASES = [("e2fgvi_hq", "stress", (60, 108), 3, 2, 2),
             ("e2fgvi_hq", "stress", (60, 108), 2, 1, 1),      # one local frame
             ("e2fgvi_hq", "default", (120, 216), 3, 3, 1),
             ("e2fgvi", "stress", (240, 432), 3, 2, 1),
             ("e2fgvi_hq", "peaked", (120, 216), 3, 2, 1)]
PIN_SEED = 21
BATCH_SEED = 22     # e2fgvi_hq stress, 2 clips of 3 frames at 60x108, l_t = 2
GRID = 8
TILE = 6            # divides every H and W above
DIFF_STEP = 2.0 ** -27


def case_key(model, kind, hw, t, lt, b):
    return "%s_%s_%dx%d_t%d_lt%d_b%d" % (model, kind, hw[0], hw[1], t, lt, b)


def out_summary(prefix, out):
    """the stored form of an output [N, 3, H, W] (see the module docstring)"""
    o = out.numpy()
    return {prefix + "out_grid": o[:, :, ::GRID, ::GRID], prefix + "out_edge_rows": o[:, :, [0, -1], :],
            prefix + "out_edge_cols": o[:, :, :, [0, -1]], prefix + "out_row_mean": out.double().mean(3).numpy(),
            prefix + "out_col_mean": out.double().mean(2).numpy(), prefix + "out_tile_mean": tile_mean(out).float().numpy()}


def tile_mean(out):
    N, C, H, W = out.shape
    return out.double().reshape(N, C, H // TILE, TILE, W // TILE, TILE).mean(dim=(3, 5))


def main():
    from oracle import ref_import
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    arrays = {"grid": np.array(GRID), "tile": np.array(TILE), "diff_step": np.array(DIFF_STEP)}
    for model in ("e2fgvi", "e2fgvi_hq"):
        net = ref_import.build_reference_model(model, synth_state_dict(model, "stress", 0))
        arrays["keys_" + model] = np.array(list(net.state_dict().keys()))
    for model, kind, hw, t, lt, b in PIN_CASES:
        net = ref_import.build_reference_model(model, synth_state_dict(model, kind, 0))
        x, _ = synth_clip(b, t, hw[0], hw[1], seed=PIN_SEED, moving=True)
        with torch.no_grad():
            out, (ff, fb) = net(x, lt)
        k = case_key(model, kind, hw, t, lt, b) + "/"
        arrays.update(out_summary(k, out))
        arrays[k + "flow_fwd"], arrays[k + "flow_bwd"] = ff.numpy(), fb.numpy()
        print(k, tuple(out.shape), flush=True)
    net = ref_import.build_reference_model("e2fgvi_hq", synth_state_dict("e2fgvi_hq", "stress", 0))
    x, _ = synth_clip(2, 3, 60, 108, seed=BATCH_SEED, moving=True)
    with torch.no_grad():
        o2 = net(x, 2)[0]
        halves = torch.cat([net(x[:1], 2)[0], net(x[1:], 2)[0]])
    arrays.update(out_summary("batch/", o2))
    q = torch.round((o2.double() - halves.double()) / DIFF_STEP)
    assert q.abs().max() < 127
    arrays["batch/halves_diff_q"] = q.to(torch.int8).numpy()
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, "%.2f MB" % (os.path.getsize(OUT) / 2 ** 20))


if __name__ == "__main__":
    main()
