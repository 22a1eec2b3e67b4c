"""Every attention kernel family, every variant, on the off-unit-scale regimes of tests/attention_regimes.py, against the oracle
in float64 on the rows the kernel reads.

What each regime holds (tests/test_attention_regimes.py checks the regimes themselves on the CPU):
  pad_mass   the analytic mass of the zero-padded pooled slots, nmask * exp2(-100 log2 e - m), in every kernel's epilogue: missing,
             mis-scaled or counted for the wrong window or frame count, it moves the output by tenths of its rms
  shifted    the same term's edge: all logits near -250, so exp2 overflows -- the pads of a border window take all the mass
             (output 0) and the interior window, which has no pads, must return the ordinary shift-invariant result, not 0 * inf
  peaked     a one-hot softmax, and (late_max) a running maximum that moves up to the last keys of the list, one key group
  late_max   holding essentially none of the mass: a rescale skipped when it was needed, a merge that drops the lighter
             group's maximum, a tail tile whose -1e30 entries win a row
  uniform    all logits 0: the plain mean of V over the key list, so a key counted once too often or too few shows (the ring's
             12 duplicates weigh double)
  control    the other tests' regime on this grid and at their tolerances

Bounds.  A logit of magnitude 100 ... 250 carries |logit| 2^-24 of absolute error in any fp32 evaluation, so the allowance is
measured against the reference, not guessed: e32 = max |oracle in float32 - oracle in float64| / rms, on the same rows (CPU).
fp32 and split-operand kernels: max(ATT_TOL, 4 e32) x rms -- the kernel and the fp32 oracle are two fp32 evaluations with other
product and summation orders, ATT_TOL itself is twice a measured maximum on the same grounds.  16-bit kernels: their usual
elementwise forms with 4 e32 added to the absolute part; they scale the fp32 scores, so their logits are fp32-level and only
P and the output are rounded.  Measured / allowed per family and regime: profiles/attention_regimes_margins.txt."""
import pytest
import torch

from tests import attention_regimes as R
from tests.util import assert_bound, assert_close, assert_close_bf16

pytestmark = pytest.mark.gpu


def _device_case(dev, name, rounding=None):
    c = R.case(name, rounding)
    tab, nk = R.key_table()
    both = torch.cat([c["tok"], c["pool"]], 0).to(dev)       # back to back: one buffer resource covers both
    rows = c["tok"].shape[0]
    return c, both, rows, torch.from_numpy(tab).to(dev), torch.from_numpy(nk).to(dev)


def _check_shifted_border(name, out, what):
    """shifted: outside the interior window the pads hold all the mass; the reference is below 1e-30 there"""
    if name != "shifted":
        return
    rest = torch.ones(out.shape[0], dtype=torch.bool)
    rest[R.window_rows(R.INTERIOR)] = False
    inner = out.detach().float().cpu()[~rest]
    assert torch.isfinite(inner).all(), what + ": non-finite output in the interior window's rows"
    assert_bound(out.detach().float().cpu()[rest].abs().max().item(), 1e-30, what + " [rows of the windows with pads]")


@pytest.mark.parametrize("name", R.REGIMES)
def test_focal_attention_regimes(dev, name):
    from e2fgvi_amd import ops
    from tests.test_gpu_ops import ATT_TOL
    c, both, rows, tab, nk = _device_case(dev, name)
    tol = max(ATT_TOL, 4 * c["e32"])
    print("%s: e32 = %.3e, allowed %.3e x rms" % (name, c["e32"], tol))
    for waves in (0, 2, 4, 12, 14, 22, 24, 32, 34):
        out = ops.focal_attention(both[:rows], both[rows:], tab, nk, R.B, R.T, R.FH, R.FW, waves=waves)
        what = "attention fp32 %s waves=%d" % (name, waves)
        _check_shifted_border(name, out, what)
        assert_close(out.cpu(), c["ref"], tol, what)


@pytest.mark.parametrize("name", R.REGIMES)
def test_focal_attention_x3_regimes(dev, name):
    from e2fgvi_amd import ops
    from tests.test_gpu_ops import ATT_TOL
    c, both, rows, tab, nk = _device_case(dev, name)
    planes = ops.split3_kv(both)
    tol = max(ATT_TOL, 4 * c["e32"])
    for waves in (0, 2, 4, 8, 14):
        out = ops.focal_attention_x3(both[:rows], planes, tab, nk, R.B, R.T, R.FH, R.FW, waves=waves)
        what = "attention x3 %s waves=%d" % (name, waves)
        _check_shifted_border(name, out, what)
        assert_close(out.cpu(), c["ref"], tol, what)


@pytest.mark.parametrize("name", R.REGIMES)
def test_focal_attention_bf16_regimes(dev, name):
    from e2fgvi_amd import ops
    c, both, rows, tab, nk = _device_case(dev, name, torch.bfloat16)
    print("%s (bf16 rows): e32 = %.3e" % (name, c["e32"]))
    for variant in (None, 1, 12, 14, 18, 22, 24, 28):
        out = ops.focal_attention_bf16(both[:rows], both[rows:], tab, nk, R.B, R.T, R.FH, R.FW, variant=variant)
        assert out.dtype == torch.bfloat16
        what = "attention bf16 %s variant %s" % (name, variant)
        _check_shifted_border(name, out, what)
        assert_close_bf16(out, c["ref"], what, ulps=1.0, abs_rms=1.2e-2 + 4 * c["e32"])


@pytest.mark.parametrize("name", R.REGIMES)
def test_focal_attention_f16_regimes(dev, name):
    from e2fgvi_amd import ops
    from tests.test_gpu_fp16 import assert_close_f16
    c, both, rows, tab, nk = _device_case(dev, name, torch.float16)
    print("%s (fp16 rows): e32 = %.3e" % (name, c["e32"]))
    ref = c["ref"].float()
    rms = ref.pow(2).mean().sqrt().item()
    for variant in (None, 1, 12, 14, 18, 22, 24, 28):
        out = ops.focal_attention_bf16(both[:rows], both[rows:], tab, nk, R.B, R.T, R.FH, R.FW, variant=variant)
        assert out.dtype == torch.float16
        what = "attention fp16 %s variant %s" % (name, variant)
        _check_shifted_border(name, out, what)
        abs_rms = 2e-3 + 4 * c["e32"]
        assert torch.isfinite(out.float()).all(), what + ": non-finite output"
        ratio = ((out.float().cpu() - ref).abs() / (2.0 ** -10 * ref.abs() + abs_rms * rms)).max().item()
        assert_bound(ratio, 1.0, what + " [fp16 elementwise]")                  # the line of the margin log
        assert_close_f16(out, c["ref"], what, ulps=1.0, abs_rms=abs_rms)
