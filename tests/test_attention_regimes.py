"""The attention regimes of tests/attention_regimes.py keep their bite: conditions on the rows and on the oracle alone (CPU), so
that the GPU tests that run the kernels on them (tests/test_gpu_attention_regimes.py) test what they claim to."""
import inspect
import types

import pytest
import torch

from tests import attention_regimes as R


def _rms(t):
    return t.double().pow(2).mean().sqrt().item()


@pytest.fixture(scope="module")
def oracle_without_pad_mass():
    """the oracle with the score of the zero-padded pooled slots moved from -100 to -1e4: their mass is gone"""
    from oracle import e2fgvi_oracle as O
    src = inspect.getsource(O)
    assert src.count("-100.0") == 1
    mod = types.ModuleType("e2fgvi_oracle_without_pad_mass")
    exec(compile(src.replace("-100.0", "-1e4"), O.__file__, "exec"), mod.__dict__)
    return mod


def test_grid_has_exactly_one_interior_window():
    tab, nk = R.key_table()
    assert (R.B, R.T, R.FH, R.FW) == (1, 2, 25, 81) and len(nk) == 45
    assert nk.min() == 180 and nk.max() == 210
    assert [int(w) for w in (nk == 210).nonzero()[0]] == [R.INTERIOR] == [2 * 9 + 4]
    tok, pool = R.build_rows("control")
    assert tuple(tok.shape) == (4050, 1536) and tuple(pool.shape) == (90, 1536) and tok.dtype == pool.dtype == torch.float32


def test_control_cannot_see_the_pad_mass(oracle_without_pad_mass):
    """the gap this file's regimes close: on unit-scale rows the operator's pad term changes no bit of the float64 result"""
    c = R.case("control")
    dropped = R.reference(c["tok"], c["pool"], oracle=oracle_without_pad_mass)
    assert (dropped - c["ref"]).abs().max().item() == 0.0


def test_pad_mass_carries_the_result(oracle_without_pad_mass):
    c = R.case("pad_mass")
    dropped = R.reference(c["tok"], c["pool"], oracle=oracle_without_pad_mass)
    change = (dropped - c["ref"]).abs().max().item() / _rms(c["ref"])
    print("pad_mass: dropping the pad term changes the output by %.3f x rms(ref)" % change)
    assert change >= 0.1


def test_shifted_lives_in_the_interior_window_alone():
    c = R.case("shifted")
    inner = R.window_rows(R.INTERIOR)
    rest = torch.ones(c["ref"].shape[0], dtype=torch.bool)
    rest[inner] = False
    r_in, r_out = _rms(c["ref"][inner]), c["ref"][rest].abs().max().item()
    print("shifted: rms of the interior window's rows %.3f, largest |value| elsewhere %.3e" % (r_in, r_out))
    assert r_in >= 0.1
    assert r_out <= 1e-30
    assert torch.isfinite(c["ref"]).all() and torch.isfinite(c["ref32"]).all()      # the fp32 oracle too


def test_peaked_is_one_hot():
    tok, pool = R.build_rows("peaked")
    logits, _ = R.interior_logits(tok, pool)
    top = logits.softmax(-1).max(-1).values.reshape(-1)
    frac = (top > 0.5).double().mean().item()
    print("peaked: largest softmax weight > 0.5 for %.3f of the interior window's (query, head) pairs" % frac)
    assert frac >= 0.5
    assert logits.abs().max().item() > 100          # far outside the +-20 of the unit-scale tests


def test_late_max_rises_to_the_last_keys():
    tok, pool = R.build_rows("late_max")
    logits, last_pool = R.interior_logits(tok, pool)
    assert int(last_pool.sum()) == 45 and bool(last_pool[-45:].all())          # the last 45 keys of the list
    lead = logits[..., last_pool].max(-1).values - logits[..., ~last_pool].max(-1).values
    print("late_max: the last frame's pooled keys lead every other key by >= %.2f" % lead.min().item())
    assert lead.min().item() >= 10
    # the running maximum moves with every frame's block of keys: tokens of frame 0 < its pooled rows, tokens of frame 1 < its pooled rows
    blocks = [logits[..., f * 210:f * 210 + 165].max(-1).values for f in range(R.T)] + \
             [logits[..., f * 210 + 165:(f + 1) * 210].max(-1).values for f in range(R.T)]
    assert bool((blocks[0] < blocks[1]).all()) and bool((blocks[0] < blocks[2]).all()) and bool((blocks[1] < blocks[3]).all())


def test_uniform_is_the_mean_of_v_over_the_key_list():
    """all logits 0: the reference is the plain mean of V over the window's key list (the ring's duplicates counted as often as
    they are listed; pads weigh e^-100), so a key counted once too often or too few moves the result by 1 / nkeys"""
    c = R.case("uniform")
    tab, nk = R.key_table()
    tok, pool = c["tok"].double(), c["pool"].double()
    for win in (0, R.INTERIOR, 44):
        refs = torch.from_numpy(tab[win, :nk[win]]).long()
        assert len(set(refs.tolist())) < len(refs)                  # duplicates are there
        v = torch.cat([torch.where((refs >= 0).view(-1, 1), tok[f * R.FH * R.FW + refs.clamp(min=0), 1024:],
                                   pool[f * R.NWH * R.NWW + (-(refs + 1)).clamp(min=0), 1024:]) for f in range(R.T)])
        got = c["ref"][R.window_rows(win)]
        assert (got - v.mean(0)).abs().max().item() <= 1e-12
