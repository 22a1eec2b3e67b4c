"""The deformable-conv cases of tests/mdcn_cases.py do what they claim (CPU): the float64 reference agrees with both oracle
restatements, every landing class is populated, the fp32 position is the intended one, and each wrong variant of the
reference moves the result by far more than the loosest bound of tests/test_gpu_mdcn_geometry.py."""
import pytest
import torch

from tests import mdcn_cases as M
from tests.util import assert_close, err

# which cases each mutation is aimed at (where the mutated quantity differs from the true one)
AIMED = {
    "clamp": M.NAMES, "allfour": M.NAMES, "swap": M.NAMES, "pad": M.NAMES,
    "stride": ("stride2_two_ntiles", "five_by_five"),
    "dil": ("dilated",),
    "cq": ("wide_group", "stride2_two_ntiles", "pointwise_short_k", "no_pad"),
    "flow_half": M.EVEN_DG,
}
BITE = 0.1            # x rms(ref), max-abs: more than 6 x the loosest GPU bound (1.5e-2, bf16 products)


@pytest.mark.parametrize("name", M.NAMES)
def test_ref64_agrees_with_both_oracles(name):
    """1e-5 x rms: the bound tests/test_oracle_dcn.py holds the two restatements to against each other"""
    from oracle.dcn import modulated_deform_conv2d
    from oracle.dcn_c import modulated_deform_conv2d_c
    c = M.case(name)
    geo = c["geo"]
    assert tuple(c["ref"].shape) == (geo.N, geo.Cout, geo.Ho, geo.Wo) and c["ref"].dtype == torch.float64
    args = (c["x"], c["off"], c["msk"], c["w"], c["b"], geo.stride, geo.pad, geo.dil, 1, geo.dg)
    assert_close(modulated_deform_conv2d(*args), c["ref"], 1e-5, "oracle.dcn vs ref64, " + name)
    assert_close(modulated_deform_conv2d_c(*args), c["ref"], 1e-5, "oracle.dcn_c vs ref64, " + name)
    f = M.fused_case(name) if name in M.EVEN_DG else None
    if f is not None:
        off, msk = M.fused_offsets(f["raw"], f["flows"], M.MAX_RESIDUE, geo.dg, geo.K)
        got = modulated_deform_conv2d(f["x"], off.float(), msk.float(), f["w"], f["b"], geo.stride, geo.pad, geo.dil, 1, geo.dg)
        assert_close(got, f["ref"], 1e-5, "oracle.dcn vs ref64, fused " + name)


def test_geometries_are_what_the_table_says():
    sizes = {n: (M.Geometry(n).Ho, M.Geometry(n).Wo) for n in M.NAMES}
    assert sizes == {"one_pixel": (1, 1), "wide_group": (7, 9), "stride2_two_ntiles": (5, 6), "dilated": (9, 11),
                     "pointwise_short_k": (5, 6), "row_kernel": (8, 8), "five_by_five": (5, 6), "no_pad": (4, 5),
                     "two_sources": (6, 8)}
    units = {n: M.Geometry(n).dg * M.Geometry(n).K * (M.Geometry(n).cg // 16) for n in M.NAMES}
    assert units["one_pixel"] == 9 and units["pointwise_short_k"] == 3 and units["five_by_five"] == 50
    assert all(M.Geometry(n).cg % 16 == 0 for n in M.NAMES)
    assert {n: M.Geometry(n).cg // 16 for n in M.NAMES if M.Geometry(n).cg > 16} == {k: M.Geometry(k).cg // 16 for k in AIMED["cq"]}
    assert [M.Geometry(n).cg // 16 for n in AIMED["cq"]] == [2, 2, 3, 3]
    g = M.Geometry("two_sources")
    assert g.chans[0] // g.cg == 2 and g.dg // 2 == 4              # source boundary after group 1, flow half after group 3


@pytest.mark.parametrize("name", M.NAMES)
def test_landing_classes(name):
    c = M.case(name)
    geo = c["geo"]
    by, bx = M.base_positions(geo)
    off = c["off"].view(geo.N, geo.dg, geo.K, 2, geo.Ho, geo.Wo)
    for t, cls, base, o, L in ((c["ty"], c["cy"], by, off[:, :, :, 0], geo.H), (c["tx"], c["cx"], bx, off[:, :, :, 1], geo.W)):
        # the position as the kernel forms it: (float)(integer base) + fp32 offset, one fp32 addition
        pos32 = base.float() + o
        near = t.abs() < 1e3
        assert torch.equal(pos32[near].double(), t[near]), name
        assert torch.equal(pos32.double() > -1, t > -1) and torch.equal(pos32.double() < L, t < L)
        counts = torch.bincount(cls.reshape(-1), minlength=M.NCLASS)
        assert counts.max() - counts.min() <= 1, counts.tolist()         # dealt out, not drawn
        if geo.samples >= 300:
            assert counts.min() >= 5, (name, counts.tolist())
        fixed = torch.tensor(M.class_positions(L), dtype=torch.float64)
        for k in range(len(fixed)):
            assert (t[cls == k] == fixed[k]).all()
        inner = t[cls >= len(fixed)]
        assert ((inner >= 0) & (inner <= L - 1) & (inner * 4 == (inner * 4).round())).all()
    inside = ((c["ty"] > -1) & (c["ty"] < geo.H) & (c["tx"] > -1) & (c["tx"] < geo.W)).double().mean().item()
    print("%s: %d samples, %.3f inside" % (name, geo.samples, inside))
    if geo.samples >= 300:
        assert 0.3 <= inside <= 0.7, (name, inside)
    assert ((c["msk"] >= 0) & (c["msk"] < 1)).all()


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_mutations_bite(mut):
    """every wrong variant of the reference moves it by >= 0.1 x rms(ref) in max-abs on every case it is aimed at: a kernel
    with that defect cannot pass the GPU test.  A condition on the INPUTS: if it fails, the inputs change, not the threshold."""
    for name in AIMED[mut]:
        geo = M.Geometry(name)
        if mut == "flow_half":
            c = M.fused_case(name)
            bad = M.ref64(c["x"], c["raw"], None, c["w"], c["b"], *geo.conv, mut=mut, flows=c["flows"], max_residue=M.MAX_RESIDUE)
        else:
            c = M.case(name)
            bad = M.ref64(c["x"], c["off"], c["msk"], c["w"], c["b"], *geo.conv, mut=mut)
        _, r = err(bad, c["ref"])
        print("%s on %s: %.3f x rms" % (mut, name, r))
        assert r >= BITE, "%s does not bite on %s: %.3e x rms" % (mut, name, r)
    # the remaining mutations are no-ops where they are not aimed (the table above is the whole of their reach)
    if mut in ("stride", "dil", "cq"):
        for name in set(M.NAMES) - set(AIMED[mut]):
            c = M.case(name)
            assert torch.equal(M.ref64(c["x"], c["off"], c["msk"], c["w"], c["b"], *c["geo"].conv, mut=mut), c["ref"]), (mut, name)


def test_nonfinite_offsets_drop_the_sample():
    """an offset of +-inf, nan, +-3e9 or 1e30 fails mmcv's guard and the tap adds 0: all three implementations return what they
    return with those offsets at +-1e6 (oracle/dcn.py multiplied the NaN weights by 0 before)"""
    from oracle.dcn import modulated_deform_conv2d
    from oracle.dcn_c import modulated_deform_conv2d_c
    c = M.case("wide_group")
    geo = c["geo"]
    off, far, ref = M.nonfinite_case("wide_group")
    assert (~torch.isfinite(off)).sum() == 9 and (off.abs() > 1e9).sum() == 15 and torch.isfinite(far).all()
    assert torch.equal(M.ref64(c["x"], off, c["msk"], c["w"], c["b"], *geo.conv), ref)
    _, moved = err(ref, c["ref"])
    assert moved >= BITE, moved                                     # the dropped samples mattered
    for fn in (modulated_deform_conv2d, modulated_deform_conv2d_c):
        got = fn(c["x"], off, c["msk"], c["w"], c["b"], geo.stride, geo.pad, geo.dil, 1, geo.dg)
        assert torch.equal(got, fn(c["x"], far, c["msk"], c["w"], c["b"], geo.stride, geo.pad, geo.dil, 1, geo.dg)), fn.__name__
        assert_close(got, ref, 1e-5, "%s vs ref64, non-finite offsets" % fn.__name__)
