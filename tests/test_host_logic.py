"""Host-side logic that needs no GPU: checkpoint layout, key tables, ABI surface, sharding maths."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_layout_matches_spec():
    import importlib
    from e2fgvi_amd.synth import state_spec, synth_state_dict
    for name, n in (("e2fgvi", 243), ("e2fgvi_hq", 244)):
        net = importlib.import_module("model." + name).InpaintGenerator()
        sd = net.state_dict()
        spec = state_spec(name)
        assert len(sd) == n
        assert list(sd.keys()) == list(spec.keys())
        for k, (shape, dt) in spec.items():
            assert tuple(sd[k].shape) == tuple(shape) and sd[k].dtype == dt, k
        net.load_state_dict(synth_state_dict(name, "stress", 0), strict=True)
        assert sum(v.numel() for v in sd.values() if v.is_floating_point()) > 41e6


def test_default_init_distribution():
    """reference random init (e2fgvi.py:29-68,203-208): N(0,0.02) weights, zero biases, zero conv_offset[-1]"""
    import importlib
    torch.manual_seed(0)
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    sd = net.state_dict()
    assert abs(sd["encoder.layers.8.weight"].std().item() - 0.02) < 1e-3
    assert sd["encoder.layers.8.bias"].abs().max() == 0
    assert sd["feat_prop_module.deform_align.forward_.conv_offset.6.weight"].abs().max() == 0
    w = sd["feat_prop_module.deform_align.forward_.weight"]
    assert abs(w.abs().max().item() - 1 / np.sqrt(256 * 9)) < 1e-4          # uniform(+-1/sqrt(C*9)) untouched
    assert abs(sd["transformer.3.pool_layers.0.weight"].std().item() - 0.02) < 8e-3   # overridden by init_weights
    assert sd["transformer.0.norm1.weight"].eq(1).all() and sd["sc.bias"].abs().max() == 0


def test_synth_is_deterministic_and_cpu_forward_refuses():
    import importlib
    from e2fgvi_amd.synth import synth_state_dict
    a, b = synth_state_dict("e2fgvi", "default", 0), synth_state_dict("e2fgvi", "default", 0)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = synth_state_dict("e2fgvi", "default", 1)
    assert not torch.equal(a["decoder.2.weight"], c["decoder.2.weight"])
    net = importlib.import_module("model.e2fgvi").InpaintGenerator()
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 2, 3, 240, 432), 2)       # no CPU path: must fail loudly


def _reference_key_ids(fh, fw, T=1):
    """Enumerate, with torch ops on an id tensor, the keys each window sees -- the reference's roll /
    window_partition / valid_ind_rolled / unfold chain (tfocal_transformer.py:235-333)."""
    from oracle import e2fgvi_oracle as O
    ids = torch.arange(fh * fw, dtype=torch.float32).view(1, 1, fh, fw, 1)
    own = O._win_part(ids, O.WIN).view(-1, 45)
    valid = O.rolled_valid_index()
    parts = []
    for sy, sx in ((-2, -4), (-2, 4), (2, -4), (2, 4)):
        parts.append(O._win_part(torch.roll(ids, shifts=(sy, sx), dims=(2, 3)), O.WIN).view(-1, 45))
    rolled = torch.cat(parts, 1)[:, valid]
    nwh, nww = fh // 5, fw // 9
    pid = torch.arange(1, nwh * nww + 1, dtype=torch.float32).view(1, 1, nwh, nww)
    un = torch.nn.functional.unfold(pid, kernel_size=(5, 9), padding=(2, 4)).view(45, nwh * nww).t()   # 0 = padded slot
    return own.long(), rolled.long(), un.long()


@pytest.mark.parametrize("fh,fw", [(5, 9), (10, 18), (20, 36), (15, 45), (60, 108)])
def test_key_table_matches_reference_enumeration(fh, fw):
    from e2fgvi_amd.engine import build_key_table
    from e2fgvi_amd.synth import rolled_valid_index
    from oracle import e2fgvi_oracle as O
    assert torch.equal(rolled_valid_index(), O.rolled_valid_index())
    tab, nk = build_key_table(fh, fw, rolled_valid_index().tolist())
    own, rolled, un = _reference_key_ids(fh, fw)
    for w in range(tab.shape[0]):
        refs = tab[w, :nk[w]].tolist()
        toks = sorted(r for r in refs if r >= 0)
        pooled = sorted(-(r + 1) for r in refs if r < 0)
        assert toks == sorted(own[w].tolist() + rolled[w].tolist())          # multiset: duplicates must match
        assert pooled == sorted((un[w][un[w] > 0] - 1).tolist())
        assert nk[w] == 165 + int((un[w] > 0).sum())
    if fh >= 10 and fw >= 18:
        # the famous 12 duplicates among the 120 ring keys (SURVEY.md 8a trap 6)
        assert len(set(rolled[0].tolist())) == 108


def test_abi_exports_every_declared_symbol():
    """the C-ABI library loads without a GPU and exports exactly what include/e2fgvi_hip.h declares"""
    from e2fgvi_amd import lib
    hdr = open(os.path.join(ROOT, "include", "e2fgvi_hip.h")).read()
    declared = set(re.findall(r"\b(e2fgvi_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.SYMBOLS), declared ^ set(lib.SYMBOLS)
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in declared:
        assert hasattr(so, name), name
    assert lib.load().e2fgvi_abi_version() == 9


def test_packing_size_functions_and_argument_checks_run_without_a_gpu():
    """host side of the C ABI: packed-weight sizes of the round-2 layouts and the error path (no launches involved)"""
    from e2fgvi_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built yet (python -m e2fgvi_amd.build)")
    L = lib.load()
    # tap-packed K-steps: (tap, 8-channel chunk) pairs cut into steps of 8 chunks of 64 x Npad elements
    def taps_size(mode, cout, kh, kw, cin):
        return L.e2fgvi_packed_conv_weight_x_size(mode, 1, cout, 1, kh, kw, 1, (ctypes.c_int32 * 1)(cin))
    assert taps_size(lib.DT_BF16, 512, 7, 7, 40) == 31 * 64 * 512       # FFN fc2 as a conv: 49 * 5 / 8 -> 31 steps
    assert taps_size(lib.DT_BF16, 32, 7, 7, 8) == 7 * 64 * 32           # SPyNet .0: 8 taps per step
    assert taps_size(lib.DT_BF16, 64, 3, 3, 24) == 4 * 64 * 64          # 9 taps x 3 chunks -> 4 steps
    assert taps_size(lib.DT_F32, 512, 7, 7, 40) == 62 * 32 * 512        # fp32: chunks of 4 channels, steps of 32
    assert taps_size(lib.DT_BF16, 64, 3, 3, 64) < 0                      # a full K-step per tap: nothing to pack
    assert taps_size(lib.DT_BF16, 64, 1, 1, 16) < 0                      # one tap
    assert b"56" in L.e2fgvi_last_error()
    # decoder tail: only 64 -> 3 is built
    assert L.e2fgvi_packed_tail_weight_size(3, 64) == 64 * 32
    assert L.e2fgvi_packed_tail_weight_size(4, 64) < 0
    assert b"64 -> 3" in L.e2fgvi_last_error()
    # wide-tile Winograd: (fy + 2) * 6 positions, channels in chunks of 8, couts padded to 32
    arr = (ctypes.c_int32 * 1)(128)
    n2 = L.e2fgvi_packed_winograd4_weight_size(256, 1, 1, arr, 2)
    assert n2 == 24 * 128 * 256
    assert L.e2fgvi_packed_winograd4_weight_size(256, 1, 1, arr, 3) < 0
    assert L.e2fgvi_packed_winograd4_weight_size(256, 1, 1, arr, 4) < 0            # F(4x4): pruned in round 6


def test_desc_struct_sizes_are_plain_c():
    from e2fgvi_amd import lib
    # pointers 8 bytes, int32 fields: sizes must be multiples of 8 and stable
    assert ctypes.sizeof(lib.ConvDesc) % 8 == 0 and ctypes.sizeof(lib.MdcnDesc) % 8 == 0 and ctypes.sizeof(lib.ConvXDesc) % 8 == 0


def test_missing_library_fails_loudly(monkeypatch):
    from e2fgvi_amd import lib
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", "/nonexistent/libe2fgvi_hip.so")
    with pytest.raises(lib.HipLibraryMissing):
        lib.load()


def test_shard_range_partitions():
    from e2fgvi_amd.runner import shard_range
    for n in (1, 7, 8, 64, 65):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1


def test_flops_formula_matches_survey():
    """bench.flops_per_clip == the evaluated figures of SURVEY.md 8(d) (GMAC x 2) for every BASELINE config"""
    import bench
    assert abs(bench.flops_per_clip(240, 432, 10, 10, False) - 2039.1) < 0.5
    assert abs(bench.flops_per_clip(240, 432, 5, 5, False) - 932.5) < 0.5
    assert abs(bench.flops_per_clip(240, 432, 10, 5, False) - 2 * 859.4) < 0.5
    assert abs(bench.flops_per_clip(720, 1296, 10, 10, True) - 2 * 9226.7) < 2
    assert abs(bench.flops_per_clip(1080, 1944, 20, 20, True) - 2 * 46980.8) < 10


def test_token_grid():
    from e2fgvi_amd.engine import token_grid
    assert token_grid(60, 108) == (20, 36) and token_grid(180, 324) == (60, 108) and token_grid(270, 486) == (90, 162)


def test_init_weights_variants_and_inference_only_guards():
    """model/e2fgvi.py:29-68: every init_type of the reference; DCN main weight untouched, conv_offset[-1] zero after
    construction; the module is inference-only and says so."""
    import importlib
    import pytest
    mod = importlib.import_module("model.e2fgvi_hq")
    net = mod.InpaintGenerator()
    dcn_w = net.feat_prop_module.deform_align["forward_"].weight.clone()
    assert float(net.feat_prop_module.deform_align["forward_"].conv_offset[-1].weight.abs().max()) == 0.0
    w = net.encoder.layers[4].weight                       # [128, 64, 3, 3]
    for kind, std in (("normal", 0.02), ("kaiming", (2.0 / (64 * 9)) ** 0.5), ("xavier", 0.02 * (2.0 / ((64 + 128) * 9)) ** 0.5)):
        net.init_weights(kind)
        assert abs(float(w.std()) / std - 1) < 0.05, kind
        assert float(net.encoder.layers[4].bias.abs().max()) == 0.0
    net.init_weights("xavier_uniform")
    bound = (6.0 / ((64 + 128) * 9)) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    net.init_weights("none")
    net.ss.embedding.weight.data.zero_()
    net.init_weights("orthogonal", gain=1.0)
    q = net.transformer[0].attn.proj.weight                # square: orthogonal up to the gain
    assert torch.allclose(q @ q.t(), torch.eye(512), atol=1e-4)
    assert torch.equal(net.feat_prop_module.deform_align["forward_"].weight, dcn_w)
    with pytest.raises(NotImplementedError):
        net.init_weights("bogus")
    with pytest.warns(UserWarning):                        # generic tooling may call .train(): the inference module stays in eval mode
        assert net.train() is net
    assert not net.training and all(not m.training for m in net.modules())
    assert net.train(True) is net and not net.training     # ... and says so only once
    assert net.eval() is net and not net.training
    with pytest.raises(NotImplementedError):
        mod.Discriminator()
    with pytest.raises(NotImplementedError):
        mod.spectral_norm(torch.nn.Conv2d(1, 1, 1))


def test_engine_cache_is_dropped_when_parameters_can_change():
    import importlib
    net = importlib.import_module("model.e2fgvi_hq").InpaintGenerator()
    sentinel = object()
    for change in (lambda: net.load_state_dict(net.state_dict()), lambda: net.init_weights(), lambda: net.float(),
                   lambda: net.refresh_engine()):
        net._engine, net._engine_key = sentinel, "k"
        change()
        assert net._engine is None and net._engine_key is None
    a = net._fingerprint()
    net.decoder[6].weight.data = net.decoder[6].weight.data.clone()          # a .data swap far down the parameter list
    assert net._fingerprint() != a


def _loop_isa(count_in_tail, n_wait):
    """a loop: head wait (marked), 2 loads, marked wait vmcnt(2), `count_in_tail` loads, back edge"""
    ins, a = [], 0x100

    def add(mn, ops=""):
        nonlocal a
        ins.append((a, mn, ops))
        a += 4
    add("s_waitcnt", "vmcnt(%d)" % n_wait); add("s_waitcnt", "vmcnt(%d)" % n_wait)        # marked wait A (claims over the back edge)
    add("v_mfma_f32_32x32x2_f32", "v[0:15], v1, v2, v[0:15]")
    add("buffer_load_dwordx4", "v[4:7], v3, s[0:3], 0 offen"); add("buffer_load_dwordx4", "v[8:11], v3, s[0:3], 0 offen")
    add("s_waitcnt", "vmcnt(2)"); add("s_waitcnt", "vmcnt(2)")                            # marked wait B: 2 loads since A
    add("s_waitcnt", "vmcnt(0)")                                                           # a compiler wait: not marked
    for _ in range(count_in_tail):
        add("buffer_load_dwordx4", "v[12:15], v3, s[4:7], 0 offen")
    back = (0x100 - (a + 4)) // 4 + 65536                                                 # as objdump prints simm16
    add("s_cbranch_scc1", str(back))
    return ins


def test_winograd_explicit_waits_are_checked_against_the_disassembly():
    """the Winograd kernels' explicit s_waitcnt vmcnt(N) counts compiler-emitted loads.  build.verify_wino_waits
    re-derives every N from the generated code at build time; here: the checker on a synthetic loop (right and wrong
    counts) and on the objects of this build."""
    from e2fgvi_amd import build
    assert build.check_kernel_waits("x.o", "k", _loop_isa(3, 3)) == 1
    with pytest.raises(RuntimeError):
        build.check_kernel_waits("x.o", "k", _loop_isa(4, 3))      # the compiler added a load in the loop
    with pytest.raises(RuntimeError):
        build.check_kernel_waits("x.o", "k", _loop_isa(2, 3))      # ... or removed one: the wait would under-wait
    import os
    if os.path.exists(build.OBJDUMP) and os.path.exists(os.path.join(build.CSRC, "build", "conv_wino.o")):
        assert build.verify_wino_waits() >= 32 + 28                 # 4 F(2x2) kernels x 8 wave roles + the wide-tile kernels


def test_kernel_table_invariants_and_nearest_size_class_lookup(monkeypatch):
    """deterministic kernel selection (ops._decision, e2fgvi_amd/tile_table.py): the table is in the format ops reads; no key
    carries round 4's `alone` suffix any more (the wide-tile kernel is a candidate everywhere since DESIGN.md C4 is closed); a size
    class the table does not hold takes the decision of the nearest class of the same geometry, a geometry it does not hold at all
    none"""
    from e2fgvi_amd import ops, tile_table
    assert tile_table.TABLE_FORMAT == ops.TABLE_FORMAT and len(tile_table.TILES) > 100
    wide = ops.W3_BASE + ops.W3_WIDE
    assert any(v == wide for v in tile_table.TILES.values())
    for k, v in tile_table.TILES.items():
        assert isinstance(k, tuple) and isinstance(k[ops._SIZE_FIELD], int) and isinstance(v, int)
        assert "alone" not in k, k
        # every code names a kernel the library instantiates (csrc/conv_bf16x.hip conv2d_x; csrc/conv_wino.hip wino_run; conv.hip)
        if k[0] == "x":
            assert v in (1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 16, 17, 18), (k, v)
        elif v >= ops.W3_BASE:
            assert v - ops.W3_BASE in ops.W3_CANDIDATES, (k, v)
        elif v >= ops.X3_BASE:
            assert v - ops.X3_BASE in ops.XTUNE_CANDIDATES, (k, v)
        elif 2000 <= v < 2100:
            assert v - 2000 in ops.XTUNE_CANDIDATES, (k, v)
    # round 5: the qkv Linear on the 256x192 tile, SPyNet layers and the propagation split's layers among the decisions
    # round 6: ... on the ping-pong form of that tile; no split-operand entry still names the one-barrier tiles 7 / 8 except the
    # tap-packed FFN convolution (the ping-pong loop does not take tap-packed weights)
    assert any(v == ops.X3_BASE + 108 for v in tile_table.TILES.values()) and any(v == ops.X3_BASE + 107 for v in tile_table.TILES.values())
    assert all(v not in (ops.X3_BASE + 7, ops.X3_BASE + 8) or (isinstance(k[0], str) and k[0].startswith("x32+")) for k, v in tile_table.TILES.items())
    assert any(k[0] != "x" and k[2] == 7 and v >= ops.X3_BASE for k, v in tile_table.TILES.items()), "no SPyNet layer on the split-operand GEMM"
    assert any(k[0] != "x" and k[1] == (128, 128, 4) for k in tile_table.TILES), "the recurrent part of conv_offset.0 is not tabled"
    if ops.AUTOTUNE:
        return
    monkeypatch.setattr(ops, "_TUNED", dict(tile_table.TILES))
    monkeypatch.setattr(ops, "_NEAREST", {})
    key = next(k for k in tile_table.TILES if k[0] != "x")
    assert ops._decision(key) == tile_table.TILES[key]
    same = sorted(k[ops._SIZE_FIELD] for k in tile_table.TILES
                  if len(k) == len(key) and k[:ops._SIZE_FIELD] == key[:ops._SIZE_FIELD] and k[ops._SIZE_FIELD + 1:] == key[ops._SIZE_FIELD + 1:])
    far = key[:ops._SIZE_FIELD] + (same[-1] + 3,) + key[ops._SIZE_FIELD + 1:]
    top = key[:ops._SIZE_FIELD] + (same[-1],) + key[ops._SIZE_FIELD + 1:]
    assert far not in tile_table.TILES and ops._decision(far) == tile_table.TILES[top]
    unknown = (7777,) + key[1:]
    assert ops._decision(unknown) is None


def _synthetic_k_loop(reuse, where="fallthrough", wait=True):
    """a toy kernel: K loop of 8 MFMAs that reloads its weight registers in place, then an epilogue.  reuse: the epilogue's
    arithmetic takes one of those registers BEFORE the post-loop wait -- directly behind the loop, behind an unconditional branch,
    or behind another wave role's exec-masked region (the layout hipcc gives `switch (wave)`)"""
    a, out = [0], []

    def emit(m, o=""):
        out.append([a[0], m, o])
        a[0] += 4
        return len(out) - 1

    def patch(i, target_index_addr):
        out[i][2] = str(((target_index_addr - (out[i][0] + 4)) // 4) & 0xFFFF)
    emit("s_mov_b32", "s0, 4")
    top = a[0]
    for _ in range(8):
        emit("v_mfma_f32_32x32x16_bf16", "v[0:15], v[100:103], v[40:43], v[0:15]")
    emit("buffer_load_dwordx4", "v[40:43], v200, s[8:11], s3 offen")
    emit("s_cmp_lg_u32", "s0, 0")
    patch(emit("s_cbranch_scc1"), top)
    bad = ("v_add_u32_e32", "v41, s2, v7")              # the epilogue's arithmetic in a register the load still targets
    if where == "fallthrough":
        if reuse:
            emit(*bad)
    elif where == "branch":
        br = emit("s_branch")
        emit("v_add_u32_e32", "v41, s2, v7")            # dead code in address order: never on the path
        emit("s_endpgm")
        patch(br, a[0])
        if reuse:
            emit(*bad)
    elif where == "role":
        # this role's `then` arm ends: flip to the `else` arm (no lane of this wave is in it), whose body is the next role:
        # its prologue loads the same registers and runs its own K loop.  The walk must pass over it and find the epilogue.
        emit("s_andn2_saveexec_b64", "s[4:5], s[4:5]")
        skip = emit("s_cbranch_execz")
        emit("buffer_load_dwordx4", "v[40:43], v200, s[8:11], s3 offen")
        emit("s_waitcnt", "vmcnt(0)")
        top2 = a[0]
        for _ in range(8):
            emit("v_mfma_f32_32x32x16_bf16", "v[0:15], v[100:103], v[40:43], v[0:15]")
        emit("buffer_load_dwordx4", "v[40:43], v200, s[8:11], s3 offen")
        patch(emit("s_cbranch_scc1"), top2)
        patch(skip, a[0])
        emit("s_or_b64", "exec, exec, s[4:5]")
        if reuse:
            emit(*bad)
    if wait:
        emit("s_waitcnt", "vmcnt(0)")
    emit("v_add_u32_e32", "v41, s2, v7" if wait else "v9, s2, v7")
    emit("s_endpgm")
    return [tuple(x) for x in out]


def test_registers_of_loads_in_flight_behind_the_k_loop_are_not_reused():
    """for hipcc an inline-asm load's destination is written when the statement ends; the Winograd kernels' weight
    loads for the stage past the end are still in flight when the K loop exits, and the compiler reused their registers for the
    epilogue's addresses above the kernels' own wait.  build.check_exit_reuse walks the control flow from every K-loop exit to the
    first vmcnt(0) (round 5: follows branches and carries the wave-uniform role regions, advisor finding of round 4): synthetic
    kernels here, the objects of this build, and -- below -- a build of the real source without the register claims."""
    from e2fgvi_amd import build
    for where in ("fallthrough", "branch", "role"):
        assert build.check_exit_reuse("x.o", "k", _synthetic_k_loop(False, where)) >= 1
        with pytest.raises(RuntimeError, match="touches a register"):
            build.check_exit_reuse("x.o", "k", _synthetic_k_loop(True, where))
        with pytest.raises(RuntimeError, match="without an s_waitcnt vmcnt"):
            build.check_exit_reuse("x.o", "k", _synthetic_k_loop(False, where, wait=False))
    if os.path.exists(build.OBJDUMP) and os.path.exists(os.path.join(build.CSRC, "build", "conv_wino_x3.o")):
        # every Winograd kernel of the three objects, 8 (or 4) wave roles each: 4 fp32 F(2x2) shapes, 3 + 1 + 1 split-operand kernels,
        # F(2x4) x 64 (round 6 pruned 5 instantiations: 76 exits, before 116)
        assert build.verify_exit_reuse() >= 76
    if os.path.exists(build.OBJDUMP) and os.path.exists(os.path.join(build.CSRC, "build", "conv_bf16x.o")):
        # round 6: the two ping-pong instantiations of the split-operand GEMM hold their accumulators in place: no private segment, no spills
        assert build.verify_no_scratch() == 2
        with pytest.raises(RuntimeError, match="no ping-pong instantiation"):
            build.verify_no_scratch(marker="ELb0ELi9ELb1EEE")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_exit_reuse_check_rejects_the_real_kernels_built_without_their_register_claims(tmp_path):
    """The regression fixture the advisor asked for: the split-operand Winograd unit compiled from the shipped source with the
    post-loop register claims defined away (-D'E2_CLAIM_AFTER_LOOP(r)=') is the pre-fix kernel of round 4 -- the check must raise
    on it (it does for all five register-staged kernels: hipcc hoists epilogue address arithmetic into the weight registers above
    the wait), and must pass on the same source built as shipped (test above)."""
    import subprocess
    from e2fgvi_amd import build
    obj = str(tmp_path / "conv_wino_x3_noclaim.o")
    subprocess.check_call([build._hipcc()] + build.FLAGS + build.NOPK + ["-DE2_WINO_X3=1", "-DE2_CLAIM_AFTER_LOOP(r)=", "-c",
                          os.path.join(build.CSRC, "conv_wino.hip"), "-o", obj], stderr=subprocess.DEVNULL)
    raised = {}
    for name, ins in build._kernels(build.device_isa(obj)).items():
        if "conv_wino" in name and "pack_" not in name:
            try:
                build.check_exit_reuse("noclaim", name, ins)
                raised[name] = False
            except RuntimeError as e:
                assert "touches a register of a weight load" in str(e)
                raised[name] = True
    wide = [n for n in raised if "conv_wino_x3w_kernel" in n]
    assert wide and all(raised[n] for n in wide), raised          # the kernel that failed on the chip in round 4
    assert sum(raised.values()) >= 3, raised


def test_sharded_step_without_graphs_ignores_in_flight_and_whole_propagation_restores_the_engine():
    """runner.ShardedStep(in_flight=K) needs HIP graphs: without them (CPU, use_graph=False) every run() is a plain forward;
    runner.whole_propagation switches an engine's propagation split off inside the context only, and tolerates nets without an engine"""
    import torch
    from e2fgvi_amd import runner

    class Eng:
        prop_split = {"backward_": 1}

    class Net:
        def __init__(self):
            self.eng, self.calls = Eng(), 0

        def engine(self):
            return self.eng

        def __call__(self, x, lt):
            self.calls += 1
            return x.reshape(-1, *x.shape[2:]) * (2.0 if self.eng.prop_split else 3.0), None

    net = Net()
    x = torch.ones(1, 2, 3, 4, 4)
    step = runner.ShardedStep(net, x, 2, in_flight=2, use_graph=False)
    outs = [step.run() for _ in range(3)]
    assert net.calls == 3 and all(o is not None and float(o.mean()) == 2.0 for o in outs) and float(step.finish().mean()) == 2.0
    with runner.whole_propagation(net):
        assert net.eng.prop_split == {} and float(net(x, 2)[0].mean()) == 3.0
    assert net.eng.prop_split == {"backward_": 1}
    with runner.whole_propagation(lambda x, lt: (x, None)):          # no engine: nothing to switch
        pass
