"""Build libe2fgvi_hip.so (gfx950) in-tree with hipcc.  ``python -m e2fgvi_amd.build``."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libe2fgvi_hip.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast"]
# No packed-fp32 VALU (v_pk_{mul,add,fma}_f32) in kernels that may run beside the bf16 MFMA tiles on another stream.
# Measured on MI355X (tools/probe/overlap_probe.hip, profiles/r02_overlap_probe_*.txt, DESIGN.md "Stream overlap"): a
# packed-fp32 instruction that consumes registers freshly written by vector-memory loads returns wrong values in lanes
# 48-63 when its wave shares a SIMD with a wave that streams 2x2 v_mfma_f32_32x32x16_bf16 tiles fed by ds_read_b128 --
# regardless of s_waitcnt / idle cycles / cache policy, never with scalar fp32 instructions on the same registers.
NOPK = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
# (source, object, extra flags).  The HBM-bound kernels lose nothing without packed math; the fp32 conv kernels keep it in
# their normal build (6-8 % on the MFMA kernels' transforms / epilogues, profiles/r02_c2_*) and get a second, packed-free
# build for the side-stream launches (SPyNet).  mdcn.hip: its sampler waves do arithmetic on freshly loaded offset / mask / flow
# words while the other waves of the SAME workgroup stream LDS-fed bf16 MFMA tiles -- with packed math the 64-row / two-K-group
# tile returned wrong rows 24-31 (lanes 48-63 of the sampler wave) in a few launches per hundred.
# attention_bf16.hip / conv_tail.hip (round 3, advisor): their fp32 VALU works on MFMA results and LDS data today, but both
# units hold bf16 MFMA streams, so they are kept free of packed fp32 as well (measured neutral) -- a later epilogue edit that
# touches VMEM-fresh registers then cannot re-enter the hazard silently; 200-launch bit-identity reruns in the GPU tests.
# conv_wino.o / conv_wino4.o (round 6, advisor): the fp32 Winograd kernels build their A operands with VALU adds on patch words and
# run wherever the kernel table (or a table miss, or E2FGVI_TILE_TABLE=0) names them -- encoder.layers.14 in front of the join
# beside SPyNet's split-operand GEMM, the propagation split's side-stream layers beside the main stream's split-operand deformable
# conv: they held 48-992 v_pk_{mul,add,fma}_f32 per kernel.  Both objects are built packed-free now and checked like the others.
UNITS = [("error.hip", "error.o", []), ("conv.hip", "conv.o", []), ("conv.hip", "conv_nopk.o", NOPK + ["-DE2_NOPK_VARIANT"]),
         ("conv_bf16x.hip", "conv_bf16x.o", NOPK), ("conv_wino.hip", "conv_wino.o", NOPK), ("conv_wino.hip", "conv_wino_x3.o", NOPK + ["-DE2_WINO_X3=1"]), ("conv_wino4.hip", "conv_wino4.o", NOPK), ("conv_tail.hip", "conv_tail.o", NOPK),
         ("mdcn.hip", "mdcn.o", NOPK), ("attention.hip", "attention.o", []),
         ("attention_bf16.hip", "attention_bf16.o", NOPK), ("attention_x3.hip", "attention_x3.o", NOPK), ("misc.hip", "misc.o", NOPK),
         ("video.hip", "video.o", NOPK), ("yuv.hip", "yuv.o", NOPK), ("metrics.hip", "metrics.o", NOPK),
         # fp64 in the order written: the numpy restatement matches the step bit for bit only without fused multiply-adds
         ("mask_track.hip", "mask_track.o", NOPK + ["-ffp-contract=off"]),
         ("defects.hip", "defects.o", NOPK),
         # the same: the restatement of tests/pixel_track_cases.py matches the origins bit for bit
         ("pixel_track.hip", "pixel_track.o", NOPK + ["-ffp-contract=off"]),
         ("grain.hip", "grain.o", NOPK),
         ("line_scratch.hip", "line_scratch.o", NOPK),
         ("flicker.hip", "flicker.o", NOPK),
         ("flicker_local.hip", "flicker_local.o", NOPK),
         ("color.hip", "color.o", NOPK),
         ("weave.hip", "weave.o", NOPK),
         ("interlace.hip", "interlace.o", NOPK),
         ("telecine.hip", "telecine.o", NOPK),
         ("denoise.hip", "denoise.o", NOPK),
         # the same: the restatement of tests/interpolate_cases.py matches the trajectories bit for bit
         ("interpolate.hip", "interpolate.o", NOPK + ["-ffp-contract=off"])]
NOPK_OBJECTS = tuple(obj for _, obj, extra in UNITS if "-packed-fp32-ops" in extra)
# Build-time checks of the generated code, object by object: (object, mangled-name marker of the kernels meant, what they are called
# in a message, whether its fp64 must be unfused).  Every kernel with the marker must be free of scratch -- no private segment, no
# spilled register (verify_no_scratch); an object whose fp64 arithmetic the tests restate bit for bit in numpy, one rounding per
# operation, is built with -ffp-contract=off and must hold no fused fp64 multiply-add (verify_no_fma64).
KERNEL_CHECKS = [
    # the ping-pong instantiations (template tail `false, 2, true`) keep 128 accumulator registers in place across four barriers per
    # K-step; two ways of writing that loop made hipcc spill 414 registers or copy the kernel arguments to scratch without a warning
    ("conv_bf16x.o", "ELb0ELi2ELb1EEE", "ping-pong", False),
    ("conv_bf16x.o", "conv_halo_x3_kernel", "split-operand halo", False),
    # four instantiations: the feathered ones hold five LDS phases in one kernel
    ("video.o", "restore_u8_kernel", "paste-back", False),
    # four: 24 sums and the next frame's 9 words in registers across the frame loop
    ("video.o", "overlay_stats_kernel", "overlay sums", False),
    # mask_track_step_kernel does its fp64 arithmetic in the order written; it has no scratch check
    ("mask_track.o", None, None, True),
    # four kernels: the candidate kernel unrolls up to 2 x 36 gathers for each of a thread's four pixels
    ("defects.o", "defect_", "dust and dirt", False),
    # two: the fill keeps the weights, offsets and flags of four corners in small arrays
    ("pixel_track.o", "pixel_", "pixel propagation", True),
    # two: the blocks pass keeps the 42 bytes of a thread's four Laplacians in small arrays
    ("grain.o", "grain_", "film grain", False),
    # four: the per-polarity counters of the columns pass are small arrays indexed in unrolled loops
    ("line_scratch.o", "line_", "line scratch", False),
    # three: the histogram and the apply kernel hold the dwords of all of a thread's groups at once
    ("flicker.o", "flicker_", "deflicker", False),
    # three: the same, and the apply kernel the four cell offsets and weights of a thread's pixels
    ("flicker_local.o", "flicker_local_", "local deflicker", False),
    # four: the histogram and the apply kernel hold the dwords of all of a thread's groups at once
    ("color.o", "color_", "colour restoration", False),
    # five: the apply kernel shifts the dwords of two tap rows into place in small arrays
    ("weave.o", "weave_", "weave stabiliser", False),
    # three: the fields kernel holds the dwords and the luma of up to twelve groups in small arrays
    ("interlace.o", "interlace_", "deinterlacer", False),
    # two: the scores kernel holds the 36 dwords of a row of three frames and the luma of four rows of 16 pixels
    ("telecine.o", "telecine_", "inverse telecine", False),
    # four: the filter kernel keeps the 7 x 5 three-byte runs of a neighbour's luma window in a small array
    ("denoise.o", "denoise_", "temporal denoiser", False),
    # one: two fp64 fixed-point searches and up to four colour taps for each of a thread's four pixels; its quotients k / d come from
    # a table so that no division is contracted
    ("interpolate.o", "interpolate_", "frame interpolation", True),
]
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return "hipcc"


def _stale(out, deps):
    return (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build(force=False, verbose=False, nopk_all=False, lib=None, tag=None, defines=()):
    """Compile every HIP source for gfx950 and link the shared library.  Returns its path.
    nopk_all: build every unit without packed-fp32 VALU (A/B measurements) into ``lib``.
    tag / defines: an A/B build with extra -D flags into csrc/build_<tag>/ and csrc/libe2fgvi_hip_<tag>.so (run it with
    E2FGVI_LIB=<that path>); the product library is the build without either."""
    hipcc = _hipcc()
    if tag:
        nopk_all = False
    objdir = os.path.join(CSRC, ("build_" + tag) if tag else ("build_nopk" if nopk_all else "build"))
    os.makedirs(objdir, exist_ok=True)
    out = lib or (os.path.join(CSRC, "libe2fgvi_hip_%s.so" % tag) if tag else
                  os.path.join(CSRC, "libe2fgvi_hip_nopk.so") if nopk_all else LIB)
    headers = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h"))
    headers += [os.path.join(HERE, "..", "include", "e2fgvi_hip.h"), os.path.abspath(__file__)]
    jobs = []
    for src, obj, extra in UNITS:
        sp, op = os.path.join(CSRC, src), os.path.join(objdir, obj)
        if nopk_all and not any(f == "-packed-fp32-ops" for f in extra):
            extra = extra + NOPK
        if force or _stale(op, [sp] + headers):
            jobs.append([hipcc] + FLAGS + extra + list(defines) + ["-c", sp, "-o", op])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(objdir, obj) for _, obj, _ in UNITS]
    if force or jobs or _stale(out, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs)
    if jobs:
        verify_isa(objdir)
        if not nopk_all:
            verify_wino_waits(objdir)
            verify_exit_reuse(objdir)
            for obj, marker, what, _ in KERNEL_CHECKS:
                if marker:
                    verify_no_scratch(objdir, obj, marker, what)
            verify_overlay_prefetch(objdir)
            verify_no_pk_u8(objdir)
            for obj, _, _, unfused in KERNEL_CHECKS:
                if unfused:
                    verify_no_fma64(objdir, obj)
    return out


def build_variant(tag, *defines):
    """python -c 'from e2fgvi_amd import build; build.build_variant("trunc", "-DE2_SPLIT_RNE=0")'"""
    return build(tag=tag, defines=defines)


def device_isa(obj):
    """Disassembly of the gfx950 code object embedded in a host object file."""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="e2isa")
    try:
        local = os.path.join(d, os.path.basename(obj))
        shutil.copy(obj, local)
        subprocess.run([OBJDUMP, "--offloading", os.path.basename(obj)], cwd=d, check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        dev = [f for f in os.listdir(d) if "gfx950" in f]
        if not dev:
            return ""
        return subprocess.run([OBJDUMP, "-d", os.path.join(d, dev[0])], check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(d, ignore_errors=True)


def verify_isa(objdir=None):
    """Build-time check of the generated code: the units that must be free of packed-fp32 VALU instructions are."""
    import re
    objdir = objdir or os.path.join(CSRC, "build")
    if not os.path.exists(OBJDUMP):
        return
    for obj in NOPK_OBJECTS:
        isa = device_isa(os.path.join(objdir, obj))
        bad = re.findall(r"v_pk_(?:mul|add|fma)_f32", isa)
        if bad or not isa:
            raise RuntimeError("%s: %s" % (obj, "%d packed-fp32 instructions in a unit that must have none" % len(bad) if isa
                                           else "no gfx950 code object found"))


def verify_no_fma64(objdir=None, obj="mask_track.o"):
    """mask_track_step_kernel (csrc/mask_track.hip) does its fp64 arithmetic in the order written, one rounding per operation: the
    numpy restatement of the tests matches it bit for bit (and so do the two kernels of csrc/pixel_track.hip, obj="pixel_track.o",
    and the kernel of csrc/interpolate.hip, obj="interpolate.o", which for that reason takes its quotients k / d from a table).  The unit is built with -ffp-contract=off; a fused multiply-add in its
    code would mean the flag was lost (or an expression was rewritten into fma()).  Returns the number of fp64 multiplies read."""
    import re
    objdir = objdir or os.path.join(CSRC, "build")
    if not os.path.exists(OBJDUMP):
        return 0
    isa = device_isa(os.path.join(objdir, obj))
    fused = re.findall(r"v_fma(?:c|ak|mk)?_f64", isa)
    if fused or not isa:
        raise RuntimeError("%s: %s" % (obj, "%d fused fp64 multiply-adds in a unit that must round every operation" % len(fused) if isa
                                       else "no gfx950 code object found"))
    return len(re.findall(r"v_mul_f64", isa))


def verify_no_pk_u8(objdir=None):
    """No unit may hold v_ashr_pk_u8_i32 / v_ashr_pk_i8_i32 (gfx950: shift two int32, clamp each to a byte, pack the pair into the
    low half of the destination).  hipcc forms it from two clipped shifts that are packed into one word with other bytes and ORs
    those bytes on top of the result; on the chip the bytes ORed on top came out wrong in csrc/yuv.hip's decoder (csrc/frame_bytes.h
    fb_byte has the account and the empty asm that keeps the pattern from forming).  Returns the number of objects read."""
    import re
    objdir = objdir or os.path.join(CSRC, "build")
    if not os.path.exists(OBJDUMP):
        return 0
    for _, obj, _ in UNITS:
        found = re.findall(r"v_ashr_pk_[ui]8_i32", device_isa(os.path.join(objdir, obj)))
        if found:
            raise RuntimeError("%s: %d v_ashr_pk_u8_i32 / v_ashr_pk_i8_i32 instructions: the bytes packed beside their result come out "
                               "wrong on the chip (csrc/frame_bytes.h fb_byte)" % (obj, len(found)))
    return len(UNITS)


def verify_no_scratch(objdir=None, obj="conv_bf16x.o", marker="ELb0ELi2ELb1EEE", what="ping-pong"):
    """Fails the build when a kernel of ``obj`` whose mangled name holds ``marker`` has a private segment or a spilled register:
    hipcc spills, or copies kernel arguments to scratch, without a warning.  KERNEL_CHECKS lists the objects this runs over on every
    build and why each is there.  Returns the number of kernels read; none found is an error too."""
    import re
    import shutil
    import tempfile
    objdir = objdir or os.path.join(CSRC, "build")
    readelf = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
    if not (os.path.exists(OBJDUMP) and os.path.exists(readelf)):
        return 0
    d = tempfile.mkdtemp(prefix="e2elf")
    try:
        shutil.copy(os.path.join(objdir, obj), os.path.join(d, obj))
        subprocess.run([OBJDUMP, "--offloading", obj], cwd=d, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        dev = [f for f in os.listdir(d) if "gfx950" in f]
        notes = subprocess.run([readelf, "--notes", os.path.join(d, dev[0])], check=True, capture_output=True, text=True).stdout if dev else ""
    finally:
        shutil.rmtree(d, ignore_errors=True)
    found = 0
    for block in notes.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or marker not in name.group(1):
            continue
        found += 1
        priv = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        if priv or spill:
            raise RuntimeError("%s: %s: private segment %d bytes, %d spilled VGPRs in a %s kernel" % (obj, name.group(1)[:70], priv, spill, what))
    if not found:
        raise RuntimeError("verify_no_scratch: no %s instantiation found in %s (mangled-name marker changed?)" % (what, obj))
    return found


def _kernels(isa):
    """{kernel name: [(address, mnemonic, operand text)]} of a disassembly"""
    import re
    out, cur = {}, None
    for line in isa.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return out


def check_kernel_waits(obj, name, ins):
    """One kernel's instruction list [(address, mnemonic, operands)]: every marked explicit wait inside a loop must carry
    the number of vector-memory instructions issued since the previous marked wait (cyclically over the back edge).
    Returns the number of loops checked; raises RuntimeError on a mismatch."""
    import re
    vmem = re.compile(r"^(buffer|global|flat|scratch)_(load|store|atomic)")
    marks = [i for i in range(len(ins) - 1) if ins[i][1] == "s_waitcnt" and ins[i + 1][1] == "s_waitcnt"
             and ins[i][2] == ins[i + 1][2] and "vmcnt" in ins[i][2]]
    if not marks:
        return 0
    addr_to_idx = {a: i for i, (a, _, _) in enumerate(ins)}
    spans = []
    for i, (a, mn, ops_) in enumerate(ins):
        if mn.startswith("s_cbranch") or mn == "s_branch":
            # objdump prints the target as the unsigned 16-bit word offset from the next instruction
            try:
                off = int(ops_.split()[0])
            except (ValueError, IndexError):
                continue
            if off >= 32768:
                off -= 65536
            tgt = a + 4 + 4 * off
            if off < 0 and tgt in addr_to_idx:
                spans.append((addr_to_idx[tgt], i))
    loops = 0
    # a kernel that opts in to another wait discipline, by (mangled) name: conv_wino_x3w_kernel reloads its single-buffered weight
    # planes in place and claims them group by group (below).  (Round 3's two-trips-ahead LDS-DMA variant of conv_wino_kernel and
    # its rule left with the kernel in round 6.)
    rolling = "conv_wino_x3w_kernel" in name
    for lo, hi in spans:
        inner = [m for m in marks if lo <= m <= hi]
        if not inner or any(lo <= l2 and h2 <= hi and (l2, h2) != (lo, hi) and any(l2 <= m <= h2 for m in inner)
                            for l2, h2 in spans):
            continue                                   # no marked wait, or an inner loop owns them
        loops += 1
        if rolling:
            # The plane loads of the next stage are the LAST vector-memory instructions of a trip, G per position; the next
            # trip claims them position by position with vmcnt(n_0 = (P - 1) G), ..., vmcnt(0), nothing issued in between.
            counts = [int(re.search(r"vmcnt\((\d+)\)", ins[m][2]).group(1)) for m in inner]
            for a, b in zip(inner, inner[1:]):
                if any(vmem.match(ins[k][1]) for k in range(a + 2, b)):
                    raise RuntimeError("%s: %s: vector-memory instruction between the group waits at 0x%x and 0x%x"
                                       % (obj, name[:60], ins[a][0], ins[b][0]))
            g = counts[0] - counts[1] if len(counts) > 1 else counts[0]
            if counts[-1] != 0 or g <= 0 or any(c != counts[0] - j * g for j, c in enumerate(counts)):
                raise RuntimeError("%s: %s: group waits %s are not (P-1) G, ..., G, 0" % (obj, name[:60], counts))
            tail = [k for k in list(range(inner[-1] + 2, hi + 1)) + list(range(lo, inner[0])) if vmem.match(ins[k][1])]
            planes = tail[-(counts[0] + g):]
            if len(planes) != counts[0] + g or any(ins[k][1] != "buffer_load_dwordx4" or " lds" in ins[k][2] for k in planes):
                raise RuntimeError("%s: %s: the %d vector-memory instructions in front of the group waits are not the plane "
                                   "loads" % (obj, name[:60], counts[0] + g))
            continue
        for j, m in enumerate(inner):
            n = int(re.search(r"vmcnt\((\d+)\)", ins[m][2]).group(1))
            if j:
                rng = range(inner[j - 1] + 2, m)
            else:                                       # over the back edge: tail of the loop + its head
                rng = list(range(inner[-1] + 2, hi + 1)) + list(range(lo, m))
            cnt = sum(1 for k in rng if vmem.match(ins[k][1]))
            if cnt != n:
                raise RuntimeError("%s: %s: explicit s_waitcnt vmcnt(%d) at 0x%x follows %d vector-memory instructions "
                                   "since the previous explicit wait" % (obj, name[:60], n, ins[m][0], cnt))
    return loops


def verify_wino_waits(objdir=None, objects=("conv_wino.o", "conv_wino_x3.o", "conv_wino4.o")):
    """The Winograd kernels issue their weight loads through pinned inline asm and wait for them with an explicit
    ``s_waitcnt vmcnt(N)`` whose N is the number of vector-memory instructions issued since (conv_wino.hip): a count the
    compiler does not maintain.  This check re-derives it from the generated code on every build.  The explicit waits are
    marked by being issued twice in a row; in every K loop (a backward branch around marked waits) the wait that follows
    another must carry exactly the number of VMEM instructions between the two -- cyclically over the loop's back edge --
    because the loads a wait claims were issued immediately before the previous marked wait.  Raises on a mismatch
    (a compiler that adds, removes or moves a load in the loop), returns the number of loops checked."""
    objdir = objdir or os.path.join(CSRC, "build")
    if not os.path.exists(OBJDUMP):
        return 0
    loops = 0
    for obj in objects:
        for name, ins in _kernels(device_isa(os.path.join(objdir, obj))).items():
            loops += check_kernel_waits(obj, name, ins)
    if not loops:
        raise RuntimeError("verify_wino_waits: no K loop with marked waits found (disassembly format changed?)")
    return loops


def verify_overlay_prefetch(objdir=None, obj="video.o", items=3):
    """overlay_stats_kernel (csrc/video.hip) asks for the next frame's bytes in front of its one barrier per frame and uses them
    only at the top of the next trip: the loads must be in flight across the barrier and the sums behind it.  Written with the
    loads inside divergent branches, hipcc waited for every one of them on the spot (``s_waitcnt vmcnt(0)`` behind each load, in
    front of the barrier) without a word.  For the two instantiations that load four pixels at once (template tail `false`) this
    check finds the frame loop -- the innermost backward branch around the ``s_barrier`` and the loads -- and requires that its
    ``global_load_dwordx3`` are OV_ITEMS = 3, that the path from the first of them over the back edge to the barrier holds no other
    branch, and that no ``s_waitcnt`` on that path names vmcnt.  Returns the number of kernels checked; raises RuntimeError."""
    objdir = objdir or os.path.join(CSRC, "build")
    if not os.path.exists(OBJDUMP):
        return 0
    found = 0
    for name, ins in _kernels(device_isa(os.path.join(objdir, obj))).items():
        if "overlay_stats_kernel" not in name or "ELb0EEE" not in name:
            continue
        found += 1
        what = "%s: %s" % (obj, name[:70])
        addr_to_idx = {a: i for i, (a, _, _) in enumerate(ins)}
        bars = [i for i, (_, mn, _) in enumerate(ins) if mn == "s_barrier"]
        if len(bars) != 1:
            raise RuntimeError("%s: %d barriers where the frame loop has one" % (what, len(bars)))
        bar, spans = bars[0], []
        for i, (a, mn, ops_) in enumerate(ins):
            if mn.startswith("s_cbranch") or mn == "s_branch":
                off = int(ops_.split()[0])                 # unsigned 16-bit word offset from the next instruction
                tgt = addr_to_idx.get(a + 4 + 4 * (off - 65536 if off >= 32768 else off))
                # the last frame of a chunk goes back to the barrier without loads: that back edge is not the one looked for
                if tgt is not None and tgt <= bar <= i and any(ins[k][1] == "global_load_dwordx3" for k in range(tgt, i + 1)):
                    spans.append((i - tgt, tgt, i))
        if not spans:
            raise RuntimeError("%s: no backward branch around the barrier (disassembly format changed?)" % what)
        _, lo, hi = min(spans)
        loads = [i for i in range(lo, hi + 1) if ins[i][1] == "global_load_dwordx3"]
        if len(loads) != items or loads[0] < bar:
            raise RuntimeError("%s: %d global_load_dwordx3 in the frame loop, the first %s the barrier; expected %d behind it"
                               % (what, len(loads), "in front of" if loads and loads[0] < bar else "behind", items))
        path = ins[loads[0]:hi] + ins[lo:bar]
        for a, mn, ops_ in path:
            if mn.startswith("s_cbranch") or mn == "s_branch" or mn == "s_endpgm":
                raise RuntimeError("%s: a branch at 0x%x between the frame loop's loads and its barrier" % (what, a))
            if mn == "s_waitcnt" and "vmcnt" in ops_:
                raise RuntimeError("%s: s_waitcnt %s at 0x%x waits for the next frame's loads in front of the barrier" % (what, ops_, a))
    if found != 2:
        raise RuntimeError("verify_overlay_prefetch: %d instantiations of overlay_stats_kernel<., false> in %s, expected 2" % (found, obj))
    return found


def _vregs(text):
    """vector registers named in an operand text"""
    import re
    r = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]", text):
        r.update(range(int(m.group(1)), int(m.group(2)) + 1))
    for m in re.finditer(r"\bv(\d+)\b", text):
        r.add(int(m.group(1)))
    return r


def _successors(ins, at):
    """control-flow successors (instruction indices) of every instruction of a kernel; objdump prints a branch target as the
    unsigned 16-bit word offset from the next instruction.  Raises on an indirect jump (nothing here has one)."""
    succ = []
    for i, (a, m, o) in enumerate(ins):
        if m in ("s_endpgm", "s_endpgm_saved"):
            succ.append(())
        elif m == "s_branch" or m.startswith("s_cbranch"):
            off = int(o.split()[0])
            off -= 65536 if off > 32767 else 0
            tgt = at.get(a + 4 + 4 * off)
            if tgt is None:
                raise RuntimeError("branch at 0x%x leaves the kernel" % a)
            succ.append((tgt,) if m == "s_branch" else (tgt, i + 1))
        elif m.startswith("s_setpc") or m.startswith("s_swappc"):
            raise RuntimeError("indirect jump at 0x%x: control flow cannot be followed" % a)
        else:
            succ.append((i + 1,) if i + 1 < len(ins) else ())
    return succ


def check_exit_reuse(obj, name, ins, min_mfma=8):
    """For hipcc the destination of an inline-asm load is written when the statement ends.  The weight loads a K loop issues for
    the stage PAST the end are still in flight when the loop exits; if the compiler reuses their registers (it did: for the
    epilogue's address arithmetic, hoisted above the kernel's own `s_waitcnt vmcnt(0)`) the late data lands on top of the new values
    whenever memory is slow -- DESIGN.md C4.  The sources name those registers behind a post-loop wait; this check re-derives from
    the disassembly that it worked:

      * weight registers = destinations of non-LDS buffer loads that feed an MFMA's B operand anywhere in the kernel;
      * K loops = the strongly connected components of the control-flow graph that hold >= min_mfma MFMAs;
      * from every control-flow edge that LEAVES such a span the walk follows the code -- unconditional branches, both arms of
        conditional ones -- until the first wait that contains vmcnt(0) on each path; any vector instruction on the way that
        reads or writes a weight register is an error, and so is reaching s_endpgm (or another K loop) without that wait;
      * the wave roles of these kernels (`switch (wave)`, wave = threadIdx.x >> 6) are compiled as exec-masked if / else regions
        although every lane of a wave takes the same arm.  The walk carries that fact: passing the flip to an `else` arm
        (s_andn2_saveexec_b64, or the s_xor_b64 exec, exec, ... that follows an s_or_saveexec_b64) with live lanes leaves none (the wave took the `then` arm with
        all its lanes), until the region's end restores the mask (s_or_b64 exec, exec, ...); with no live lane vector instructions
        do nothing, s_cbranch_execz is taken and s_cbranch_execnz is not.  Without this the walk would run from one role's loop
        exit straight into the next role's prologue (the round-4 version of this check stopped there, at that prologue's wait,
        and could pass without having seen the shared epilogue).

    Returns the number of exit edges walked; raises RuntimeError on a violation."""
    import re
    at = {a: i for i, (a, _, _) in enumerate(ins)}
    succ = _successors(ins, at)
    is_mfma = [("mfma" in m) for _, m, _ in ins]
    breg = set()
    for (_, m, o), f in zip(ins, is_mfma):
        if f:
            breg |= _vregs([x.strip() for x in o.split(",")][2])
    wregs = set()
    for _, m, o in ins:
        if re.match(r"buffer_load_dword", m) and not o.rstrip().endswith(" lds"):
            d = _vregs(o.split(",")[0])
            if d & breg:
                wregs |= d
    if not wregs:
        return 0
    # K loops: the strongly connected components of the control-flow graph that hold >= min_mfma MFMAs (Tarjan, iterative).  Address
    # ranges of backward branches would not do: block placement puts parts of the epilogue in front of the loops.
    n = len(ins)
    index, low, comp = [-1] * n, [0] * n, [-1] * n
    stack, onstack, counter, ncomp = [], [False] * n, 0, 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, pi = work.pop()
            if pi == 0:
                index[v] = low[v] = counter
                counter += 1
                stack.append(v)
                onstack[v] = True
            recurse = False
            for j in range(pi, len(succ[v])):
                w = succ[v][j]
                if index[w] < 0:
                    work.append((v, j + 1))
                    work.append((w, 0))
                    recurse = True
                    break
                if onstack[w]:
                    low[v] = min(low[v], index[w])
            if recurse:
                continue
            if low[v] == index[v]:
                while True:
                    w = stack.pop()
                    onstack[w] = False
                    comp[w] = ncomp
                    if w == v:
                        break
                ncomp += 1
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    members = {}
    for k in range(n):
        members.setdefault(comp[k], []).append(k)
    loops = [m for m in members.values() if len(m) > 1 and sum(1 for k in m if is_mfma[k]) >= min_mfma]
    inside = [False] * n
    for m in loops:
        for k in m:
            inside[k] = True
    edges = 0
    for m in loops:
        mine = set(m)
        starts = set()
        for k in m:
            for t in succ[k]:
                if t not in mine:
                    starts.add(t)
        for st in sorted(starts):
            edges += 1
            seen, todo = set(), [(st, False)]
            while todo:
                k, dead = todo.pop()                 # dead: no live lane (the wave is passing over another role's region)
                if (k, dead) in seen:
                    continue
                seen.add((k, dead))
                a, m, o = ins[k]
                if m == "s_waitcnt" and "vmcnt(0)" in o:
                    continue
                if m.startswith("s_endpgm") or (inside[k] and not dead):
                    raise RuntimeError("%s: %s: the path from the K-loop exit at 0x%x reaches 0x%x (%s) without an s_waitcnt vmcnt(0): "
                                       "weight loads may still be in flight" % (obj, name[:60], ins[st][0], a,
                                                                                "another K loop" if inside[k] else m))
                if not dead and not m.startswith("s_") and _vregs(o) & wregs:
                    raise RuntimeError("%s: %s: 0x%x %s %s touches a register of a weight load that may still be in flight behind the "
                                       "K loop left at 0x%x (no vmcnt(0) yet)" % (obj, name[:60], a, m, o, ins[st][0]))
                flip = m == "s_andn2_saveexec_b64" or (m == "s_xor_b64" and o.startswith("exec"))
                if flip and not dead:
                    dead = True
                elif m in ("s_or_b64", "s_mov_b64") and o.startswith("exec"):
                    dead = False
                nxt = succ[k]
                if dead and m == "s_cbranch_execz":
                    nxt = nxt[:1]
                elif dead and m == "s_cbranch_execnz":
                    nxt = nxt[1:]
                todo.extend((t, dead) for t in nxt)
    return edges


EXIT_REUSE_OBJECTS = ("conv_wino.o", "conv_wino_x3.o", "conv_wino4.o")


def verify_exit_reuse(objdir=None, objects=EXIT_REUSE_OBJECTS):
    """check_exit_reuse over every Winograd kernel of the library (all of them prefetch their weights past the end of the K loop
    through inline asm); returns the number of K-loop exit edges walked"""
    objdir = objdir or os.path.join(CSRC, "build")
    if not os.path.exists(OBJDUMP):
        return 0
    n = 0
    for obj in objects:
        for name, ins in _kernels(device_isa(os.path.join(objdir, obj))).items():
            if "conv_wino" not in name or "pack_" in name:
                continue
            k = check_exit_reuse(obj, name, ins)
            if not k:
                raise RuntimeError("verify_exit_reuse: no K-loop exit found in %s: %s (disassembly format changed?)" % (obj, name[:60]))
            n += k
    if not n:
        raise RuntimeError("verify_exit_reuse: no Winograd kernel found")
    return n


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, nopk_all="--nopk-all" in sys.argv))
