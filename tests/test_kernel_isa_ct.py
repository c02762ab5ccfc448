"""k_msm_fixed_ct in the gfx950 code object that build() cross-compiled (same fixture style as tests/test_kernel_isa.py).

What this shows: the kernel is there, does not spill, has the LDS and VGPR figures DESIGN.md 9 states, and has the instruction forms
of the scalar-register design - NO vector load from the table: its only global loads are a term's scalar (two dwordx4 at an address
given by the proof index); the table arrives through scalar loads, whose addresses live in scalar registers and are wave-uniform by
construction of the hardware; the only execution-mask branch is the ragged batch's `b < B`; LDS traffic is the digit column only.
What it cannot show: that the scalar addresses and the uniform branches are functions of public values - a scalar register could
still hold something read back from a secret (v_readfirstlane).  That is the trace test's business
(tests/test_secret_independent.py: the same body under the simulator's recorder, two batches with different secrets).

And k_msm_fixed2 is untouched: the hash of its instructions is the one of the commit before this kernel existed."""
import collections
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bulletproofs-r1cs-gadgets_amd", "csrc", "libbpr1cs_hip.so")

# tools/kernel_isa_stats.py --hash k_msm_fixed2 on a build of the parent commit (data, not a measurement of this tree)
K_MSM_FIXED2_PARENT_HASH = "79525bf77097da0a"
# DESIGN.md 9
CT_LDS_BYTES = 8192
CT_VGPRS = 102


@pytest.fixture(scope="module")
def ct_kernel():
    import subprocess
    import tempfile
    import kernel_isa_stats as K
    if not os.path.exists(LIB):
        pytest.skip("libbpr1cs_hip.so is not built (run __graft_entry__.build())")
    if not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(K.code_object(LIB, "k_msm_fixed_ct"))
        co = f.name
    try:
        syms = subprocess.run([K.LLVM + "/llvm-readelf", "-sW", co], capture_output=True, text=True).stdout
        notes = subprocess.run([K.LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
        names = sorted(set(l.split()[-1] for l in syms.split("\n") if " FUNC " in l and "k_msm_fixed_ct" in l))
        assert len(names) == 1, "k_msm_fixed_ct is not in the code object: %r" % names
        name = names[0]
        blk = next((e for e in notes.split("\n  - ") if (".name:           " + name + "\n") in e + "\n"), "")
        meta = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", blk)}
        dis = subprocess.run([K.LLVM + "/llvm-objdump", "-d", "--disassemble-symbols=" + name, co], capture_output=True, text=True).stdout
        ins = [l.split("//")[0].strip() for l in dis.split("\n") if l.startswith("\t") and l.split()]
        return meta, ins
    finally:
        os.unlink(co)


def test_ct_kernel_resources(ct_kernel):
    meta, ins = ct_kernel
    assert meta["private_segment_fixed_size"] == 0, "k_msm_fixed_ct spills to scratch"
    assert not any(t.startswith("scratch_") for t in ins)
    assert meta["group_segment_fixed_size"] == CT_LDS_BYTES
    assert meta["vgpr_count"] == CT_VGPRS, "DESIGN.md 9 states %d VGPRs, the build has %d" % (CT_VGPRS, meta["vgpr_count"])
    assert meta["vgpr_count"] <= 168   # three wavefronts per SIMD


def test_ct_kernel_has_no_vector_load_from_the_table(ct_kernel):
    meta, ins = ct_kernel
    c = collections.Counter(t.split()[0] for t in ins)
    vloads = [t for t in ins if re.match(r"(global|flat|buffer)_load", t)]
    # the 32 bytes of a term's scalar, nothing else
    assert [t.split()[0] for t in vloads] == ["global_load_dwordx4", "global_load_dwordx4"], vloads
    assert not any(t.startswith(("flat_", "buffer_")) for t in ins)
    # the row: 27 limbs of a slot as wide scalar loads, inside the kernel's loops (beyond the kernel-argument loads of the prologue)
    wide = c["s_load_dwordx16"] + c["s_load_dwordx8"]
    assert wide >= 4, "the slot loads are no longer wide scalar loads: %r" % {k: v for k, v in c.items() if k.startswith("s_load")}
    # LDS: the digit column only - 16-bit writes by the recoding, one 16-bit read per window, no other form (no cross-lane traffic)
    ds = {k: v for k, v in c.items() if k.startswith("ds_")}
    assert set(ds) == {"ds_write_b16", "ds_read_u16"} and ds["ds_read_u16"] == 1, ds
    # divergent control flow: the ragged batch's `b < B` around the final store, nothing else; no vote anywhere
    assert c["s_and_saveexec_b64"] <= 2 and c["s_or_saveexec_b64"] == 0, c
    assert not any(t.startswith(("v_cmpx", "s_ballot")) or "ballot" in t for t in ins)
    # every conditional branch on vcc takes a vcc that was built from a SCALAR condition (s_and / s_andn2 with exec of an s_cselect mask),
    # never from a vector compare
    for i, t in enumerate(ins):
        if t.startswith(("s_cbranch_vccz", "s_cbranch_vccnz")):
            back = [x for x in ins[max(0, i - 40):i] if re.search(r"\bvcc\b", x) and not x.startswith(("v_cndmask", "v_addc", "v_subb", "v_add_co", "v_sub_co"))]
            assert back and back[-1].startswith(("s_and_b64 vcc", "s_andn2_b64 vcc", "s_mov_b64 vcc")), (t, back[-3:])
    # stores: vector stores of the chunk sum only
    assert all(t.startswith("global_store") for t in ins if "store" in t.split()[0]), [t for t in ins if "store" in t.split()[0]]
    assert sum(v for k, v in c.items() if k.startswith("global_store")) >= 1
    # the addition itself is the dominant kernel's: 7 field multiplications
    mads = c["v_mad_i64_i32"] + c["v_mad_u64_u32"]
    assert mads >= 700


def test_dominant_kernel_is_untouched():
    import kernel_isa_stats as K
    if not os.path.exists(LIB) or not os.path.exists(K.LLVM + "/llvm-objdump"):
        pytest.skip("libbpr1cs_hip.so is not built / no llvm-objdump")
    assert K.kernel_hash(LIB, "k_msm_fixed2") == K_MSM_FIXED2_PARENT_HASH


def test_shipped_library_has_no_recorder():
    """the simulator's recorder and its entry point are compiled out of libbpr1cs_hip.so: 47 exports, as before"""
    import subprocess
    if not os.path.exists(LIB):
        pytest.skip("libbpr1cs_hip.so is not built")
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    names = [l.split()[-1] for l in out.split("\n") if " T " in l and l.split()[-1].startswith("bpr1cs_")]
    assert "bpr1cs_sim_msm_trace" not in names
    assert len(names) == 47, len(names)
