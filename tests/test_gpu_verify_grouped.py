"""Grouped batch verification (BPR1CS_OPT_VERIFY_GROUP) on the device: the wavefront kernels k_combine_scalars_range_wave,
k_range_points_wave and k_range_finish_wave (csrc/kernels_hip.hpp) with the groups as ranges and the fixed-base MSM with batch = number of
groups, through the C ABI.
Cases and checker: tests/verify_group_cases.py (the reference is the per-proof path on a default handle); the simulator twin is
tests/test_verify_grouped.py.  The runs with BPR1CS_OPT_VERIFY_GROUP_FALLBACK = 0 are the ones that show what the kernels computed."""
import pytest

import verify_group_cases as V
import test_batched_verify as tb

pytestmark = pytest.mark.gpu
bp = V.bp
GPU_CASES = ["b9_g4", "b6_g4", "b9_g2", "b9_g3", "b9_g64", "factors_b5_g2", "vsmt_b3_g2", "b141_g70"]


@pytest.fixture(scope="module")
def e(hip_lib, hip_glib):
    return V.env(hip_lib, hip_glib)


def test_c_level_option_is_known_gpu(hip_lib):
    g = bp.Gens(4, lib=hip_lib, window_bits=8)
    assert hip_lib.bpr1cs_gens_set_option(g.h, 12, 4) == 0
    assert hip_lib.bpr1cs_gens_set_option(g.h, 13, 0) == 0


@pytest.mark.parametrize("name", GPU_CASES)
def test_valid_batches_gpu(e, name):
    V.check_valid(e, name)


@pytest.mark.parametrize("name", GPU_CASES)
def test_one_tampered_proof_gpu(e, name):
    if name == "b141_g70":
        assert V.single_positions(141, 70) == [69, 70, 140]
    V.check_single_tamper(e, name)


def test_two_tampered_proofs_under_three_seed_sets_gpu(e):
    V.check_two_tampered(e, "b9_g4", [(1, 2), (1, 5)])
    V.check_two_tampered(e, "b141_g70", [(3, 66), (69, 70)])


def test_malformed_proofs_and_swapped_commitment_gpu(e):
    V.check_malformed(e, "b9_g4")
    V.check_malformed(e, "b141_g70")


def test_malformed_lone_proof_of_the_last_group_gpu(e):
    """B = 9, G = 4, proof 8 malformed: the last group's sums run over no proof at all - the identity - and the group fails by the flag"""
    V.check_malformed_at(e, "b9_g4", 8)


def test_malformed_proof_in_a_lanes_second_pass_gpu(e):
    """B = 141, G = 70, proof 65 malformed: lane 1 of the combining wavefront holds proofs 1 and 65, the skipped term is in its second pass"""
    V.check_malformed_at(e, "b141_g70", 65)


def test_null_seeds_gpu(e):
    assert V.verify_null_seeds(e, "b9_g4", 0) == [True] * 9
    assert V.verify_null_seeds(e, "b6_g4", 1) == [True] * 6


def test_off_switches_gpu(e):
    """verify_group = 0, 1, -1 and a batch of one with G = 4 give the reference verdicts"""
    b = e.batch("bound", 9)
    P = b["P"][:9]
    P[4] = V.flip(P[4], V.T_X + 3)
    want = [i != 4 for i in range(9)]
    grp = b["grp"]
    try:
        for v in (0, 1, -1):
            grp.set_option("verify_group", v)
            assert bp.verify_batch(grp, b["circ"], b["label"], P, b["C"][:9], 9) == want
        grp.set_option("verify_group", 4)
        assert bp.verify_batch(grp, b["circ"], b["label"], P[4:5], b["C"][4:5], 1) == [False]
        assert bp.verify_batch(grp, b["circ"], b["label"], P[3:4], b["C"][3:4], 1) == [True]
    finally:
        grp.set_option("verify_group", -1)


def test_more_outputs_than_the_combining_grid_gpu(e, hip_lib, hip_glib):
    """260 four-level tree proofs (N = 4096: 8192 rows) in groups of 2: 8192 x 130 outputs are more than the 2^20 wavefronts
    k_combine_scalars_range_wave is launched with at most (csrc/api_verify.hpp GROUP_COMBINE_MAX_WGS; a launch of 2^32 threads is
    refused by the runtime), so wavefronts take a second output a grid apart - and 130 groups are more than the MSM's lane path
    takes.  Proofs made by the library from the benchmark's workload generator (the oracle would need a minute per proof)."""
    import importlib
    wl = importlib.import_module("bulletproofs-r1cs-gadgets_amd.workloads")
    B, G = 260, 2
    assert 8192 * ((B + G - 1) // G) > 1 << 20
    h = e.batch("vsmt_4_l4", 3)
    w = wl.vsmt4(bp, hip_glib, 4, B, 16, 0)
    circ = bp.CompiledGadget(w["gadget"], w["ip"], w["sp"], lib=hip_lib, glib=hip_glib)
    assert 1 << (circ.n - 1).bit_length() == 4096
    P, C = bp.prove_batch(h["ref"], circ, w["label"], w["values"], w["blindings"], w["seeds"], B, wires=None)
    seeds = V.seed_sets(B)[0]
    assert bp.verify_batch(h["ref"], circ, w["label"], P, C, B, seeds) == [True] * B
    P2 = list(P)
    P2[B - 1] = V.flip(P2[B - 1], V.T_X + 3)
    grp = h["grp"]
    try:
        grp.set_option("verify_group", G)
        for fb in (0, 1):
            grp.set_option("verify_group_fallback", fb)
            assert bp.verify_batch(grp, circ, w["label"], P, C, B, seeds) == [True] * B
            assert bp.verify_batch(grp, circ, w["label"], P2, C, B, seeds) == [True] * (B - 2) + [bool(fb), False]
    finally:
        grp.set_option("verify_group", -1)
        grp.set_option("verify_group_fallback", -1)


def test_other_verifier_entry_points_ignore_the_option_gpu(hip_lib, hip_glib, monkeypatch):
    real = bp.Gens
    monkeypatch.setattr(bp, "Gens", lambda cap, lib=None, **kw: real(cap, lib=lib, verify_group=4, **kw))
    assert tb.check_batched_verify(hip_lib, hip_glib, batch=6)
