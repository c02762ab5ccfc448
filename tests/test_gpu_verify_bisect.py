"""BPR1CS_OPT_VERIFY_GROUP_FALLBACK = 2 (bisection inside a failing group) on the device: the wavefront kernels
k_combine_scalars_range_wave, k_range_points_wave and k_range_finish_wave (csrc/kernels_hip.hpp), the fixed-base MSM whose batch is the
number of ranges of a depth, and the lane form of the range finish for a depth of more than 64 ranges - through the C ABI.
Cases, split-rule mirror and checker: tests/verify_bisect_cases.py (the reference is the per-proof path on a default handle).  A wrong
range sum or subtraction turns into a wrong verdict for a good or a bad proof.  On the device the mode differs from mode 1 by its rate
only (tools/verify_group_probe.py); that it takes the columns of the mirror and no others is shown by the simulator's recorder in
tests/test_verify_bisect.py."""
import pytest

import verify_bisect_cases as VB
import verify_group_cases as VG

pytestmark = pytest.mark.gpu
bp = VB.bp
SMALL = ["b9_g64", "b9_g4", "b9_g3", "b9_g2", "b6_g4", "factors_b5_g2"]


@pytest.fixture(scope="module")
def e(hip_lib, hip_glib):
    return VG.env(hip_lib, hip_glib)


@pytest.mark.parametrize("name", SMALL + ["b141_g70", "b141_g2"])
def test_valid_batches_gpu(e, name):
    VB.check_tampered(e, name, set(), all_seeds=True)


@pytest.mark.parametrize("name", ["b9_g64", "b9_g4", "b9_g3", "b9_g2"])
def test_every_single_position_gpu(e, name):
    VB.check_every_single_position(e, name)


@pytest.mark.parametrize("name", ["b6_g4", "factors_b5_g2", "b141_g70", "b141_g2"])
def test_one_tampered_proof_per_group_gpu(e, name):
    kind, B, G = VB.CASES[name]
    for pos in VG.single_positions(B, G):
        VB.check_tampered(e, name, {pos})


def test_siblings_halves_and_groups_under_three_seed_sets_gpu(e):
    for bad in ({0, 1}, {3, 4}, {7, 8}):      # both children of a split fail: [0,2), [3,5), [7,9)
        VB.check_tampered(e, "b9_g64", bad, all_seeds=True)
    VB.check_tampered(e, "b9_g64", {1, 6}, all_seeds=True)      # different halves of [0,9)
    VB.check_tampered(e, "b9_g4", {1, 5}, all_seeds=True)       # different groups
    VB.check_tampered(e, "b9_g4", {2, 3, 8}, all_seeds=True)    # siblings of [2,4) and the lone proof
    VB.check_tampered(e, "b9_g3", {3, 5}, all_seeds=True)
    VB.check_tampered(e, "b9_g2", {0, 1, 6}, all_seeds=True)
    VB.check_tampered(e, "b141_g70", {64, 65}, all_seeds=True)  # siblings, past the first 64 proofs of the group
    VB.check_tampered(e, "b141_g70", {3, 69, 70, 140}, all_seeds=True)


@pytest.mark.parametrize("name", SMALL + ["b141_g70"])
def test_all_proofs_bad_gpu(e, name):
    VB.check_tampered(e, name, set(range(VB.CASES[name][1])), all_seeds=True)


def test_seventy_ranges_at_depth_one_gpu(e):
    """B = 141, G = 2, every even proof tampered: 71 groups, of which the 70 of two proofs fail - 70 ranges at depth 1, more than the
    MSM's lane path and the wavefront form of the range finish take (64)"""
    bad = set(range(0, 141, 2))
    assert VB.columns_per_depth(141, 2, bad) == [71, 70]
    VB.check_tampered(e, "b141_g2", bad, all_seeds=True)
    VB.check_tampered(e, "b141_g2", set(range(1, 141, 2)))


def test_malformed_proof_alone_and_with_a_tampered_proof_gpu(e):
    VB.check_malformed(e, "b9_g4", 0)
    VB.check_malformed(e, "b9_g4", 0, also_tampered={2})
    VB.check_malformed(e, "b9_g4", 8)
    VB.check_malformed(e, "b9_g64", 4)
    VB.check_malformed(e, "b9_g64", 4, also_tampered={3})
    VB.check_malformed(e, "b9_g64", 1, also_tampered={0, 7})
    VB.check_malformed(e, "b6_g4", 5, also_tampered={4})
    VB.check_malformed(e, "b141_g70", 68, also_tampered={2, 69})
    VB.check_malformed(e, "b141_g70", 140)


def test_swapped_commitment_gpu(e):
    for name in ("b9_g4", "b9_g3", "b141_g70"):
        VB.check_swapped_commitment(e, name)


def test_tree_proofs_several_chunks_per_column_gpu(hip_lib, hip_glib):
    """16 four-level tree proofs (N = 4096: a column of the MSM spans several chunks) in one group of 16 - four real depths - with
    proofs {5}, {0, 15} and {7, 8} tampered.  Proofs made by the library from the benchmark's workload generator."""
    import importlib
    wl = importlib.import_module("bulletproofs-r1cs-gadgets_amd.workloads")
    B, G = 16, 16
    w = wl.vsmt4(bp, hip_glib, 4, B, 16, 0)
    circ = bp.CompiledGadget(w["gadget"], w["ip"], w["sp"], lib=hip_lib, glib=hip_glib)
    assert 1 << (circ.n - 1).bit_length() == 4096
    ref, grp = bp.Gens(4096, lib=hip_lib, window_bits=8), bp.Gens(4096, lib=hip_lib, window_bits=8, verify_group=G)
    P, C = bp.prove_batch(ref, circ, w["label"], w["values"], w["blindings"], w["seeds"], B, wires=None)
    seeds = VG.seed_sets(B)[0]
    assert VB.columns_per_depth(B, G, {5}) == [1, 1, 1, 1, 1]
    try:
        for bad in (set(), {5}, {0, 15}, {7, 8}):
            P2 = [VB.flip(p, VB.T_X + 3) if i in bad else p for i, p in enumerate(P)]
            want = bp.verify_batch(ref, circ, w["label"], P2, C, B, seeds)
            assert want == [i not in bad for i in range(B)]
            for mode in (2, 1):
                grp.set_option("verify_group_fallback", mode)
                assert bp.verify_batch(grp, circ, w["label"], P2, C, B, seeds) == want, (sorted(bad), mode)
    finally:
        ref.close()
        grp.close()
