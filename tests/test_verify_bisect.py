"""BPR1CS_OPT_VERIFY_GROUP_FALLBACK = 2 (bisection inside a failing group) on the CPU simulator: the functor forms of the range kernels
(csrc/kernels.hpp K_combine_scalars_ranges, K_range_points, K_range_finish) and the level-synchronous host logic around them
(csrc/api_verify.hpp verify_batch_bisect_once).  Cases, split-rule mirror and checker: tests/verify_bisect_cases.py; the wavefront
kernels run in tests/test_gpu_verify_bisect.py.

That the mode exists is shown here by the simulator's recorder (csrc/msm_trace.hpp): it counts the scalar loads of the fixed-base sums,
2N per column, so a call's count is the number of MSM columns it evaluated - the mirror's count in mode 2, one column per group plus
one per re-checked proof in mode 1.

Left out here (the device runs them): of "b141_g70" and "b141_g2" - about ten seconds of transcript replays per call on the
simulator - only a valid batch, one tampered proof per group and a sibling pair of the first, and the 70-ranges case of the second
under one seed set; the bad sets under three seed sets run on the B = 9 shapes."""
import pytest

import verify_bisect_cases as VB
import verify_group_cases as VG
from test_secret_independent import recorded, SCALAR

bp = VB.bp
SMALL = ["b9_g64", "b9_g4", "b9_g3", "b9_g2", "b6_g4", "factors_b5_g2"]


@pytest.fixture(scope="module")
def e(sim_lib, sim_glib):
    return VG.env(sim_lib, sim_glib)


def test_split_rule_mirror():
    VB.check_mirror()


def test_option_values(sim_lib):
    assert (bp.VERIFY_GROUP_FALLBACK_NONE, bp.VERIFY_GROUP_FALLBACK_RECHECK, bp.VERIFY_GROUP_FALLBACK_BISECT) == (0, 1, 2)
    g = bp.Gens(4, lib=sim_lib)
    for v in (2, 3, 1 << 20, 0, 1, -1):
        assert sim_lib.bpr1cs_gens_set_option(g.h, bp.OPT_VERIFY_GROUP_FALLBACK, v) == 0


@pytest.mark.parametrize("name", SMALL)
def test_valid_batches(e, name):
    VB.check_tampered(e, name, set(), all_seeds=True)


@pytest.mark.parametrize("name", ["b9_g64", "b9_g4", "b9_g3", "b9_g2"])
def test_every_single_position(e, name):
    VB.check_every_single_position(e, name)


@pytest.mark.parametrize("name", ["b6_g4", "factors_b5_g2"])
def test_one_tampered_proof_per_group(e, name):
    kind, B, G = VB.CASES[name]
    for pos in VG.single_positions(B, G):
        VB.check_tampered(e, name, {pos})


def test_siblings_halves_and_groups_under_three_seed_sets(e):
    for bad in ({0, 1}, {3, 4}, {7, 8}):      # both children of a split fail: [0,2), [3,5), [7,9)
        VB.check_tampered(e, "b9_g64", bad, all_seeds=True)
    VB.check_tampered(e, "b9_g64", {1, 6}, all_seeds=True)      # different halves of [0,9)
    VB.check_tampered(e, "b9_g4", {1, 5}, all_seeds=True)       # different groups
    VB.check_tampered(e, "b9_g4", {2, 3, 8}, all_seeds=True)    # siblings of [2,4) and the lone proof
    VB.check_tampered(e, "b9_g3", {3, 5}, all_seeds=True)       # [3,6) -> [3,5) | 5
    VB.check_tampered(e, "b9_g2", {0, 1, 6}, all_seeds=True)


@pytest.mark.parametrize("name", SMALL)
def test_all_proofs_bad(e, name):
    VB.check_tampered(e, name, set(range(VB.CASES[name][1])), all_seeds=True)


def test_malformed_proof_alone_and_with_a_tampered_proof(e):
    VB.check_malformed(e, "b9_g4", 0)
    VB.check_malformed(e, "b9_g4", 0, also_tampered={2})
    VB.check_malformed(e, "b9_g4", 8)                            # the lone proof of the last group
    VB.check_malformed(e, "b9_g64", 4)
    VB.check_malformed(e, "b9_g64", 4, also_tampered={3})        # its sibling
    VB.check_malformed(e, "b9_g64", 1, also_tampered={0, 7})
    VB.check_malformed(e, "b6_g4", 5, also_tampered={4})         # host transcript replay


def test_swapped_commitment(e):
    VB.check_swapped_commitment(e, "b9_g4")
    VB.check_swapped_commitment(e, "b9_g3")


def test_two_proofs_per_lane_shape(e):
    VB.check_tampered(e, "b141_g70", set())
    VB.check_tampered(e, "b141_g70", {69, 70, 140}, mode1=False)
    VB.check_tampered(e, "b141_g70", {64, 65}, mode1=False)


def test_seventy_ranges_at_depth_one(e):
    """B = 141, G = 2, every even proof tampered: 70 ranges at depth 1 - the MSM takes its wavefront path (more than 64 columns)"""
    bad = set(range(0, 141, 2))
    assert VB.columns_per_depth(141, 2, bad) == [71, 70]
    VB.check_tampered(e, "b141_g2", bad, mode1=False)


# ---- the recorder: MSM columns of a call
def _loads(e, gens, P, C):
    b = e.batch("bound", 9)
    B = len(P)
    res, rec = recorded(e.lib, lambda: bp.verify_batch(gens, b["circ"], b["label"], P, C, B, VG.seed_sets(B)[0]))
    return res, (rec["count"][SCALAR], rec["hash"][SCALAR])


@pytest.fixture(scope="module")
def L(e):
    """L[k] = (count, hash) of the scalar loads of a per-proof verification of k valid proofs on the reference handle"""
    b = e.batch("bound", 9)
    out = {}
    for k in range(1, 10):
        res, out[k] = _loads(e, b["ref"], b["P"][:k], b["C"][:k])
        assert res == [True] * k
    assert all(out[k][0] == k * out[1][0] > 0 for k in out)     # 2N loads per column
    return out


def _mode(e, G, fallback, P, C):
    grp = e.batch("bound", 9)["grp"]
    grp.set_option("verify_group", G)
    grp.set_option("verify_group_fallback", fallback)
    try:
        return _loads(e, grp, P, C)
    finally:
        grp.set_option("verify_group", -1)
        grp.set_option("verify_group_fallback", -1)


@pytest.mark.parametrize("pos", range(9))
def test_one_tampered_proof_costs_the_mirrors_columns(e, L, pos):
    """B = 9, G = 64, proof `pos` tampered: mode 2 loads the scalars of one column per tested range - at most 5 - where mode 1 loads
    those of the group's column and of 9 re-checked proofs"""
    P, C = VB.tampered(e, "b9_g64", {pos})
    want = [b != pos for b in range(9)]
    depths = VB.columns_per_depth(9, 64, {pos})
    assert depths[0] == 1 and 4 <= sum(depths) <= 5
    res2, loads2 = _mode(e, 64, 2, P, C)
    res1, loads1 = _mode(e, 64, 1, P, C)
    assert res2 == want and res1 == want
    assert loads1[0] == L[1][0] + L[9][0]
    assert loads2[0] == sum(L[r][0] for r in depths)
    assert loads2[0] < loads1[0]


def test_a_malformed_proof_among_good_ones_costs_nothing_more(e, L):
    b = e.batch("bound", 9)
    for broken in VB.malformed_forms(b["P"][4]):
        P = b["P"][:4] + [broken] + b["P"][5:9]
        res2, loads2 = _mode(e, 64, 2, P, b["C"][:9])
        assert res2 == [i != 4 for i in range(9)]
        assert loads2 == L[1]                                    # the group's single test (count and sequence of offsets)
        assert _mode(e, 64, 1, P, b["C"][:9])[1][0] == L[1][0] + L[8][0]


def test_all_bad_costs_the_mirrors_columns(e, L):
    P, C = VB.tampered(e, "b9_g64", set(range(9)))
    depths = VB.columns_per_depth(9, 64, set(range(9)))
    assert sum(depths) - 1 == 8 < 9                              # 8 splits for 9 bad proofs
    res2, loads2 = _mode(e, 64, 2, P, C)
    assert res2 == [False] * 9
    assert loads2[0] == sum(L[r][0] for r in depths) == 9 * L[1][0]
    P, C = VB.tampered(e, "b9_g4", {1, 5, 8})
    res2, loads2 = _mode(e, 4, 2, P, C)
    assert res2 == [i not in (1, 5, 8) for i in range(9)]
    assert VB.columns_per_depth(9, 4, {1, 5, 8}) == [3, 2, 2]
    assert loads2[0] == 7 * L[1][0]


def test_modes_0_1_and_default_record_what_they_did(e, L):
    """fallback 0, 1, -1 and values above 2 (which mean 1) are untouched by the new value: the loads of B = 9, G = 4 with proof 4
    tampered, counted - a column per group, and in mode 1 one per re-checked proof of the failing group - and pinned (count, hash)
    as recorded before the value 2 existed"""
    P, C = VB.tampered(e, "b9_g4", {4})
    want = [i != 4 for i in range(9)]
    res0, loads0 = _mode(e, 4, 0, P, C)
    assert res0 == [True] * 4 + [False] * 4 + [True]
    assert loads0 == L[3]
    for v in (1, -1, 3, 7):
        res, loads = _mode(e, 4, v, P, C)
        assert res == want and loads[0] == L[3][0] + L[4][0]
        assert loads == PINNED_MODE_1
    assert loads0 == PINNED_MODE_0
    res, loads = _mode(e, 4, 1, *VB.tampered(e, "b9_g4", set()))
    assert res == [True] * 9 and loads == L[3] == PINNED_MODE_0


# (count, hash) of the recorder's scalar loads for the call above, recorded on the commit before this mode
PINNED_MODE_0 = (96, 13690649544801033951)
PINNED_MODE_1 = (224, 4656267073409092344)
