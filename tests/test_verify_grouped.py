"""Grouped batch verification (BPR1CS_OPT_VERIFY_GROUP) on the CPU simulator: the functor forms of the segmented sums
(csrc/kernels.hpp K_combine_scalars_ranges, K_range_points, K_range_finish with the groups as ranges), the host logic around them, the
off switches and the options.
Cases and checker: tests/verify_group_cases.py; the wavefront kernels run in tests/test_gpu_verify_grouped.py.

Left out here: "vsmt_b3_g2" (N = 4096 is minutes on the simulator); "b141_g70" runs valid and with its tampered positions (69, 70,
140) - about half a minute - and leaves the rest of the properties to the small shapes."""
import ctypes

import pytest

import verify_group_cases as V
import test_batched_verify as tb
from test_secret_independent import recorded, SCALAR

bp = V.bp
SIM_CASES = ["b9_g4", "b6_g4", "b9_g2", "b9_g3", "b9_g64", "factors_b5_g2"]


@pytest.fixture(scope="module")
def e(sim_lib, sim_glib):
    return V.env(sim_lib, sim_glib)


def test_c_level_option_is_known(sim_lib):
    """bpr1cs_gens_set_option(g, 12, 4) returns 0 (BPR1CS_ERR_INVALID_ARGUMENT before the option existed); both options at creation"""
    g = bp.Gens(4, lib=sim_lib)
    assert sim_lib.bpr1cs_gens_set_option(g.h, 12, 4) == 0
    assert sim_lib.bpr1cs_gens_set_option(g.h, 13, 0) == 0
    assert (bp.OPT_VERIFY_GROUP, bp.OPT_VERIFY_GROUP_FALLBACK) == (12, 13)
    assert bp.OPTIONS["verify_group"] == 12 and bp.OPTIONS["verify_group_fallback"] == 13
    h = ctypes.c_void_p()
    pairs = (ctypes.c_int32 * 4)(12, 64, 13, 0)
    assert sim_lib.bpr1cs_gens_create_opts(4, pairs, 2, ctypes.byref(h)) == 0
    sim_lib.bpr1cs_gens_destroy(h)


@pytest.mark.parametrize("name", SIM_CASES)
def test_valid_batches(e, name):
    V.check_valid(e, name)


@pytest.mark.parametrize("name", SIM_CASES)
def test_one_tampered_proof(e, name):
    V.check_single_tamper(e, name)


def test_two_tampered_proofs_under_three_seed_sets(e):
    V.check_two_tampered(e, "b9_g4", [(1, 2), (1, 5)])


def test_malformed_proofs_and_swapped_commitment(e):
    V.check_malformed(e, "b9_g4")


def test_malformed_lone_proof_of_the_last_group(e):
    """B = 9, G = 4, proof 8 malformed: the last group's sums run over no proof at all - the identity - and the group fails by the flag"""
    V.check_malformed_at(e, "b9_g4", 8)


def test_malformed_proof_in_a_lanes_second_pass(e):
    """B = 141, G = 70, proof 65 malformed (a point that does not decode): lane 1 of the combining wavefront holds proofs 1 and 65.
    One call per mode, without the reference call (the shape is slow here; the device runs all three forms)"""
    V.check_malformed_at(e, "b141_g70", 65, forms=(0,), reference=False)


def test_null_seeds(e):
    assert V.verify_null_seeds(e, "b9_g4", 0) == [True] * 9
    assert V.verify_null_seeds(e, "b6_g4", 1) == [True] * 6


def test_two_proofs_per_lane_shape(e):
    V.check_valid(e, "b141_g70")
    assert V.single_positions(141, 70) == [69, 70, 140]
    V.check_single_tamper(e, "b141_g70")


def _scalar_loads(e, gens, B):
    b = e.batch("bound", 9)
    seeds = V.seed_sets(B)[0]
    res, rec = recorded(e.lib, lambda: bp.verify_batch(gens, b["circ"], b["label"], b["P"][:B], b["C"][:B], B, seeds))
    return res, (rec["count"][SCALAR], rec["hash"][SCALAR])


def test_off_switches_are_todays_path(e):
    """verify_group = 0, 1, -1 and a batch of one with G = 4: the reference verdicts, and the simulator's recorder sees the scalar loads
    of the per-proof path (same count, same sequence of offsets) - while G = 4 on 9 valid proofs loads strictly fewer: 2N scalars
    per GROUP instead of per proof"""
    b = e.batch("bound", 9)
    P = b["P"][:9]
    P[4] = V.flip(P[4], V.T_X + 3)
    want = [i != 4 for i in range(9)]
    ref9, loads9 = _scalar_loads(e, b["ref"], 9)
    assert ref9 == [True] * 9 and loads9[0] > 0
    grp = b["grp"]
    try:
        for v in (0, 1, -1):
            grp.set_option("verify_group", v)
            assert bp.verify_batch(grp, b["circ"], b["label"], P, b["C"][:9], 9) == want
            assert _scalar_loads(e, grp, 9) == (ref9, loads9)
        grp.set_option("verify_group", 4)
        assert bp.verify_batch(grp, b["circ"], b["label"], P[4:5], b["C"][4:5], 1) == [False]
        assert _scalar_loads(e, grp, 1) == _scalar_loads(e, b["ref"], 1)
        res, loads = _scalar_loads(e, grp, 9)
        assert res == ref9 and 0 < loads[0] < loads9[0]
        assert loads[0] * 3 == loads9[0]       # 3 groups against 9 proofs, 2N loads each
    finally:
        grp.set_option("verify_group", -1)


def test_combining_launch_stays_below_the_thread_limit(sim_lib):
    """A launch of 2^32 threads or more is refused by the HIP runtime.  k_combine_scalars_range_wave has one 64-lane workgroup per output
    up to a cap and walks the rest a grid apart; the host function that sizes it (csrc/api_verify.hpp combine_grouped_wgs, here through
    a simulator-only export) is asked for shapes no test can afford to run: the depth-32 circuit (65536 rows) with 4096 proofs in groups of
    4 - exactly 2^32 threads at a workgroup per output -, of 2, 16384 proofs in groups of 1 .. 16, a depth-253 circuit (524288 rows)"""
    grid = sim_lib.bpr1cs_sim_group_combine_grid
    grid.argtypes, grid.restype = [ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int
    w = ctypes.c_uint32()
    for rows, NG in [(65536, 1024), (65536, 2048), (65536, 16384), (65536, 1023), (524288, 2048), (524288, 8191), (2, 1 << 19),
                     (32, 3), (8192, 2), (8192, 128), (8192, 129), (2, 1)]:
        assert grid(rows, NG, ctypes.byref(w)) == 0
        assert 0 < w.value <= rows * NG and w.value * 64 < 1 << 32, (rows, NG, w.value)
        if rows * NG <= 1 << 20:
            assert w.value == rows * NG      # a wavefront per output while that fits
    assert grid(1 << 20, 1 << 13, ctypes.byref(w)) == -17      # the output index itself must fit 32 bits: refused, not wrapped
    assert grid(65536, 65535, ctypes.byref(w)) == 0 and grid(65536, 65536, ctypes.byref(w)) == -17


def test_options_plumbing(e, sim_lib, sim_glib):
    b = e.batch("bound", 9)
    grp = b["grp"]
    P = b["P"][:9]
    P[0] = V.flip(P[0], V.T_X + 3)
    args = (b["circ"], b["label"], P, b["C"][:9], 9)
    try:
        grp.set_option("verify_group", 4)
        for v, want in ((0, [False] * 4 + [True] * 5), (1, [False] + [True] * 8), (-1, [False] + [True] * 8)):
            grp.set_option("verify_group_fallback", v)
            assert bp.verify_batch(grp, *args) == want
        grp.set_option("verify_group_fallback", 0)
        grp.set_option("verify_group", -1)          # the default is off: per-proof verdicts whatever the fallback says
        assert bp.verify_batch(grp, *args) == [False] + [True] * 8
        grp.set_option("verify_group", 1 << 20)     # clamped to 4096: one group
        assert bp.verify_batch(grp, *args) == [False] * 9
    finally:
        grp.set_option("verify_group", -1)
        grp.set_option("verify_group_fallback", -1)


def test_other_verifier_entry_points_ignore_the_option(sim_lib, sim_glib, monkeypatch):
    """tb.check_batched_verify (combined, sharded and per-proof verdicts) on handles created with G = 4 (fallback at its default: its
    verify_batch assertions expect per-proof verdicts)"""
    real = bp.Gens
    monkeypatch.setattr(bp, "Gens", lambda cap, lib=None, **kw: real(cap, lib=lib, verify_group=4, **kw))
    assert tb.check_batched_verify(sim_lib, sim_glib)
