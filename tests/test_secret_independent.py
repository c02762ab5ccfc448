"""BPR1CS_OPT_SECRET_INDEPENDENT on the CPU simulator: the commit phase through msm_fixed_ct_body - the body the gfx950
kernel k_msm_fixed_ct is built from, run lane by lane.

  * bytes: handles with the mode on reproduce the oracle's proofs and commitments;
  * the contract itself: the simulator's recorder (csrc/msm_trace.hpp: every global / LDS address the body forms, relative to its
    buffers, every loop trip count, every launched grid) gives EQUAL recordings for two batches of the same circuit with different
    secrets, the second chosen to be hostile;
  * the control: the same recorder on msm_fixed2_body (mode off) gives DIFFERENT recordings for those two batches - the equality
    above is not the equality of two empty recordings;
  * option handling."""
import ctypes
import hashlib

import pytest

from pyref import scenarios as S
from pyref import gadgets as G
from pyref.ed import L
import common
import frontend_cases as fc

KINDS = 7   # csrc/msm_trace.hpp: scalar loads, table loads, LDS, stores, trip counts, votes, grids
SCALAR, TABLE, LDS, STORE, TRIP, VOTE, GRID = range(KINDS)


def recorded(lib, fn):
    """run fn() with the recorder on -> (result, dict(count=[..], hash=[..], ct_launches, fixed2_launches))"""
    lib.bpr1cs_sim_msm_trace.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    lib.bpr1cs_sim_msm_trace.restype = None
    buf = (ctypes.c_uint64 * (2 * KINDS + 2))()
    lib.bpr1cs_sim_msm_trace(1, None)
    try:
        res = fn()
    finally:
        lib.bpr1cs_sim_msm_trace(0, buf)
    v = list(buf)
    return res, dict(count=v[:KINDS], hash=v[KINDS:2 * KINDS], ct_launches=v[2 * KINDS], fixed2_launches=v[2 * KINDS + 1])


def ct_gens(lib, cap, **kw):
    return common.bp.Gens(cap, lib=lib, secret_independent=1, **kw)


def enc(rows):
    return b"".join(int(x).to_bytes(32, "little") for r in rows for x in r)


# ---------------------------------------------------------------------------------------------------------------- bytes
def test_bytes_host_wires_bound_check_and_factors(sim_lib):
    common.check_against_oracle(sim_lib, lambda j: S.bound_check(37 + j, 10, 100, 7), 16, 2, 4, gens=ct_gens(sim_lib, 16))
    common.check_against_oracle(sim_lib, lambda j: S.bound_check(37 + j, 10, 100, 7), 16, 2, 1, gens=ct_gens(sim_lib, 16, window_bits=5))
    common.check_against_oracle(sim_lib, lambda j: S.factors(), 4, 2, 4, gens=ct_gens(sim_lib, 4))


def test_bytes_poseidon_inverse_compiled_and_host_wires(sim_lib, sim_glib):
    """a Poseidon circuit with Inverse S-boxes: through the compiled circuit (device witness program; the merged S-box tables and the
    a_O - 1 form are NOT used in this mode - plain n-term sums), with an S-box input of 0, and through host wires"""
    name = "poseidon_hash_2_inverse_pr1"
    cap = fc.case(name, 0)[4]
    cache = {(id(sim_lib), cap): ct_gens(sim_lib, cap, window_bits=8)}
    _, ref = recorded(sim_lib, lambda: fc.check_compiled(sim_lib, sim_glib, name, batch=3, gens_cache=cache))
    assert ref["ct_launches"] > 0
    fc.check_compiled(sim_lib, sim_glib, name + "_zero", batch=2, gens_cache=cache)
    ob = common.oracle_batch(lambda j: fc.case(name, j)[3], cap, 3, key=name)
    circ = common.circuit_from_oracle(ob, sim_lib)
    P, C = common.bp.prove_batch(cache[(id(sim_lib), cap)], circ, ob["label"], ob["values"], ob["blindings"], ob["seeds"], 3, wires=ob["wires"])
    assert P == ob["proofs"]
    assert all(C[j][:len(ob["comms"][j])] == ob["comms"][j] for j in range(3))


def _c_oracle_batch(o, gname, ip, sp, label, values, blindings, seeds, m, B):
    return [o.prove_case(gname, ip, sp, label, values[j * m * 32:(j + 1) * m * 32], blindings[j * m * 32:(j + 1) * m * 32], seeds[32 * j:32 * j + 32])["proof"]
            for j in range(B)]


def test_bytes_ragged_batch_and_two_device_jobs(sim_lib, sim_glib):
    """70 proofs (64 + 6 lanes) of the 7-bit bound check, all bytes the C oracle's; the same call cut into two device jobs (40 + 30);
    and the commit shape of bpr1cs_msm_fixed (two terms over B and B~) on such a handle equals the default handle's"""
    from cref import COracle
    bp = common.bp
    o = COracle()
    B = 70
    gname, ip, sp, _, cap = fc.case("bound_check", 0)
    circ = bp.CompiledGadget(gname, ip, sp, lib=sim_lib, glib=sim_glib)
    vals = [[37 + j % 50, 27 + j % 50, 63 - j % 50] for j in range(B)]
    bls = [[S.synth_scalar(b"hb", 3 * j + i) for i in range(3)] for j in range(B)]
    values, blindings = enc(vals), enc(bls)
    seeds = b"".join(hashlib.sha256(b"hs%d" % j).digest() for j in range(B))
    want = _c_oracle_batch(o, gname, ip, sp, b"BoundsTest", values, blindings, seeds, circ.m, B)
    gens = ct_gens(sim_lib, cap)
    P, _ = bp.prove_batch(gens, circ, b"BoundsTest", values, blindings, seeds, B)
    assert P == want
    st = bp.last_prove_stats(sim_lib)
    assert st["jobs"] == 1
    gens.set_option("job_proofs", 40)
    P2, _ = bp.prove_batch(gens, circ, b"BoundsTest", values, blindings, seeds, B)
    st = bp.last_prove_stats(sim_lib)
    assert P2 == want and (st["jobs"], st["job_proofs"]) == (2, 40)
    # Prover::commit through the low-level entry point: 70 commitments and a single one
    plain = bp.Gens(cap, lib=sim_lib)
    sc = b"".join(int(x).to_bytes(32, "little") for j in range(B) for x in (vals[j][0], bls[j][0]))
    (got, rec) = recorded(sim_lib, lambda: gens.msm_fixed([0, 1], sc, B))
    assert got == plain.msm_fixed([0, 1], sc, B) and rec["ct_launches"] == 1
    edge = b"".join(int(x).to_bytes(32, "little") for x in (0, L - 1))
    assert gens.msm_fixed([0, 1], edge, 1) == plain.msm_fixed([0, 1], edge, 1)


def test_bytes_two_jobs_in_flight(sim_lib):
    ob1 = common.oracle_batch(lambda j: S.bound_check(37 + j, 10, 100, 7), 16, 2)
    ob2 = common.oracle_batch(lambda j: S.bound_check(50 + j, 10, 100, 7), 16, 3)
    gens = ct_gens(sim_lib, 16, unfold=2)
    c1, c2 = common.circuit_from_oracle(ob1, sim_lib), common.circuit_from_oracle(ob2, sim_lib)
    j1 = common.bp.ProveJob(gens, c1, ob1["label"], ob1["values"], ob1["blindings"], ob1["seeds"], 2, wires=ob1["wires"])
    j2 = common.bp.ProveJob(gens, c2, ob2["label"], ob2["values"], ob2["blindings"], ob2["seeds"], 3, wires=ob2["wires"])
    P2, _ = j2.finish()
    P1, _ = j1.finish()
    assert P1 == ob1["proofs"] and P2 == ob2["proofs"]


# ------------------------------------------------------------------------------------------------- the contract: traces
def _poseidon_batches(B, special):
    """two batches for ONE compiled Poseidon 2:1 circuit (Inverse S-boxes, 1 partial round; n = 147): `tame` - synthetic secrets;
    `hostile` - other secrets throughout, proof `special` with a first-round S-box input of 0 (the batch of
    test_zero_sbox_input_inside_a_full_wavefront_batch in tests/test_gpu_frontend.py: its a_L and a_O wires are 0 where every other
    proof's are not), a value blinding of 0 and one of l - 1.  The public output is the hostile proof's in both, so the circuit is
    the same (most proofs then prove a false statement, which changes no byte the prover computes)."""
    params = S.poseidon_params(1)
    xz = (-params.round_keys[1]) % L
    out = G.Poseidon_hash_2(xz, S.synth_scalar(b"zy", special), params, G.INVERSE)
    tame_v = [[S.synth_scalar(b"ax", j), S.synth_scalar(b"ay", j), 0, 101, 0, 0] for j in range(B)]
    tame_b = [[S.synth_scalar(b"ab", 2 * j), S.synth_scalar(b"ab", 2 * j + 1), 0, 0, 0, 0] for j in range(B)]
    host_v = [[xz if j == special else S.synth_scalar(b"zx", j), S.synth_scalar(b"zy", j), 0, 101, 0, 0] for j in range(B)]
    host_b = [[S.synth_scalar(b"zb", 2 * j), S.synth_scalar(b"zb", 2 * j + 1), 0, 0, 0, 0] for j in range(B)]
    host_b[special][0], host_b[special][1] = 0, L - 1
    host_b[B - 1][0], host_b[B - 1][1] = L - 1, 0
    seeds = lambda tag: b"".join(hashlib.sha256(tag + b"%d" % j).digest() for j in range(B))
    return out, (enc(tame_v), enc(tame_b), seeds(b"tame")), (enc(host_v), enc(host_b), seeds(b"hostile"))


def _prove_recorded(lib, gens, circ, label, batch, B, wires=None):
    bp = common.bp
    (P, C), rec = recorded(lib, lambda: bp.prove_batch(gens, circ, label, batch[0], batch[1], batch[2], B, wires=wires))
    st = bp.last_prove_stats(lib)
    return P, C, rec, {k: st[k] for k in ("msm_terms", "msm_adds", "msm_launches")}


def test_recordings_equal_for_different_secrets_compiled_poseidon(sim_lib, sim_glib):
    """THE test of the contract.  Same circuit, same B = 70 (two wavefronts per chunk, the second ragged), same options, different
    secrets: every address, trip count and grid of msm_fixed_ct_body is the same, and so are the statistics.  The recorder sees
    the sums of A_I1 / A_O1 / S1 with their blinding terms, the V's and the T's - everything the mode routes through the body.
    All 70 hostile proofs are the C oracle's bytes (so the recording is of a correct run, S-box input 0 included).
    Control: with the mode off the same two batches give different recordings (gathers by digit, votes on zero scalars, the a_O - 1
    form), so the recorder does see secrets where they reach addresses."""
    from cref import COracle, POSEIDON_HASH_2
    from pyref.ed import sc_to_bytes
    bp = common.bp
    B, special = 70, 40
    out, tame, hostile = _poseidon_batches(B, special)
    circ = bp.CompiledGadget("poseidon_hash_2", [1, 1], [out], lib=sim_lib, glib=sim_glib)
    assert circ.n == 147
    gens = ct_gens(sim_lib, 256)
    P1, C1, r1, s1 = _prove_recorded(sim_lib, gens, circ, b"Poseidon_hash_2", tame, B)
    P2, C2, r2, s2 = _prove_recorded(sim_lib, gens, circ, b"Poseidon_hash_2", hostile, B)
    assert P1 != P2
    o = COracle()
    m = circ.m
    for j in (0, special, 63, 64, B - 1):
        r = o.prove(POSEIDON_HASH_2, [1, 1], sc_to_bytes(out), b"Poseidon_hash_2", hostile[0][j * m * 32:(j + 1) * m * 32],
                    hostile[1][j * m * 32:(j + 1) * m * 32], hostile[2][32 * j:32 * j + 32])
        assert P2[j] == r["proof"], "hostile proof %d differs from the C oracle" % j
    assert r1["ct_launches"] == r2["ct_launches"] == 4 and r1["fixed2_launches"] == r2["fixed2_launches"]   # V's; A_I || A_O; S || blindings; T's
    n, w = circ.n, 64
    # what was recorded is the whole commit phase: (2n + n) + (2n + 3) + 2m + 10 terms per proof, 64 windows each, 9 slots per window
    # (lane-terms: the spare lanes of a ragged wavefront walk the same addresses)
    lanes = lambda outputs: -(-outputs // 64) * 64
    lt = (5 * n + 3) * lanes(B) + 2 * lanes(m * B) + 2 * lanes(5 * B)
    assert r1["count"][SCALAR] == lt and r1["count"][LDS] == lt * w and r1["count"][TABLE] == lt * w * 9
    assert r1["count"][VOTE] == 0
    assert r1 == r2, "the recordings of two batches with different secrets differ: %r / %r" % (r1, r2)
    assert s1 == s2 and s1["msm_terms"] >= (5 * n + 3 + 10) * B and s1["msm_launches"] >= 3   # (the argument's launches are counted too)
    # ---- the control
    plain = bp.Gens(256, lib=sim_lib)
    Q1, D1, q1, t1 = _prove_recorded(sim_lib, plain, circ, b"Poseidon_hash_2", tame, B)
    Q2, D2, q2, t2 = _prove_recorded(sim_lib, plain, circ, b"Poseidon_hash_2", hostile, B)
    assert (Q1, D1, Q2, D2) == (P1, C1, P2, C2), "the mode changes bytes"
    assert q1["ct_launches"] == q2["ct_launches"] == 0 and q1["fixed2_launches"] > 0
    assert q1["count"][TABLE] > 0 and q1["count"][VOTE] > 0
    assert q1["hash"][TABLE] != q2["hash"][TABLE], "control: the recorder does not see k_msm_fixed2's gathers"
    assert q1["hash"][VOTE] != q2["hash"][VOTE] or q1["count"][VOTE] != q2["count"][VOTE], "control: the a_O - 1 form's vote went unseen"
    assert t1["msm_adds"] > 0


def test_recordings_equal_for_all_zero_wires_in_one_wavefront(sim_lib):
    """host wires: the second batch gives the six proofs of the ragged second wavefront wires that are ALL zero (k_msm_fixed2 skips
    every term of that wavefront; the new body must not notice), zero values and zero blindings"""
    bp = common.bp
    B = 70
    ob = common.oracle_batch(lambda j: S.bound_check(37 + j % 50, 10, 100, 7), 16, B, key="ct-bound70")
    circ = common.circuit_from_oracle(ob, sim_lib)
    m, n = circ.m, circ.n
    cut = 64
    wires = ob["wires"][:cut * 96 * n] + bytes((B - cut) * 96 * n)
    values = ob["values"][:cut * m * 32] + bytes((B - cut) * m * 32)
    blind = ob["blindings"][:cut * m * 32] + bytes((B - cut) * m * 32)
    seeds = b"".join(hashlib.sha256(b"other%d" % j).digest() for j in range(B))
    gens = ct_gens(sim_lib, 16)
    P1, _, r1, s1 = _prove_recorded(sim_lib, gens, circ, ob["label"], (ob["values"], ob["blindings"], ob["seeds"]), B, wires=ob["wires"])
    assert P1 == ob["proofs"]
    P2, _, r2, s2 = _prove_recorded(sim_lib, gens, circ, ob["label"], (values, blind, seeds), B, wires=wires)
    assert P2[:cut] != P1[:cut]
    assert r1["ct_launches"] == 4 and r1["count"][TABLE] > 0
    assert r1 == r2 and s1 == s2
    plain = bp.Gens(16, lib=sim_lib)
    _, _, q1, t1 = _prove_recorded(sim_lib, plain, circ, ob["label"], (ob["values"], ob["blindings"], ob["seeds"]), B, wires=ob["wires"])
    _, _, q2, t2 = _prove_recorded(sim_lib, plain, circ, ob["label"], (values, blind, seeds), B, wires=wires)
    assert q1["ct_launches"] == 0
    assert q1["count"][TABLE] != q2["count"][TABLE], "control: the all-zero wavefront's skipped terms went unseen"


# -------------------------------------------------------------------------------------------------------------- options
def test_option_is_creation_only_and_takes_0_or_1(sim_lib):
    bp = common.bp
    assert bp.OPT_SECRET_INDEPENDENT == 11 and bp.OPTIONS["secret_independent"] == 11
    on, off, dflt = ct_gens(sim_lib, 16, window_bits=8), bp.Gens(16, lib=sim_lib, window_bits=8, secret_independent=0), bp.Gens(16, lib=sim_lib, window_bits=8)
    for g in (on, off, dflt):
        for v in (0, 1, -1):
            with pytest.raises(bp.R1CSError):
                g.set_option("secret_independent", v)
    for v in (2, -1, 5):
        with pytest.raises(bp.R1CSError):
            bp.Gens(16, lib=sim_lib, secret_independent=v)
    # bpr1cs_gens_table_info keeps describing the wide set
    assert on.table_info() == off.table_info() == dflt.table_info()
    assert (on.table_info()["window_bits"], on.table_info()["windows"]) == (8, 32)
    # the default handle takes the old code paths: not one launch of the new body, the same bytes, the statistics of a handle without the option
    ob = common.oracle_batch(lambda j: S.bound_check(37 + j, 10, 100, 7), 16, 2)
    circ = common.circuit_from_oracle(ob, sim_lib)
    stats = []
    for g in (dflt, off):
        P, _, rec, st = _prove_recorded(sim_lib, g, circ, ob["label"], (ob["values"], ob["blindings"], ob["seeds"]), 2, wires=ob["wires"])
        assert P == ob["proofs"] and rec["ct_launches"] == 0
        stats.append((rec, st))
    assert stats[0] == stats[1]
    P, _, rec, st = _prove_recorded(sim_lib, on, circ, ob["label"], (ob["values"], ob["blindings"], ob["seeds"]), 2, wires=ob["wires"])
    assert P == ob["proofs"] and rec["ct_launches"] == 4
