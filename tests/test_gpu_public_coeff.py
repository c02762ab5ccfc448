"""Public coefficients (BPR1CS_VAR_SCALE) on the device: the whole table of tests/public_coeff_cases.py through the shipped library -
K_flatten_scaled_chunks / K_flatten_scaled on the prover and on every verifier form, k_witness_team_scaled with teams of 4, 8 and 16
lanes, batches of 1, 3, 9 and 70 proofs, every prove entry point, one call cut into jobs, host wires and the device program, a default
and a secret-independent handle, the witness check, the refusals of bpr1cs_circuit_create and the gadgets "set_membership_lean" /
"weighted_sum_bound".  Every expectation is the oracle's on the baked circuit; nothing of the table is skipped here."""
import pytest

import public_coeff_cases as pc

bp = pc.bp
pytestmark = pytest.mark.gpu


def test_circuit_create(hip_lib):
    pc.check_create(hip_lib)


@pytest.mark.parametrize("name,B", pc.PROVER_CASES)
def test_prover_host_wires(hip_lib, name, B):
    pc.check_prover(hip_lib, name, B)


@pytest.mark.parametrize("name,B", pc.PROVER_CASES)
def test_prover_witness_program(hip_lib, name, B):
    pc.check_prover(hip_lib, name, B, program=True)


@pytest.mark.parametrize("team", [4, 8, 16])
@pytest.mark.parametrize("name,B", pc.TEAM_CASES)
def test_witness_team(hip_lib, name, B, team):
    pc.check_prover(hip_lib, name, B, program=True, witness_team=team)


@pytest.mark.parametrize("program", [False, True])
@pytest.mark.parametrize("entry", [e for e in pc.ENTRIES if e != "batch"])
def test_entry_points(hip_lib, entry, program):
    pc.check_prover(hip_lib, "lc", 3, entry=entry, program=program)
    pc.check_prover(hip_lib, "kinds", 3, entry=entry, program=program)


@pytest.mark.parametrize("program", [False, True])
@pytest.mark.parametrize("in_flight", [1, 2])
def test_batch_cut_into_jobs(hip_lib, in_flight, program):
    pc.check_job_slices(hip_lib, in_flight, program)


@pytest.mark.parametrize("program", [False, True])
def test_secret_independent_handle(hip_lib, program):
    pc.check_prover(hip_lib, "lc", 3, program=program, creation=dict(secret_independent=1))
    pc.check_prover(hip_lib, "kinds", 3, program=program, creation=dict(secret_independent=1))
    pc.check_prover(hip_lib, "chunks", 3, program=program, creation=dict(secret_independent=1))


def test_witness_check_names_the_row_an_altered_coefficient_violates(hip_lib):
    pc.check_witness_check(hip_lib)


@pytest.mark.parametrize("name,B,bad,k", pc.VERIFIER_CASES)
def test_verifier(hip_lib, name, B, bad, k):
    pc.check_verifier(hip_lib, name, B, bad, k)


@pytest.mark.parametrize("k", pc.SET_CASES)
def test_set_membership_lean(hip_lib, hip_glib, k):
    pc.check_set_membership_lean(hip_lib, hip_glib, k)


@pytest.mark.parametrize("k,bits", pc.WSB_CASES)
def test_weighted_sum_bound(hip_lib, hip_glib, k, bits):
    pc.check_weighted_sum_bound(hip_lib, hip_glib, k, bits)


@pytest.mark.parametrize("team", [0, 4, 8, 16])
def test_annotated_poseidon_permutation_over_scaled_inputs(hip_lib, team):
    pc.check_annotated_poseidon(hip_lib, **(dict(witness_team=team) if team else {}))
    pc.check_annotated_poseidon(hip_lib, B=9, **(dict(witness_team=team) if team else {}))
