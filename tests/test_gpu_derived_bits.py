"""Bits of a linear combination (BPR1CS_W_LCBIT / BPR1CS_W_LCNOTBIT) on the device: the cases of tests/derived_bits_cases.py through the
shipped library - team_operand / k_witness_team with teams of 4, 8 and 16 lanes (the combination spread over the team, the value kept
in the team's LDS slot, the fence before a wire is read back), batches of 1, 3, 9 and 70 proofs, a batch cut into jobs, two jobs in
flight, the witness check, the verifiers over public bounds and the gadget "bound_check_1".  Every expectation is the oracle's."""
import pytest

import derived_bits_cases as db

bp = db.bp
pytestmark = pytest.mark.gpu


def test_circuit_create(hip_lib):
    db.check_create(hip_lib)


def test_kinds_0_to_3_prove_the_golden_vectors(hip_lib, hip_glib):
    db.check_golden_unchanged(hip_lib, hip_glib)


@pytest.mark.parametrize("name,B", db.PROGRAM_CASES)
def test_witness_program(hip_lib, name, B):
    db.check_program(hip_lib, name, B)


@pytest.mark.parametrize("team", [4, 8, 16])
@pytest.mark.parametrize("name,B", db.TEAM_CASES)
def test_witness_team(hip_lib, name, B, team):
    db.check_program(hip_lib, name, B, witness_team=team)


@pytest.mark.parametrize("name,B", db.HOST_WIRE_CASES)
def test_host_wires_give_the_same_bytes(hip_lib, name, B):
    db.check_program(hip_lib, name, B, program=False)


@pytest.mark.parametrize("name", ["b8", "swap"])
def test_batch_cut_into_jobs(hip_lib, name):
    db.check_program(hip_lib, name, 5, job_proofs=2)


@pytest.mark.parametrize("entry", ["transcripts", "begin_end"])
def test_entry_points(hip_lib, entry):
    db.check_program(hip_lib, "b8", 3, entry=entry)
    db.check_program(hip_lib, "inv0", 3, entry=entry)


def test_secret_independent_handle(hip_lib):
    db.check_program(hip_lib, "b8", 3, creation=dict(secret_independent=1))
    db.check_program(hip_lib, "swap", 3, creation=dict(secret_independent=1))


def test_inverse_of_a_zero_left_wire_is_zero(hip_lib):
    db.check_inverse_of_zero(hip_lib)


@pytest.mark.parametrize("program", [True, False])
def test_witness_check_names_the_overflowing_sum_row(hip_lib, program):
    db.check_witness_check(hip_lib, program)


def test_verifiers_with_public_bounds(hip_lib):
    db.check_verifiers(hip_lib)


@pytest.mark.parametrize("bits", [8, 64])
def test_bound_check_1_gadget(hip_lib, hip_glib, bits):
    db.check_frontend(hip_lib, hip_glib, bits)
