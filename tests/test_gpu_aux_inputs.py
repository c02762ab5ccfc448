"""Auxiliary inputs (BPR1CS_W_AUX) on the device: the whole table of tests/aux_input_cases.py through the shipped library - team_operand /
k_witness_team reading value rows m + p + k with teams of 4, 8 and 16 lanes, batches of 1, 3, 9 and 70 proofs, every prove entry point,
one call cut into jobs (one and two in flight), the host chain off, a secret-independent handle, host wires without the block, the
witness check, the verifiers, the refusals, and the lean tree gadgets "vsmt_4_aux" / "vsmt_2_aux".  Every expectation is the oracle's."""
import pytest

import aux_input_cases as ax

bp = ax.bp
pytestmark = pytest.mark.gpu


def test_circuit_create(hip_lib):
    ax.check_create(hip_lib)


def test_descriptions_without_the_kind_prove_the_golden_vectors(hip_lib, hip_glib):
    ax.check_golden_unchanged(hip_lib, hip_glib)


@pytest.mark.parametrize("name,B", ax.PROGRAM_CASES)
def test_witness_program(hip_lib, name, B):
    ax.check_program(hip_lib, name, B)


@pytest.mark.parametrize("team", [4, 8, 16])
@pytest.mark.parametrize("name,B", ax.TEAM_CASES)
def test_witness_team(hip_lib, name, B, team):
    ax.check_program(hip_lib, name, B, witness_team=team)


@pytest.mark.parametrize("name,B", ax.HOST_WIRE_CASES)
def test_host_wires_need_no_auxiliary_block(hip_lib, name, B):
    ax.check_program(hip_lib, name, B, program=False)


@pytest.mark.parametrize("entry", [e for e in ax.ENTRIES if e != "batch"])
def test_entry_points(hip_lib, entry):
    ax.check_program(hip_lib, "mix", 3, entry=entry)
    ax.check_program(hip_lib, "pair", 3, entry=entry)
    ax.check_program(hip_lib, "gap", 3, entry=entry)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_batch_cut_into_jobs(hip_lib, in_flight):
    ax.check_job_slices(hip_lib, in_flight)


def test_host_chain_off_against_the_default(hip_lib):
    ax.check_program(hip_lib, "mix", 9, host_chain_proofs=0)
    ax.check_program(hip_lib, "mix", 9)


def test_secret_independent_handle(hip_lib):
    ax.check_program(hip_lib, "mix", 3, creation=dict(secret_independent=1))
    ax.check_program(hip_lib, "gap", 3, creation=dict(secret_independent=1))
    ax.check_program(hip_lib, "wide", 3, creation=dict(secret_independent=1))


def test_witness_check_names_the_row_an_altered_auxiliary_value_violates(hip_lib):
    ax.check_witness_check(hip_lib)


def test_verifiers_never_see_the_block(hip_lib):
    ax.check_verifiers(hip_lib)


def test_prove_call_refusals(hip_lib):
    ax.check_prove_refusals(hip_lib)


def test_wrappers_size_the_block(hip_lib):
    ax.check_tail_length(hip_lib)


@pytest.mark.parametrize("form", ["t4", "t2"])
def test_lean_tree_gadget(hip_lib, hip_glib, form):
    ax.check_frontend(hip_lib, hip_glib, form)


def test_verifiers_over_lean_tree_proofs(hip_lib, hip_glib):
    ax.check_tree_verifiers(hip_lib, hip_glib, "t4")
