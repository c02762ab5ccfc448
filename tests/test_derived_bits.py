"""Bits of a linear combination (BPR1CS_W_LCBIT / BPR1CS_W_LCNOTBIT) and the one-commitment bound check on the CPU simulator:
bpr1cs_circuit_create's validation and kind mapping, K_witness::operand with its one-entry cache, the front-end's bit_of_lc hint,
positive_no_gadget_lc and the gadget "bound_check_1".  Every expectation is the oracle's (tests/derived_bits_cases.py)."""
import os
import re

import pytest

import derived_bits_cases as db

bp = db.bp


def test_abi_constants():
    hdr = open(os.path.join(db.ROOT, "include", "bpr1cs.h")).read()
    val = lambda name: int(re.search(r"#define %s\s+(\w+?)u?\s" % name, hdr).group(1), 0)
    assert (val("BPR1CS_W_LCBIT"), val("BPR1CS_W_LCNOTBIT")) == (4, 5) == (bp.W_LCBIT, bp.W_LCNOTBIT)
    assert (val("BPR1CS_W_LC"), val("BPR1CS_W_INV_LEFT"), val("BPR1CS_W_BIT"), val("BPR1CS_W_NOTBIT")) == (0, 1, 2, 3)


def test_shapes():
    db.check_shapes()


def test_circuit_create(sim_lib):
    db.check_create(sim_lib)


def test_kinds_0_to_3_prove_the_golden_vectors(sim_lib, sim_glib):
    db.check_golden_unchanged(sim_lib, sim_glib)


@pytest.mark.parametrize("name,B", db.PROGRAM_CASES)
def test_witness_program(sim_lib, name, B):
    db.check_program(sim_lib, name, B)


@pytest.mark.parametrize("team", [4, 8, 16])
@pytest.mark.parametrize("name,B", db.TEAM_CASES)
def test_witness_team(sim_lib, name, B, team):
    db.check_program(sim_lib, name, B, witness_team=team)


@pytest.mark.parametrize("name,B", db.HOST_WIRE_CASES)
def test_host_wires_give_the_same_bytes(sim_lib, name, B):
    db.check_program(sim_lib, name, B, program=False)


@pytest.mark.parametrize("name", ["b8", "swap"])
def test_batch_cut_into_jobs(sim_lib, name):
    db.check_program(sim_lib, name, 5, job_proofs=2)


@pytest.mark.parametrize("entry", ["transcripts", "begin_end"])
def test_entry_points(sim_lib, entry):
    db.check_program(sim_lib, "b8", 3, entry=entry)
    db.check_program(sim_lib, "inv0", 3, entry=entry)


def test_secret_independent_handle(sim_lib):
    db.check_program(sim_lib, "b8", 3, creation=dict(secret_independent=1))
    db.check_program(sim_lib, "swap", 3, creation=dict(secret_independent=1))


def test_inverse_of_a_zero_left_wire_is_zero(sim_lib):
    db.check_inverse_of_zero(sim_lib)


@pytest.mark.parametrize("program", [True, False])
def test_witness_check_names_the_overflowing_sum_row(sim_lib, program):
    db.check_witness_check(sim_lib, program)


def test_verifiers_with_public_bounds(sim_lib):
    db.check_verifiers(sim_lib)


@pytest.mark.parametrize("bits", [8, 64])
def test_bound_check_1_gadget(sim_lib, sim_glib, bits):
    db.check_frontend(sim_lib, sim_glib, bits)
