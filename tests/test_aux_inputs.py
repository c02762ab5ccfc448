"""Auxiliary inputs (BPR1CS_W_AUX) and the lean tree gadgets on the CPU simulator: bpr1cs_circuit_create's validation and row mapping,
the auxiliary block of the prove calls' `values` (staging, per-job slices, refusals), K_witness reading value rows m + p + k, the
front-end's Aux hint and the gadgets "vsmt_4_aux" / "vsmt_2_aux".  Every expectation is the oracle's (tests/aux_input_cases.py);
the device runs the whole table (tests/test_gpu_aux_inputs.py)."""
import os
import re

import pytest

import aux_input_cases as ax

bp = ax.bp


def test_abi_constants():
    hdr = open(os.path.join(ax.ROOT, "include", "bpr1cs.h")).read()
    val = lambda name: int(re.search(r"#define %s\s+(\w+?)u?\s" % name, hdr).group(1), 0)
    assert val("BPR1CS_W_AUX") == 10 == bp.W_AUX
    assert (val("BPR1CS_W_LCBIT"), val("BPR1CS_W_LCNOTBIT")) == (4, 5)


def test_shapes():
    ax.check_shapes()


def test_circuit_create(sim_lib):
    ax.check_create(sim_lib)


def test_descriptions_without_the_kind_prove_the_golden_vectors(sim_lib, sim_glib):
    ax.check_golden_unchanged(sim_lib, sim_glib)


@pytest.mark.parametrize("name,B", ax.SIM_PROGRAM_CASES)
def test_witness_program(sim_lib, name, B):
    ax.check_program(sim_lib, name, B)


@pytest.mark.parametrize("name,B", ax.HOST_WIRE_CASES)
def test_host_wires_need_no_auxiliary_block(sim_lib, name, B):
    ax.check_program(sim_lib, name, B, program=False)


@pytest.mark.parametrize("entry", [e for e in ax.ENTRIES if e != "batch"])
def test_entry_points(sim_lib, entry):
    ax.check_program(sim_lib, "mix", 3, entry=entry)
    ax.check_program(sim_lib, "pair", 3, entry=entry)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_batch_cut_into_jobs(sim_lib, in_flight):
    ax.check_job_slices(sim_lib, in_flight)


def test_host_chain_off(sim_lib):
    ax.check_program(sim_lib, "mix", 3, host_chain_proofs=0)


def test_secret_independent_handle(sim_lib):
    ax.check_program(sim_lib, "mix", 3, creation=dict(secret_independent=1))
    ax.check_program(sim_lib, "gap", 3, creation=dict(secret_independent=1))


def test_witness_check_names_the_row_an_altered_auxiliary_value_violates(sim_lib):
    ax.check_witness_check(sim_lib)


def test_verifiers_never_see_the_block(sim_lib):
    ax.check_verifiers(sim_lib)


def test_prove_call_refusals(sim_lib):
    ax.check_prove_refusals(sim_lib)


def test_wrappers_size_the_block(sim_lib):
    ax.check_tail_length(sim_lib)


@pytest.mark.parametrize("form,B", [("t4", 1), ("t2", 3)])     # (N = 1024 on the simulator: one tree; the device takes three of each)
def test_lean_tree_gadget(sim_lib, sim_glib, form, B):
    ax.check_frontend(sim_lib, sim_glib, form, B)


def test_verifiers_over_lean_tree_proofs(sim_lib, sim_glib):
    ax.check_tree_verifiers(sim_lib, sim_glib, "t2")
