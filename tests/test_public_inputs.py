"""Per-proof public inputs (BPR1CS_VAR_PUBLIC) on the CPU simulator: the functor bodies of K_verify_public, K_batch_leaf's public
message, the slot order of bpr1cs_circuit_create and the job plumbing of the tail block.  Every expectation is the oracle's, on the
baked circuit (tests/public_input_cases.py)."""
import os
import re
import subprocess

import pytest

import public_input_cases as pi

bp = pi.bp


def test_abi_constant():
    hdr = open(os.path.join(pi.ROOT, "include", "bpr1cs.h")).read()
    assert int(re.search(r"#define BPR1CS_VAR_PUBLIC\s+(\w+?)u?\s", hdr).group(1), 0) == 5 == bp.VAR_PUBLIC == pi.PUBLIC


def test_circuit_create(sim_lib):
    pi.check_create(sim_lib)


def test_no_public_inputs_nothing_changes(sim_lib):
    pi.check_no_publics(sim_lib)


@pytest.mark.parametrize("name,B", [("p1", 1), ("p3", 3), ("m0", 3), ("p70", 70)])
def test_prover_host_wires(sim_lib, name, B):
    pi.check_prover(sim_lib, name, B)


@pytest.mark.parametrize("name,B", [("p1", 1), ("p3", 3), ("m0", 3), ("p70", 70)])
def test_prover_witness_program(sim_lib, name, B):
    pi.check_prover(sim_lib, name, B, program=True)


@pytest.mark.parametrize("program", [False, True])
def test_prover_batch_cut_into_jobs(sim_lib, program):
    pi.check_prover(sim_lib, "p3", 5, program=program, job_proofs=2)


@pytest.mark.parametrize("entry", ["transcripts", "begin_end"])
def test_prover_entry_points(sim_lib, entry):
    pi.check_prover(sim_lib, "p3", 3, entry=entry)
    pi.check_prover(sim_lib, "p1", 3, entry=entry, program=True)


def test_noncanonical_public_input_is_refused_by_the_prover(sim_lib):
    pi.check_noncanonical_prover(sim_lib)


def test_wrappers_refuse_a_tail_block_of_the_wrong_length(sim_lib):
    pi.check_tail_length(sim_lib)


def test_compiled_description_differs_in_the_root_term_only(sim_lib, sim_glib):
    """tests/hostsim/public_root_check.cpp: vsmt_4 and vsmt_2 through CircuitCompiler with the root baked and with the root public -
    constraint rows, witness ops and Poseidon annotations identical but for the last row's (One, -root) against (Public 0, -1); and a
    Prover refuses a Public variable"""
    bdir = os.path.join(pi.ROOT, "tests", "hostsim", "_build")
    exe = os.path.join(bdir, "public_root_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DBPR1CS_HOST_ONLY", os.path.join(pi.ROOT, "tests", "hostsim", "public_root_check.cpp"), "-o", exe,
                           "-L" + bdir, "-lbpr1cs_gadgets_sim", "-lbpr1cs_sim", "-Wl,-rpath," + bdir, "-pthread"])
    r = subprocess.run([exe, bp.POSEIDON_PARAMS_PATH], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_witness_check_names_the_row(sim_lib):
    pi.check_witness_check(sim_lib, "p3", 5, bad=3, k=2)
    pi.check_witness_check(sim_lib, "p70", 3, bad=0, k=69)


@pytest.mark.parametrize("name,B,bad,k", pi.VERIFIER_CASES)
def test_verifier(sim_lib, name, B, bad, k):
    pi.check_verifier(sim_lib, name, B, bad, k)


def test_commitments_pointer_is_required(sim_lib):
    """m = 0 and p > 0: a NULL `commitments` is BPR1CS_ERR_INVALID_ARGUMENT (with p = 0 it is fine, as before)"""
    import ctypes
    P, C = pi.made(sim_lib, "m0", 3)
    g, circ = pi.gens(sim_lib, 4), pi.circuit(sim_lib, "m0")
    ok = (ctypes.c_int * 3)()
    lab = pi.label("m0")
    assert sim_lib.bpr1cs_verify_batch(g.h, circ.h, lab, len(lab), b"".join(P), None, None, 3, ok) == -17


@pytest.mark.parametrize("arity", [4, 2])
def test_tree_gadgets_with_a_public_root(sim_lib, sim_glib, arity):
    pi.check_frontend(sim_lib, sim_glib, arity)
