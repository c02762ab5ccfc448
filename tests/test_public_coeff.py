"""Public coefficients (BPR1CS_VAR_SCALE) on the CPU simulator: bpr1cs_circuit_create's folding of marker + term, validation and the
second CSC, K_flatten_scaled_chunks / K_flatten_scaled behind K_flatten on the prover and on every verifier form, K_check_rows with
row_scale, K_witness_scaled, the Python shim's three-element terms and the front-end's public factor with the gadgets
"set_membership_lean" / "weighted_sum_bound".  Every expectation is the oracle's on the baked circuit (tests/public_coeff_cases.py).
Every case fails on a library without the feature: bpr1cs_circuit_create refuses variable kind 8 there.

Left to the device (tests/test_gpu_public_coeff.py), because of the simulator's running time: the 70-proof batches, the 600-entry circuit
at more than one batch size and the larger "lcbits" batch (pc.SIM_LEFT_OUT), the verifier cases above three proofs, the teams of 4, 8 and
16 lanes (the simulator has no teams), and the gadgets at k = 70."""
import os
import re
import subprocess

import pytest

import public_coeff_cases as pc

bp = pc.bp


def test_abi_constants():
    hdr = open(os.path.join(pc.ROOT, "include", "bpr1cs.h")).read()
    val = lambda name: int(re.search(r"#define %s\s+(\w+?)u?\s" % name, hdr).group(1), 0)
    assert val("BPR1CS_VAR_SCALE") == 8 == bp.VAR_SCALE == pc.SCALE
    assert val("BPR1CS_VAR_PUBLIC") == 5
    assert "is not provided" not in hdr.split("Public coefficients.")[0].split("Public inputs.")[1]


def test_left_out_on_the_simulator():
    assert pc.SIM_LEFT_OUT == [("chunks", 1), ("chunks", 9), ("kinds", 70), ("lc", 70), ("lcbits", 9), ("p70", 70)]


def test_the_oracle_accepts_right_and_rejects_altered_inputs():
    pc.check_oracle()


def test_circuit_create(sim_lib):
    pc.check_create(sim_lib)


@pytest.mark.parametrize("name,B", pc.SIM_PROVER_CASES)
def test_prover_host_wires(sim_lib, name, B):
    pc.check_prover(sim_lib, name, B)


@pytest.mark.parametrize("name,B", pc.SIM_PROVER_CASES)
def test_prover_witness_program(sim_lib, name, B):
    pc.check_prover(sim_lib, name, B, program=True)


@pytest.mark.parametrize("program", [False, True])
@pytest.mark.parametrize("entry", [e for e in pc.ENTRIES if e != "batch"])
def test_entry_points(sim_lib, entry, program):
    pc.check_prover(sim_lib, "lc", 3, entry=entry, program=program)
    pc.check_prover(sim_lib, "kinds", 3, entry=entry, program=program)


@pytest.mark.parametrize("program", [False, True])
@pytest.mark.parametrize("in_flight", [1, 2])
def test_batch_cut_into_jobs(sim_lib, in_flight, program):
    pc.check_job_slices(sim_lib, in_flight, program)


@pytest.mark.parametrize("program", [False, True])
def test_secret_independent_handle(sim_lib, program):
    pc.check_prover(sim_lib, "lc", 3, program=program, creation=dict(secret_independent=1))
    pc.check_prover(sim_lib, "kinds", 3, program=program, creation=dict(secret_independent=1))


def test_witness_check_names_the_row_an_altered_coefficient_violates(sim_lib):
    pc.check_witness_check(sim_lib)


@pytest.mark.parametrize("name,B,bad,k", pc.SIM_VERIFIER_CASES)
def test_verifier(sim_lib, name, B, bad, k):
    pc.check_verifier(sim_lib, name, B, bad, k)


def test_front_end_descriptions_and_refusals(sim_lib, sim_glib):
    """tests/hostsim/public_coeff_check.cpp: the two gadgets through CircuitCompiler with their data baked and public - rows and witness
    ops identical but for constant coefficients against public factors; the factor's algebra and export; Prover / Verifier refuse it"""
    bdir = os.path.join(pc.ROOT, "tests", "hostsim", "_build")
    exe = os.path.join(bdir, "public_coeff_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DBPR1CS_HOST_ONLY", os.path.join(pc.ROOT, "tests", "hostsim", "public_coeff_check.cpp"), "-o", exe,
                           "-L" + bdir, "-lbpr1cs_gadgets_sim", "-lbpr1cs_sim", "-Wl,-rpath," + bdir, "-pthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


@pytest.mark.parametrize("k", [1, 5])
def test_set_membership_lean(sim_lib, sim_glib, k):
    pc.check_set_membership_lean(sim_lib, sim_glib, k)


@pytest.mark.parametrize("k,bits", [(1, 8), (5, 64)])
def test_weighted_sum_bound(sim_lib, sim_glib, k, bits):
    pc.check_weighted_sum_bound(sim_lib, sim_glib, k, bits)


def test_annotated_poseidon_permutation_over_scaled_inputs(sim_lib):
    pc.check_annotated_poseidon(sim_lib)
