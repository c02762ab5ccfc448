"""Per-proof public inputs (BPR1CS_VAR_PUBLIC) on the device: the cases of tests/public_input_cases.py through the shipped library -
k_verify_public_wave (batches of at most 64 proofs, 70 public inputs on 64 lanes) and the functor's launch (70 proofs), the public
message of K_batch_leaf across two leaves, the public block behind the committed values in the prove jobs (host wires, witness program,
a batch cut into jobs, two jobs in flight), the witness check.  Every expectation is the oracle's, on the baked circuit."""
import pytest

import public_input_cases as pi

bp = pi.bp
pytestmark = pytest.mark.gpu


def test_circuit_create(hip_lib):
    pi.check_create(hip_lib)


def test_no_public_inputs_nothing_changes(hip_lib):
    pi.check_no_publics(hip_lib)


@pytest.mark.parametrize("name,B", [("p1", 1), ("p3", 3), ("m0", 3), ("p70", 70)])
@pytest.mark.parametrize("program", [False, True])
def test_prover(hip_lib, name, B, program):
    pi.check_prover(hip_lib, name, B, program=program)


@pytest.mark.parametrize("program", [False, True])
def test_prover_batch_cut_into_jobs(hip_lib, program):
    pi.check_prover(hip_lib, "p3", 5, program=program, job_proofs=2)


@pytest.mark.parametrize("entry", ["transcripts", "begin_end"])
def test_prover_entry_points(hip_lib, entry):
    pi.check_prover(hip_lib, "p3", 3, entry=entry)
    pi.check_prover(hip_lib, "p1", 3, entry=entry, program=True)


def test_noncanonical_public_input_is_refused_by_the_prover(hip_lib):
    pi.check_noncanonical_prover(hip_lib)


def test_witness_check_names_the_row(hip_lib):
    pi.check_witness_check(hip_lib, "p3", 5, bad=3, k=2)
    pi.check_witness_check(hip_lib, "p70", 3, bad=0, k=69)


@pytest.mark.parametrize("name,B,bad,k", pi.VERIFIER_CASES)
def test_verifier(hip_lib, name, B, bad, k):
    pi.check_verifier(hip_lib, name, B, bad, k)


@pytest.mark.parametrize("arity", [4, 2])
def test_tree_gadgets_with_a_public_root(hip_lib, hip_glib, arity):
    pi.check_frontend(hip_lib, hip_glib, arity)
