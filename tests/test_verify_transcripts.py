"""The verifiers on the caller's transcripts (BPR1CS_LABEL_TRANSCRIPTS, `transcripts=`) on the CPU simulator: the checkers of
tests/verify_transcript_cases.py - the oracle is the yardstick - and the C++ twin (tests/hostsim/verifier_transcript_check.cpp).

Left to the device (tests/test_gpu_verify_transcripts.py): the one batch of 168 proofs that starts from every position of the STROBE
rate (here: the ten lengths that give positions 0, 1, 7, 8, 9, 63, 64, 163, 164 and 165) and the batches of 64 and 65 proofs, the
grouped one included - the simulator needs a second per proof.  The simulator has no host replay of its own (it runs every functor on
the host), so "device replay" is the same code path here."""
import os
import subprocess

import pytest

import verify_transcript_cases as VT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def e(sim_lib, sim_glib):
    return VT.env(sim_lib, sim_glib)


def test_the_context_lengths_reach_every_position_of_the_rate():
    VT.check_positions_table()


def test_starting_positions(e):
    ks = VT.sim_lengths()
    VT.check_sweep(e, [VT.ctx(k) for k in ks], b"sweep", oracle_made=(0, 4, len(ks) - 1))


def test_a_squeeze_or_a_proof_before_the_proof(e):
    VT.check_sweep(e, [VT.squeezed(0), VT.squeezed(5), VT.squeezed(150)], b"squeezed", oracle_made=(1,))
    VT.check_composition(e)


def test_wrong_context(e):
    VT.check_wrong_context(e)


def test_shared_handle(e):
    VT.check_shared_handle(e)


@pytest.mark.parametrize("B", [1, 8, 9, 16, 17])
def test_replay_forms(e, B):
    VT.check_forms(e, B)


@pytest.mark.parametrize("B", [1, 8])
def test_replay_forms_without_the_host_replay(e, B):
    VT.check_forms(e, B, device_replay=True)


def test_grouped(e):
    VT.check_grouped(e, 9, 4)


def test_combined_and_sharded(e):
    VT.check_combined_and_sharded(e)


def test_public_inputs_are_still_bound(sim_lib):
    VT.check_public_inputs(sim_lib)


def test_refusals(e):
    VT.check_refusals(e)


def test_cpp_verifier_on_advanced_transcripts(sim_lib, sim_glib):
    """host/r1cs.hpp: Prover and Verifier on Transcripts advanced alike accept and then draw the same challenge; a differing message
    rejects; two proofs in sequence on one pair of transcripts; a second verify on a used transcript is the next proof, not a GadgetError"""
    bdir = os.path.join(ROOT, "tests", "hostsim", "_build")
    exe = os.path.join(bdir, "verifier_transcript_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DBPR1CS_HOST_ONLY", os.path.join(ROOT, "tests", "hostsim", "verifier_transcript_check.cpp"), "-o", exe,
                           "-L" + bdir, "-lbpr1cs_gadgets_sim", "-lbpr1cs_sim", "-Wl,-rpath," + bdir, "-pthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
