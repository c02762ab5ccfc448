"""The verifiers on the caller's transcripts (BPR1CS_LABEL_TRANSCRIPTS, `transcripts=`) on the device: the checkers of
tests/verify_transcript_cases.py, the oracle as the yardstick.  Beyond the simulator's file: ONE batch of 168 proofs whose contexts put
the proof's first byte at every one of the 166 positions of the STROBE rate, and the batches of 64 and 65 proofs (a lane per proof)."""
import pytest

import verify_transcript_cases as VT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def e(hip_lib, hip_glib):
    return VT.env(hip_lib, hip_glib)


def test_every_starting_position_in_one_batch(e):
    VT.check_positions_table()
    VT.check_sweep(e, [VT.ctx(k) for k in range(168)], b"sweep168", oracle_made=(0, 83, 167))


def test_a_squeeze_or_a_proof_before_the_proof(e):
    VT.check_sweep(e, [VT.squeezed(0), VT.squeezed(5), VT.squeezed(150)], b"squeezed", oracle_made=(1,))
    VT.check_composition(e)


def test_wrong_context(e):
    VT.check_wrong_context(e)


def test_shared_handle(e):
    VT.check_shared_handle(e)


@pytest.mark.parametrize("B", VT.FORM_SIZES)
def test_replay_forms(e, B):
    VT.check_forms(e, B)


@pytest.mark.parametrize("B", [1, 8])
def test_replay_forms_on_the_device_below_the_host_threshold(e, B):
    VT.check_forms(e, B, device_replay=True)


@pytest.mark.parametrize("B,G", [(9, 4), (65, 64)])
def test_grouped(e, B, G):
    VT.check_grouped(e, B, G)


def test_combined_and_sharded(e):
    VT.check_combined_and_sharded(e)


def test_public_inputs_are_still_bound(hip_lib):
    VT.check_public_inputs(hip_lib)


def test_refusals(e):
    VT.check_refusals(e)
