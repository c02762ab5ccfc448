"""What the verifier computes on the device against the oracle - the device-only forms of the verifier kernels: the Straus path
k_verify_win_wave + K_ipa_vb_horner + k_verify_finish_wave (B <= 64), the host / lockstep / lane-per-proof transcript replay (B <= 8 / <= 16
/ > 16), k_pow_tables_wave and the wavefront forms of K_sum_partials.  Mirror, case table and tamper table:
tests/verify_scalar_cases.py; the simulator twin is tests/test_verify_scalars.py."""
import pytest

import verify_scalar_cases as V

pytestmark = pytest.mark.gpu
TAMPER_BATCHES = [1, 8, 9, 16, 17, 64, 65]
WIDTHS = {"default": {}, "w4": {"window_bits": 4}}     # W = 4: 128 table items per base in k_verify_finish_wave - several trips per lane


@pytest.fixture(scope="module")
def e(hip_lib, hip_glib):
    return V.env(hip_lib, hip_glib, 217)


@pytest.mark.parametrize("name", list(V.SCALAR_CASES))
def test_scalars_match_the_mirror_gpu(e, name):
    V.check_scalar_case(e, name)


@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("B", TAMPER_BATCHES)
@pytest.mark.parametrize("src", sorted(V.TAMPER_SOURCES))
def test_tamper_table_gpu(e, src, B, width):
    """every entry, none skipped (run_table asserts it), at every batch size and on both table widths"""
    assert V.run_table(e, src, B, WIDTHS[width]) == len(V.check_table_conditions(src))


@pytest.mark.parametrize("B", [64, 65])
def test_unsatisfied_witness_among_valid_proofs_gpu(e, B):
    """a violated multiplication gate in the first and the last proof of a batch of valid proofs of the same random circuit"""
    want = V.check_verdicts(e, "rc3+bad", B)
    assert want.count(False) in (1, 2) and not want[0] and all(want[1:B - 1])


@pytest.mark.parametrize("B", [64, 65])
def test_identity_commitment_is_accepted_gpu(e, B):
    """is_zero(0) committed with blinding 0: V is 32 zero bytes, which upstream's commit() does not validate"""
    assert e.batch("is_zero_identity", B).C[0] == [bytes(32)]
    assert V.check_verdicts(e, "is_zero_identity", B) == [True] * B


@pytest.mark.parametrize("width", sorted(WIDTHS))
def test_more_own_points_than_a_wavefront_has_lanes_gpu(e, width):
    """P = 66 own points per proof: k_verify_win_wave's lanes 0 and 1 take a second term (p = 64, 65: R_2 and L_2.. of the proof)"""
    b = e.batch("rc_wide", 2)
    assert 8 + b.circ.m + 2 * (b.N.bit_length() - 1) == 66
    gens = e.gens(b.case.cap, **WIDTHS[width]) if WIDTHS[width] else None
    assert V.check_verdicts(e, "rc_wide", 2, gens) == [True, True]
    assert V.check_verdicts(e, "rc_wide", 1, gens) == [True]
