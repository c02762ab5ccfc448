"""What the verifier computes on the CPU simulator (the functor forms of the verifier kernels) against the oracle: combined scalars,
own-points sum, well-formed flag and verdicts.  Mirror, case table and tamper table: tests/verify_scalar_cases.py; the device's own forms
of the kernels run in tests/test_gpu_verify_scalars.py.

Left to the device: bound_b217 (a minute of proving here), mimc_b2 (the capacity-1024 tables and one proof are a minute as it is) and
vsmt_b2 (N = 4096)."""
import pytest

import verify_scalar_cases as V


@pytest.fixture(scope="module")
def e(sim_lib, sim_glib):
    return V.env(sim_lib, sim_glib, 65)


@pytest.mark.parametrize("src", sorted(V.TAMPER_SOURCES))
def test_tamper_table_conditions(src):
    """the table itself (no library involved): every reason class, a forgery of every element that only the equation rejects"""
    table = V.check_table_conditions(src)
    assert len(table) >= 7 * V.proof_elements(table[0].proof)[0] // 2


@pytest.mark.parametrize("name", V.SIM_SCALAR_CASES)
def test_scalars_match_the_mirror(e, name):
    V.check_scalar_case(e, name)


@pytest.mark.parametrize("src", sorted(V.TAMPER_SOURCES))
def test_tamper_table_b2(e, src):
    V.run_table(e, src, 2, {})


def test_more_own_points_than_a_wavefront_has_lanes(e):
    assert V.check_verdicts(e, "rc_wide", 2) == [True, True]
    b = e.batch("rc_wide", 2)
    assert 8 + b.circ.m + 2 * (b.N.bit_length() - 1) == 66
