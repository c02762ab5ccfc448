"""BPR1CS_OPT_CHECK_WITNESS on the device: the case table of tests/witness_check_cases.py through the shipped library - the wavefront
geometry of K_check_gates / K_check_rows (gid = chunk x Bpad + b), their atomics, the stream order of the check against the commit
sums and against the next job in flight.  Every expectation is the pure-Python checker's."""
import pytest

import witness_check_cases as wc

bp = wc.bp
pytestmark = pytest.mark.gpu


def test_option_on_the_device(hip_lib):
    g = bp.Gens(8, lib=hip_lib, window_bits=8)
    for v in (1, 0, 7, -1):
        assert hip_lib.bpr1cs_gens_set_option(g.h, bp.OPT_CHECK_WITNESS, v) == 0
    g.close()


@pytest.mark.parametrize("case", sorted(wc.TABLE))
def test_case(hip_lib, hip_glib, case):
    wc.TABLE[case](hip_lib, hip_glib)
