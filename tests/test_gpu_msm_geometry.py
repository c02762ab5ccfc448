"""The multiscalar-multiplication entry points of libbpr1cs_hip.so across every launch-geometry boundary (tests/msm_cases.py):
bpr1cs_msm_fixed on both sides of every threshold of run_msm_multi - the lane kernel, k_msm_small_wave and k_ge_reduce_wave, paired
and unpaired launches, k_msm_fixed2 with ragged wavefronts, zero terms and one-term chunks, four window widths - bpr1cs_msm on both
sides of its Straus / Pippenger switch and chunk rules, bpr1cs_points_sum, and the two commitment kernels at their switch.
Everything goes through the C ABI; every expectation is the C oracle's."""
import os
import subprocess
import time

import pytest

import common
import msm_cases as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bp = common.bp


@pytest.fixture(scope="module")
def oracle():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "c")])
    from cref import COracle
    return COracle()


@pytest.fixture(scope="module")
def handles(hip_lib):
    """one handle per (window bits, capacity), made when a case first asks for it and closed with the module -> (gens, its points)"""
    made = {}

    def get(name):
        if name not in made:
            W, cap = M.HANDLES[name]
            t0 = time.time()
            g = bp.Gens(cap, lib=hip_lib, window_bits=W)
            info = g.table_info()
            assert info["window_bits"] == W
            print("handle %s: W = %d, capacity %d, %.0f MB, created in %.2f s" % (name, W, cap, info["bytes"] / 1e6, time.time() - t0))
            made[name] = (g, M.handle_points(g))
        return made[name]
    yield get
    for g, _ in made.values():
        g.close()


def _names(group):
    return [c["name"] for c in M.cases() if c["group"] == group]


def _run(hip_lib, oracle, handles, name):
    c = M.case(name)
    gens, pts = handles(c["handle"])
    how = M.run_case(gens, oracle, pts, c)
    assert how == ("full" if c["terms"] * c["B"] <= M.FULL_CHECK_MAX else "sampled")


@pytest.mark.parametrize("name", _names("small"))
def test_small_path(hip_lib, oracle, handles, name):
    """batches of up to 64 proofs: the lane kernel or k_msm_small_wave, then zero to two k_ge_reduce_wave levels"""
    _run(hip_lib, oracle, handles, name)


@pytest.mark.parametrize("name", _names("fixed2"))
def test_fixed2_path(hip_lib, oracle, handles, name):
    """batches from 65 proofs on: k_msm_fixed2, a wavefront per (chunk, 64 proofs), then zero to two K_ge_reduce levels"""
    _run(hip_lib, oracle, handles, name)


@pytest.mark.parametrize("name", _names("widths"))
def test_window_widths(hip_lib, oracle, handles, name):
    """W = 8, 11 and 15 with the edge scalars of the digit recoding on proofs 0, 63, 64 and B - 1"""
    _run(hip_lib, oracle, handles, name)


@pytest.mark.parametrize("n", M.VAR_MSM_SIZES)
def test_variable_base_msm(hip_lib, oracle, handles, n):
    """bpr1cs_msm: Straus with 1, 2, 3 and 64 chunks, Pippenger with 2 and 3 chunks and at the 64-chunk cap with a ragged last one"""
    M.check_var_msm(bp, hip_lib, oracle, handles("geo")[1], n)


def test_variable_base_msm_special_inputs(hip_lib, oracle, handles):
    M.check_var_msm_special(bp, hip_lib, oracle, handles("geo")[1], pippenger=True)


def test_points_sum(hip_lib, oracle, handles):
    M.check_points_sum(bp, hip_lib, oracle, handles("geo")[1])


def test_commitments_on_both_sides_of_the_wavefront_kernel_limit(hip_lib, oracle, handles):
    """256 commitments: k_commit_wave, a wavefront each; 257: K_commit_v, a lane each"""
    assert M.constants()["COMMIT_WAVE_MAX"] == 256
    gens, pts = handles("w8")
    M.check_commit_switch(bp, gens, oracle, pts)
