"""The default host share of a call's first job (csrc/host_chain.hpp host_chain_share_first): the balance of the host's workers against
k_rng_stream above one wavefront per SIMD, none at or below it, none without workers or the eight-way chain, monotone in the workers -
the rule compiled for the host alone (tests/hostsim/first_share_check.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bulletproofs-r1cs-gadgets_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("fshare") / "first_share_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-DBPR1CS_HOST_ONLY", "-I" + CSRC, os.path.join(ROOT, "tests", "hostsim", "first_share_check.cpp"),
                           "-o", exe, "-pthread"])
    return exe


def test_first_job_share_rule(checker):
    out = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
