"""The eight-way host TranscriptRng chain (csrc/host_chain.hpp: AVX-512, and its scalar fallback) draw for draw against the scalar
host_front_chain - the chain the library already checks against the oracle and the device stream - compiled for the host alone."""
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
    exe = str(tmp_path_factory.mktemp("hc8") / "host_chain8_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-DBPR1CS_HOST_ONLY", "-I" + CSRC, os.path.join(ROOT, "tests", "hostsim", "host_chain8_check.cpp"),
                           "-o", exe, "-pthread"])
    return exe


def _avx512():
    try:
        with open("/proc/cpuinfo") as f:
            return " avx512f" in f.read()
    except OSError:
        return False


@pytest.mark.parametrize("avx", [1, 0])
def test_eight_way_chain_equals_the_scalar_chain(checker, avx):
    out = subprocess.run([checker, str(avx)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    # avx = 0 always takes the scalar fallback; avx = 1 the AVX-512 path wherever the CPU has it
    assert out.stdout.startswith("path %s" % ("avx512" if avx and _avx512() else "scalar")), out.stdout
