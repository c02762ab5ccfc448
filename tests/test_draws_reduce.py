"""The K_rng_reduce launches a prove job describes for its TranscriptRng draws (csrc/prove_draws.hpp DrawsLayout: whole batch, host part,
device part, a draw range each, and the lead-draw form), run through the kernel's functor on the CPU for n in {0, 1, 128, 254}, 1 / 2 /
65 / 130 proofs, host parts of 0, 1, half, B - 1 and B proofs, cut behind draw n + 1 and uncut: every slot of blind[1..8), s_L and s_R
written exactly once, with the value one whole-batch launch writes (tests/hostsim/draws_reduce_check.cpp)."""
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
    exe = str(tmp_path_factory.mktemp("draws") / "draws_reduce_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-DBPR1CS_HOSTSIM", "-I" + CSRC, os.path.join(ROOT, "tests", "hostsim", "draws_reduce_check.cpp"),
                           "-o", exe])
    return exe


def test_draw_ranges_cover_every_slot_once_with_the_whole_batch_values(checker):
    out = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
