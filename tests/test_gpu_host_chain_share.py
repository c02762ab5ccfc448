"""BPR1CS_OPT_HOST_CHAIN_SHARE: a job's TranscriptRng chains split between host threads (eight proofs per AVX-512 register
set, streamed to the device in chunks of draws) and k_rng_stream.  The c4 fixture batch (VSMT-4 depth 32, 2024 proofs) with
none, half and all of its chains on the host, and cut into four jobs with the default split: every proof equals the C oracle's
(tests/golden/fullsize_digests.json)."""
import importlib

import pytest

pytestmark = pytest.mark.gpu


def _avx512():
    try:
        with open("/proc/cpuinfo") as f:
            return " avx512f" in f.read()
    except OSError:
        return False


@pytest.fixture(scope="module")
def gens(hip_lib):
    import gc
    bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
    gc.collect()
    bp.release_cached_memory(hip_lib)
    g = bp.Gens(32768, lib=hip_lib)
    yield g
    g.close()
    bp.release_cached_memory(hip_lib)


def test_c4_fixture_with_the_chains_split_between_host_and_device(hip_lib, hip_glib, gens):
    import fullsize_cases as fc
    bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
    name = "c4_vsmt4_d32_x2024"
    case = fc.CASES[name](bp, hip_glib)
    values, blindings, seeds = case["values"], case["blindings"], case["seeds"]
    circ = bp.CompiledGadget("vsmt_4", case["ip"], case["sp"], lib=hip_lib, glib=hip_glib)
    B = 2024
    try:
        for share in (0, 50, 100):
            gens.set_option("host_chain_share", share)
            P, C = bp.prove_batch(gens, circ, b"VSMT", values, blindings, seeds, B)
            fc.check_digests(name, case, P, C)
            st = bp.last_prove_stats(hip_lib)
            assert st["jobs"] == 1 and st["host_chains"] == (B * share + 50) // 100, (share, st["host_chains"])
        # the default: four jobs of 512 / 512 / 512 / 488 proofs, the first on the device, the three that follow it on the host
        # (with AVX-512; none without)
        gens.set_option("host_chain_share", -1)
        gens.release_scratch()
        gens.set_option("job_proofs", 512)
        P, C = bp.prove_batch(gens, circ, b"VSMT", values, blindings, seeds, B)
        fc.check_digests(name, case, P, C)
        st = bp.last_prove_stats(hip_lib)
        assert st["jobs"] == 4 and st["host_chains"] == ((B - 512) if _avx512() else 0)
    finally:
        gens.set_option("host_chain_share", -1)
        gens.set_option("job_proofs", -1)
        gens.release_scratch()
