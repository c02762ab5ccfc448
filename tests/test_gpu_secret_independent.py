"""BPR1CS_OPT_SECRET_INDEPENDENT on the device: k_msm_fixed_ct over the narrow table set computes the commit phase of
handles created with the option, and the bytes are the ones the default path gives - the committed digests of the C oracle
(tests/golden/fullsize_digests.json) for the bench-size batches, the C oracle itself for the S-box-input-0 batch, the Python oracle
for one proof per call.  That the kernel's addresses do not follow secrets is the CPU suite's business (tests/test_secret_independent.py:
the same body under the simulator's recorder; tests/test_kernel_isa_ct.py: the instruction forms); here: the shipped code object
computes the right points, in every shape the prover launches it."""
import importlib
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _avx512():
    try:
        with open("/proc/cpuinfo") as f:
            return " avx512f" in f.read()
    except OSError:
        return False


@pytest.fixture(scope="module")
def ct_gens(hip_lib):
    import gc
    bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
    gc.collect()
    bp.release_cached_memory(hip_lib)
    g = bp.Gens(32768, lib=hip_lib, secret_independent=1)
    yield g
    g.close()
    bp.release_cached_memory(hip_lib)


def test_c4_all_2024_proofs_default_job_size_and_four_jobs(hip_lib, hip_glib, ct_gens):
    """the flagship batch on a capacity-32768 handle with the mode on: all 2024 proofs and commitments, as one job and as four jobs
    of 512 with the host-chain split; msm_terms is a function of the circuit and B alone (two batches with different secrets)"""
    import fullsize_cases as fc
    bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
    name = "c4_vsmt4_d32_x2024"
    case = fc.CASES[name](bp, hip_glib)
    values, blindings, seeds, m = case["values"], case["blindings"], case["seeds"], case["m"]
    circ = bp.CompiledGadget("vsmt_4", case["ip"], case["sp"], lib=hip_lib, glib=hip_glib)
    B = 2024
    try:
        P, C = bp.prove_batch(ct_gens, circ, b"VSMT", values, blindings, seeds, B)
        fc.check_digests(name, case, P, C)
        st = bp.last_prove_stats(hip_lib)
        assert st["jobs"] == 1
        ct_gens.release_scratch()
        ct_gens.set_option("job_proofs", 512)
        P, C = bp.prove_batch(ct_gens, circ, b"VSMT", values, blindings, seeds, B)
        fc.check_digests(name, case, P, C)
        st = bp.last_prove_stats(hip_lib)
        assert st["jobs"] == 4 and st["host_chains"] == ((B - 512) if _avx512() else 0)
        # two batches of 512 with different secrets (different proofs of the fixture): the same counts
        counts = []
        for lo in (0, 512):
            Pk, _ = bp.prove_batch(ct_gens, circ, b"VSMT", values[lo * m * 32:(lo + 512) * m * 32], blindings[lo * m * 32:(lo + 512) * m * 32], seeds[32 * lo:32 * (lo + 512)], 512)
            assert Pk == P[lo:lo + 512]
            st = bp.last_prove_stats(hip_lib)
            counts.append((st["msm_terms"], st["msm_adds"], st["msm_launches"]))
        assert counts[0] == counts[1]
    finally:
        ct_gens.set_option("job_proofs", -1)
        ct_gens.release_scratch()


@pytest.mark.parametrize("name,gadget,cap", [("c1_bound_check64_x4096", "bound_check", 128), ("c2_poseidon2_cube_x4096", "poseidon_hash_2", 512),
                                             ("c5_mimc_set_x8192", "mimc_set_membership", 1024)])
def test_small_circuit_fixtures(hip_lib, hip_glib, name, gadget, cap):
    import fullsize_cases as fc
    bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
    case = fc.CASES[name](bp, hip_glib)
    assert case["gadget"] == gadget
    circ = bp.CompiledGadget(gadget, case["ip"], case["sp"], lib=hip_lib, glib=hip_glib)
    gens = bp.Gens(cap, lib=hip_lib, window_bits=8, secret_independent=1)
    try:
        P, C = bp.prove_batch(gens, circ, case["label"], case["values"], case["blindings"], case["seeds"], case["B"])
        fc.check_digests(name, case, P, C)
    finally:
        gens.close()


@pytest.mark.parametrize("case,batch", [("bound_check_64", 9), ("poseidon_hash_2_inverse", 3), ("vsmt_4_l4", 3)])
def test_one_proof_per_call(hip_lib, hip_glib, case, batch):
    """bpr1cs_gadget_prove_on(batch = 1): per-commit device calls (the commit shape of bpr1cs_msm_fixed), host wires, a job of one
    proof through the same kernel; then `batch` witnesses in one call"""
    import frontend_cases as fc
    bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
    cap = fc.case(case, 0)[4]
    gens = bp.Gens(cap, lib=hip_lib, window_bits=8, secret_independent=1)
    try:
        fc.check_prove_on(hip_lib, hip_glib, case, batch, gens_cache={(id(hip_lib), cap): gens})
    finally:
        gens.close()


def test_zero_sbox_input_inside_a_full_wavefront_batch(hip_lib, hip_glib):
    """the batch of tests/test_gpu_frontend.py's test of the same name - 96 proofs, ONE with an Inverse-S-box input of 0 - on a handle
    with the mode on, compared the way that test compares it: all 96 proofs equal the C oracle's"""
    import subprocess
    from pyref import scenarios as S, gadgets as g
    from pyref.ed import sc_to_bytes, L
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "c")])
    from cref import COracle, POSEIDON_HASH_2
    bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
    o = COracle()
    pr, B, special = 1, 96, 40
    params = S.poseidon_params(pr)
    xz = (-params.round_keys[1]) % L
    xs = [(xz if j == special else S.synth_scalar(b"zx", j), S.synth_scalar(b"zy", j)) for j in range(B)]
    out = g.Poseidon_hash_2(xs[special][0], xs[special][1], params, g.INVERSE)
    vals = [b"".join(sc_to_bytes(x) for x in (a, b, 0, 101, 0, 0)) for a, b in xs]
    bls = [sc_to_bytes(S.synth_scalar(b"zb", 2 * j)) + sc_to_bytes(S.synth_scalar(b"zb", 2 * j + 1)) + bytes(128) for j in range(B)]
    seeds = [S.synth_seed(7 * 10**6 + j) for j in range(B)]
    circ = bp.CompiledGadget("poseidon_hash_2", [1, pr], [out], lib=hip_lib, glib=hip_glib)
    assert circ.n == 147 and hip_lib.bpr1cs_circuit_macro_perms(circ.h) == 1
    gens = bp.Gens(256, lib=hip_lib, secret_independent=1)
    try:
        P, C = bp.prove_batch(gens, circ, b"Poseidon_hash_2", b"".join(vals), b"".join(bls), b"".join(seeds), B)
        for j in range(B):
            r = o.prove(POSEIDON_HASH_2, [1, pr], sc_to_bytes(out), b"Poseidon_hash_2", vals[j], bls[j], seeds[j], want_wires=(j == special))
            assert P[j] == r["proof"], "proof %d differs from the C oracle" % j
            if j == special:
                n = r["n"]
                aO = [r["wires"][32 * (2 * n + i):32 * (2 * n + i) + 32] for i in range(n)]
                assert sum(1 for w in aO if w == sc_to_bytes(1)) == 2 * 49 - 2
        assert bp.verify_batch(gens, circ, b"Poseidon_hash_2", [P[special], P[0]], [C[special], C[0]], 2) == [False, False]
    finally:
        gens.close()
