"""The start of a prove call: the first job's TranscriptRng chains run in two legs cut behind draw n + 1, on the device
(k_rng_stream resumed from the states its first launch wrote back) and on host threads (chunks of 256 draws), each half reduced when it
ends, and S1 is summed in two launches, <s_L, G> behind the chain's second leg.  Every proof must stay the oracle's, byte for byte:

  * n + 2 inside the first host chunk (n = 128), exactly at a chunk boundary (n = 254: n + 2 = 256) and far behind it (n = 18 656) -
    the 2:1 Poseidon circuit over the Cube S-box with 16 and 79 partial rounds against the C oracle, the depth-32 VSMT-4 circuit against
    the committed digests of the C oracle's proofs (tests/golden/fullsize_digests.json);
  * batches of 65 and 130 proofs (just above the small-job path; at share 50 the device part is odd: the last wavefront carries one proof);
  * the host's share pinned to 0, 50 and 100 percent; one job per call, the call cut into three jobs, and a call of three jobs of 65
    proofs - the first takes the two-sum path, those that follow it the single launch;
  * host wires as well as the device witness program."""
import importlib
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BMAX = 195   # three jobs of 65


def _bp():
    return importlib.import_module("bulletproofs-r1cs-gadgets_amd")


@pytest.fixture(scope="module")
def oracle():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "c")])
    from cref import COracle
    return COracle()


_REF = {}


def _poseidon_cube(oracle, pr):
    """BMAX witnesses of the 2:1 Poseidon circuit (Cube, `pr` partial rounds: n = 2 (48 + pr)) and the C oracle's proofs of them, once per
    session; every proof claims proof 0's output (byte parity is the point, as in test_gpu_frontend.py)"""
    if pr in _REF:
        return _REF[pr]
    from cref import POSEIDON_HASH_2
    from pyref import scenarios as S, gadgets as g
    from pyref.ed import sc_to_bytes
    params = S.poseidon_params(pr)
    xs = [(S.synth_scalar(b"csx%d" % pr, j), S.synth_scalar(b"csy%d" % pr, j)) for j in range(BMAX)]
    out = g.Poseidon_hash_2(xs[0][0], xs[0][1], params, g.CUBE)
    vals = [b"".join(sc_to_bytes(x) for x in (a, b, 0, 101, 0, 0)) for a, b in xs]
    bls = [sc_to_bytes(S.synth_scalar(b"csb", 2 * j)) + sc_to_bytes(S.synth_scalar(b"csb", 2 * j + 1)) + bytes(128) for j in range(BMAX)]
    seeds = [S.synth_seed(9 * 10**6 + 1000 * pr + j) for j in range(BMAX)]

    def one(j):   # (ctypes releases the interpreter lock: the oracle's proofs are made side by side)
        return oracle.prove(POSEIDON_HASH_2, [0, pr], sc_to_bytes(out), b"Poseidon_hash_2", vals[j], bls[j], seeds[j], want_wires=j < 65)
    first = one(0)   # (alone: the oracle builds its generators on first use)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = [first] + list(ex.map(one, range(1, BMAX)))
    n = res[0]["n"]
    assert n == 2 * (48 + pr)
    _REF[pr] = dict(pr=pr, out=out, n=n, values=b"".join(vals), blindings=b"".join(bls), seeds=b"".join(seeds), proofs=[r["proof"] for r in res],
                    wires=b"".join(r["wires"][:96 * n] for r in res[:65]), comms=[r["comms"] for r in res])
    return _REF[pr]


def _jobs(B, J):
    return [min(J, B - k) for k in range(0, B, J)]


def _prove_and_check(bp, lib, gens, prove, check, B, share):
    """one job per call, the call cut into three jobs, and (B = 65 only) three jobs of 65: the proofs and the host's part of the chains"""
    gens.set_option("host_chain_share", share)
    gens.set_option("host_chain_proofs", 0)   # (no job small enough for the whole-chain-on-the-host path: the split is what is tested)
    try:
        shapes = [(B, B), (B, (B + 2) // 3)] + ([(3 * B, B)] if B == 65 else [])
        for total, J in shapes:
            gens.set_option("job_proofs", J)
            check(prove(total), total)
            st = bp.last_prove_stats(lib)
            want = sum((b * share + 50) // 100 for b in _jobs(total, J))
            assert st["jobs"] == len(_jobs(total, J)) and st["host_chains"] == want, (total, J, share, st["jobs"], st["host_chains"], want)
    finally:
        for k in ("host_chain_share", "host_chain_proofs", "job_proofs"):
            gens.set_option(k, -1)


@pytest.fixture(scope="module")
def gens256(hip_lib):
    g = _bp().Gens(256, lib=hip_lib)
    yield g
    g.close()


@pytest.mark.parametrize("share", [0, 50, 100])
@pytest.mark.parametrize("B", [65, 130])
@pytest.mark.parametrize("pr", [16, 79])   # n = 128: n + 2 inside host chunk 0; n = 254: n + 2 = 256, the first draw of chunk 1
def test_poseidon_cube_first_job_in_two_sums(hip_lib, hip_glib, oracle, gens256, pr, B, share):
    bp = _bp()
    ref = _poseidon_cube(oracle, pr)
    circ = bp.CompiledGadget("poseidon_hash_2", [0, pr], [ref["out"]], lib=hip_lib, glib=hip_glib)
    assert circ.n == ref["n"] and circ.has_witness_program

    def prove(total):
        return bp.prove_batch(gens256, circ, b"Poseidon_hash_2", ref["values"][:total * 192], ref["blindings"][:total * 192], ref["seeds"][:total * 32], total)[0]

    def check(P, total):
        bad = [j for j in range(total) if P[j] != ref["proofs"][j]]
        assert not bad, "n = %d, %d proofs, share %d: %d proofs differ from the C oracle's, first: %s" % (ref["n"], total, share, len(bad), bad[:8])
    _prove_and_check(bp, hip_lib, gens256, prove, check, B, share)


@pytest.mark.parametrize("share", [0, 50, 100])
def test_host_wires_first_job_in_two_sums(hip_lib, hip_glib, oracle, gens256, share):
    """the same path with the caller's wires instead of the device witness program (65 proofs of the n = 254 circuit)"""
    bp = _bp()
    ref = _poseidon_cube(oracle, 79)
    circ = bp.CompiledGadget("poseidon_hash_2", [0, 79], [ref["out"]], lib=hip_lib, glib=hip_glib)
    B = 65
    gens256.set_option("host_chain_share", share)
    gens256.set_option("host_chain_proofs", 0)
    try:
        P, _ = bp.prove_batch(gens256, circ, b"Poseidon_hash_2", ref["values"][:B * 192], ref["blindings"][:B * 192], ref["seeds"][:B * 32], B, wires=ref["wires"])
        assert P == ref["proofs"][:B]
        assert bp.last_prove_stats(hip_lib)["host_chains"] == (B * share + 50) // 100
    finally:
        gens256.set_option("host_chain_share", -1)
        gens256.set_option("host_chain_proofs", -1)


def test_callers_draws_in_a_call_of_two_jobs(hip_lib, hip_glib, oracle, gens256):
    """bpr1cs_prove_batch_draws with more than one job in flight: 130 proofs of the n = 128 circuit in jobs of 65, so that the second job's
    upload and reduction of the caller's draws wait for the first job's events (raw draws wiped, l(x) / r(x) done).  Transcripts as the
    single-job case of tests/witness_check_cases.py builds them (Prover::new's, commit's and "m" messages); the 2n + 8 draws per proof
    through the library's own host-side TranscriptRng (bpr1cs_transcript_build_rng, what host/r1cs.hpp's Prover calls: the oracle's
    Merlin in Python would take 20 s here) - a wrong draw is a proof that differs from the C oracle's."""
    import ctypes
    bp = _bp()
    ref = _poseidon_cube(oracle, 16)
    circ = bp.CompiledGadget("poseidon_hash_2", [0, 16], [ref["out"]], lib=hip_lib, glib=hip_glib)
    B, m, n = 130, 6, ref["n"]
    vp, cp, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t
    hip_lib.bpr1cs_transcript_build_rng.restype = vp
    hip_lib.bpr1cs_transcript_build_rng.argtypes = [vp, cp, sz, cp, sz, sz, cp]
    hip_lib.bpr1cs_transcript_rng_fill_bytes.argtypes = [vp, cp, sz, sz]
    hip_lib.bpr1cs_transcript_rng_free.argtypes = [vp]
    hip_lib.bpr1cs_prove_batch_draws.argtypes = [vp, vp, ctypes.POINTER(vp), cp, cp, cp, cp, sz, cp]
    ts, draws = [], b""
    for j in range(B):
        t = bp.Transcript(b"Poseidon_hash_2", lib=hip_lib)
        t.append_message(b"dom-sep", b"r1cs v1")
        for c in ref["comms"][j]:
            t.append_message(b"V", c)
        t.append_message(b"m", m.to_bytes(8, "little"))
        rng = hip_lib.bpr1cs_transcript_build_rng(t.h, b"v_blinding", 10, ref["blindings"][32 * m * j:32 * m * (j + 1)], 32, m, ref["seeds"][32 * j:32 * j + 32])
        buf = ctypes.create_string_buffer(64 * (2 * n + 8))
        hip_lib.bpr1cs_transcript_rng_fill_bytes(rng, buf, 64, 2 * n + 8)
        hip_lib.bpr1cs_transcript_rng_free(rng)
        draws += buf.raw
        ts.append(t)
    out = ctypes.create_string_buffer(B * circ.proof_len)
    gens256.set_option("job_proofs", 65)
    try:
        rc = hip_lib.bpr1cs_prove_batch_draws(gens256.h, circ.h, (vp * B)(*[t.h for t in ts]), ref["values"][:B * 32 * m], ref["blindings"][:B * 32 * m], draws, None, B, out)
        st = bp.last_prove_stats(hip_lib)
    finally:
        gens256.set_option("job_proofs", -1)
    assert rc == 0, rc
    P = [out.raw[j * circ.proof_len:(j + 1) * circ.proof_len] for j in range(B)]
    bad = [j for j in range(B) if P[j] != ref["proofs"][j]]
    assert not bad, "%d proofs differ from the C oracle's, first: %s" % (len(bad), bad[:8])
    assert st["jobs"] == 2 and st["host_chains"] == 0, (st["jobs"], st["host_chains"])


@pytest.fixture(scope="module")
def c4(hip_lib, hip_glib):
    import gc
    import fullsize_cases as fc
    bp = _bp()
    gc.collect()
    bp.release_cached_memory(hip_lib)
    name = "c4_vsmt4_d32_x2024"
    case = fc.CASES[name](bp, hip_glib)
    gens = bp.Gens(32768, lib=hip_lib)
    circ = bp.CompiledGadget("vsmt_4", case["ip"], case["sp"], lib=hip_lib, glib=hip_glib)
    yield name, case, gens, circ
    gens.close()
    bp.release_cached_memory(hip_lib)


@pytest.mark.parametrize("share", [0, 50, 100])
@pytest.mark.parametrize("B", [65, 130])
def test_depth32_tree_first_job_in_two_sums(hip_lib, c4, B, share):
    """n = 18 656: draw n + 1 lies in host chunk 72 of 146"""
    import fullsize_cases as fc
    bp = _bp()
    name, case, gens, circ = c4
    m = case["m"]

    def prove(total):
        return bp.prove_batch(gens, circ, case["label"], case["values"][:total * m * 32], case["blindings"][:total * m * 32], case["seeds"][:total * 32], total)[0]

    def check(P, total):
        fc.check_digests(name, case, P, first=total)
    try:
        _prove_and_check(bp, hip_lib, gens, prove, check, B, share)
    finally:
        gens.release_scratch()
