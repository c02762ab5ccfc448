"""The first generator fold of the IPA in its unit form (csrc/kernels.hpp K_ipa_fold_scal / K_ipa_fold_idx / K_ipa_fold_unit,
csrc/ipa.hpp): 2^r - 1 table terms per output and one point addition, the coefficient of block 0 in linv, y^-j of the H side in the
scalars of the variable-base rounds.  Every case compares whole proofs byte for byte with the C oracle (bpr1cs_ipa_create: with the
Python oracle), on the CPU simulator (unmarked) and on the device (marked gpu).

Shapes: the fold runs in the unit form for jobs of more than 64 proofs (the shipped MSM kernel); n < N and n not a power of two, so
the H side has a padded region (n <= i < N) where a wrong power of y or a wrong padding flag shows:
  N = 16: bound check of 7 bits (n = 14), N = 64: of 25 bits (n = 50), N = 256: Poseidon hash, Inverse S-box, 1 partial round (n = 147).
"""
import hashlib
import random

import pytest

import common
import frontend_cases as fc
from pyref import scenarios as S

bp = common.bp
_WANT, _GENS, _CIRC = {}, {}, {}


def _inputs(N, B):
    """-> (gadget name, iparams, sparams, label, values, blindings, seeds) of B different proofs of the circuit with N generators"""
    if N == 256:
        gname, ip, sp, _, cap = fc.case("poseidon_hash_2_inverse_pr1", 0)
        xl, xr = S.synth_scalar(b"xl", 0), S.synth_scalar(b"xr", 0)
        vals = [[xl, xr, 0, 101, 0, 0]] * B
        bls = [[S.synth_scalar(b"fb", 2 * j), S.synth_scalar(b"fb", 2 * j + 1), 0, 0, 0, 0] for j in range(B)]
        label = b"Poseidon_hash_2"
    else:
        bits = {16: 7, 64: 25}[N]
        gname, ip, sp, cap, label = "bound_check", [bits, 10, 0, 100, 0], [], N, b"BoundsTest"
        vals = [[37 + j % 50, 27 + j % 50, 63 - j % 50] for j in range(B)]
        bls = [[S.synth_scalar(b"fb", 3 * j + i) for i in range(3)] for j in range(B)]
    assert cap == N
    enc = lambda rows: b"".join(int(x).to_bytes(32, "little") for r in rows for x in r)
    seeds = b"".join(hashlib.sha256(b"fold%d" % j).digest() for j in range(B))
    return gname, ip, sp, label, enc(vals), enc(bls), seeds


def _want(N, B):
    """the oracle's proofs: computed once per (N, B), shared by every case and both libraries"""
    if (N, B) not in _WANT:
        from cref import COracle
        o = COracle()
        gname, ip, sp, label, values, blindings, seeds = _inputs(N, B)
        m = len(values) // (32 * B)
        _WANT[(N, B)] = tuple(o.prove_case(gname, ip, sp, label, values[j * m * 32:(j + 1) * m * 32], blindings[j * m * 32:(j + 1) * m * 32],
                                           seeds[32 * j:32 * j + 32])["proof"] for j in range(B))
    return _WANT[(N, B)]


def _check(lib, glib, N, B, unfold, **opts):
    gname, ip, sp, label, values, blindings, seeds = _inputs(N, B)
    key = (id(lib), N)
    if key not in _GENS:
        _GENS[key] = bp.Gens(N, lib=lib, window_bits=8)
        _CIRC[key] = bp.CompiledGadget(gname, ip, sp, lib=lib, glib=glib)
    gens, circ = _GENS[key], _CIRC[key]
    n = circ.n
    assert N // 2 < n < N and n & (n - 1), n
    opts = dict(opts, unfold=unfold)
    try:
        for k, v in opts.items():
            gens.set_option(k, v)
        P, _ = bp.prove_batch(gens, circ, label, values, blindings, seeds, B)
    finally:
        for k in opts:
            gens.set_option(k, -1)
    want = _want(N, B)
    bad = [j for j in range(B) if P[j] != want[j]]
    assert not bad, "N=%d B=%d unfold=%d %r: proofs %r differ from the oracle's" % (N, B, unfold, opts, bad[:8])


# unfold rounds x capacity (r = 4 at N = 16: all rounds from the tables, no fold at all), 65 proofs: the first size on the MSM path
UNFOLD_CAP = [(r, N) for N in (16, 64, 256) for r in (1, 2, 4)]
# r + 1 = lg N: one variable-base round follows the fold, no pair (K_ipa_vb_tab only) ; r + 2 = lg N: exactly one pair (K_ipa_vb_dig2,
# no K_ipa_vb_fold2) - both sizes of circuit
LAST_ROUNDS = [(3, 16), (2, 16), (5, 64), (4, 64)]
# the lane path (1, 3, 64: all terms, linv = 1), the first size of the MSM path, a ragged last wavefront, two proof blocks
BATCHES = [1, 3, 64, 65, 130]
# lg N = 6, r = 2: the hand-off to the tail stream at round max(6 - 2, r + 2) = 4, the pair right after the fold's own (the H side's
# power tables travel with the job's copies), and no hand-off at all
TAIL = [2, 0]


def _ipa_create_random_factors(lib, n=64):
    """bpr1cs_ipa_create with RANDOM factor vectors (no closed form: all 2^r terms, linv = 1) == the oracle's, for every split of the
    rounds between tables and variable-base that changes the path"""
    from pyref.ed import L, BASEPOINT
    from pyref.merlin import Transcript
    from pyref.r1cs import ipa_create
    rnd = random.Random(6400 + n)
    obp = common.oracle_gens(n)
    gens = bp.Gens(n, lib=lib, window_bits=8)
    a, b, gf, hf = ([rnd.randrange(1, L) for _ in range(n)] for _ in range(4))
    Q = BASEPOINT * rnd.randrange(1, L) + obp.G[1] * 5
    T = Transcript(b"fold-unit-ipa")
    ipp = ipa_create(T, Q, gf, hf, obp.G[:n], obp.H[:n], a, b)
    after = T.challenge_bytes(b"after", 32)
    for unfold in (4, 2, 1):
        gens.set_option(bp.OPT_UNFOLD_ROUNDS, unfold)
        t = bp.Transcript(b"fold-unit-ipa", lib=lib)
        Ls, Rs, af, bf = bp.ipa_create(gens, t, Q.compress(), gf, hf, a, b)
        assert Ls == ipp.L_vec and Rs == ipp.R_vec and (af, bf) == (ipp.a, ipp.b), unfold
        assert t.challenge_bytes(b"after", 32) == after


# ---- CPU simulator
@pytest.mark.parametrize("r,N", UNFOLD_CAP)
def test_unfold_and_capacity(sim_lib, sim_glib, r, N):
    _check(sim_lib, sim_glib, N, 65, r)


@pytest.mark.parametrize("r,N", LAST_ROUNDS)
def test_last_rounds_after_the_fold(sim_lib, sim_glib, r, N):
    _check(sim_lib, sim_glib, N, 65, r)


@pytest.mark.parametrize("B", BATCHES)
def test_batch_sizes(sim_lib, sim_glib, B):
    _check(sim_lib, sim_glib, 16, B, 2)


@pytest.mark.parametrize("tail", TAIL)
def test_tail_hand_off(sim_lib, sim_glib, tail):
    _check(sim_lib, sim_glib, 64, 65, 2, tail_rounds=tail)


def test_ipa_create_random_factors(sim_lib):
    _ipa_create_random_factors(sim_lib)


# ---- the same cases on the device
@pytest.mark.gpu
@pytest.mark.parametrize("r,N", UNFOLD_CAP)
def test_gpu_unfold_and_capacity(hip_lib, hip_glib, r, N):
    _check(hip_lib, hip_glib, N, 65, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r,N", LAST_ROUNDS)
def test_gpu_last_rounds_after_the_fold(hip_lib, hip_glib, r, N):
    _check(hip_lib, hip_glib, N, 65, r)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
def test_gpu_batch_sizes(hip_lib, hip_glib, B):
    _check(hip_lib, hip_glib, 16, B, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("tail", TAIL)
def test_gpu_tail_hand_off(hip_lib, hip_glib, tail):
    _check(hip_lib, hip_glib, 64, 65, 2, tail_rounds=tail)


@pytest.mark.gpu
def test_gpu_ipa_create_random_factors(hip_lib):
    _ipa_create_random_factors(hip_lib)
