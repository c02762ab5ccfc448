"""The verifiers on the CALLER'S transcripts (include/bpr1cs.h, BPR1CS_LABEL_TRANSCRIPTS; the Python keyword `transcripts=`): the case
table, the mirror and the checkers shared by the CPU simulator (tests/test_verify_transcripts.py) and the device
(tests/test_gpu_verify_transcripts.py).

Yardstick: the oracle only.  pyref.merlin.Transcript advanced by the same messages as the library's handle, pyref.r1cs.Prover(PC, t) and
Verifier(t) on it (both take a transcript), the cross-proof weights of tests/verify_scalar_cases.py (imported, not copied; with public
inputs: tests/public_input_cases.weights).  That file's _replay hard-wires Transcript(case.label): the replay here takes the messages
the transcript holds before the proof - a CONTEXT, a tuple of ("m", label, message) / ("c", label, length) steps on Transcript(LABEL).

Statements: S.bound_check(37 + j, 10, 100, 7) on capacity 16 (n = 14, N = 16); proof j of a batch proves statement j % 64 with blindings and
a seed of its own.  Proofs are made by the library (bpr1cs_prove_batch_transcripts on the same contexts); where a checker says so they
are ALSO made by the oracle's Prover and compared byte for byte.  What the verifier must say about them comes from the oracle alone."""
import ctypes
import hashlib

from pyref import scenarios as S
from pyref.ed import L, decompress, sc_to_bytes
from pyref.merlin import Transcript
from pyref.r1cs import Prover, R1CSProof, Verifier
import common
import public_input_cases as PI
import verify_group_cases as VG
import verify_scalar_cases as VS

bp = common.bp
PC = common.PC
CAP = 16
LABEL = b"verify transcripts"
RATE = 166                      # STROBE-128: positions 0 .. 165 of the rate
FLAG = bp.LABEL_TRANSCRIPTS
INVALID_ARGUMENT, INVALID_GENERATORS_LENGTH = -17, -1
T_X = 1 + 8 * 32                # offset of the scalar t_x in a proof
SIM_POSITIONS = (0, 1, 7, 8, 9, 63, 64, 163, 164, 165)
FORM_SIZES = (1, 8, 9, 16, 17, 64, 65)      # host replay <= 8 < lockstep launch <= 16 < a lane per proof; 64 / 65: a wavefront and one more
BARE = ()


def ctx(k):
    return (("m", b"ctx", bytes(k)),)


def squeezed(k):
    """a message and a challenge drawn after it: the state after a squeeze"""
    return (("m", b"ctx", bytes(k)), ("c", b"nonce", 32))


def advance(t, ops):
    """the oracle's Transcript and the library's have the same two methods"""
    for kind, label, x in ops:
        if kind == "m":
            t.append_message(label, x)
        else:
            t.challenge_bytes(label, x)
    return t


def oracle_t(ops, label=LABEL):
    return advance(Transcript(label), ops)


def lib_t(lib, ops, label=LABEL):
    return advance(bp.Transcript(label, lib=lib), ops)


def handles(lib, ctxs, label=LABEL):
    return [lib_t(lib, c, label) for c in ctxs]


def probe(t):
    """what a transcript (either kind) would answer next, without advancing it"""
    return t.clone().challenge_bytes(b"probe", 32)


def positions():
    """length k of the ("ctx", bytes(k)) message -> position in the STROBE rate of a transcript that holds it, for k = 0 .. 167"""
    return [oracle_t(ctx(k)).strobe.pos for k in range(168)]


def sim_lengths():
    pos = positions()
    return [pos.index(p) for p in SIM_POSITIONS]


def scen(j):
    return S.bound_check(37 + j % 64, 10, 100, 7)


CASE = VS.Case(scen(0), CAP)      # the verifier's side does not depend on the value


def blindings(j):
    return [S.synth_scalar(b"vtb%d" % j, i) for i in range(3)]


def prover_seed(j):
    return S.synth_seed(5000 + j)


def vseeds(tag, B):
    return [hashlib.sha256(b"vt seed " + tag + b" %d" % j).digest() for j in range(B)]


def flip(proof):
    """bit 0 of t_x: the proof stays well-formed unless t_x = l - 1, only the equation rejects it"""
    out = VG.flip(proof, T_X)
    assert int.from_bytes(out[T_X:T_X + 32], "little") < L
    return out


# ---------------------------------------------------------------- the oracle's side
def oracle_prove(j, t):
    """the oracle's Prover of statement j on the transcript t (advanced as upstream's `&mut`) -> (proof, commitments)"""
    p = Prover(PC, t)
    comms = scen(j).build_prover(p, blindings(j))
    return p.prove(common.oracle_gens(CAP), prover_seed(j)).to_bytes(), comms


def scalars_on(t, proof, comms, seed, case=CASE):
    """the oracle's Verifier on the transcript t, which it leaves in the state after the last inner-product challenge (build_rng works
    on a clone) -> (scalars, own points, N, index of the B scalar, bind value) as tests/verify_scalar_cases._replay"""
    pf = R1CSProof.from_bytes(proof)
    v = Verifier(t)
    case.scenario.build_verifier(v, list(comms)[:case.visible], PC)
    scalars, comp, tail, N = v.verification_scalars(pf, VS._Capacity(case.cap), seed)
    assert v.transcript is t
    k = 11 + len(v.V)
    assert len(comp) == k and len(scalars) == k + 2 + 2 * N + len(tail)
    own = [(i, comp[i]) for i in range(k) if not 3 <= i <= 5]
    own += [(k + 2 + 2 * N + i, x) for i, x in enumerate(tail)]
    c = t.clone()
    c.append_message(b"ipp_a", sc_to_bytes(pf.ipp_proof.a))
    c.append_message(b"ipp_b", sc_to_bytes(pf.ipp_proof.b))
    return scalars, own, N, k, c.challenge_bytes(b"bpr1cs-bind", 32)


def accepted(rep, cap=CAP):
    """the mega-check of a replay: verification_scalars + the C oracle's multiscalar multiplication"""
    scalars, own, N, k, _ = rep
    assert all(decompress(pt) is not None for _, pt in own)
    sc = [scalars[i] for i, _ in own] + scalars[k:k + 2 + 2 * N]
    return VS.coracle().msm(sc, [pt for _, pt in own] + VS.shared_bases(cap, N)) == bytes(32)


_REPLAYS = {}


def replay(ops, proof, comms, seed, case=CASE, label=LABEL):
    """a proof verified from the context `ops` -> (replay, accepted, probe of the verifier's transcript afterwards); once per input"""
    key = (ops, proof, tuple(comms), seed, id(case), label)
    if key not in _REPLAYS:
        t = oracle_t(ops, label)
        rep = scalars_on(t, proof, comms, seed, case)
        _REPLAYS[key] = (rep, accepted(rep, case.cap), probe(t))
    return _REPLAYS[key]


def expected_scalars(reps, batch_seed, index_base, pubs=None):
    """-> ((2N + 2) x 32 bytes, own-points sum) of a well-formed batch, as verify_scalar_cases._expected"""
    binds = [r[4] for r in reps]
    rho = VS.weights(binds, batch_seed, index_base) if pubs is None else PI.weights(binds, pubs, batch_seed, index_base)
    N = reps[0][2]
    out = b"".join(sc_to_bytes(sum(w * r[0][r[3] + i] for w, r in zip(rho, reps)) % L) for i in range(2 * N + 2))
    sc, pts = [], []
    for w, (scalars, own, _, _, _) in zip(rho, reps):
        sc += [w * scalars[i] % L for i, _ in own]
        pts += [pt for _, pt in own]
    return out, VS.coracle().msm(sc, pts)


# ---------------------------------------------------------------- the library's side
class Env:
    """per library: the circuit, a default handle, a handle whose transcripts always replay on the device, proofs made once"""

    def __init__(self, lib, glib):
        self.lib = lib
        self.circ = bp.CompiledGadget("bound_check", [7, 10, 0, 100, 0], [], lib=lib, glib=glib)
        self.gens = bp.Gens(CAP, lib=lib)
        self.dev = bp.Gens(CAP, lib=lib, host_chain_proofs=0)
        self._made = {}

    def prove(self, items):
        """items: (statement j, context) -> proofs, commitments, probes of the prover's handles afterwards; the missing ones in ONE call"""
        todo = [it for it in dict.fromkeys(items) if it not in self._made]
        if todo:
            ts = handles(self.lib, [c for _, c in todo])
            enc = lambda xs: b"".join(sc_to_bytes(x) for x in xs)
            vals = b"".join(enc((37 + j % 64, 27 + j % 64, 63 - j % 64)) for j, _ in todo)
            P, C = bp.prove_batch_transcripts(self.gens, self.circ, ts, vals, b"".join(enc(blindings(j)) for j, _ in todo),
                                              b"".join(prover_seed(j) for j, _ in todo), len(todo))
            for it, p, c, t in zip(todo, P, C, ts):
                self._made[it] = (p, c, probe(t))
        made = [self._made[it] for it in items]
        return [m[0] for m in made], [m[1] for m in made], [m[2] for m in made]


_ENVS = {}


def env(lib, glib):
    if id(lib) not in _ENVS:
        _ENVS[id(lib)] = Env(lib, glib)
    return _ENVS[id(lib)]


def verify(gens, circ, ts, P, C, seeds, **opts):
    """bp.verify_batch on the caller's transcripts; opts: handle options for this call"""
    try:
        for k, v in opts.items():
            gens.set_option(k, v)
        return bp.verify_batch(gens, circ, None, P, C, len(P), seeds=b"".join(seeds), transcripts=ts)
    finally:
        for k in opts:
            gens.set_option(k, -1)


# ---------------------------------------------------------------- 1. every starting position
def check_positions_table():
    """the lengths 0 .. 167 reach all 166 positions of the rate, position 0 at one length only"""
    pos = positions()
    assert set(pos) == set(range(RATE)), sorted(set(range(RATE)) - set(pos))
    assert pos.count(0) == 1
    assert sorted(pos[k] for k in sim_lengths()) == sorted(SIM_POSITIONS)


def check_sweep(e, ctxs, tag, oracle_made=()):
    """ONE batch, proof i from its own handle in context ctxs[i]: bpr1cs_verify_batch_scalars == the mirror byte for byte, every verdict 1,
    every verifier handle afterwards == the oracle's verifier transcript == the prover's handle; the proofs `oracle_made` are also the
    oracle's Prover's, byte for byte"""
    B = len(ctxs)
    P, C, prover_probes = e.prove([(i, c) for i, c in enumerate(ctxs)])
    for i in oracle_made:
        t = oracle_t(ctxs[i])
        assert oracle_prove(i, t) == (P[i], C[i]), "proof %d (context %r) is not the oracle's" % (i, ctxs[i])
        assert probe(t) == prover_probes[i]
    seeds, bseed = vseeds(tag, B), hashlib.sha256(b"vt batch seed " + tag).digest()
    reps = [replay(ctxs[i], P[i], C[i], seeds[i]) for i in range(B)]
    assert all(r[1] for r in reps), "the oracle rejects %r" % [i for i in range(B) if not reps[i][1]]
    want = expected_scalars([r[0] for r in reps], bseed, 3)
    ts = handles(e.lib, ctxs)
    got = bp.verify_batch_scalars(e.gens, e.circ, None, P, C, B, batch_seed=bseed, index_base=3, seeds=b"".join(seeds), transcripts=ts)
    assert got[2] is True and got[1] == want[1], "%s: own-points sum / wellformed" % tag.decode()
    if got[0] != want[0]:
        diff = [i for i in range(2 * CAP + 2) if got[0][32 * i:32 * i + 32] != want[0][32 * i:32 * i + 32]]
        raise AssertionError("%s: %d combined scalars differ, first at %r" % (tag.decode(), len(diff), diff[:8]))
    ts2 = handles(e.lib, ctxs)
    assert verify(e.gens, e.circ, ts2, P, C, seeds) == [True] * B
    for i in range(B):
        assert probe(ts[i]) == probe(ts2[i]) == reps[i][2] == prover_probes[i], "handle %d (context %r) afterwards" % (i, ctxs[i])


# ---------------------------------------------------------------- 2. wrong context
def check_wrong_context(e):
    own = [ctx(3), ctx(4), ctx(5)]
    P, C, _ = e.prove([(i, c) for i, c in enumerate(own)])
    used = [ctx(3), ctx(5), BARE]          # its own prefix; a neighbour's; the bare label
    seeds = vseeds(b"wrong", 3)
    want = [replay(used[i], P[i], C[i], seeds[i])[1] for i in range(3)]
    assert want == [True, False, False]
    assert verify(e.gens, e.circ, handles(e.lib, used), P, C, seeds) == want


# ---------------------------------------------------------------- 3. shared handle
def check_shared_handle(e):
    c = squeezed(9)
    P, C, _ = e.prove([(j, c) for j in range(3)])
    seeds = vseeds(b"shared", 3)
    t, twin = lib_t(e.lib, c), lib_t(e.lib, c)
    assert verify(e.gens, e.circ, t, P, C, seeds) == [True] * 3            # count = 1 < batch
    assert probe(t) == probe(twin), "a shared handle was touched"
    assert verify(e.gens, e.circ, t, P[:1], C[:1], seeds[:1]) == [True]    # count = 1 = batch
    assert probe(t) == replay(c, P[0], C[0], seeds[0])[2] != probe(twin), "the one handle of a batch of one is advanced"


# ---------------------------------------------------------------- 4. replay forms
def forms_batch(e, B):
    """B proofs with per-proof contexts, one with a flipped bit in t_x, one verified from a context nobody proved from (B = 1: the valid proof
    only) -> (contexts to verify from, proofs, commitments, seeds, the bad positions)"""
    ctxs = [ctx(k) for k in range(B)]
    P, C, _ = e.prove([(i, c) for i, c in enumerate(ctxs)])
    bad = set()
    if B > 1:
        fl, wr = (B - 1) // 2, B - 1
        P[fl] = flip(P[fl])
        ctxs[wr] = ctx(200)
        bad = {fl, wr}
    return ctxs, P, C, vseeds(b"forms", B), bad


def check_forms(e, B, device_replay=False):
    """verdicts == the oracle's, and the after-states of ALL handles == the oracle's replay of the same bytes, rejected proofs included"""
    ctxs, P, C, seeds, bad = forms_batch(e, B)
    reps = [replay(ctxs[i], P[i], C[i], seeds[i]) for i in range(B)]
    assert [r[1] for r in reps] == [i not in bad for i in range(B)]
    runs = [(ctxs, P)]
    if B == 1:      # a batch of one holds one proof: the two bad ones in calls of their own
        runs += [(ctxs, [flip(P[0])]), ([ctx(200)], P)]
    for cs, pf in runs:
        want = [replay(cs[i], pf[i], C[i], seeds[i]) for i in range(B)]
        ts = handles(e.lib, cs)
        assert verify(e.dev if device_replay else e.gens, e.circ, ts, pf, C, seeds) == [w[1] for w in want]
        assert [probe(t) for t in ts] == [w[2] for w in want], "B = %d: states afterwards" % B
    assert B == 1 or not all(w[1] for w in want)


# ---------------------------------------------------------------- 5. grouped
def check_grouped(e, B, G):
    """bad proofs first, last and in the middle; fallback 0, 1, 2: the verdicts of the per-proof path on a default handle (fallback 0:
    the group verdicts), and the same after-states under every mode - the handles are written once, from the first replay"""
    ctxs = [ctx(k) for k in range(B)]
    P, C, _ = e.prove([(i, c) for i, c in enumerate(ctxs)])
    bad = {0, B // 2, B - 1}
    P[0], P[B - 1] = flip(P[0]), flip(P[B - 1])
    ctxs[B // 2] = ctx(200)
    seeds = vseeds(b"grouped", B)
    ts = handles(e.lib, ctxs)
    ref = verify(e.gens, e.circ, ts, P, C, seeds)
    assert ref == [i not in bad for i in range(B)]
    after = [probe(t) for t in ts]
    for i in sorted(bad) + [1]:
        assert after[i] == replay(ctxs[i], P[i], C[i], seeds[i])[2]
    for fb in (0, 1, 2):
        ts = handles(e.lib, ctxs)
        got = verify(e.gens, e.circ, ts, P, C, seeds, verify_group=G, verify_group_fallback=fb)
        assert got == (VG.group_verdicts(B, G, bad) if fb == 0 else ref), "G = %d, fallback %d: %r" % (G, fb, got)
        assert [probe(t) for t in ts] == after, "G = %d, fallback %d: states afterwards" % (G, fb)


# ---------------------------------------------------------------- 6. combined and sharded
def check_combined_and_sharded(e):
    B = 5
    ctxs = [squeezed(10 + i) for i in range(B)]
    P, C, _ = e.prove([(i, c) for i, c in enumerate(ctxs)])
    seeds, bseed = vseeds(b"combined", B), hashlib.sha256(b"vt combined").digest()
    bad = list(P)
    bad[2] = flip(bad[2])
    kw = dict(batch_seed=bseed, index_base=7, seeds=b"".join(seeds))
    assert bp.verify_batch_combined(e.gens, e.circ, None, P, C, B, transcripts=handles(e.lib, ctxs), **kw) == (bytes(32), True)
    pt, wf = bp.verify_batch_combined(e.gens, e.circ, None, bad, C, B, transcripts=handles(e.lib, ctxs), **kw)
    assert wf is True and pt != bytes(32)
    for pf, want in ((P, True), (bad, False)):
        ts = handles(e.lib, ctxs)
        assert bp.verify_batch_sharded(e.gens, e.circ, None, pf, C, B, comm=None, transcripts=ts, **kw) is want
        assert [probe(t) for t in ts] == [replay(ctxs[i], pf[i], C[i], seeds[i])[2] for i in range(B)]


def check_public_inputs(lib, name="p3", B=3):
    """a seeded circuit of tests/public_input_cases.py with p > 0: the mirror's leaves absorb the public inputs, the scalars match"""
    assert PI.npub(name) > 0
    inp = PI.Inputs(name, B)
    g, circ, label = PI.gens(lib, PI.CIRCUITS[name][4]), PI.circuit(lib, name), PI.label(name)
    ctxs = [ctx(20 + j) for j in range(B)]
    P, C = bp.prove_batch_transcripts(g, circ, handles(lib, ctxs, label), inp.values, inp.blindings, inp.seeds, B, wires=inp.wires, publics=inp.publics)
    seeds, bseed = vseeds(b"public", B), hashlib.sha256(b"vt public").digest()
    cases = [PI.case(name, inp.pub[j]) for j in range(B)]
    reps = [replay(ctxs[j], P[j], C[j], seeds[j], cases[j], label) for j in range(B)]
    assert all(r[1] for r in reps)
    want = expected_scalars([r[0] for r in reps], bseed, 1 << 32, [PI.enc(p) for p in inp.pub])
    ts = handles(lib, ctxs, label)
    got = bp.verify_batch_scalars(g, circ, None, P, C, B, batch_seed=bseed, index_base=1 << 32, seeds=b"".join(seeds), publics=inp.publics, transcripts=ts)
    assert got == (want[0], want[1], True)
    assert [probe(t) for t in ts] == [r[2] for r in reps]
    assert expected_scalars([r[0] for r in reps], bseed, 1 << 32) != want, "the public message changes nothing"


# ---------------------------------------------------------------- 7. composition
def check_composition(e):
    """prove A then B on ONE prover handle, verify A then B on ONE verifier handle: both accepted, in the other order both rejected;
    prover, verifier and oracle (two Provers / two Verifiers on one transcript each) end in the same state"""
    c = ctx(11)
    enc = lambda xs: b"".join(sc_to_bytes(x) for x in xs)
    tp, made = lib_t(e.lib, c), []
    for j in (1, 2):
        P, C = bp.prove_batch_transcripts(e.gens, e.circ, [tp], enc((37 + j, 27 + j, 63 - j)), enc(blindings(j)), prover_seed(j), 1)
        made.append((P[0], C[0]))
    op = oracle_t(c)
    assert [oracle_prove(j, op) for j in (1, 2)] == made, "the library's two proofs on one transcript are not the oracle's"
    seeds = vseeds(b"composition", 2)
    for order, want in (((0, 1), True), ((1, 0), False)):
        tv, ov = lib_t(e.lib, c), oracle_t(c)
        for i in order:
            assert accepted(scalars_on(ov, made[i][0], made[i][1], seeds[i])) is want
            assert verify(e.gens, e.circ, [tv], [made[i][0]], [made[i][1]], [seeds[i]]) == [want]
            assert probe(tv) == probe(ov)
        if want:
            assert probe(tv) == probe(tp) == probe(op)


# ---------------------------------------------------------------- 8. refusals
def check_refusals(e):
    """every refusal is BPR1CS_ERR_INVALID_ARGUMENT and leaves every handle where it was; so does a call that fails for another reason"""
    B = 3
    ctxs = [ctx(30 + i) for i in range(B)]
    P, C, _ = e.prove([(i, c) for i, c in enumerate(ctxs)])
    ts = handles(e.lib, ctxs)
    extra = lib_t(e.lib, ctx(40))
    before = [probe(t) for t in ts + [extra]]
    seeds = b"".join(vseeds(b"refusals", B))
    calls = dict(batch=lambda g, t: bp.verify_batch(g, e.circ, None, P, C, B, seeds=seeds, transcripts=t),
                 combined=lambda g, t: bp.verify_batch_combined(g, e.circ, None, P, C, B, seeds=seeds, transcripts=t),
                 scalars=lambda g, t: bp.verify_batch_scalars(g, e.circ, None, P, C, B, seeds=seeds, transcripts=t),
                 sharded=lambda g, t: bp.verify_batch_sharded(g, e.circ, None, P, C, B, seeds=seeds, transcripts=t))
    lists = dict(count0=[], count2=ts[:2], count4=ts + [extra], null=[ts[0], None, ts[2]], duplicate=[ts[0], ts[1], ts[0]])

    def refused(what, fn, code):
        try:
            fn()
        except bp.R1CSError as err:
            assert err.code == code, "%s: %d" % (what, err.code)
        else:
            raise AssertionError("%s went through" % what)
        assert [probe(t) for t in ts + [extra]] == before, "%s: a handle moved" % what
    for cname, call in calls.items():
        for lname, lst in lists.items():
            refused(cname + "/" + lname, lambda: call(e.gens, lst), INVALID_ARGUMENT)
        small = bp.Gens(CAP // 2, lib=e.lib)        # fails for a reason of its own, after the list was accepted
        refused(cname + "/small generators", lambda: call(small, ts), INVALID_GENERATORS_LENGTH)
    # the flag on the two prove entry points that take a label
    lib = e.lib
    arr = (ctypes.c_void_p * B)(*[t.h for t in ts])
    as_label = ctypes.cast(arr, ctypes.c_char_p)
    enc = lambda xs: b"".join(sc_to_bytes(x) for x in xs)
    vals = b"".join(enc((37 + j, 27 + j, 63 - j)) for j in range(B))
    bls, ps = b"".join(enc(blindings(j)) for j in range(B)), b"".join(prover_seed(j) for j in range(B))
    out, cm, job = ctypes.create_string_buffer(B * e.circ.proof_len), ctypes.create_string_buffer(B * 96), ctypes.c_void_p()
    for count in (B, 1):
        assert lib.bpr1cs_prove_batch(e.gens.h, e.circ.h, as_label, FLAG | count, vals, bls, ps, None, B, out, cm) == INVALID_ARGUMENT
        assert lib.bpr1cs_prove_batch_begin(e.gens.h, e.circ.h, as_label, FLAG | count, vals, bls, ps, None, B, ctypes.byref(job)) == INVALID_ARGUMENT
        assert not job.value
    assert [probe(t) for t in ts + [extra]] == before
    assert calls["batch"](e.gens, ts) == [True] * B      # and the same lists are good for a call that is not refused
