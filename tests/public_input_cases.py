"""Per-proof public inputs (BPR1CS_VAR_PUBLIC, include/bpr1cs.h "Public inputs"): circuits, mirrors and checkers shared by the CPU
simulator (tests/test_public_inputs.py) and the device (tests/test_gpu_public_inputs.py).

The oracle knows no public inputs, and needs none: a proof over public inputs p_0 .. p_{p-1} is, byte for byte, the proof of the BAKED
circuit - the same rows with every term coeff x Public(k) replaced by One x (coeff x p_k) - and a verifier of the baked circuit accepts it.
That identity is the oracle of everything here.  One seeded `_build` emits both forms of a circuit: driven by the oracle's Prover /
Verifier with pub[k] = One() * p_k it is proof j's baked circuit; driven by the oracle's Verifier (which only collects rows) with
pub[k] = Variable(5, k) it yields the rows - and the witness program - the library gets ONCE for all proofs.

Circuits (random constraint systems in the style of tests/random_circuits.py, n <= 16, window_bits = 8): multipliers over random
combinations of committed values, the constant, earlier wires and public inputs; rows that hold for every witness because each is closed
by a "closing" multiplier (e, 0) whose left wire is the value of the row's combination - so no row carries a constant that depends on the
witness, and every public input is free; one wide row over every used public input (the only place 70 of them fit on 4 multipliers).
Public inputs, committed values, blindings and seeds differ from proof to proof.

Verifier expectations: pyref's Verifier.verification_scalars on proof j's baked circuit (tests/verify_scalar_cases._replay), the C
oracle's multiscalar multiplication for the identity test, and `weights` below - verify_scalar_cases.weights re-stated with the
("public", p_j,0 || .. || p_j,p-1) message the leaves absorb behind each proof's binding value."""
import hashlib
import os
import random

from pyref import scenarios as S
from pyref.ed import L, decompress, sc_to_bytes
from pyref.merlin import Transcript, VerificationError
from pyref.r1cs import LinearCombination, One, Prover, R1CSError, Variable, Verifier
import common
import random_circuits as rc
import verify_scalar_cases as VS
import witness_check_cases as WC

bp = common.bp
PC = common.PC
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = 5
NONCANONICAL = L.to_bytes(32, "little")        # l itself: the smallest non-canonical encoding

# name -> (seed, multiply gates, committed values, closed random rows, capacity, public indices used).  n = gates + rows + 1.
CIRCUITS = {
    "p1": (11, 4, 2, 3, 8, [0]),                       # one public input; n = 8 = N
    "p3": (12, 8, 3, 4, 16, [0, 2]),                   # index 1 is never used: p = 3 all the same; n = 13 of N = 16
    "p70": (13, 2, 1, 1, 4, list(range(70))),          # more public inputs than lanes of a wavefront; n = 4
    "m0": (14, 2, 0, 1, 4, [0, 1]),                    # no committed value: the public block is all the commitments array holds
}


def npub(name):
    return 1 + max(CIRCUITS[name][5])


def label(name):
    return b"PublicInputs-" + name.encode()


def _build(name, cs, cv, pub):
    """the same sequence of calls whoever `cs` is; pub: index -> LinearCombination standing for that public input.
    -> ops: per multiplier ("mul", left, right) or ("close", e), the combinations as they were handed to `cs`"""
    seed, n_mul, m, rows, cap, used = CIRCUITS[name]
    rr = random.Random(seed * 7919 + 5)
    pool = list(cv) + [One()]
    ops = []

    def coeff():
        return rr.choice([0, 1, L - 1, 2, L - 2]) if rr.random() < 0.3 else rr.randrange(L)

    def lc(k):
        out = LinearCombination()
        for _ in range(k):
            if rr.random() < 0.4:
                out = out + pub[rr.choice(used)] * (coeff() or 3)     # (a public term with coefficient 0 is refused: check_create)
            else:
                out = out + rr.choice(pool) * coeff()
        return out

    def close(e):
        val = cs.evaluate_lc(e)                 # the Prover's value; None for a Verifier
        l, _, _ = cs.allocate_multiplier(None if val is None else (val, 0))
        cs.constrain(e - l)
        ops.append(("close", e))
        pool.append(l)
    for _ in range(n_mul):
        la, lb = lc(rr.randrange(0, 4)), lc(rr.randrange(1, 5))
        l, r, o = cs.multiply(la, lb)
        ops.append(("mul", la, lb))
        pool.extend([l, r, o])
    for _ in range(rows):
        close(lc(rr.choice([0, 1, 2, 6])))
    e = rr.choice(pool) * 1
    for k in used:                              # +1, -1 and general coefficients
        e = e + pub[k] * (1 if k % 3 == 0 else L - 1 if k % 3 == 1 else coeff() or 5)
    close(e)
    return ops


# ------------------------------------------------------------------ per-proof inputs
def values(name, j):
    m = CIRCUITS[name][2]
    return [S.synth_scalar(b"pi-v" + name.encode(), 16 * j + i) if (i + j) % 5 else (0, 1, L - 1)[j % 3] for i in range(m)]


def blindings(name, j):
    return [S.synth_scalar(b"pi-bl" + name.encode(), 16 * j + i) for i in range(CIRCUITS[name][2])]


def seed(j):
    return S.synth_seed(1000 + j)


def publics(name, j):
    """the p public inputs of proof j (ints); 0, 1 and l - 1 among them"""
    out = [S.synth_scalar(b"pi-p" + name.encode(), 128 * j + k) for k in range(npub(name))]
    out[j % len(out)] = (0, 1, L - 1, 2)[j % 4]
    return out


def enc(xs):
    return b"".join(sc_to_bytes(x % L) for x in xs)


def altered(pub, k, delta=1):
    out = list(pub)
    out[k] = (out[k] + delta) % L
    return out


# ------------------------------------------------------------------ the two forms
_SHAPES = {}


def shape(name):
    """the library's form: -> dict(n, m, p, rows with (5, k) terms, wops, lcs) from ONE pass of the oracle's Verifier"""
    if name not in _SHAPES:
        m = CIRCUITS[name][2]
        v = Verifier(Transcript(label(name)))
        cv = [v.commit(bytes(32)) for _ in range(m)]
        ops = _build(name, v, cv, {k: Variable(PUBLIC, k) * 1 for k in range(npub(name))})
        rows = [[((var[0], var[1]), c) for var, c in lc.terms] for lc in v.constraints]
        wops, lcs = [], []

        def add(e):
            lcs.append([((var[0], var[1]), c) for var, c in e.terms])
            return len(lcs) - 1
        for op in ops:
            wops.append((bp.W_LC, add(op[1]), bp.W_LC, add(op[2] if op[0] == "mul" else LinearCombination())))
        _SHAPES[name] = dict(n=v.num_vars, m=m, p=npub(name), rows=rows, wops=wops, lcs=lcs)
    return _SHAPES[name]


def baked(name, pub):
    """-> pyref Scenario of the baked circuit for the public inputs `pub` (values: the caller's)"""
    m = CIRCUITS[name][2]
    as_lc = {k: One() * (x % L) for k, x in enumerate(pub)}

    def bpv(pr, bl, vals=None):
        raise NotImplementedError      # (proofs are made by oracle_proof below, which needs the Prover object)

    def bv(vr, comms, pc):
        _build(name, vr, [vr.commit(c) for c in comms], as_lc)
    return S.Scenario(label(name), [0] * m, bpv, bv)


def case(name, pub):
    return VS.Case(baked(name, pub), CIRCUITS[name][4])


_PROOFS = {}


def oracle_proof(name, j, pub=None, prove=True):
    """the oracle's Prover on proof j's baked circuit -> dict(proof, comms, wires, values, blindings, constraints, n); prove=False:
    synthesis only (no proof)"""
    pub = publics(name, j) if pub is None else pub
    key = (name, j, tuple(pub), prove)
    if key not in _PROOFS:
        vals, bls = values(name, j), blindings(name, j)
        pr = Prover(PC, Transcript(label(name)))
        comms, cv = [], []
        for x, b in zip(vals, bls):
            c, var = pr.commit(x, b)
            comms.append(c)
            cv.append(var)
        _build(name, pr, cv, {k: One() * (x % L) for k, x in enumerate(pub)})
        out = dict(comms=comms, values=enc(vals), blindings=enc(bls), wires=enc(pr.a_L + pr.a_R + pr.a_O), n=len(pr.a_L),
                   constraints=[list(lc.terms) for lc in pr.constraints], proof=None)
        if prove:
            out["proof"] = pr.prove(common.oracle_gens(CIRCUITS[name][4]), seed(j)).to_bytes()
        _PROOFS[key] = out
    return _PROOFS[key]


# ------------------------------------------------------------------ library objects, one per (library, circuit)
_CTX = {}


def gens(lib, cap):
    if (id(lib), cap) not in _CTX:
        _CTX[(id(lib), cap)] = bp.Gens(cap, lib=lib, window_bits=8)
    return _CTX[(id(lib), cap)]


def circuit(lib, name, program=False):
    key = (id(lib), name, program)
    if key not in _CTX:
        sh = shape(name)
        _CTX[key] = bp.Circuit(sh["n"], sh["m"], sh["rows"], wops=sh["wops"] if program else None, lcs=sh["lcs"] if program else None, lib=lib)
        assert _CTX[key].p == sh["p"]
    return _CTX[key]


class Inputs:
    """B proofs' worth of everything a prove call takes; tampers: {proof: (public index, delta)}"""

    def __init__(self, name, B, tampers=None, first=0):
        js = range(first, first + B)
        obs = [oracle_proof(name, j, prove=False) for j in js]
        self.name, self.B = name, B
        self.values = b"".join(o["values"] for o in obs)
        self.blindings = b"".join(o["blindings"] for o in obs)
        self.seeds = b"".join(seed(j) for j in js)
        self.wires = b"".join(o["wires"] for o in obs)
        self.pub = [publics(name, j) for j in js]
        for j, (k, delta) in (tampers or {}).items():
            self.pub[j] = altered(self.pub[j], k, delta)
        self.publics = b"".join(enc(p) for p in self.pub)


def prove(lib, name, inp, entry="batch", program=False, **opts):
    """-> (proofs, commitments) through one of the prove entry points; opts: handle options for the call"""
    g, circ = gens(lib, CIRCUITS[name][4]), circuit(lib, name, program)
    wires = None if program else inp.wires
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        if entry == "batch":
            return bp.prove_batch(g, circ, label(name), inp.values, inp.blindings, inp.seeds, inp.B, wires=wires, publics=inp.publics)
        if entry == "transcripts":
            ts = [bp.Transcript(label(name), lib=lib) for _ in range(inp.B)]
            return bp.prove_batch_transcripts(g, circ, ts, inp.values, inp.blindings, inp.seeds, inp.B, wires=wires, publics=inp.publics)
        assert entry == "begin_end"     # two jobs in flight, each with its own tail block
        sh, h = shape(name), max(1, inp.B // 2)
        cut = lambda raw, sz, lo, hi: raw[lo * sz:hi * sz]
        jobs = [bp.ProveJob(g, circ, label(name), cut(inp.values, 32 * sh["m"], lo, hi), cut(inp.blindings, 32 * sh["m"], lo, hi),
                            cut(inp.seeds, 32, lo, hi), hi - lo, wires=None if program else cut(inp.wires, 96 * sh["n"], lo, hi),
                            publics=cut(inp.publics, 32 * sh["p"], lo, hi)) for lo, hi in ((0, h), (h, inp.B)) if hi > lo]
        P, C = [], []
        for job in jobs:
            p, c = job.finish()
            P += p
            C += c
        return P, C
    finally:
        for k in opts:
            g.set_option(k, -1)


def check_prover(lib, name, B, entry="batch", program=False, **opts):
    """the library's proofs and commitments of B proofs with distinct public inputs == the oracle's proofs of the B baked circuits"""
    P, C = prove(lib, name, Inputs(name, B), entry, program, **opts)
    for j in range(B):
        ob = oracle_proof(name, j)
        assert C[j] == ob["comms"], "%s: commitments of proof %d" % (name, j)
        assert P[j] == ob["proof"], "%s (%s%s): proof %d of %d differs from the oracle's proof of the baked circuit" % (
            name, entry, ", witness program" if program else "", j, B)


def check_noncanonical_prover(lib):
    """the circuit exists and the batch proves; the same batch with ONE public input replaced by l is BPR1CS_ERR_INVALID_ARGUMENT"""
    circuit(lib, "p3")
    inp = Inputs("p3", 3)
    P, _ = prove(lib, "p3", inp)
    assert P[1] == oracle_proof("p3", 1)["proof"]
    inp.publics = inp.publics[:32 * 4] + NONCANONICAL + inp.publics[32 * 5:]
    try:
        prove(lib, "p3", inp)
        assert False, "a non-canonical public input was proved"
    except bp.R1CSError as e:
        assert e.code == -17


def check_tail_length(lib):
    """the library cannot see how long the caller's arrays are: the Python wrappers size the tail block from Circuit.p - which must be
    the library's p, shown by every case above proving and verifying - and refuse a `publics` of any other length"""
    g, circ, inp = gens(lib, CIRCUITS["p3"][4]), circuit(lib, "p3"), Inputs("p3", 3)
    assert circ.p == 3 and len(inp.publics) == 3 * 3 * 32
    P, C = made(lib, "p3", 3)
    for pub in (None, b"", inp.publics[:-32], inp.publics + bytes(32), inp.publics[:3 * 32]):
        for call in (lambda: bp.prove_batch(g, circ, label("p3"), inp.values, inp.blindings, inp.seeds, 3, wires=inp.wires, publics=pub),
                     lambda: bp.ProveJob(g, circ, label("p3"), inp.values, inp.blindings, inp.seeds, 3, wires=inp.wires, publics=pub),
                     lambda: bp.verify_batch(g, circ, label("p3"), P, C, 3, publics=pub),
                     lambda: bp.verify_batch_combined(g, circ, label("p3"), P, C, 3, publics=pub),
                     lambda: bp.verify_batch_scalars(g, circ, label("p3"), P, C, 3, publics=pub)):
            try:
                call()
                assert False, "a tail block of %r bytes went through" % (None if pub is None else len(pub))
            except AssertionError as e:
                assert "publics" in str(e), e


# ------------------------------------------------------------------ witness check
def check_witness_check(lib, name, B, bad, k):
    """check_witness = 1, host wires, proof `bad` with public input k off by one: a refusal record naming what the pure-Python checker
    names on the baked circuit of the SUBMITTED public inputs; every other proof is the oracle's"""
    inp = Inputs(name, B, {bad: (k, 1)})
    P, C = prove(lib, name, inp, check_witness=1)
    sh = shape(name)
    n, m = sh["n"], sh["m"]
    for j in range(B):
        ob = oracle_proof(name, j, pub=inp.pub[j], prove=False)       # (rows with the constants as submitted; wires are the honest ones)
        want = WC.violations(dict(n=n, constraints=ob["constraints"]), inp.wires[96 * n * j:96 * n * (j + 1)], inp.values[32 * m * j:32 * m * (j + 1)])
        if j == bad:
            assert want is not None and want["gates"] == 0 and want["rows"] >= 1 and want["row"] is not None
            assert bp.refusal(P[j]) == want and P[j] == WC.record(len(P[j]), want), (bp.refusal(P[j]), want)
        else:
            assert want is None and P[j] == oracle_proof(name, j)["proof"], j
    assert bp.last_prove_stats(lib)["refused"] == 1
    return P


# ------------------------------------------------------------------ the verifier's mirror
def weights(binds, pubs, batch_seed, index_base):
    """tests/verify_scalar_cases.weights with the public message: pubs[b] = the p x 32 bytes of proof b (empty: no message)"""
    leaves = []
    for g in range((len(binds) + VS.BATCH_LEAF - 1) // VS.BATCH_LEAF):
        t = Transcript(b"bpr1cs batch leaf")
        t.append_u64(b"leaf", g)
        for b in range(VS.BATCH_LEAF * g, min(len(binds), VS.BATCH_LEAF * (g + 1))):
            t.append_message(b"proof", binds[b])
            if pubs[b]:
                t.append_message(b"public", pubs[b])
        leaves.append(t.challenge_bytes(b"leaf", 32))
    t = Transcript(b"bpr1cs batch verify")
    t.append_message(b"seed", batch_seed)
    t.append_u64(b"base", index_base)
    t.append_u64(b"count", len(binds))
    for leaf in leaves:
        t.append_message(b"leaf", leaf)
    digest = t.challenge_bytes(b"digest", 32)
    rho = []
    for b in range(len(binds)):
        t = Transcript(b"bpr1cs batch weight")
        t.append_message(b"digest", digest)
        t.append_u64(b"j", index_base + b)
        rho.append(t.challenge_scalar(b"rho"))
    return rho


_REPLAYS = {}


def replay(name, pub, proof, comms, sd):
    """verify_scalar_cases._replay on the baked circuit (its own cache does not know the public inputs)"""
    key = (name, tuple(pub), proof, tuple(comms), sd)
    if key not in _REPLAYS:
        _REPLAYS[key] = VS._replay(case(name, pub), proof, comms, sd)
    return _REPLAYS[key]


def oracle_accepts(name, pub, proof, comms, sd):
    """the oracle's verifier on the baked circuit: verification_scalars + the C oracle's multiscalar multiplication"""
    scalars, own, N, k, _ = replay(name, pub, proof, comms, sd)
    assert all(decompress(pt) is not None for _, pt in own)
    sc = [scalars[i] for i, _ in own] + scalars[k:k + 2 + 2 * N]
    pts = [pt for _, pt in own] + VS.shared_bases(CIRCUITS[name][4], N)
    return VS.coracle().msm(sc, pts) == bytes(32)


def expected_scalars(name, pubs, P, C, seeds, batch_seed, index_base):
    """-> ((2N + 2) x 32 bytes, own-points sum) as verify_scalar_cases._expected, with a baked circuit per proof and the public message"""
    reps = [replay(name, pub, pf, cm, sd) for pub, pf, cm, sd in zip(pubs, P, C, seeds)]
    rho = weights([r[4] for r in reps], [enc(p) for p in pubs], batch_seed, index_base)
    N = reps[0][2]
    out = b"".join(sc_to_bytes(sum(w * r[0][r[3] + i] for w, r in zip(rho, reps)) % L) for i in range(2 * N + 2))
    sc, pts = [], []
    for w, (scalars, own, _, _, _) in zip(rho, reps):
        sc += [w * scalars[i] % L for i, _ in own]
        pts += [pt for _, pt in own]
    return out, VS.coracle().msm(sc, pts)


# ------------------------------------------------------------------ the verifier forms
FORMS = ("per_proof", "group_fb1", "group_fb2")


def verdicts(lib, name, P, C, seeds, pub_bytes, form):
    g, circ = gens(lib, CIRCUITS[name][4]), circuit(lib, name)
    B = len(P)
    opts = {} if form == "per_proof" else dict(verify_group=4, verify_group_fallback=1 if form == "group_fb1" else 2)
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        return bp.verify_batch(g, circ, label(name), P, C, B, seeds=b"".join(seeds), publics=pub_bytes)
    finally:
        for k in opts:
            g.set_option(k, -1)


def combined(lib, name, P, C, seeds, pub_bytes, batch_seed, index_base=0):
    g, circ = gens(lib, CIRCUITS[name][4]), circuit(lib, name)
    return bp.verify_batch_combined(g, circ, label(name), P, C, len(P), batch_seed=batch_seed, index_base=index_base, seeds=b"".join(seeds), publics=pub_bytes)


def scalars(lib, name, P, C, seeds, pub_bytes, batch_seed, index_base=0):
    g, circ = gens(lib, CIRCUITS[name][4]), circuit(lib, name)
    return bp.verify_batch_scalars(g, circ, label(name), P, C, len(P), batch_seed=batch_seed, index_base=index_base, seeds=b"".join(seeds), publics=pub_bytes)


# (circuit, batch, proof with the bad public input, its index): batches 1, 3, 33 (two leaves), 70 (above a wavefront of proofs); p = 1, 3, 70
VERIFIER_CASES = [("p1", 1, 0, 0), ("p3", 3, 1, 2), ("p3", 3, 2, 1), ("m0", 3, 0, 1), ("p1", 33, 32, 0), ("p70", 70, 64, 69), ("p70", 3, 1, 64)]
_MADE = {}


def made(lib, name, B):
    """B proofs of the circuit with their right public inputs: the oracle's where a prover test has made them anyway (at most 5, and
    the 70 of "p70"), else the library's through the witness program - what the verifier must say about them is the mirror's business"""
    if (id(lib), name, B) not in _MADE:
        if B <= 5 or name == "p70":
            obs = [oracle_proof(name, j) for j in range(B)]
            P, C = [o["proof"] for o in obs], [o["comms"] for o in obs]
        else:
            P, C = prove(lib, name, Inputs(name, B), program=True)
        _MADE[(id(lib), name, B)] = (P, C)
    return _MADE[(id(lib), name, B)]


def check_verifier(lib, name, B, bad, k):
    """every verifier form over B proofs: right public inputs; public input k of proof `bad` altered; the same made non-canonical"""
    P, C = made(lib, name, B)
    pubs = [publics(name, j) for j in range(B)]
    seeds = [hashlib.sha256(b"pi-vseed %d" % j).digest() for j in range(B)]
    right = b"".join(enc(p) for p in pubs)
    tag = ("%s-%d" % (name, B)).encode()
    bseeds = (bytes(32), hashlib.sha256(b"pi batch seed " + tag).digest())     # a constant batch seed leaves the binding alone
    everyone = [True] * B
    # ---- right public inputs
    assert all(oracle_accepts(name, pubs[j], P[j], C[j], seeds[j]) for j in sorted({0, bad, B - 1}))
    for form in FORMS:
        assert verdicts(lib, name, P, C, seeds, right, form) == everyone, form
    own_right = None
    for bs in bseeds:
        assert combined(lib, name, P, C, seeds, right, bs) == (bytes(32), True)
        got = scalars(lib, name, P, C, seeds, right, bs, index_base=5)
        want = expected_scalars(name, pubs, P, C, seeds, bs, 5)
        assert got[2] is True and got[1] == want[1], "%s, B = %d: own-points sum" % (name, B)
        assert got[0] == want[0], "%s, B = %d: combined scalars differ from the mirror's" % (name, B)
        own_right = scalars(lib, name, P, C, seeds, right, bs)[1]
    # ---- one public input altered: the oracle's verifier of the baked circuit with that constant rejects the proof
    pubs_bad = list(pubs)
    pubs_bad[bad] = altered(pubs[bad], k)
    wrong = b"".join(enc(p) for p in pubs_bad)
    used = k in CIRCUITS[name][5]
    assert oracle_accepts(name, pubs_bad[bad], P[bad], C[bad], seeds[bad]) is (not used)
    want_v = [j != bad or not used for j in range(B)]
    for form in FORMS:
        assert verdicts(lib, name, P, C, seeds, wrong, form) == want_v, form
    pt, wf = combined(lib, name, P, C, seeds, wrong, bseeds[1])
    assert wf is True and (pt == bytes(32)) is (not used)
    got = scalars(lib, name, P, C, seeds, wrong, bseeds[1])
    assert got[:2] == expected_scalars(name, pubs_bad, P, C, seeds, bseeds[1], 0) and got[2] is True
    assert got[1] != own_right, "the weights do not depend on the public inputs"       # the binding is live (an unused index included)
    # ---- a non-canonical public input: that proof is malformed, the rest are judged
    off = 32 * (npub(name) * bad + k)
    nonc = right[:off] + NONCANONICAL + right[off + 32:]
    for form in FORMS:
        assert verdicts(lib, name, P, C, seeds, nonc, form) == [j != bad for j in range(B)], form
    assert combined(lib, name, P, C, seeds, nonc, bseeds[1])[1] is False
    assert scalars(lib, name, P, C, seeds, nonc, bseeds[1])[2] is False


# ------------------------------------------------------------------ p = 0: nothing changes
def check_no_publics(lib):
    """an existing random case (tests/random_circuits.CASES[0]) through the wrappers with and without an (empty) publics argument"""
    sd, n_mul, m, rows, cap, sat = rc.CASES[0]
    ob = common.oracle_batch(lambda j: rc.scenario(sd * 100 + j, n_mul, m, rows, sat), cap, 1, satisfiable=sat, key=("rc", sd))
    g, circ = gens(lib, cap), common.circuit_from_oracle(ob, lib)
    assert circ.p == 0
    for pub in (None, b"", []):
        P, C = bp.prove_batch(g, circ, ob["label"], ob["values"], ob["blindings"], ob["seeds"], 1, wires=ob["wires"], publics=pub)
        assert P == ob["proofs"] and C[0] == ob["comms"][0]
        assert bp.verify_batch(g, circ, ob["label"], P, C, 1, publics=pub) == [True]
        assert bp.verify_batch_combined(g, circ, ob["label"], P, C, 1, publics=pub) == (bytes(32), True)
    sc1 = bp.verify_batch_scalars(g, circ, ob["label"], P, C, 1, batch_seed=bytes(32), seeds=bytes(32), publics=None)
    case0 = VS.Case(rc.scenario(sd * 100, n_mul, m, rows, sat), cap)
    assert sc1[:2] == VS.expected(case0, P, C, [bytes(32)], bytes(32), 0)[:2]     # the derivation without the message, as pinned before


# ------------------------------------------------------------------ bpr1cs_circuit_create
def check_create(lib):
    """kind 5 is accepted and p is right; kind 6, an index >= 2^20 and a bit of a public input are BPR1CS_ERR_INVALID_ARGUMENT"""
    row = lambda *terms: [list(terms)]
    one = ((bp.VAR_ONE, 0), 1)
    for used, p in (([0], 1), ([0, 2], 3), (list(range(70)), 70)):
        c = bp.Circuit(1, 1, row(one, *[((bp.VAR_PUBLIC, k), 3 + k) for k in used]), lib=lib)
        assert c.p == p
    assert bp.Circuit(1, 1, row(((bp.VAR_PUBLIC, (1 << 20) - 1), 1)), lib=lib).p == 1 << 20
    # (a public term with coefficient 0, or l, says nothing and would still size every call's tail block: refused)
    for bad in (row(((6, 0), 1)), row(((bp.VAR_PUBLIC, 1 << 20), 1)), row(one, ((7, 0), 1)), row(one, ((bp.VAR_PUBLIC, 0), 0)),
                row(((bp.VAR_PUBLIC, 0), 2), ((bp.VAR_PUBLIC, 1), NONCANONICAL))):
        try:
            bp.Circuit(1, 1, bad, lib=lib)
            assert False, "accepted %r" % bad
        except bp.R1CSError as e:
            assert e.code == -17
    # a witness program: kind 5 in a linear combination is fine (and counts towards p); the bits of a public input are not on offer -
    # W_BIT / W_NOTBIT index the m committed values, and value row m + k is refused like any index >= m
    lcs = [[((bp.VAR_PUBLIC, 4), 1), ((bp.VAR_COMMITTED, 0), 2)], []]
    c = bp.Circuit(1, 1, [], wops=[(bp.W_LC, 0, bp.W_LC, 1)], lcs=lcs, lib=lib)
    assert c.p == 5
    for kind in (bp.W_BIT, bp.W_NOTBIT):
        for arg in ((1 + 0) << 8, ((1 + 4) << 8) | 3):
            try:
                bp.Circuit(1, 1, [], wops=[(kind, arg, bp.W_LC, 1)], lcs=lcs, lib=lib)
                assert False, "a bit of public input %d accepted" % ((arg >> 8) - 1)
            except bp.R1CSError as e:
                assert e.code == -17
    for bad_lc in ([((6, 0), 1)], [((bp.VAR_PUBLIC, 1 << 20), 1)], [((bp.VAR_COMMITTED, 0), 1), ((bp.VAR_PUBLIC, 0), 0)]):
        try:
            bp.Circuit(1, 1, [], wops=[(bp.W_LC, 0, bp.W_LC, 1)], lcs=[bad_lc, []], lib=lib)
            assert False, "accepted %r" % bad_lc
        except bp.R1CSError as e:
            assert e.code == -17


# ------------------------------------------------------------------ the front-end: tree gadgets compiled with the root public
def tree_witness(glib, arity, k):
    """tree k (leaves i -> i + 100 k for i in 1..5, Cube S-box, 2 partial rounds: the smallest trees of tests/frontend_cases.py) and the
    membership witness of leaf 1 + k in the gadget's commitment order -> (root, values, number of static commitments)"""
    levels = 4 if arity == 4 else 3
    t = bp.SparseMerkleTree(arity, levels, 2, glib=glib, inverse=False)
    for i in range(1, 6):
        t.update(i, i + 100 * k)
    idx = 1 + k
    leaf, nodes = t.get(idx)
    assert leaf == sc_to_bytes(idx + 100 * k)
    if arity == 4:
        return t.root(), leaf + sc_to_bytes(idx) + b"".join(nodes) + enc([0, 101]), 2
    bits = enc([(idx >> b) & 1 for b in range(levels)])
    return t.root(), leaf + bits + b"".join(reversed(nodes)) + enc([0, 101, 0, 0]), 4


def check_frontend(lib, glib, arity):
    """three membership proofs about three DIFFERENT trees in one call of the device witness program on ONE compiled circuit, each equal
    to the proof the baked front-end path makes for its tree (bpr1cs_gadget_prove_on, sp = [root_j]: host synthesis, the root a
    constant) and accepted by the baked verifier (bpr1cs_gadget_verify_on); a swapped pair of roots rejects both proofs"""
    gname, levels, cap, lab = ("vsmt_4", 4, 512, b"VSMT") if arity == 4 else ("vsmt_2", 3, 512, b"VSMT")
    ip = [levels, 2, 0]
    B = 3
    wit = [tree_witness(glib, arity, k) for k in range(B)]
    roots = [w[0] for w in wit]
    assert len(set(roots)) == B
    circ = bp.CompiledGadget(gname, ip, [], lib=lib, glib=glib)
    base = bp.CompiledGadget(gname, ip, [roots[0]], lib=lib, glib=glib)
    assert circ.p == 1 and base.p == 0 and circ.has_witness_program and (circ.n, circ.q, circ.m) == (base.n, base.q, base.m)
    m, statics = circ.m, wit[0][2]
    assert all(len(w[1]) == 32 * m for w in wit)
    g = gens(lib, cap)
    vals = b"".join(w[1] for w in wit)
    bls = b"".join(enc([S.synth_scalar(b"pi-tree-bl%d" % j, i) for i in range(m - statics)]) + bytes(32 * statics) for j in range(B))
    seeds = b"".join(seed(50 + j) for j in range(B))
    P, C = bp.prove_batch(g, circ, lab, vals, bls, seeds, B, wires=None, publics=b"".join(roots))
    for j in range(B):
        cut = lambda raw, sz: raw[j * sz:(j + 1) * sz]
        ref, refc, _ = bp.gadget_prove_on(g, gname, ip, [roots[j]], lab, cut(vals, 32 * m), cut(bls, 32 * m), m, 1, cut(seeds, 32), glib=glib)
        assert P[j] == ref[0], "arity %d: proof %d over the public root differs from the baked front-end's" % (arity, j)
        assert C[j] == refc[0]
        assert bp.gadget_verify_on(g, gname, ip, [roots[j]], lab, P[j], C[j], glib=glib)[0]
        assert not bp.gadget_verify_on(g, gname, ip, [roots[(j + 1) % B]], lab, P[j], C[j], glib=glib)[0]
    # the baked circuit through the device witness program as well: the same bytes (the description differs in the last row's root term only)
    Pb, _ = bp.prove_batch(g, base, lab, vals[:32 * m], bls[:32 * m], seeds[:32], 1, wires=None)
    assert Pb[0] == P[0]
    vs = b"".join(hashlib.sha256(b"pi-tree-vseed %d" % j).digest() for j in range(B))
    assert bp.verify_batch(g, circ, lab, P, C, B, seeds=vs, publics=b"".join(roots)) == [True] * B
    assert bp.verify_batch(g, circ, lab, P, C, B, seeds=vs, publics=b"".join([roots[1], roots[0], roots[2]])) == [False, False, True]
    assert bp.verify_batch(g, base, lab, P[:1], C[:1], 1, seeds=vs[:32]) == [True]
