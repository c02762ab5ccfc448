"""Bits of a linear combination (BPR1CS_W_LCBIT / BPR1CS_W_LCNOTBIT, include/bpr1cs.h) and the one-commitment bound check built on
them: circuits, the case table and the checkers shared by the CPU simulator (tests/test_derived_bits.py) and the device
(tests/test_gpu_derived_bits.py).

Every expectation is the oracle's.  One `_build` per circuit drives whoever `cs` is through a recorder (`Rec`): with the oracle's
Prover it allocates every multiplier with an assignment computed HERE, in Python integers - the value of a combination, its bit
(x >> k) & 1 of the canonical 0 <= x < l, the inverse x^(l-2) (0 for x = 0) - on proof j's BAKED circuit (public inputs folded into
One, the tests/public_input_cases.py pattern); with the oracle's Verifier and pub[k] = Variable(5, k) it yields the rows, the `wops`
and the `lcs` the library gets once for all proofs.  The library's proofs with wires=None (the device witness program) must be the
oracle's proof bytes, and the oracle's verifier of the baked circuit must accept them.

Circuits - the smallest shapes that reach each way the operand can go wrong:
  b8     bound_check_1 as host/frontend.cpp builds it, bits = 8: n = 16, m = 1, q = 34; bounds public (p = 2) and baked ("b8k")
  wide   multiply(v0, v1), then bits 0..252 of X = 5 x OUT + Public(0): n = 254 of N = 256.  Targets with bits set on both sides of every
         32-bit word boundary, l - 1 and 0.  The left wires of the first six bit multipliers name bit indices 253..255 of X instead of
         1 - bit: W_LCBIT reads 0, W_LCNOTBIT reads 1 (rows pin them)
  fence  combinations whose only wire is the OUT of the multiplier right before (the register cache / fence path of team_operand)
  swap   two combinations (one of 21 terms: more than the lanes of a team) named alternately, A, B, A, B, left and right of one
         multiplier taking different ones: the one-entry cache must be invalidated and refilled
  inv0   W_LC left, W_INV_LEFT right over v0 - Public(0), which is 0 for every other proof of the batch (neighbours in one team block),
         then bit 0 of the product wire: an "is zero" of a derived value"""
import hashlib
import json
import os

from pyref import scenarios as S
from pyref.ed import L, decompress, sc_to_bytes
from pyref.merlin import Transcript
from pyref.r1cs import LinearCombination, One, Prover, Variable, Verifier
import common
import public_input_cases as PI
import verify_scalar_cases as VS
import witness_check_cases as WC

bp = common.bp
PC = common.PC
ROOT = PI.ROOT
PUBLIC = 5
enc, NONCANONICAL = PI.enc, PI.NONCANONICAL

# name -> (committed values, public inputs, capacity)
CIRCUITS = {"b8": (1, 2, 16), "b8k": (1, 0, 16), "wide": (2, 1, 256), "fence": (1, 0, 8), "swap": (2, 1, 8), "inv0": (1, 1, 4)}
B8_BAKED = (1000, 1255)             # the bounds of "b8k"
# canonical values of X in "wide": every word 0x80000001 (the top word 0x08000001 < l's 0x10000000), l - 1 (the combination is -1), 0
WIDE_TARGETS = [sum((0x80000001 if w < 7 else 0x08000001) << (32 * w) for w in range(8)), L - 1, 0]


def label(name):
    return b"DerivedBits-" + name.encode()


# ------------------------------------------------------------------ the recorder
def lc(e):
    return ("lc", LinearCombination.of(e))


def bit(e, k):
    return ("bit", e, k)          # e: the SAME LinearCombination object for every bit of one value (one `lcs` entry per object)


def notbit(e, k):
    return ("notbit", e, k)


INV = ("inv",)


class Rec:
    def __init__(self, cs):
        self.cs, self.ops, self.prover = cs, [], isinstance(cs, Prover)

    def val(self, spec, left=None):
        if spec[0] == "lc":
            return self.cs.eval(spec[1])
        if spec[0] == "inv":
            return pow(left, L - 2, L)                     # Scalar::invert: 0 -> 0
        b = (self.cs.eval(spec[1]) >> spec[2]) & 1          # 0 <= x < l < 2^253: bits 253..255 are 0
        return b if spec[0] == "bit" else 1 - b

    def mul(self, lspec, rspec):
        asg = None
        if self.prover:
            l = self.val(lspec)
            asg = (l, self.val(rspec, l))
        self.ops.append((lspec, rspec))
        return self.cs.allocate_multiplier(asg)

    def multiply(self, la, lb):                            # cs.multiply, recorded
        la, lb = LinearCombination.of(la), LinearCombination.of(lb)
        l, r, o = self.mul(lc(la), lc(lb))
        self.cs.constrain(la - l)
        self.cs.constrain(lb - r)
        return l, r, o


def _decompose(rec, e, bits, odd_left=False):
    """positive_no_gadget_lc of host/gadgets.hpp: per bit (1 - bit, bit), out = 0, left + right = 1; at the end sum right_i 2^i = e.
    odd_left ("wide"): the left wires of multipliers 0..2 are W_LCBIT 253..255 (= 0), those of 3..5 W_LCNOTBIT 253..255 (= 1)"""
    cs, total = rec.cs, -e
    for i in range(bits):
        if odd_left and i < 3:
            l, r, o = rec.mul(bit(e, 253 + i), bit(e, i))
            cs.constrain(LinearCombination.of(l))
            cs.constrain(LinearCombination.of(o))
        elif odd_left and i < 6:
            l, r, o = rec.mul(notbit(e, 250 + i), bit(e, i))
            cs.constrain(l - One())
            cs.constrain(o - r)
        else:
            l, r, o = rec.mul(notbit(e, i), bit(e, i))
            cs.constrain(LinearCombination.of(o))
            cs.constrain(l + r - One())
        total = total + r * (1 << i)
    cs.constrain(total)


def _build(name, rec, cv, pub):
    cs = rec.cs
    if name in ("b8", "b8k"):
        v = cv[0]
        _decompose(rec, v - pub[0], 8)
        _decompose(rec, pub[1] - v, 8)
    elif name == "wide":
        _, _, o = rec.multiply(cv[0], cv[1])
        _decompose(rec, o * 5 + pub[0], 253, odd_left=True)
    elif name == "fence":
        v = cv[0]
        _, _, o0 = rec.multiply(v, v + One())
        e0 = o0 * 1
        l, r, o = rec.mul(notbit(e0, 0), bit(e0, 0))
        cs.constrain(LinearCombination.of(o))
        cs.constrain(l + r - One())
        _, r2, _ = rec.mul(bit(e0, 1), bit(e0, 2))
        _, _, o3 = rec.multiply(o0 + r2, r2 + v)
        e3 = o3 * (L - 1)
        rec.mul(bit(e3, 5), notbit(e3, 200))
        _, _, o5 = rec.multiply(o3, One() * 3)
        e5 = o5 * 1
        rec.mul(notbit(e5, 31), bit(e5, 32))
    elif name == "swap":
        l0, r0, o0 = rec.multiply(cv[0] + pub[0], cv[1] - One())
        A = cv[0] + pub[0] * 3
        B = cv[1] * 7 - One() + o0 * 11
        for t in range(9):                                  # 21 terms: a second pass over the lanes of a team of 16
            B = B + (l0, r0)[t % 2] * S.synth_scalar(b"db-swap", t) + cv[t % 2] * (t + 2)
        rec.mul(bit(A, 0), notbit(B, 0))
        rec.mul(bit(B, 1), notbit(A, 1))
        rec.mul(bit(A, 251), bit(B, 252))
        rec.mul(notbit(B, 33), bit(A, 64))
        rec.mul(bit(A, 2), bit(A, 3))
        rec.mul(notbit(B, 2), bit(B, 3))
    else:
        assert name == "inv0"
        e = cv[0] - pub[0]
        l, r, o = rec.mul(lc(e), INV)
        cs.constrain(e - l)
        eo = o * 1
        l1, r1, _ = rec.mul(notbit(eo, 0), bit(eo, 0))      # (is zero, is not zero) of the derived value
        cs.constrain(r1 - o)
        cs.constrain(l1 + r1 - One())
        rec.mul(lc(e * 2 + One()), INV)


# ------------------------------------------------------------------ per-proof inputs
def witness(name, j):
    """-> (committed values, public inputs) of proof j, as integers"""
    if name == "b8":
        a, b = ((0, 255), (77, 3), (255, 0), (1, 254), (128, 127))[j] if j < 5 else ((j * 37) % 256, (j * 91 + 5) % 256)
        lo = S.synth_scalar(b"db-lo", j) >> (8 * (j % 24)) if j % 3 else 10 * j     # bounds of every size, 0 among them
        return [(lo + a) % L], [lo % L, (lo + a + b) % L]
    if name == "b8k":
        return [B8_BAKED[0] + (0, 255, 100, 1)[j % 4]], []
    if name == "wide":
        vals = [S.synth_scalar(b"db-wide", 2 * j), S.synth_scalar(b"db-wide", 2 * j + 1)]
        target = WIDE_TARGETS[j] if j < len(WIDE_TARGETS) else S.synth_scalar(b"db-wide-t", j)
        return vals, [(target - 5 * vals[0] * vals[1]) % L]
    if name == "fence":
        return [S.synth_scalar(b"db-fence", j) if j else L - 1], []
    if name == "swap":
        return [S.synth_scalar(b"db-swap-v", 2 * j), S.synth_scalar(b"db-swap-v", 2 * j + 1) if j != 1 else 0], [S.synth_scalar(b"db-swap-p", j)]
    v = S.synth_scalar(b"db-inv", j)
    return [v], [v if j % 2 == 0 else (v + 1 + j) % L]     # v0 - Public(0) = 0 for every even proof


def blindings(name, j):
    return [S.synth_scalar(b"db-bl" + name.encode(), 8 * j + i) for i in range(CIRCUITS[name][0])]


def seed(j):
    return S.synth_seed(3000 + j)


# ------------------------------------------------------------------ the two forms
_SHAPES = {}


def _baked_pub(name, pub):
    if name == "b8k":
        pub = B8_BAKED
    return {k: One() * (x % L) for k, x in enumerate(pub)}


def shape(name):
    """the library's form: dict(n, m, p, rows with (5, k) terms, wops, lcs) from ONE pass of the oracle's Verifier"""
    if name not in _SHAPES:
        m, p, _ = CIRCUITS[name]
        v = Verifier(Transcript(label(name)))
        cv = [v.commit(bytes(32)) for _ in range(m)]
        rec = Rec(v)
        _build(name, rec, cv, {k: Variable(PUBLIC, k) * 1 for k in range(p)} if p else _baked_pub(name, ()))
        terms = lambda e: [((var[0], var[1]), c) for var, c in e.terms]
        lcs, objects = [], {}

        def add(e, shared):
            if shared and id(e) in objects:
                return objects[id(e)]
            lcs.append(terms(e))
            if shared:
                objects[id(e)] = len(lcs) - 1
            return len(lcs) - 1

        def operand(spec):
            if spec[0] == "lc":
                return bp.W_LC, add(spec[1], False)
            if spec[0] == "inv":
                return bp.W_INV_LEFT, 0
            return (bp.W_LCBIT if spec[0] == "bit" else bp.W_LCNOTBIT), (add(spec[1], True) << 8) | spec[2]
        wops = [operand(l) + operand(r) for l, r in rec.ops]
        _SHAPES[name] = dict(n=v.num_vars, m=m, p=p, rows=[terms(e) for e in v.constraints], wops=wops, lcs=lcs, keep=rec.ops)
    return _SHAPES[name]


def case(name, pub):
    """what the oracle's verifier needs of the baked circuit for the public inputs `pub`"""
    m, _, cap = CIRCUITS[name]

    def bv(vr, comms, pc):
        _build(name, Rec(vr), [vr.commit(c) for c in comms], _baked_pub(name, pub))
    return VS.Case(S.Scenario(label(name), [0] * m, None, bv), cap)


def oracle_accepts(name, pub, proof, comms, sd):
    """the oracle's verifier on the baked circuit: verification_scalars + the C oracle's multiscalar multiplication"""
    scalars, own, N, k, _ = VS._replay(case(name, pub), proof, comms, sd)
    assert all(decompress(pt) is not None for _, pt in own)
    sc = [scalars[i] for i, _ in own] + scalars[k:k + 2 + 2 * N]
    pts = [pt for _, pt in own] + VS.shared_bases(CIRCUITS[name][2], N)
    return VS.coracle().msm(sc, pts) == bytes(32)


_PROOFS = {}


def oracle_proof(name, j, vals=None, prove=True):
    """the oracle's Prover on proof j's baked circuit -> dict(proof, comms, wires, values, pub, constraints, n); vals: other committed
    values than witness(name, j)'s (a violated witness); prove=False: synthesis only"""
    key = (name, j, None if vals is None else tuple(vals), prove)
    if key not in _PROOFS:
        wv, pub = witness(name, j)
        vals = wv if vals is None else vals
        pr = Prover(PC, Transcript(label(name)))
        comms, cv = [], []
        for x, b in zip(vals, blindings(name, j)):
            c, var = pr.commit(x, b)
            comms.append(c)
            cv.append(var)
        _build(name, Rec(pr), cv, _baked_pub(name, pub))
        out = dict(comms=comms, values=enc(vals), wires=enc(pr.a_L + pr.a_R + pr.a_O), n=len(pr.a_L), pub=pub,
                   constraints=[list(e.terms) for e in pr.constraints], proof=None)
        if prove:
            out["proof"] = pr.prove(common.oracle_gens(CIRCUITS[name][2]), seed(j)).to_bytes()
        _PROOFS[key] = out
    return _PROOFS[key]


# ------------------------------------------------------------------ library objects, one per (library, circuit)
_CTX = {}


def gens(lib, cap, **creation):
    key = (id(lib), cap, tuple(sorted(creation.items())))
    if key not in _CTX:
        _CTX[key] = bp.Gens(cap, lib=lib, window_bits=8, **creation)
    return _CTX[key]


def circuit(lib, name, program=True):
    key = (id(lib), name, program)
    if key not in _CTX:
        sh = shape(name)
        _CTX[key] = bp.Circuit(sh["n"], sh["m"], sh["rows"], wops=sh["wops"] if program else None, lcs=sh["lcs"] if program else None, lib=lib)
        assert _CTX[key].p == sh["p"]
    return _CTX[key]


class Inputs:
    def __init__(self, name, B, bad=None):
        """bad: {proof: committed values} - witnesses that violate the circuit"""
        obs = [oracle_proof(name, j, vals=(bad or {}).get(j), prove=False) for j in range(B)]
        self.name, self.B, self.obs = name, B, obs
        self.values = b"".join(o["values"] for o in obs)
        self.blindings = b"".join(enc(blindings(name, j)) for j in range(B))
        self.seeds = b"".join(seed(j) for j in range(B))
        self.wires = b"".join(o["wires"] for o in obs)
        self.publics = b"".join(enc(o["pub"]) for o in obs)


def prove(lib, name, inp, entry="batch", program=True, creation=None, **opts):
    """-> (proofs, commitments) through one of the prove entry points; opts: handle options for the call"""
    sh = shape(name)
    g, circ = gens(lib, CIRCUITS[name][2], **(creation or {})), circuit(lib, name, program)
    wires = None if program else inp.wires
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        if entry == "batch":
            return bp.prove_batch(g, circ, label(name), inp.values, inp.blindings, inp.seeds, inp.B, wires=wires, publics=inp.publics)
        if entry == "transcripts":
            ts = [bp.Transcript(label(name), lib=lib) for _ in range(inp.B)]
            return bp.prove_batch_transcripts(g, circ, ts, inp.values, inp.blindings, inp.seeds, inp.B, wires=wires, publics=inp.publics)
        assert entry == "begin_end"     # two jobs in flight
        h = max(1, inp.B // 2)
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


def check_program(lib, name, B, entry="batch", program=True, creation=None, **opts):
    """B proofs through the device witness program (program=False: the oracle's wires) == the oracle's proofs of the B baked circuits,
    which the oracle's verifier accepts (first and last proof: the rest differ in values only)"""
    P, C = prove(lib, name, Inputs(name, B), entry, program, creation, **opts)
    for j in range(B):
        ob = oracle_proof(name, j)
        assert C[j] == ob["comms"], "%s: commitments of proof %d" % (name, j)
        assert P[j] == ob["proof"], "%s (%s, %s, %r): proof %d of %d differs from the oracle's proof of the baked circuit" % (
            name, entry, "witness program" if program else "host wires", opts, j, B)
    for j in sorted({0, B - 1}):
        assert oracle_accepts(name, oracle_proof(name, j)["pub"], P[j], C[j], seed(100 + j)), "%s: the oracle rejects proof %d" % (name, j)
    return P, C


# (circuit, batch): 1, 3, 9 (with 8 lanes per team a block of seven idle teams) and 70 proofs
PROGRAM_CASES = [("b8", 1), ("b8", 9), ("b8k", 3), ("wide", 3), ("fence", 3), ("swap", 9), ("inv0", 9), ("inv0", 70), ("swap", 1)]
TEAM_CASES = [("b8", 9), ("swap", 9), ("wide", 3), ("inv0", 9)]          # witness_team = 4, 8, 16
HOST_WIRE_CASES = [("b8", 3), ("b8k", 3), ("wide", 3), ("fence", 3), ("swap", 3), ("inv0", 3)]


def check_shapes():
    """the shapes the issue states, and one `lcs` entry per combination object"""
    b8 = shape("b8")
    assert (b8["n"], len(b8["rows"]), b8["m"], b8["p"], len(b8["lcs"])) == (16, 34, 1, 2, 2)
    w = shape("wide")
    assert (w["n"], w["p"], len(w["lcs"])) == (254, 1, 3)
    named = {(k, a & 0xff) for lk, la, rk, ra in w["wops"] for k, a in ((lk, la), (rk, ra)) if k in (bp.W_LCBIT, bp.W_LCNOTBIT)}
    assert {(bp.W_LCBIT, i) for i in range(256)} <= named and {(bp.W_LCNOTBIT, i) for i in (253, 254, 255)} <= named
    t = WIDE_TARGETS[0]
    assert all((t >> (32 * w_ - 1)) & 3 == 3 for w_ in range(1, 8)) and t < L
    for j, want in enumerate(WIDE_TARGETS):          # the canonical value of X is the target
        vals, pub = witness("wide", j)
        assert (5 * vals[0] * vals[1] + pub[0]) % L == want
    assert [witness("inv0", j)[0][0] == witness("inv0", j)[1][0] for j in range(4)] == [True, False, True, False]


def check_inverse_of_zero(lib):
    """W_INV_LEFT of a left wire of 0 is 0 (include/bpr1cs.h): in the oracle's wires - computed here as x^(l-2) - and in the library's
    proof through the program, which equals the oracle's"""
    o = oracle_proof("inv0", 0)
    w = WC._scalars(o["wires"])
    n = o["n"]
    assert (w[0], w[n], w[2 * n]) == (0, 0, 0) and (w[1], w[n + 1]) == (1, 0)          # left = 0: right = 0, "is zero" = 1
    o1 = oracle_proof("inv0", 1)
    w1 = WC._scalars(o1["wires"])
    assert w1[0] != 0 and w1[0] * w1[n] % L == 1 == w1[2 * n] and (w1[1], w1[n + 1]) == (0, 1)
    P, _ = prove(lib, "inv0", Inputs("inv0", 2))
    assert P == [o["proof"], o1["proof"]]


# ------------------------------------------------------------------ witness check
def check_witness_check(lib, program=True):
    """check_witness = 1: satisfied witnesses are proved as ever; a b8 proof whose v lies one above max is refused with a record that
    names the sum row of the second decomposition (max - v = -1 = l - 1: eight bits of 1 sum to 255), as the pure-Python checker of
    tests/witness_check_cases.py computes it on the baked rows; its neighbours are the oracle's proofs"""
    check_program(lib, "b8", 3, program=program, check_witness=1)
    vals, pub = witness("b8", 1)
    bad = {1: [(pub[1] + 1) % L]}
    assert (bad[1][0] - pub[0]) % L < 256                   # v - min still fits: only max - v overflows
    inp = Inputs("b8", 3, bad)
    P, C = prove(lib, "b8", inp, program=program, check_witness=1)
    sh = shape("b8")
    n, m = sh["n"], sh["m"]
    for j in range(3):
        ob = inp.obs[j]
        want = WC.violations(dict(n=n, constraints=ob["constraints"]), ob["wires"], ob["values"])
        if j == 1:
            assert want == dict(gate=None, row=33, gates=0, rows=1), want
            assert bp.refusal(P[j]) == want and P[j] == WC.record(len(P[j]), want), (bp.refusal(P[j]), want)
        else:
            assert want is None and P[j] == oracle_proof("b8", j)["proof"], j
    assert bp.last_prove_stats(lib)["refused"] == 1


# ------------------------------------------------------------------ verifiers (b8, public bounds)
FORMS = ("per_proof", "group_fb1", "group_fb2")


def _verdicts(lib, P, C, seeds, pub_bytes, form):
    g, circ = gens(lib, CIRCUITS["b8"][2]), circuit(lib, "b8")
    opts = {} if form == "per_proof" else dict(verify_group=4, verify_group_fallback=1 if form == "group_fb1" else 2)
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        return bp.verify_batch(g, circ, label("b8"), P, C, len(P), seeds=b"".join(seeds), publics=pub_bytes)
    finally:
        for k in opts:
            g.set_option(k, -1)


def check_verifiers(lib, B=5, bad=3):
    """verify_batch (per proof, grouped with fallback 1 and 2) and verify_batch_combined over B proofs of b8 with the right bounds, one
    bound altered and one bound non-canonical, against the oracle's verifier on the baked circuit"""
    obs = [oracle_proof("b8", j) for j in range(B)]
    P, C, pubs = [o["proof"] for o in obs], [o["comms"] for o in obs], [o["pub"] for o in obs]
    seeds = [hashlib.sha256(b"db-vseed %d" % j).digest() for j in range(B)]
    bseed = hashlib.sha256(b"db batch seed").digest()
    g, circ = gens(lib, CIRCUITS["b8"][2]), circuit(lib, "b8")
    comb = lambda pb: bp.verify_batch_combined(g, circ, label("b8"), P, C, B, batch_seed=bseed, index_base=0, seeds=b"".join(seeds), publics=pb)
    right = b"".join(enc(p) for p in pubs)
    assert all(oracle_accepts("b8", pubs[j], P[j], C[j], seeds[j]) for j in (0, bad, B - 1))
    for form in FORMS:
        assert _verdicts(lib, P, C, seeds, right, form) == [True] * B, form
    assert comb(right) == (bytes(32), True)
    for k in (0, 1):                                         # min, max of proof `bad` one higher
        pubs_bad = [list(p) for p in pubs]
        pubs_bad[bad][k] = (pubs_bad[bad][k] + 1) % L
        assert not oracle_accepts("b8", pubs_bad[bad], P[bad], C[bad], seeds[bad])
        wrong = b"".join(enc(p) for p in pubs_bad)
        for form in FORMS:
            assert _verdicts(lib, P, C, seeds, wrong, form) == [j != bad for j in range(B)], (k, form)
        pt, wf = comb(wrong)
        assert wf is True and pt != bytes(32)
        off = 32 * (2 * bad + k)
        nonc = right[:off] + NONCANONICAL + right[off + 32:]
        for form in FORMS:
            assert _verdicts(lib, P, C, seeds, nonc, form) == [j != bad for j in range(B)], (k, form)
        assert comb(nonc)[1] is False


# ------------------------------------------------------------------ bpr1cs_circuit_create
def check_create(lib):
    """refusals of W_LCBIT / W_LCNOTBIT (BPR1CS_ERR_INVALID_ARGUMENT, as for W_LC) and what is accepted"""
    v0, one = ((bp.VAR_COMMITTED, 0), 1), ((bp.VAR_ONE, 0), 1)
    zero = (bp.W_LC, 1)                                       # combination 1: empty
    ok_lcs = [[v0, ((bp.VAR_PUBLIC, 4), 3)], []]
    # a combination only these kinds refer to counts towards p; both kinds on either side; every bit index
    c = bp.Circuit(2, 1, [], wops=[(bp.W_LCBIT, 0 << 8 | 255) + zero, zero + (bp.W_LCNOTBIT, 0 << 8 | 7)], lcs=ok_lcs, lib=lib)
    assert c.p == 5
    # wires of EARLIER multipliers are fine
    bp.Circuit(2, 1, [], wops=[zero + zero, (bp.W_LCBIT, 0 << 8 | 1, bp.W_LCNOTBIT, 0 << 8 | 2)], lcs=[[((bp.VAR_MUL_OUT, 0), 1), ((bp.VAR_MUL_LEFT, 0), 2)], []], lib=lib)
    bad = []
    for kind in (bp.W_LCBIT, bp.W_LCNOTBIT):
        for side in (0, 1):
            op = lambda arg: ((kind, arg) + zero) if side == 0 else (zero + (kind, arg))
            bad.append(("index >= n_lc", 2, [op(2 << 8), zero + zero], ok_lcs))
            bad.append(("index far beyond n_lc", 2, [op(0xffffff << 8 | 3), zero + zero], ok_lcs))
            for vk in (bp.VAR_MUL_LEFT, bp.VAR_MUL_RIGHT, bp.VAR_MUL_OUT):
                bad.append(("its own multiplier", 2, [zero + zero, op(0 << 8)], [[v0, ((vk, 1), 1)], []]))
                bad.append(("a later multiplier", 2, [op(0 << 8), zero + zero], [[one, ((vk, 1), 5)], []]))
            bad.append(("a public term with coefficient 0", 1, [op(0 << 8)], [[v0, ((bp.VAR_PUBLIC, 0), 0)], []]))
            bad.append(("a committed value >= m", 1, [op(0 << 8)], [[((bp.VAR_COMMITTED, 1), 1)], []]))
    bad.append(("no combinations at all", 1, [(bp.W_LCBIT, 0, bp.W_LCNOTBIT, 0)], []))
    for why, n, wops, lcs in bad:
        try:
            bp.Circuit(n, 1, [], wops=wops, lcs=lcs, lib=lib)
            assert False, "accepted: %s (%r)" % (why, wops)
        except bp.R1CSError as e:
            assert e.code == -17, why
    # kinds 6 and up stay refused
    for kind in (6, 7, 8, 9):
        try:
            bp.Circuit(1, 1, [], wops=[(kind, 0) + zero], lcs=ok_lcs, lib=lib)
            assert False, "operand kind %d accepted" % kind
        except bp.R1CSError as e:
            assert e.code == -17


def check_golden_unchanged(lib, glib, name="bound_check"):
    """a description that uses only kinds 0..3 (the reference's bound check: W_BIT / W_NOTBIT of committed values) proves what it proved
    before: the committed vectors of tests/golden/proofs.json"""
    gd = json.load(open(os.path.join(ROOT, "tests", "golden", "proofs.json")))[name]
    circ = bp.CompiledGadget(gd["gadget"], gd["iparams"], [bytes.fromhex(s) for s in gd["sparams"]], lib=lib, glib=glib)
    assert circ.has_witness_program and (circ.n, circ.q, circ.m) == (gd["n"], gd["q"], gd["m"])
    g = bp.Gens(gd["capacity"], lib=lib)
    P, _ = bp.prove_batch(g, circ, gd["label"].encode(), bytes.fromhex(gd["values"]), bytes.fromhex(gd["blindings"]), bytes.fromhex(gd["seeds"]), 2, wires=None)
    assert [p.hex() for p in P] == gd["proofs"]


# ------------------------------------------------------------------ the front-end
def frontend_bounds(bits, j):
    """(v, min, max) of proof j: both differences below 2^bits, 0 and 2^bits - 1 among them"""
    top = (1 << bits) - 1
    a, b = [(0, top), (top, 0), (top // 3, top // 5)][j % 3]
    lo = (j * 1000003) % (1 << 20) if bits < 64 else (1 << 63) + j
    return lo + a, lo, lo + a + b


def check_frontend(lib, glib, bits, B=3):
    """CompiledGadget("bound_check_1", [bits]): the shape; B proofs with B different bound pairs in one call of the device witness
    program == proof for proof bpr1cs_gadget_prove_on with sp = [min_j, max_j] (host synthesis, bounds baked), each accepted by
    bpr1cs_gadget_verify_on with the same sp and rejected with its neighbour's; the same bytes with the bounds baked at compile time"""
    gname, ip, lab = "bound_check_1", [bits], b"BoundCheck1"
    circ = bp.CompiledGadget(gname, ip, [], lib=lib, glib=glib)
    assert (circ.n, circ.q, circ.m, circ.p) == (2 * bits, 2 * (2 * bits + 1), 1, 2) and circ.has_witness_program
    if bits == 8:
        sh = shape("b8")
        assert (circ.n, circ.q, circ.m, circ.p) == (sh["n"], len(sh["rows"]), sh["m"], sh["p"])
    cap = 1 << (2 * bits - 1).bit_length()
    g = gens(lib, cap)
    wit = [frontend_bounds(bits, j) for j in range(B)]
    vals = enc([w[0] for w in wit])
    bls = enc([S.synth_scalar(b"db-fe-bl", 64 * bits + j) for j in range(B)])
    seeds = b"".join(seed(200 + j) for j in range(B))
    pubs = b"".join(enc(w[1:]) for w in wit)
    P, C = bp.prove_batch(g, circ, lab, vals, bls, seeds, B, wires=None, publics=pubs)
    for j in range(B):
        cut = lambda raw: raw[32 * j:32 * (j + 1)]
        sp = [sc_to_bytes(x) for x in wit[j][1:]]
        ref, refc, _ = bp.gadget_prove_on(g, gname, ip, sp, lab, cut(vals), cut(bls), 1, 1, cut(seeds), glib=glib)
        assert P[j] == ref[0], "bits = %d: proof %d over public bounds differs from the baked front-end's" % (bits, j)
        assert C[j] == refc[0]
        assert bp.gadget_verify_on(g, gname, ip, sp, lab, P[j], C[j], glib=glib)[0]
        other = [sc_to_bytes(x) for x in wit[(j + 1) % B][1:]]
        assert not bp.gadget_verify_on(g, gname, ip, other, lab, P[j], C[j], glib=glib)[0]
    vs = b"".join(hashlib.sha256(b"db-fe-vseed %d" % j).digest() for j in range(B))
    assert bp.verify_batch(g, circ, lab, P, C, B, seeds=vs, publics=pubs) == [True] * B
    base = bp.CompiledGadget(gname, ip, [sc_to_bytes(x) for x in wit[0][1:]], lib=lib, glib=glib)
    assert base.p == 0 and base.has_witness_program and (base.n, base.q, base.m) == (circ.n, circ.q, circ.m)
    Pb, _ = bp.prove_batch(g, base, lab, vals[:32], bls[:32], seeds[:32], 1, wires=None)
    assert Pb[0] == P[0]
    assert bp.verify_batch(g, base, lab, P[:1], C[:1], 1, seeds=vs[:32]) == [True]
