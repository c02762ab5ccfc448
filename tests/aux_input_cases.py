"""Auxiliary inputs (BPR1CS_W_AUX, include/bpr1cs.h "Auxiliary inputs") and the tree gadgets whose proof nodes are allocated instead of
committed ("vsmt_4_aux", "vsmt_2_aux"): circuits, the case table and the checkers shared by the CPU simulator
(tests/test_aux_inputs.py) and the device (tests/test_gpu_aux_inputs.py).

Every expectation is the oracle's.  One `_build` per circuit drives whoever `cs` is through a recorder (`Rec`, the one of
tests/derived_bits_cases.py with two more operand specs): with the oracle's Prover it calls allocate_multiplier with assignments
computed HERE, in Python integers - an auxiliary value is simply handed over, as upstream's `allocate_multiplier(Some((l, r)))` takes
it - on proof j's BAKED circuit (public inputs folded into One); with the oracle's Verifier it yields the rows, the `wops` and the `lcs`
the library gets once for all proofs.  The library's proofs with wires=None (the device witness program reading the auxiliary block
of `values`) must be the oracle's proof bytes, and the oracle's verifier of the baked circuit must accept them.

Circuits - the smallest shapes that can go wrong:
  pair   m = 1, a = 2: one multiplier (aux0, aux1), row out - v0; n = N = 1
  gap    m = 0, a = 3, index 1 named by nothing: (aux2, aux0), (aux0, aux2) - index 2 left of one multiplier and right of the next - and
         multiply(l0 + r1, o0) directly behind them (the register cache / fence path of team_operand)
  mix    m = 2, p = 2, a = 5 - committed, public and auxiliary value rows, a odd: (aux0, lc(v0 - pub0)); (aux1, INV_LEFT) with aux1 = 0 in
         every other proof; (aux2, aux3) = v1; W_LCNOTBIT / W_LCBIT over a combination of aux-fed wires; W_BIT of v1 beside W_LCBIT;
         (aux4, the empty combination)
  wide   a = 70 in 35 pair multipliers of N = 64; the row ties the sum of the products to v0; 0, 1 and l - 1 among the values
  t4/t2  "vsmt_4_aux" with levels = 4 (the smallest: the gadget takes the index four levels at a time), "vsmt_2_aux" with depth = 3 (Inverse S-box, 2 partial rounds: the permutations are evaluated
         jointly, and their input combinations read aux-fed wires), root baked and public"""
import ctypes
import hashlib
import json
import os

from pyref import gadgets as G
from pyref import scenarios as S
from pyref.ed import L, decompress, sc_to_bytes
from pyref.merlin import Transcript
from pyref.r1cs import LinearCombination, One, Prover, Variable, Verifier
import common
import derived_bits_cases as DB
import frontend_cases as FC
import public_input_cases as PI
import verify_scalar_cases as VS
import witness_check_cases as WC

bp = common.bp
PC = common.PC
ROOT = PI.ROOT
PUBLIC = 5
enc, NONCANONICAL = PI.enc, PI.NONCANONICAL
lc, bit, notbit, INV = DB.lc, DB.bit, DB.notbit, DB.INV

# name -> (committed values, public inputs, auxiliary inputs, capacity)
CIRCUITS = {"pair": (1, 0, 2, 1), "gap": (0, 0, 3, 4), "mix": (2, 2, 5, 8), "wide": (1, 0, 70, 64)}
MIX_V1_ROW = 1      # "mix": the row o2 - v1 (the product of aux2 and aux3 is the committed v1)


def label(name):
    return b"AuxInputs-" + name.encode()


# ------------------------------------------------------------------ the recorder
def aux(k):
    return ("aux", k)                    # BPR1CS_W_AUX: auxiliary input k of the proof at hand


def cbit(var, i, k):
    return ("cbit", var, i, k)           # BPR1CS_W_BIT: bit k of committed value i (var: its Variable)


class Rec(DB.Rec):
    def __init__(self, cs, aux_values=None):
        DB.Rec.__init__(self, cs)
        self.aux = aux_values

    def val(self, spec, left=None):
        if spec[0] == "aux":
            return self.aux[spec[1]] % L
        if spec[0] == "cbit":
            return (self.cs.eval(LinearCombination.of(spec[1])) >> spec[3]) & 1
        return DB.Rec.val(self, spec, left)


def _build(name, rec, cv, pub):
    cs = rec.cs
    if name == "pair":
        _, _, o = rec.mul(aux(0), aux(1))
        cs.constrain(o - cv[0])
    elif name == "gap":
        l0, _, o0 = rec.mul(aux(2), aux(0))
        _, r1, o1 = rec.mul(aux(0), aux(2))
        rec.multiply(l0 + r1, o0 * 1)
        cs.constrain(o0 - o1)
    elif name == "mix":
        e0 = cv[0] - pub[0]
        l0, r0, _ = rec.mul(aux(0), lc(e0))
        cs.constrain(e0 - r0)                                   # row 0
        _, _, o1 = rec.mul(aux(1), INV)
        _, _, o2 = rec.mul(aux(2), aux(3))
        cs.constrain(o2 - cv[1])                                # row 1 = MIX_V1_ROW
        e = l0 * 3 + o2 + o1 * 5 + pub[1]
        l3, r3, o3 = rec.mul(notbit(e, 0), bit(e, 0))
        cs.constrain(LinearCombination.of(o3))
        cs.constrain(l3 + r3 - One())
        rec.mul(cbit(cv[1], 1, 3), bit(e, 7))
        _, r5, o5 = rec.mul(aux(4), lc(LinearCombination()))
        cs.constrain(LinearCombination.of(r5))
        cs.constrain(LinearCombination.of(o5))
    else:
        assert name == "wide"
        total = -LinearCombination.of(cv[0])
        for i in range(35):
            _, _, o = rec.mul(aux(2 * i), aux(2 * i + 1))
            total = total + o
        cs.constrain(total)


# ------------------------------------------------------------------ per-proof inputs
def aux_values(name, j):
    a = CIRCUITS[name][2]
    out = [S.synth_scalar(b"ax-" + name.encode(), 128 * j + k) for k in range(a)]
    if name == "mix" and j % 2 == 0:
        out[1] = 0                                              # INV_LEFT of 0 in every other proof
    if name == "wide":
        for t, x in enumerate((0, 1, L - 1)):
            out[(7 * j + 23 * t) % a] = x
    return out


def witness(name, j, ax=None):
    """-> (committed values, public inputs, auxiliary inputs) of proof j, as integers; ax: other auxiliary values (the committed ones
    stay those of the honest witness)"""
    hon = aux_values(name, j)
    ax = hon if ax is None else ax
    if name == "pair":
        return [hon[0] * hon[1] % L], [], ax
    if name == "gap":
        return [], [], ax
    if name == "mix":
        pub = [S.synth_scalar(b"ax-pub", 2 * j), S.synth_scalar(b"ax-pub", 2 * j + 1) if j != 1 else 0]
        return [S.synth_scalar(b"ax-v", j), hon[2] * hon[3] % L], pub, ax
    return [sum(hon[2 * i] * hon[2 * i + 1] for i in range(35)) % L], [], ax


def blindings(name, j):
    return [S.synth_scalar(b"ax-bl" + name.encode(), 8 * j + i) for i in range(CIRCUITS[name][0])]


def seed(j):
    return S.synth_seed(4000 + j)


# ------------------------------------------------------------------ the two forms
_SHAPES = {}


def _baked_pub(pub):
    return {k: One() * (x % L) for k, x in enumerate(pub)}


def shape(name):
    """the library's form: dict(n, m, p, a, rows with (5, k) terms, wops, lcs) from ONE pass of the oracle's Verifier"""
    if name not in _SHAPES:
        m, p, a, _ = CIRCUITS[name]
        v = Verifier(Transcript(label(name)))
        cv = [v.commit(bytes(32)) for _ in range(m)]
        rec = Rec(v)
        _build(name, rec, cv, {k: Variable(PUBLIC, k) * 1 for k in range(p)})
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
            if spec[0] == "aux":
                return bp.W_AUX, spec[1]
            if spec[0] == "cbit":
                return bp.W_BIT, (spec[2] << 8) | spec[3]
            if spec[0] == "lc":
                return bp.W_LC, add(spec[1], False)
            if spec[0] == "inv":
                return bp.W_INV_LEFT, 0
            return (bp.W_LCBIT if spec[0] == "bit" else bp.W_LCNOTBIT), (add(spec[1], True) << 8) | spec[2]
        wops = [operand(l) + operand(r) for l, r in rec.ops]
        _SHAPES[name] = dict(n=v.num_vars, m=m, p=p, a=a, rows=[terms(e) for e in v.constraints], wops=wops, lcs=lcs, keep=rec.ops)
    return _SHAPES[name]


def case(name, pub):
    """what the oracle's verifier needs of the baked circuit for the public inputs `pub`"""
    m, _, _, cap = CIRCUITS[name]

    def bv(vr, comms, pc):
        _build(name, Rec(vr), [vr.commit(c) for c in comms], _baked_pub(pub))
    return VS.Case(S.Scenario(label(name), [0] * m, None, bv), cap)


def _accepts(cs_case, cap, proof, comms, sd):
    scalars, own, N, k, _ = VS._replay(cs_case, proof, comms, sd)
    assert all(decompress(pt) is not None for _, pt in own)
    sc = [scalars[i] for i, _ in own] + scalars[k:k + 2 + 2 * N]
    pts = [pt for _, pt in own] + VS.shared_bases(cap, N)
    return VS.coracle().msm(sc, pts) == bytes(32)


def oracle_accepts(name, pub, proof, comms, sd):
    """the oracle's verifier on the baked circuit: verification_scalars + the C oracle's multiscalar multiplication"""
    return _accepts(case(name, pub), CIRCUITS[name][3], proof, comms, sd)


_PROOFS = {}


def oracle_proof(name, j, ax=None, prove=True):
    """the oracle's Prover on proof j's baked circuit, the auxiliary values handed to allocate_multiplier -> dict(proof, comms, wires,
    values, pub, aux, constraints, n); ax: other auxiliary values than the witness's (a violated witness); prove=False: synthesis only"""
    key = (name, j, None if ax is None else tuple(ax), prove)
    if key not in _PROOFS:
        vals, pub, ax = witness(name, j, ax)
        pr = Prover(PC, Transcript(label(name)))
        comms, cv = [], []
        for x, b in zip(vals, blindings(name, j)):
            c, var = pr.commit(x, b)
            comms.append(c)
            cv.append(var)
        _build(name, Rec(pr, ax), cv, _baked_pub(pub))
        out = dict(comms=comms, values=enc(vals), wires=enc(pr.a_L + pr.a_R + pr.a_O), n=len(pr.a_L), pub=pub, aux=ax,
                   constraints=[list(e.terms) for e in pr.constraints], proof=None)
        if prove:
            out["proof"] = pr.prove(common.oracle_gens(CIRCUITS[name][3]), seed(j)).to_bytes()
        _PROOFS[key] = out
    return _PROOFS[key]


# ------------------------------------------------------------------ library objects, one per (library, circuit)
_CTX = {}
gens = DB.gens


def circuit(lib, name, program=True):
    key = (id(lib), "aux", name, program)
    if key not in _CTX:
        sh = shape(name)
        _CTX[key] = bp.Circuit(sh["n"], sh["m"], sh["rows"], wops=sh["wops"] if program else None, lcs=sh["lcs"] if program else None, lib=lib)
        assert not program or (_CTX[key].p, _CTX[key].a) == (sh["p"], sh["a"])
    return _CTX[key]


class Inputs:
    def __init__(self, name, B, bad=None, first=0):
        """bad: {proof: auxiliary values} - witnesses that violate the circuit"""
        js = range(first, first + B)
        obs = [oracle_proof(name, j, ax=(bad or {}).get(j), prove=False) for j in js]
        self.name, self.B, self.obs = name, B, obs
        self.values = b"".join(o["values"] for o in obs)
        self.blindings = b"".join(enc(blindings(name, j)) for j in js)
        self.seeds = b"".join(seed(j) for j in js)
        self.wires = b"".join(o["wires"] for o in obs)
        self.publics = b"".join(enc(o["pub"]) for o in obs)
        self.aux = b"".join(enc(o["aux"]) for o in obs)


def prove_draws(lib, g, circ, name, inp, wires):
    """bpr1cs_prove_batch_draws as its caller uses it (tests/witness_check_cases.prove_draws): transcripts past "m" and the 2n + 8 raw
    draws per proof made with the oracle's Merlin; `values` = committed | public | auxiliary"""
    from pyref.merlin import Transcript as OracleTranscript
    sh = shape(name)
    n, m, B = sh["n"], sh["m"], inp.B
    ts, draws = [], b""
    for j in range(B):
        ot, t = OracleTranscript(label(name)), bp.Transcript(label(name), lib=lib)
        ot.append_message(b"dom-sep", b"r1cs v1"); t.append_message(b"dom-sep", b"r1cs v1")
        for c in inp.obs[j]["comms"]:
            ot.append_point(b"V", c); t.append_message(b"V", c)
        ot.append_u64(b"m", m); t.append_message(b"m", m.to_bytes(8, "little"))
        b = ot.build_rng()
        for k in range(m):
            b = b.rekey_with_witness_bytes(b"v_blinding", inp.blindings[32 * (m * j + k):32 * (m * j + k + 1)])
        rng = b.finalize(inp.seeds[32 * j:32 * j + 32])
        draws += b"".join(rng.fill_bytes(64) for _ in range(2 * n + 8))
        ts.append(t)
    vp, cp = ctypes.c_void_p, ctypes.c_char_p
    lib.bpr1cs_prove_batch_draws.argtypes = [vp, vp, ctypes.POINTER(vp), cp, cp, cp, cp, ctypes.c_size_t, cp]
    out = ctypes.create_string_buffer(B * circ.proof_len)
    vals = inp.values + inp.publics + (inp.aux if wires is None else b"")
    rc = lib.bpr1cs_prove_batch_draws(g.h, circ.h, (vp * B)(*[t.h for t in ts]), vals or b"\0", inp.blindings or b"\0", draws, wires, B, out)
    bp._chk(rc)
    raw = out.raw
    return [raw[i * circ.proof_len:(i + 1) * circ.proof_len] for i in range(B)], [o["comms"] for o in inp.obs]


ENTRIES = ("batch", "raw", "transcripts", "begin_end", "draws")


def prove(lib, name, inp, entry="batch", program=True, creation=None, **opts):
    """-> (proofs, commitments) through one of the prove entry points; program=False: the oracle's wires and NO auxiliary block"""
    sh = shape(name)
    g, circ = gens(lib, CIRCUITS[name][3], **(creation or {})), circuit(lib, name)     # (with its program and a > 0 in either case)
    wires, ax = (None, inp.aux) if program else (inp.wires, None)
    m, plen = sh["m"], circ.proof_len
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        if entry == "batch":
            return bp.prove_batch(g, circ, label(name), inp.values, inp.blindings, inp.seeds, inp.B, wires=wires, publics=inp.publics, aux=ax)
        if entry == "raw":
            assert program
            praw, craw = bp.prove_batch_raw(g, circ, label(name), inp.values, inp.blindings, inp.seeds, inp.B, publics=inp.publics, aux=ax)
            return ([praw[i * plen:(i + 1) * plen] for i in range(inp.B)],
                    [[craw[(i * m + j) * 32:(i * m + j + 1) * 32] for j in range(m)] for i in range(inp.B)])
        if entry == "transcripts":
            ts = [bp.Transcript(label(name), lib=lib) for _ in range(inp.B)]
            return bp.prove_batch_transcripts(g, circ, ts, inp.values, inp.blindings, inp.seeds, inp.B, wires=wires, publics=inp.publics, aux=ax)
        if entry == "draws":
            return prove_draws(lib, g, circ, name, inp, wires)
        assert entry == "begin_end"     # two jobs in flight, each with its own tail blocks
        h = max(1, inp.B // 2)
        cut = lambda raw, sz, lo, hi: raw[lo * sz:hi * sz]
        jobs = [bp.ProveJob(g, circ, label(name), cut(inp.values, 32 * m, lo, hi), cut(inp.blindings, 32 * m, lo, hi),
                            cut(inp.seeds, 32, lo, hi), hi - lo, wires=None if program else cut(inp.wires, 96 * sh["n"], lo, hi),
                            publics=cut(inp.publics, 32 * sh["p"], lo, hi), aux=cut(inp.aux, 32 * sh["a"], lo, hi) if program else None)
                for lo, hi in ((0, h), (h, inp.B)) if hi > lo]
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
    """B proofs through the device witness program and the auxiliary block (program=False: the oracle's wires, no block) == the
    oracle's proofs of the B baked circuits, which the oracle's verifier accepts (first and last proof)"""
    P, C = prove(lib, name, Inputs(name, B), entry, program, creation, **opts)
    for j in range(B):
        ob = oracle_proof(name, j)
        assert C[j] == ob["comms"], "%s: commitments of proof %d" % (name, j)
        assert P[j] == ob["proof"], "%s (%s, %s, %r): proof %d of %d differs from the oracle's proof of the baked circuit" % (
            name, entry, "witness program" if program else "host wires", opts, j, B)
    for j in sorted({0, B - 1}):
        assert oracle_accepts(name, oracle_proof(name, j)["pub"], P[j], C[j], seed(100 + j)), "%s: the oracle rejects proof %d" % (name, j)
    return P, C


# (circuit, batch): 1, 3, 9 (with 8 lanes per team a block of seven idle teams) and 70 proofs (ragged, more than one wavefront)
PROGRAM_CASES = [("pair", 1), ("pair", 70), ("gap", 3), ("gap", 70), ("mix", 1), ("mix", 9), ("wide", 3)]
SIM_PROGRAM_CASES = [("pair", 1), ("pair", 9), ("gap", 3), ("gap", 70), ("mix", 9), ("wide", 3)]
TEAM_CASES = [("pair", 9), ("gap", 9), ("mix", 9), ("wide", 3)]          # witness_team = 4, 8, 16
HOST_WIRE_CASES = [("pair", 3), ("gap", 3), ("mix", 3), ("wide", 3)]


def check_shapes():
    """the shapes the issue states"""
    want = {"pair": (1, 1, 0, 2), "gap": (3, 0, 0, 3), "mix": (6, 2, 2, 5), "wide": (35, 1, 0, 70)}
    for name, (n, m, p, a) in want.items():
        sh = shape(name)
        assert (sh["n"], sh["m"], sh["p"], sh["a"]) == (n, m, p, a), name
        named = {arg for lk, la, rk, ra in sh["wops"] for k, arg in ((lk, la), (rk, ra)) if k == bp.W_AUX}
        assert named == ({0, 2} if name == "gap" else set(range(a))), name
    g = shape("gap")["wops"]
    assert g[0][:2] == (bp.W_AUX, 2) and g[1][2:] == (bp.W_AUX, 2) and g[2][0] == g[2][2] == bp.W_LC
    mx = shape("mix")["wops"]
    assert mx[1] == (bp.W_AUX, 1, bp.W_INV_LEFT, 0) and mx[4][0] == bp.W_BIT and mx[4][2] == bp.W_LCBIT and mx[3][0] == bp.W_LCNOTBIT
    assert mx[5][0] == bp.W_AUX and mx[5][2] == bp.W_LC and shape("mix")["lcs"][mx[5][3]] == []
    assert [witness("mix", j)[2][1] == 0 for j in range(4)] == [True, False, True, False]
    assert {0, 1, L - 1} <= set(witness("wide", 0)[2])


def check_job_slices(lib, in_flight):
    """ONE bpr1cs_prove_batch call of 9 proofs of "mix" cut into jobs of 4, 4 and 1: every job must get its slice of the committed, the
    public and the auxiliary block"""
    check_program(lib, "mix", 9, entry="raw", job_proofs=4, jobs_in_flight=in_flight)
    assert bp.last_prove_stats(lib)["jobs"] == 3


# ------------------------------------------------------------------ witness check
def check_witness_check(lib, name="mix", B=3, bad=1, k=2):
    """check_witness = 1 through the device program: satisfied witnesses are proved as ever; with auxiliary value k of proof `bad` one
    higher that proof is refused with a record naming the lowest violated row as the pure-Python checker of
    tests/witness_check_cases.py computes it on the wires the oracle synthesises from the altered value; its neighbours are the oracle's"""
    check_program(lib, name, B, check_witness=1)
    ax = list(aux_values(name, bad))
    ax[k] = (ax[k] + 1) % L
    inp = Inputs(name, B, {bad: ax})
    P, C = prove(lib, name, inp, check_witness=1)
    n = shape(name)["n"]
    for j in range(B):
        ob = inp.obs[j]
        want = WC.violations(dict(n=n, constraints=ob["constraints"]), ob["wires"], ob["values"])
        if j == bad:
            assert want is not None and want["gate"] is None and want["row"] is not None, want
            if (name, k) == ("mix", 2):
                assert want == dict(gate=None, row=MIX_V1_ROW, gates=0, rows=1), want
            assert bp.refusal(P[j]) == want and P[j] == WC.record(len(P[j]), want), (bp.refusal(P[j]), want)
        else:
            assert want is None and P[j] == oracle_proof(name, j)["proof"], j
    assert bp.last_prove_stats(lib)["refused"] == 1


# ------------------------------------------------------------------ verifiers
FORMS = ("per_proof", "group_fb1", "group_fb2")


def tampered(proof):
    bad = bytearray(proof)
    bad[1 + 8 * 32 + 3] ^= 1          # a low byte of t_x: still a canonical scalar
    return bytes(bad)


def _check_verifier_forms(lib, g, circ, lab, cases, P, C, pub_bytes, bad, cap):
    """the verifier forms over P (proof `bad` tampered) against the oracle's verdicts; cases[j]: the oracle's baked circuit of proof j"""
    B = len(P)
    seeds = [hashlib.sha256(b"ax-vseed %d" % j).digest() for j in range(B)]
    bseed = hashlib.sha256(b"ax batch seed").digest()
    want = [_accepts(cases[j], cap, P[j], C[j], seeds[j]) for j in range(B)]
    assert want == [j != bad for j in range(B)], want
    for form in FORMS:
        opts = {} if form == "per_proof" else dict(verify_group=4, verify_group_fallback=1 if form == "group_fb1" else 2)
        try:
            for k, v in opts.items():
                g.set_option(k, v)
            assert bp.verify_batch(g, circ, lab, P, C, B, seeds=b"".join(seeds), publics=pub_bytes) == want, form
        finally:
            for k in opts:
                g.set_option(k, -1)
    pt, wf = bp.verify_batch_combined(g, circ, lab, P, C, B, batch_seed=bseed, index_base=0, seeds=b"".join(seeds), publics=pub_bytes)
    assert wf is True and pt != bytes(32)
    good = [j for j in range(B) if j != bad]
    sub = lambda xs: [xs[j] for j in good]
    p = len(pub_bytes) // (32 * B)
    gpub = b"".join(pub_bytes[32 * p * j:32 * p * (j + 1)] for j in good)
    assert bp.verify_batch_combined(g, circ, lab, sub(P), sub(C), len(good), batch_seed=bseed, index_base=0, seeds=b"".join(sub(seeds)),
                                    publics=gpub) == (bytes(32), True)
    # the combined scalars and the own-points sum: the mirror of tests/public_input_cases.expected_scalars on the baked circuits
    reps = [VS._replay(cases[j], P[j], C[j], seeds[j]) for j in range(B)]
    rho = PI.weights([r[4] for r in reps], [pub_bytes[32 * p * j:32 * p * (j + 1)] for j in range(B)], bseed, 5)
    N = reps[0][2]
    want_sc = b"".join(sc_to_bytes(sum(w * r[0][r[3] + i] for w, r in zip(rho, reps)) % L) for i in range(2 * N + 2))
    sc, pts = [], []
    for w, (scalars, own, _, _, _) in zip(rho, reps):
        sc += [w * scalars[i] % L for i, _ in own]
        pts += [pt for _, pt in own]
    got = bp.verify_batch_scalars(g, circ, lab, P, C, B, batch_seed=bseed, index_base=5, seeds=b"".join(seeds), publics=pub_bytes)
    assert got[2] is True and got[0] == want_sc and got[1] == VS.coracle().msm(sc, pts)


def check_verifiers(lib, B=5, bad=3):
    """the verifiers never see the auxiliary block: "mix" proofs (the oracle's), one tampered, through every form"""
    obs = [oracle_proof("mix", j) for j in range(B)]
    P, C = [o["proof"] for o in obs], [o["comms"] for o in obs]
    P[bad] = tampered(P[bad])
    g, circ = gens(lib, CIRCUITS["mix"][3]), circuit(lib, "mix")
    _check_verifier_forms(lib, g, circ, label("mix"), [case("mix", o["pub"]) for o in obs], P, C, b"".join(enc(o["pub"]) for o in obs), bad,
                          CIRCUITS["mix"][3])


# ------------------------------------------------------------------ bpr1cs_circuit_create and the prove calls' refusals
def _refused(call, why):
    try:
        call()
        assert False, "accepted: %s" % why
    except bp.R1CSError as e:
        assert e.code == -17, why


def check_create(lib):
    """what bpr1cs_circuit_create accepts (either side, INV_LEFT behind it, unused and repeated indices, the highest index) and refuses
    (index >= 2^20, a variable of kind 6 or of the operand kind's own number in a row or a combination, operand kinds 6 .. 9 and 11)"""
    zero = (bp.W_LC, 0)
    lcs = [[], [((bp.VAR_COMMITTED, 0), 1)]]
    mk = lambda wops, lcs_=lcs, rows=(): bp.Circuit(len(wops), 1, list(rows), wops=wops, lcs=lcs_, lib=lib)
    assert mk([(bp.W_AUX, 0) + zero]).a == 1
    assert mk([zero + (bp.W_AUX, 4)]).a == 5                                   # indices 0..3 named by nothing
    assert mk([(bp.W_AUX, 3, bp.W_INV_LEFT, 0), (bp.W_AUX, 3, bp.W_AUX, 3)]).a == 4    # one index, three operands
    assert mk([(bp.W_AUX, (1 << 20) - 1) + zero]).a == 1 << 20
    assert mk([zero + zero]).a == 0
    assert bp.Circuit(1, 1, [], lib=lib).a == 0                              # no wops
    for side in (0, 1):
        op = lambda arg: ((bp.W_AUX, arg) + zero) if side == 0 else (zero + (bp.W_AUX, arg))
        _refused(lambda: mk([op(1 << 20)]), "index 2^20")
        _refused(lambda: mk([op(0xffffffff)]), "index 2^32 - 1")
    _refused(lambda: mk([(bp.W_INV_LEFT, 0, bp.W_AUX, 0)]), "INV_LEFT on the left")
    # an auxiliary value is not a variable
    for vk in (6, bp.W_AUX):
        _refused(lambda: mk([(bp.W_AUX, 0) + zero], rows=[[((vk, 0), 1)]]), "kind %d in term_var" % vk)
        _refused(lambda: bp.Circuit(1, 1, [[((vk, 0), 1)]], lib=lib), "kind %d in term_var, no program" % vk)
        _refused(lambda: mk([(bp.W_AUX, 0, bp.W_LC, 1)], [[], [((vk, 0), 1)]]), "kind %d in lc_var" % vk)
        _refused(lambda: mk([(bp.W_LCBIT, 1 << 8, bp.W_AUX, 0)], [[], [((vk, 0), 1)]]), "kind %d in lc_var under W_LCBIT" % vk)
    # the operand kinds beside it stay refused (6 .. 9 are internal numbers, never part of the ABI)
    for kind in (6, 7, 8, 9, 11):
        _refused(lambda: mk([(kind, 0) + zero]), "operand kind %d" % kind)


def check_prove_refusals(lib):
    """a non-canonical auxiliary scalar and values = NULL with a > 0 are BPR1CS_ERR_INVALID_ARGUMENT; with host wires the block is not
    read: the same call goes through without it (and with a non-canonical one behind the public inputs it never looks at)"""
    inp = Inputs("mix", 3)
    P, _ = prove(lib, "mix", inp)
    assert P[1] == oracle_proof("mix", 1)["proof"]
    good = inp.aux
    for pos in (0, 5 * 1 + 4, 5 * 3 - 1):
        inp.aux = good[:32 * pos] + NONCANONICAL + good[32 * (pos + 1):]
        for entry in ("batch", "raw", "transcripts", "draws"):
            _refused(lambda: prove(lib, "mix", inp, entry), "non-canonical auxiliary scalar %d (%s)" % (pos, entry))
        # (bpr1cs_prove_batch_begin over the whole batch: a refused call leaves no job in flight behind)
        _refused(lambda: bp.ProveJob(gens(lib, CIRCUITS["mix"][3]), circuit(lib, "mix"), label("mix"), inp.values, inp.blindings, inp.seeds, 3,
                                     publics=inp.publics, aux=inp.aux), "non-canonical auxiliary scalar %d (begin)" % pos)
    inp.aux = good
    # values = NULL: a circuit with m = 0, p = 0, a > 0
    g, circ = gens(lib, CIRCUITS["gap"][3]), circuit(lib, "gap")
    gi = Inputs("gap", 2)
    vp, cp = ctypes.c_void_p, ctypes.c_char_p
    fn = lib.bpr1cs_prove_batch
    saved = fn.argtypes
    try:
        fn.argtypes = [vp, vp, cp, ctypes.c_size_t, cp, cp, cp, cp, ctypes.c_size_t, cp, cp]
        out, cm = ctypes.create_string_buffer(2 * circ.proof_len), ctypes.create_string_buffer(32)
        lab = label("gap")
        assert fn(g.h, circ.h, lab, len(lab), None, None, gi.seeds, None, 2, out, cm) == -17
        assert fn(g.h, circ.h, lab, len(lab), gi.aux, None, gi.seeds, None, 2, out, cm) == 0
        assert [out.raw[:circ.proof_len], out.raw[circ.proof_len:]] == [oracle_proof("gap", j)["proof"] for j in range(2)]
        # host wires: no block, NULL values
        hc = circuit(lib, "gap", program=False)
        assert fn(g.h, hc.h, lab, len(lab), None, None, gi.seeds, gi.wires, 2, out, cm) == 0
        assert out.raw[:circ.proof_len] == oracle_proof("gap", 0)["proof"]
        # ... and on the circuit WITH the program, host wires: a = 3, nothing read
        assert fn(g.h, circ.h, lab, len(lab), None, None, gi.seeds, gi.wires, 2, out, cm) == 0
        assert out.raw[circ.proof_len:] == oracle_proof("gap", 1)["proof"]
    finally:
        fn.argtypes = saved


def check_tail_length(lib):
    """the Python wrappers size the auxiliary block from Circuit.a and refuse an `aux` of any other length (tests/public_input_cases
    .check_tail_length); with host wires `aux` may be None"""
    g, circ, inp = gens(lib, CIRCUITS["mix"][3]), circuit(lib, "mix"), Inputs("mix", 3)
    assert circ.a == 5 and len(inp.aux) == 3 * 5 * 32
    lab = label("mix")
    ts = lambda: [bp.Transcript(lab, lib=lib) for _ in range(3)]
    for ax in (None, b"", inp.aux[:-32], inp.aux + bytes(32), inp.aux[:5 * 32]):
        for call in (lambda: bp.prove_batch(g, circ, lab, inp.values, inp.blindings, inp.seeds, 3, publics=inp.publics, aux=ax),
                     lambda: bp.ProveJob(g, circ, lab, inp.values, inp.blindings, inp.seeds, 3, publics=inp.publics, aux=ax),
                     lambda: bp.prove_batch_transcripts(g, circ, ts(), inp.values, inp.blindings, inp.seeds, 3, publics=inp.publics, aux=ax),
                     lambda: bp.prove_batch_raw(g, circ, lab, inp.values, inp.blindings, inp.seeds, 3, publics=inp.publics, aux=ax)):
            try:
                call()
                assert False, "an auxiliary block of %r bytes went through" % (None if ax is None else len(ax))
            except AssertionError as e:
                assert "aux" in str(e), e
    P, _ = bp.prove_batch(g, circ, lab, inp.values, inp.blindings, inp.seeds, 3, wires=inp.wires, publics=inp.publics, aux=None)
    assert P == [oracle_proof("mix", j)["proof"] for j in range(3)]
    # lists of per-proof lists are encoded like `publics`
    P, _ = bp.prove_batch(g, circ, lab, inp.values, inp.blindings, inp.seeds, 3, publics=inp.publics, aux=[o["aux"] for o in inp.obs])
    assert P[2] == oracle_proof("mix", 2)["proof"]


def check_golden_unchanged(lib, glib):
    """descriptions without the kind prove what they proved before: the committed vectors of tests/golden/proofs.json"""
    DB.check_golden_unchanged(lib, glib)
    circ = bp.CompiledGadget("bound_check", [8, 10, 0, 200, 0], [], lib=lib, glib=glib)
    assert circ.a == 0 and circ.p == 0


# ------------------------------------------------------------------ the front-end: the lean tree forms
# form -> (plain gadget, arity, levels / depth, capacity).  Four levels are the smallest 4-ary tree there is: the gadget consumes the
# leaf index a byte - four base-4 digits - at a time (LeafIndexBytes = levels / 4, gadget_vsmt_4.rs), so n = 4 x (19 + 150) + 6 of N = 1024
TREES = {"t4": ("vsmt_4", 4, 4, 1024), "t2": ("vsmt_2", 2, 3, 512)}
TREE_LABEL, TREE_PR = b"VSMT", 2


def tree_witness(glib, form, k):
    """tree k (leaves i -> i + 100 k for i in 1..5; Inverse S-box, 2 partial rounds) and the membership witness of leaf 1 + k
    -> (root, the plain gadget's values, positions of the proof nodes in them, number of statics)"""
    _, arity, levels, _ = TREES[form]
    t = bp.SparseMerkleTree(arity, levels, TREE_PR, glib=glib, inverse=True)
    for i in range(1, 6):
        t.update(i, i + 100 * k)
    idx = 1 + k
    leaf, nodes = t.get(idx)
    assert leaf == sc_to_bytes(idx + 100 * k)
    if arity == 4:
        return t.root(), leaf + sc_to_bytes(idx) + b"".join(nodes) + enc([0, 101]), range(2, 2 + 3 * levels), 2
    bits = enc([(idx >> b) & 1 for b in range(levels)])
    return t.root(), leaf + bits + b"".join(reversed(nodes)) + enc([0, 101, 0, 0]), range(1 + levels, 1 + 2 * levels), 4


def _pick(raw, idxs):
    return b"".join(raw[32 * i:32 * i + 32] for i in idxs)


def _py_tree(form):
    _, arity, levels, _ = TREES[form]
    return FC._tree4(levels, TREE_PR) if arity == 4 else FC._tree2(levels, TREE_PR)


def py_harness(form, cs, idx, bl=None, comms=None):
    """the Python harness of the lean forms on the oracle's Prover (bl: blindings of the committed values in gadget order) or Verifier
    (comms: the non-static commitments): the order of commits and allocations of host/frontend.cpp - leaf, index (bits), the proof
    nodes paired by allocate_multiplier((v_k, v_k+1)), an odd count ending with (v_k, 0), then the statics -> the commitments made"""
    tree = _py_tree(form)
    prover = isinstance(cs, Prover)
    leaf_val, proof = tree.get(idx, True)
    made = []

    def commit(x):
        if prover:
            c, v = cs.commit(x, bl[len(made)])
            made.append(c)
            return G.Alloc(v, x)
        made.append(comms[len(made)])
        return G.Alloc(cs.commit(made[-1]), None)

    def allocated(xs):
        out = []
        for i in range(0, len(xs), 2):
            pair = i + 1 < len(xs)
            l, r = xs[i], xs[i + 1] if pair else 0
            lv, rv, _ = cs.allocate_multiplier((l, r) if prover else None)
            out.append(G.Alloc(lv, l if prover else None))
            if pair:
                out.append(G.Alloc(rv, r if prover else None))
        return out
    statics = lambda k: G.allocate_statics_for_prover(cs, k) if prover else G.allocate_statics_for_verifier(cs, k, PC)
    if form == "t4":
        leaf, index = commit(leaf_val), commit(idx)
        nodes = allocated([x for node in proof for x in node])          # root level first
        G.vanilla_merkle_merkle_tree_4_verif_gadget(cs, tree.depth, tree.root, leaf, index, nodes, statics(2), tree.hash_params,
                                                    tree.leaf_index_bytes, tree.sbox)
    else:
        leaf = commit(leaf_val)
        ib = [commit(b) for b in G.get_bits(idx, tree.depth)]          # LSB first
        nodes = allocated(proof[::-1])                                  # leaf level first
        G.vanilla_merkle_merkle_tree_verif_gadget(cs, tree.depth, tree.root, leaf, ib, nodes, statics(4), tree.hash_params, tree.sbox)
    return made


_TREE_ORACLE = {}


def tree_oracle(form, idx=1):
    """the oracle's proof of the Python harness, computed once per session -> dict(proof, comms (without statics), values, root, bl)"""
    if (form, idx) not in _TREE_ORACLE:
        tree = _py_tree(form)
        leaf_val, proof = tree.get(idx, True)
        ncom = 2 if form == "t4" else 1 + tree.depth
        bl = [S.synth_scalar(b"ax-tree-bl" + form.encode(), i) for i in range(ncom)]
        pr = Prover(PC, Transcript(TREE_LABEL))
        comms = py_harness(form, pr, idx, bl=bl)
        pf = pr.prove(common.oracle_gens(TREES[form][3]), seed(70)).to_bytes()
        if form == "t4":
            flat = [x for node in proof for x in node]
            vals, nodes_at = [leaf_val, idx] + flat + [0, 101], range(2, 2 + len(flat))
        else:
            vals = [leaf_val] + G.get_bits(idx, tree.depth) + proof[::-1] + [0, 101, 0, 0]
            nodes_at = range(1 + tree.depth, 1 + 2 * tree.depth)
        # blindings in the plain gadget's layout: those of the nodes are ignored, the statics' are 0
        if form == "t4":
            bls = bl + [S.synth_scalar(b"ax-ignored", i) for i in range(len(flat))] + [0, 0]
        else:
            bls = bl + [S.synth_scalar(b"ax-ignored", i) for i in range(tree.depth)] + [0] * 4
        _TREE_ORACLE[(form, idx)] = dict(proof=pf, comms=comms, values=enc(vals), blindings=enc(bls), root=sc_to_bytes(tree.root), nodes_at=nodes_at,
                                         n=len(pr.a_L), m=len(pr.v))
    return _TREE_ORACLE[(form, idx)]


def tree_case(form, idx=1):
    def bv(vr, comms, pc):
        py_harness(form, vr, idx, comms=comms)
    return VS.Case(S.Scenario(TREE_LABEL, [0] * (2 if form == "t4" else 1 + TREES[form][2]), None, bv), TREES[form][3])


def check_frontend(lib, glib, form, B=3):
    """the lean tree form: shape; B membership proofs about B different trees in one call of the compiled program with the nodes as
    auxiliary inputs and the roots public == proof for proof the C++ Prover's by host synthesis (bpr1cs_gadget_prove_on, root baked);
    bpr1cs_gadget_verify_on accepts them over the committed values alone and rejects a tampered proof and a foreign root; on the
    oracle's tree the compiled program (root baked), the C++ Prover (one proof and a batch) and the oracle's proof of the Python
    harness are equal bytes"""
    plain, arity, levels, cap = TREES[form]
    gname, ip, lab = plain + "_aux", [levels, TREE_PR], TREE_LABEL
    wit = [tree_witness(glib, form, k) for k in range(B)]
    roots = [w[0] for w in wit]
    assert len(set(roots)) == B
    nodes_at, statics = wit[0][2], wit[0][3]
    a = len(nodes_at)
    m_plain = len(wit[0][1]) // 32
    kept = [i for i in range(m_plain) if i not in nodes_at]
    circ = bp.CompiledGadget(gname, ip, [], lib=lib, glib=glib)
    full = bp.CompiledGadget(plain, ip, [], lib=lib, glib=glib)
    assert full.m == m_plain == (4 + 3 * levels if arity == 4 else 5 + 2 * levels)
    assert (circ.m, circ.a, circ.p) == ((4, 3 * levels, 1) if arity == 4 else (5 + levels, levels, 1)) and circ.has_witness_program
    assert (circ.n, circ.q) == (full.n + (a + 1) // 2, full.q) and len(kept) == circ.m
    assert lib.bpr1cs_circuit_macro_perms(circ.h) >= 1           # the permutations are evaluated jointly
    g = gens(lib, cap)
    vals = b"".join(w[1] for w in wit)
    bls = b"".join(enc([S.synth_scalar(b"ax-tree-bl%d" % j, i) for i in range(m_plain - statics)]) + bytes(32 * statics) for j in range(B))
    seeds = b"".join(seed(50 + j) for j in range(B))
    cut = lambda raw, sz, j: raw[j * sz:(j + 1) * sz]
    cvals = b"".join(_pick(cut(vals, 32 * m_plain, j), kept) for j in range(B))
    cbls = b"".join(_pick(cut(bls, 32 * m_plain, j), kept) for j in range(B))
    ax = b"".join(_pick(cut(vals, 32 * m_plain, j), nodes_at) for j in range(B))
    P, C = bp.prove_batch(g, circ, lab, cvals, cbls, seeds, B, wires=None, publics=b"".join(roots), aux=ax)
    for j in range(B):
        ref, refc, _ = bp.gadget_prove_on(g, gname, ip, [roots[j]], lab, cut(vals, 32 * m_plain, j), cut(bls, 32 * m_plain, j), m_plain, 1,
                                          cut(seeds, 32, j), glib=glib)
        assert P[j] == ref[0], "%s: proof %d of the compiled program differs from the C++ Prover's" % (form, j)
        assert C[j] == refc[0] and len(C[j]) == circ.m
        assert bp.gadget_verify_on(g, gname, ip, [roots[j]], lab, P[j], C[j], glib=glib)[0]
        assert not bp.gadget_verify_on(g, gname, ip, [roots[j]], lab, tampered(P[j]), C[j], glib=glib)[0]
        if B > 1:
            assert not bp.gadget_verify_on(g, gname, ip, [roots[(j + 1) % B]], lab, P[j], C[j], glib=glib)[0]
    vs = b"".join(hashlib.sha256(b"ax-tree-vseed %d" % j).digest() for j in range(B))
    assert bp.verify_batch(g, circ, lab, P, C, B, seeds=vs, publics=b"".join(roots)) == [True] * B
    if B == 3:
        assert bp.verify_batch(g, circ, lab, P, C, B, seeds=vs, publics=b"".join([roots[1], roots[0], roots[2]])) == [False, False, True]
    # ---- the oracle's tree: root baked
    ob = tree_oracle(form)
    assert (ob["n"], ob["m"]) == (circ.n, circ.m)
    base = bp.CompiledGadget(gname, ip, [ob["root"]], lib=lib, glib=glib)
    assert (base.p, base.a, base.m, base.n, base.q) == (0, a, circ.m, circ.n, circ.q) and base.has_witness_program
    sd = seed(70)
    Pb, Cb = bp.prove_batch(g, base, lab, _pick(ob["values"], kept), _pick(ob["blindings"], kept), sd, 1, wires=None, aux=_pick(ob["values"], nodes_at))
    assert Pb[0] == ob["proof"], "%s: the compiled program's proof differs from the oracle's proof of the Python harness" % form
    assert Cb[0][:len(ob["comms"])] == ob["comms"]
    ref, refc, _ = bp.gadget_prove_on(g, gname, ip, [ob["root"]], lab, ob["values"], ob["blindings"], m_plain, 1, sd, glib=glib)
    assert ref[0] == ob["proof"] and refc[0] == Cb[0]
    ref2, refc2, _ = bp.gadget_prove_on(g, gname, ip, [ob["root"]], lab, ob["values"] * 2, ob["blindings"] * 2, m_plain, 2, sd + seed(71), glib=glib)
    assert ref2[0] == ob["proof"] and refc2 == [Cb[0], Cb[0]] and ref2[1] != ref2[0]
    wires, n, q = bp.gadget_synthesize(gname, ip, [ob["root"]], ob["values"], m_plain, glib=glib)
    assert (n, q) == (circ.n, circ.q)
    # the same proof over host wires and no auxiliary block
    Ph, _ = bp.prove_batch(g, base, lab, _pick(ob["values"], kept), _pick(ob["blindings"], kept), sd, 1, wires=wires)
    assert Ph[0] == ob["proof"]
    return ob, Cb[0]


def check_tree_verifiers(lib, glib, form="t4"):
    """the verifier forms over three proofs of the lean tree circuit (root baked: the oracle's tree), one tampered, against the oracle's
    verdicts on the Python harness run by the oracle's Verifier"""
    plain, arity, levels, cap = TREES[form]
    ob = tree_oracle(form)
    base = bp.CompiledGadget(plain + "_aux", [levels, TREE_PR], [ob["root"]], lib=lib, glib=glib)
    g = gens(lib, cap)
    kept = [i for i in range(len(ob["values"]) // 32) if i not in ob["nodes_at"]]
    B = 3
    seeds = b"".join(seed(70 + j) for j in range(B))
    P, C = bp.prove_batch(g, base, TREE_LABEL, _pick(ob["values"], kept) * B, _pick(ob["blindings"], kept) * B, seeds, B, wires=None,
                          aux=_pick(ob["values"], ob["nodes_at"]) * B)
    assert P[0] == ob["proof"]
    P[1] = tampered(P[1])
    _check_verifier_forms(lib, g, base, TREE_LABEL, [tree_case(form)] * B, P, C, b"", 1, cap)
