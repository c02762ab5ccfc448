"""Public coefficients (BPR1CS_VAR_SCALE, include/bpr1cs.h "Public coefficients"): circuits, mirrors and checkers shared by the CPU
simulator (tests/test_public_coeff.py) and the device (tests/test_gpu_public_coeff.py).

The oracle knows no public inputs, and needs none: a proof of a circuit whose term (marker (SCALE, k, s), (var, c)) stands for
s c p_k x var is, byte for byte, the proof of the BAKED circuit - the same rows with the constant coefficient s c p_k in the pair's
place - and a verifier of the baked circuit accepts it.  That identity is the oracle of everything here.  A circuit is written once, as a
small symbolic program (`Prog`: multipliers whose operands are combinations or bits of combinations, and rows; a term is (variable,
coefficient, public index or None[, marker coefficient])), and emitted in two forms: rows, wops and combinations with markers, which the
library gets ONCE for all proofs; and, per proof, the baked rows driven through the oracle's Prover / Verifier with the assignments
computed here.

Circuits (capacity <= 128, n <= 64, window_bits = 8):
  kinds   scaled terms on a left, a right, an output wire and a committed value (the negated w_V); one variable plain and scaled in one
          row; one variable under two markers with different k; folded coefficients +1, -1 (by s = 1 and by s c = +-1 with s = 2) and
          general; a marker with s != 1; the highest index p - 1 named by a marker alone; Public (linear) terms beside scaled ones
  chunks  two committed values with 600 scaled entries each (k cycling over p = 3) in 600 consecutive rows of a 642-row circuit - three
          chunks of FLATTEN_CHUNK (256 + 256 + 88), crossing rows 255 / 256 and 511 / 512 of the power tables -, a slot with exactly 256
          scaled entries, one with 257, one with a single one; slots with plain AND scaled entries, slots with scaled entries only
  p70     70 public inputs, every one a coefficient, in one row over committed values and wires
  lc      the witness program: a scaled term under W_LC (a single term with coefficient 1 among them: no plain copy), a scaled term over
          the wires of the previous multiplier (register cache / fence path of the team kernel), a 17-term combination (two trips of a
          16-lane team) with scaled terms
  lcbits  64 multipliers, the bits of budget - w_0 x_0 - w_1 x_1 under W_LCNOTBIT / W_LCBIT, weights as public coefficients, the
          budget a Public (linear) term
  poseidon  one annotated Poseidon permutation (width 2, one full round of Inverse S-boxes) whose input combinations hold scaled terms;
          proved through the plain program (bp.Circuit hands over no annotation) and through the joint evaluation (annotated_circuit)
Rows hold for every witness and every public input because each is closed by a multiplier (e, 0) whose left wire is the value of the
row's combination ("chunks": because the two values of a pair are equal), so the public inputs are free; they, the committed values,
blindings and seeds differ from proof to proof.
"""
import ctypes
import hashlib
import os

from pyref import scenarios as S
from pyref.ed import L, decompress, sc_to_bytes
from pyref.merlin import Transcript
from pyref.r1cs import LinearCombination, One, Prover, Variable
import common
import derived_bits_cases as DB
import public_input_cases as PI
import verify_scalar_cases as VS
import witness_check_cases as WC

bp = common.bp
PC = common.PC
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONCANONICAL = L.to_bytes(32, "little")        # l itself: the smallest non-canonical encoding
CV, ML, MR, MO, ONE, PUB, SCALE = 0, 1, 2, 3, 4, 5, 8
HALF = (L + 1) // 2                            # 2 x HALF = 1 (mod l)


def label(name):
    return b"PublicCoeff-" + name.encode()


# ------------------------------------------------------------------ the symbolic program
def _t(term):
    """(var, c) | (var, c, k) | (var, c, k, s) -> (var, c, k, s)"""
    return tuple(term) + (None, 1)[len(term) - 2:]


def neg(terms):
    return [(v, (-c) % L, k, s) for v, c, k, s in map(_t, terms)]


class Prog:
    def __init__(self, m):
        self.m, self.gates, self.rows = m, [], []

    def _gate(self, left, right):
        self.gates.append((left, right))
        return len(self.gates) - 1

    def mul(self, left, right):
        """cs.multiply: a multiplier over two combinations and the two rows that tie its wires to them"""
        i = self._gate(("lc", list(left)), ("lc", list(right)))
        self.rows.append(list(left) + [((ML, i), L - 1)])
        self.rows.append(list(right) + [((MR, i), L - 1)])
        return i

    def close(self, terms):
        """a row that holds whatever the inputs are: the multiplier (value of `terms`, 0) and the row terms - left wire"""
        i = self._gate(("lc", list(terms)), ("lc", []))
        self.rows.append(list(terms) + [((ML, i), L - 1)])
        return i

    def bits(self, terms, nbits):
        """positive_no_gadget_lc (host/gadgets.hpp): per bit a multiplier (1 - bit, bit) of the combination's canonical value"""
        terms = list(terms)
        total = neg(terms)
        for b in range(nbits):
            i = self._gate(("notbit", terms, b), ("bit", terms, b))
            self.rows.append([((MO, i), 1)])
            self.rows.append([((ML, i), 1), ((MR, i), 1), ((ONE, 0), L - 1)])
            total.append(((MR, i), pow(2, b, L)))
        self.rows.append(total)

    def sbox(self, terms):
        """an Inverse S-box as the Poseidon gadget allocates it: the multiplier (x, 1/x), the row that ties x to its combination, x / x = 1"""
        i = self._gate(("lc", list(terms)), ("inv",))
        self.rows.append(list(terms) + [((ML, i), L - 1)])
        self.rows.append([((MO, i), 1), ((ONE, 0), L - 1)])
        return i

    def row(self, terms):
        self.rows.append(list(terms))

    @property
    def p(self):
        ks = [k for row in self._all() for v, c, k, s in map(_t, row) if k is not None] + \
             [v[1] for row in self._all() for v, c, k, s in map(_t, row) if v[0] == PUB]
        return 1 + max(ks) if ks else 0

    def _all(self):
        return self.rows + [op[1] for g in self.gates for op in g if len(op) > 1] + list(getattr(self, "perm_in", []))


def _eval(terms, st, pub):
    """value of a combination: st = (values, a_L, a_R, a_O)"""
    acc = 0
    for (kind, idx), c, k, s in map(_t, terms):
        x = 1 if kind == ONE else pub[idx] if kind == PUB else st[kind][idx]
        acc += c * s * (pub[k] if k is not None else 1) * x
    return acc % L


def _lib_terms(terms):
    """the library's form: a marker with s = 1 as the shim's 3-tuple, any other marker written out"""
    out = []
    for var, c, k, s in map(_t, terms):
        if k is None:
            out.append((var, c))
        elif s == 1:
            out.append((var, c, k))
        else:
            out += [((SCALE, k), s), (var, c)]
    return out


def baked_terms(terms, pub):
    """the oracle's form for the public inputs `pub`: constant coefficients"""
    out = []
    for (kind, idx), c, k, s in map(_t, terms):
        if kind == PUB:
            out.append((One(), c * pub[idx] % L))
        else:
            out.append((One() if kind == ONE else Variable(kind, idx), c * s * (pub[k] if k is not None else 1) % L))
    return out


# ------------------------------------------------------------------ the circuits
def _c(tag, i):
    return S.synth_scalar(b"pc-coeff-" + tag, i) or 3


def _kinds():
    g = Prog(2)
    g.mul([((CV, 0), 1)], [((CV, 1), 1)])
    g.close([((ML, 0), 3, 0), ((MR, 0), L - 1, 1), ((MO, 0), 1, 2), ((CV, 0), _c(b"k", 0), 0), ((CV, 1), 5)])
    g.close([((CV, 0), 7), ((CV, 0), 1, 1), ((CV, 1), 1, 0), ((CV, 1), L - 1, 2), ((ONE, 0), 9), ((PUB, 1), 4), ((MO, 1), _c(b"k", 1), 2)])
    g.close([((MO, 0), 2, 3, 11), ((ML, 0), HALF, 0, 2), ((MR, 0), (L - 1) // 2, 1, 2), ((PUB, 0), L - 1)])
    return g, 8


def _chunks():
    g = Prog(5)
    g.mul([((CV, 0), 1)], [((CV, 1), 1)])
    for j in range(600):
        c = (1, L - 1, _c(b"c", j))[j % 3 if j % 7 else 2]
        row = [((CV, 0), c, j % 3), ((CV, 1), (-c) % L, j % 3)]
        if j < 256:
            d = (L - 1, _c(b"d", j), 1)[j % 3]
            row += [((CV, 2), d, (j + 1) % 3), ((CV, 3), (-d) % L, (j + 1) % 3)]
        if j == 256:
            row += [((CV, 3), 6, 0), ((CV, 4), L - 6, 0)]
        g.row(row)
    for j in range(40):
        f = _c(b"f", j) if j % 2 else 1
        g.row([((CV, 0), f), ((CV, 1), (-f) % L)])
    return g, 2


def _p70():
    g = Prog(2)
    g.mul([((CV, 0), 1)], [((CV, 1), 1)])
    pool = [(CV, 0), (CV, 1), (ML, 0), (MR, 0), (MO, 0)]
    g.close([(pool[k % 5], (1, L - 1, _c(b"p", k))[k % 3], k) for k in range(70)])
    return g, 4


def _lc():
    g = Prog(2)
    g.mul([((CV, 0), 5, 0)], [((CV, 1), 1)])
    g.mul([((CV, 0), 1, 1)], [((ML, 0), 1, 0)])          # one term, coefficient 1, scaled: not the plain copy a {1 * var} combination becomes
    pool = [(CV, 0), (CV, 1), (ML, 0), (MR, 0), (MO, 0), (ML, 1), (MR, 1), (MO, 1)]
    wide = [(pool[t % 8], _c(b"w", t), (None, 0, 1, 2)[t % 4]) for t in range(16)] + [((ONE, 0), 12)]
    g.mul(wide, [((MO, 1), 3, 2), ((MR, 1), L - 1, 0), ((ONE, 0), 1)])
    g.close([((MO, 2), 1, 0), ((PUB, 1), 2), ((ML, 2), L - 1, 2)])
    return g, 4


def _lcbits():
    g = Prog(2)
    g.bits([((PUB, 2), 1), ((CV, 0), L - 1, 0), ((CV, 1), L - 1, 1)], 64)
    return g, 64


POS_KEYS = [_c(b"rk", 0), _c(b"rk", 1)]
POS_MDS = [1, 2, 3, 5]


def _poseidon():
    """one annotated Poseidon permutation of width 2 with a single full round (two Inverse S-boxes) whose INPUT combinations hold scaled
    terms over committed values and a wire of the multiplier before it; the S-box operands are input + round key, as the gadget's"""
    g = Prog(2)
    g.mul([((CV, 0), 1)], [((CV, 1), 1)])
    g.perm_in = [[((CV, 0), 3, 0), ((MO, 0), 1, 1)], [((CV, 1), 1, 1), ((ONE, 0), 5), ((ML, 0), L - 1, 2)]]
    for k in range(2):
        g.sbox(g.perm_in[k] + [((ONE, 0), POS_KEYS[k])])
    g.close([((MR, 1), 1, 2), ((MR, 2), 7)])
    return g, 4


_BUILDERS = dict(kinds=_kinds, chunks=_chunks, p70=_p70, lc=_lc, lcbits=_lcbits, poseidon=_poseidon)
_PROGS = {}


def prog(name):
    if name not in _PROGS:
        _PROGS[name] = _BUILDERS[name]()
    return _PROGS[name][0]


def cap(name):
    prog(name)
    return _PROGS[name][1]


def shape(name):
    """the library's form -> dict(n, m, p, rows, wops, lcs)"""
    g = prog(name)
    lcs, wops, last = [], [], (None, None)
    for gate in g.gates:
        w = ()
        for op in gate:
            if op[0] == "lc":
                lcs.append(_lib_terms(op[1]))
                w += (bp.W_LC, len(lcs) - 1)
            elif op[0] == "inv":
                w += (bp.W_INV_LEFT, 0)
            else:
                if last[0] is not op[1]:                 # one entry per decomposition, named 2 x bits times in a row
                    lcs.append(_lib_terms(op[1]))
                    last = (op[1], len(lcs) - 1)
                w += (bp.W_LCBIT if op[0] == "bit" else bp.W_LCNOTBIT, last[1] << 8 | op[2])
        wops.append(w)
    perm_in = []
    for terms in getattr(g, "perm_in", []):              # the annotation's input combinations, behind the operands'
        lcs.append(_lib_terms(terms))
        perm_in.append(len(lcs) - 1)
    return dict(n=len(g.gates), m=g.m, p=g.p, rows=[_lib_terms(r) for r in g.rows], wops=wops, lcs=lcs, perm_in=perm_in)


# ------------------------------------------------------------------ per-proof inputs
def values(name, j):
    if name == "chunks":
        a, b = S.synth_scalar(b"pc-v-chunks", 2 * j), S.synth_scalar(b"pc-v-chunks", 2 * j + 1)
        return [a, a, b, b, b]
    if name == "lcbits":
        return [S.synth_scalar(b"pc-v-bits", 2 * j + i) % (1 << 20) for i in range(2)]
    return [S.synth_scalar(b"pc-v" + name.encode(), 16 * j + i) if (i + j) % 5 else (0, 1, L - 1)[j % 3] for i in range(prog(name).m)]


def blindings(name, j):
    return [S.synth_scalar(b"pc-bl" + name.encode(), 16 * j + i) for i in range(prog(name).m)]


def seed(j):
    return S.synth_seed(3000 + j)


def publics(name, j):
    """the p public inputs of proof j (ints), distinct per proof; 1 and l - 1 among the general ones"""
    p = prog(name).p
    if name == "lcbits":
        w = [1 + S.synth_scalar(b"pc-p-bits", 2 * j + i) % (1 << 20) for i in range(2)]
        v = values(name, j)
        slack = (0, (1 << 64) - 1, S.synth_scalar(b"pc-slack", j) % (1 << 64))[j % 3]
        return w + [w[0] * v[0] + w[1] * v[1] + slack]
    out = [S.synth_scalar(b"pc-p" + name.encode(), 128 * j + k) or 2 for k in range(p)]
    if j % 4 in (1, 2):
        out[j % p] = (1, L - 1)[j % 4 - 1]
    return out


def enc(xs):
    return b"".join(sc_to_bytes(x % L) for x in xs)


def altered(pub, k, delta=1):
    out = list(pub)
    out[k] = (out[k] + delta) % L
    return out


def wires(name, j, pub=None):
    """the assignment of proof j -> (a_L, a_R, a_O)"""
    g, pub = prog(name), publics(name, j) if pub is None else pub
    st = (values(name, j), [], [], [])

    def operand(op):
        if op[0] == "lc":
            return _eval(op[1], st, pub)
        bit = (_eval(op[1], st, pub) >> op[2]) & 1
        return bit if op[0] == "bit" else 1 - bit
    for left, right in g.gates:
        l = operand(left)
        r = pow(l, L - 2, L) if right[0] == "inv" else operand(right)
        st[1].append(l); st[2].append(r); st[3].append(l * r % L)
    return st[1], st[2], st[3]


# ------------------------------------------------------------------ the oracle on the baked circuit
def _drive(name, cs, pub, assignment):
    g = prog(name)
    for i in range(len(g.gates)):
        cs.allocate_multiplier(None if assignment is None else (assignment[0][i], assignment[1][i]))
    for row in g.rows:
        cs.constrain(LinearCombination(baked_terms(row, pub)))


def case(name, pub):
    m = prog(name).m

    def bpv(pr, bl, vals=None):
        raise NotImplementedError      # (proofs are made by oracle_proof below)

    def bv(vr, comms, pc):
        for c in comms:
            vr.commit(c)
        _drive(name, vr, pub, None)
    return VS.Case(S.Scenario(label(name), [0] * m, bpv, bv), cap(name))


_PROOFS = {}


def oracle_proof(name, j, pub=None, prove=True):
    """the oracle's Prover on proof j's baked circuit -> dict(proof, comms, wires, values, blindings, constraints, n); `pub`: other public
    inputs for the ROWS than proof j's (the wires stay the honest ones: a violated witness); prove=False: synthesis only"""
    honest = publics(name, j)
    pub = honest if pub is None else pub
    key = (name, j, tuple(pub), prove)
    if key not in _PROOFS:
        vals, bls = values(name, j), blindings(name, j)
        pr = Prover(PC, Transcript(label(name)))
        comms = [pr.commit(x, b)[0] for x, b in zip(vals, bls)]
        _drive(name, pr, pub, wires(name, j, honest))
        out = dict(comms=comms, values=enc(vals), blindings=enc(bls), wires=enc(pr.a_L + pr.a_R + pr.a_O), n=len(pr.a_L),
                   constraints=[list(lc.terms) for lc in pr.constraints], proof=None)
        if prove:
            out["proof"] = pr.prove(common.oracle_gens(cap(name)), seed(j)).to_bytes()
        _PROOFS[key] = out
    return _PROOFS[key]


_REPLAYS = {}


def replay(name, pub, proof, comms, sd):
    key = (name, tuple(pub), proof, tuple(comms), sd)
    if key not in _REPLAYS:
        _REPLAYS[key] = VS._replay(case(name, pub), proof, comms, sd)
    return _REPLAYS[key]


def oracle_accepts(name, pub, proof, comms, sd):
    """the oracle's verifier on the baked circuit: verification_scalars + the C oracle's multiscalar multiplication"""
    scalars, own, N, k, _ = replay(name, pub, proof, comms, sd)
    assert all(decompress(pt) is not None for _, pt in own)
    sc = [scalars[i] for i, _ in own] + scalars[k:k + 2 + 2 * N]
    pts = [pt for _, pt in own] + VS.shared_bases(cap(name), N)
    return VS.coracle().msm(sc, pts) == bytes(32)


def expected_scalars(name, pubs, P, C, seeds, batch_seed, index_base):
    """-> ((2N + 2) x 32 bytes, own-points sum): verify_scalar_cases' derivation with a baked circuit per proof and the public message"""
    reps = [replay(name, pub, pf, cm, sd) for pub, pf, cm, sd in zip(pubs, P, C, seeds)]
    rho = PI.weights([r[4] for r in reps], [enc(p) for p in pubs], batch_seed, index_base)
    N = reps[0][2]
    out = b"".join(sc_to_bytes(sum(w * r[0][r[3] + i] for w, r in zip(rho, reps)) % L) for i in range(2 * N + 2))
    sc, pts = [], []
    for w, (scalars, own, _, _, _) in zip(rho, reps):
        sc += [w * scalars[i] % L for i, _ in own]
        pts += [pt for _, pt in own]
    return out, VS.coracle().msm(sc, pts)


def check_oracle():
    """the oracle itself (CPU only): it accepts its own proof of every circuit's baked form under the right public inputs and rejects it
    under every altered coefficient input the verifier tests use; the library's form sizes p as the table says"""
    assert {n: (prog(n).p, len(prog(n).gates), prog(n).m) for n in _BUILDERS} == dict(
        kinds=(4, 4, 2), chunks=(3, 1, 5), p70=(70, 2, 2), lc=(3, 4, 2), lcbits=(3, 64, 2), poseidon=(3, 4, 2))
    ch = shape("chunks")
    per_slot = lambda idx: sum(1 for r in ch["rows"] for t in r if len(t) == 3 and t[0] == (CV, idx))
    assert [per_slot(i) for i in range(5)] == [600, 600, 256, 257, 1] and len(ch["rows"]) == 642
    assert max(len(t) for t in shape("lc")["lcs"]) == 17
    for name, B, bad, k in VERIFIER_CASES:
        ob, pub = oracle_proof(name, bad), publics(name, bad)
        sd = hashlib.sha256(b"pc-oracle").digest()
        assert oracle_accepts(name, pub, ob["proof"], ob["comms"], sd), name
        assert not oracle_accepts(name, altered(pub, k), ob["proof"], ob["comms"], sd), (name, k)


# ------------------------------------------------------------------ library objects, one per (library, circuit)
_CTX = {}
gens = DB.gens


def circuit(lib, name, program=False):
    key = (id(lib), "pc", name, program)
    if key not in _CTX:
        sh = shape(name)
        _CTX[key] = bp.Circuit(sh["n"], sh["m"], sh["rows"], wops=sh["wops"] if program else None, lcs=sh["lcs"] if program else None, lib=lib)
        assert _CTX[key].p == sh["p"]
    return _CTX[key]


class _PoseidonParams(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("full_rounds_beginning", ctypes.c_uint32), ("partial_rounds", ctypes.c_uint32),
                ("full_rounds_end", ctypes.c_uint32), ("mds", ctypes.c_char_p), ("round_keys", ctypes.c_char_p)]


class _PoseidonPerm(ctypes.Structure):
    _fields_ = [("params", ctypes.c_uint32), ("in_lc", ctypes.c_uint32 * 8), ("sbox_mul", ctypes.POINTER(ctypes.c_uint32))]


def annotated_circuit(lib):
    """the circuit "poseidon" with its bpr1cs_poseidon_perm annotation (include/bpr1cs.h), which bp.Circuit does not hand over: the same
    description arrays as bp.Circuit builds, the annotation beside them; asserts that the library took the joint evaluation"""
    key = (id(lib), "pc", "poseidon", "annotated")
    if key not in _CTX:
        sh = shape("poseidon")
        var, coeff, off = [], bytearray(), [0]
        for row in sh["rows"]:
            for term in row:
                bp._emit_term(term, var, coeff)
            off.append(len(var))
        lvar, lcoeff, loff = [], bytearray(), [0]
        for terms in sh["lcs"]:
            for term in terms:
                bp._emit_term(term, lvar, lcoeff)
            loff.append(len(lvar))
        d = bp._CircuitDesc()
        d.n, d.q, d.m = sh["n"], len(sh["rows"]), sh["m"]
        params = _PoseidonParams(2, 1, 0, 0, enc(POS_MDS), enc(POS_KEYS))
        sbox = bp._u32arr([1, 2])
        perm = _PoseidonPerm(0, (ctypes.c_uint32 * 8)(*sh["perm_in"]), sbox)
        keep = [bp._u32arr(off), bp._u32arr(var), bytes(coeff), (bp._WOp * len(sh["wops"]))(*[bp._WOp(*w) for w in sh["wops"]]),
                bp._u32arr(loff), bp._u32arr(lvar), bytes(lcoeff), params, sbox, perm]
        d.row_off, d.term_var, d.term_coeff, d.wops, d.lc_off, d.lc_var, d.lc_coeff = keep[:7]
        d.n_lc = len(sh["lcs"])
        d.n_poseidon_params, d.poseidon_params = 1, ctypes.cast(ctypes.pointer(params), ctypes.c_void_p)
        d.n_poseidon_perms, d.poseidon_perms = 1, ctypes.cast(ctypes.pointer(perm), ctypes.c_void_p)
        c = bp.Circuit.__new__(bp.Circuit)
        c.lib, c.n, c.m, c.q, c.p, c.a, c._keep = lib, d.n, d.m, d.q, sh["p"], 0, keep
        h = ctypes.c_void_p()
        bp._chk(lib.bpr1cs_circuit_create(ctypes.byref(d), ctypes.byref(h)))
        c.h, c.proof_len = h, lib.bpr1cs_proof_len(h)
        assert lib.bpr1cs_circuit_macro_perms(h) == 1, "the annotation was not taken"
        _CTX[key] = c
    return _CTX[key]


def check_annotated_poseidon(lib, B=3, **opts):
    """a scaled combination as the input of an annotated Poseidon permutation: the joint evaluation's wires prove what the oracle proves
    on the baked circuit (the plain program of the same description is PROVER_CASES' "poseidon")"""
    circ, g, inp = annotated_circuit(lib), gens(lib, cap("poseidon")), Inputs("poseidon", B)
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        P, C = bp.prove_batch(g, circ, label("poseidon"), inp.values, inp.blindings, inp.seeds, B, wires=None, publics=inp.publics)
    finally:
        for k in opts:
            g.set_option(k, -1)
    for j in range(B):
        assert P[j] == oracle_proof("poseidon", j)["proof"], "annotated Poseidon permutation (%r): proof %d of %d" % (opts, j, B)


class Inputs:
    """B proofs' worth of everything a prove call takes; tampers: {proof: (public index, delta)}"""

    def __init__(self, name, B, tampers=None, first=0):
        js = range(first, first + B)
        self.obs = [oracle_proof(name, j, prove=False) for j in js]
        self.name, self.B = name, B
        self.values = b"".join(o["values"] for o in self.obs)
        self.blindings = b"".join(o["blindings"] for o in self.obs)
        self.seeds = b"".join(seed(j) for j in js)
        self.wires = b"".join(o["wires"] for o in self.obs)
        self.pub = [publics(name, j) for j in js]
        for j, (k, delta) in (tampers or {}).items():
            self.pub[j] = altered(self.pub[j], k, delta)
        self.publics = b"".join(enc(p) for p in self.pub)


def prove_draws(lib, g, circ, name, inp, wires):
    """bpr1cs_prove_batch_draws as its caller uses it (tests/witness_check_cases.prove_draws): transcripts past "m" and the 2n + 8 raw
    draws per proof made with the oracle's Merlin; `values` = committed | public"""
    sh = shape(name)
    n, m, B = sh["n"], sh["m"], inp.B
    ts, draws = [], b""
    for j in range(B):
        ot, t = Transcript(label(name)), bp.Transcript(label(name), lib=lib)
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
    rc = lib.bpr1cs_prove_batch_draws(g.h, circ.h, (vp * B)(*[t.h for t in ts]), (inp.values + inp.publics) or b"\0", inp.blindings or b"\0", draws, wires, B, out)
    bp._chk(rc)
    raw = out.raw
    return [raw[i * circ.proof_len:(i + 1) * circ.proof_len] for i in range(B)], [o["comms"] for o in inp.obs]


ENTRIES = ("batch", "transcripts", "draws", "begin_end")


def prove(lib, name, inp, entry="batch", program=False, creation=None, **opts):
    """-> (proofs, commitments) through one of the prove entry points; opts: handle options for the call"""
    sh = shape(name)
    g, circ = gens(lib, cap(name), **(creation or {})), circuit(lib, name, program)
    wires = None if program else inp.wires
    m = sh["m"]
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        if entry == "batch":
            return bp.prove_batch(g, circ, label(name), inp.values, inp.blindings, inp.seeds, inp.B, wires=wires, publics=inp.publics)
        if entry == "transcripts":
            ts = [bp.Transcript(label(name), lib=lib) for _ in range(inp.B)]
            return bp.prove_batch_transcripts(g, circ, ts, inp.values, inp.blindings, inp.seeds, inp.B, wires=wires, publics=inp.publics)
        if entry == "draws":
            return prove_draws(lib, g, circ, name, inp, wires)
        assert entry == "begin_end"     # two jobs in flight, each with its own tail block
        h = max(1, inp.B // 2)
        cut = lambda raw, sz, lo, hi: raw[lo * sz:hi * sz]
        jobs = [bp.ProveJob(g, circ, label(name), cut(inp.values, 32 * m, lo, hi), cut(inp.blindings, 32 * m, lo, hi),
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


def check_prover(lib, name, B, entry="batch", program=False, creation=None, **opts):
    """the library's proofs and commitments of B proofs with distinct public inputs == the oracle's proofs of the B baked circuits"""
    P, C = prove(lib, name, Inputs(name, B), entry, program, creation, **opts)
    for j in range(B):
        ob = oracle_proof(name, j)
        assert C[j] == ob["comms"], "%s: commitments of proof %d" % (name, j)
        assert P[j] == ob["proof"], "%s (%s, %s, %r): proof %d of %d differs from the oracle's proof of the baked circuit" % (
            name, entry, "witness program" if program else "host wires", opts, j, B)
    return P, C


# (circuit, batch) for the prover, host wires and witness program alike: 1, 3, 9 and 70 proofs
PROVER_CASES = [("kinds", 1), ("kinds", 3), ("kinds", 9), ("kinds", 70), ("chunks", 1), ("chunks", 3), ("chunks", 9), ("p70", 3), ("p70", 70),
                ("lc", 1), ("lc", 3), ("lc", 9), ("lc", 70), ("lcbits", 3), ("lcbits", 9), ("poseidon", 3)]
# what the simulator can afford: no 70-proof batch, the 600-entry circuit at one batch size
SIM_PROVER_CASES = [("kinds", 1), ("kinds", 3), ("kinds", 9), ("chunks", 3), ("p70", 3), ("lc", 1), ("lc", 3), ("lc", 9), ("lcbits", 3), ("poseidon", 3)]
SIM_LEFT_OUT = sorted(set(PROVER_CASES) - set(SIM_PROVER_CASES))
TEAM_CASES = [("lc", 9), ("lcbits", 3), ("kinds", 9)]              # witness_team = 4, 8, 16


def check_job_slices(lib, in_flight, program):
    """ONE bpr1cs_prove_batch call of 9 proofs cut into jobs of 4, 4 and 1: every job must get its slice of the public block"""
    check_prover(lib, "lc", 9, program=program, job_proofs=4, jobs_in_flight=in_flight)
    assert bp.last_prove_stats(lib)["jobs"] == 3


# ------------------------------------------------------------------ witness check
def check_witness_check(lib, name="kinds", B=9, bad=4, k=0):
    """check_witness = 1: satisfied witnesses are proved as ever (host wires and the device program); with public coefficient k of
    proof `bad` one higher - the wires are the honest ones - that proof is refused with the record the pure-Python checker of
    tests/witness_check_cases.py computes on the baked rows of the SUBMITTED public inputs; the other proofs are the oracle's"""
    check_prover(lib, name, 3, check_witness=1)
    check_prover(lib, "lc", 3, program=True, check_witness=1)
    inp = Inputs(name, B, {bad: (k, 1)})
    P, C = prove(lib, name, inp, check_witness=1)
    sh = shape(name)
    n, m = sh["n"], sh["m"]
    for j in range(B):
        ob = oracle_proof(name, j, pub=inp.pub[j], prove=False)
        want = WC.violations(dict(n=n, constraints=ob["constraints"]), inp.wires[96 * n * j:96 * n * (j + 1)], inp.values[32 * m * j:32 * m * (j + 1)])
        if j == bad:
            assert want is not None and want["gates"] == 0 and want["rows"] >= 1 and want["row"] is not None
            assert bp.refusal(P[j]) == want and P[j] == WC.record(len(P[j]), want), (bp.refusal(P[j]), want)
        else:
            assert want is None and P[j] == oracle_proof(name, j)["proof"], j
    assert bp.last_prove_stats(lib)["refused"] == 1


# ------------------------------------------------------------------ the verifier forms
FORMS = ("per_proof", "group_fb1", "group_fb2")


def verdicts(lib, name, P, C, seeds, pub_bytes, form):
    g, circ = gens(lib, cap(name)), circuit(lib, name)
    opts = {} if form == "per_proof" else dict(verify_group=4, verify_group_fallback=1 if form == "group_fb1" else 2)
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        return bp.verify_batch(g, circ, label(name), P, C, len(P), seeds=b"".join(seeds), publics=pub_bytes)
    finally:
        for k in opts:
            g.set_option(k, -1)


def combined(lib, name, P, C, seeds, pub_bytes, batch_seed, index_base=0):
    g, circ = gens(lib, cap(name)), circuit(lib, name)
    return bp.verify_batch_combined(g, circ, label(name), P, C, len(P), batch_seed=batch_seed, index_base=index_base, seeds=b"".join(seeds), publics=pub_bytes)


def scalars(lib, name, P, C, seeds, pub_bytes, batch_seed, index_base=0):
    g, circ = gens(lib, cap(name)), circuit(lib, name)
    return bp.verify_batch_scalars(g, circ, label(name), P, C, len(P), batch_seed=batch_seed, index_base=index_base, seeds=b"".join(seeds), publics=pub_bytes)


# (circuit, batch, proof with the bad public input, its index): batches 1, 3, 33 (two leaves) and 70 (above a wavefront of proofs)
VERIFIER_CASES = [("kinds", 1, 0, 0), ("kinds", 3, 1, 3), ("lc", 3, 2, 1), ("p70", 3, 1, 64), ("chunks", 3, 1, 2), ("lcbits", 3, 0, 1),
                  ("kinds", 33, 32, 1), ("p70", 70, 64, 69)]
SIM_VERIFIER_CASES = [c for c in VERIFIER_CASES if c[1] <= 3]
_MADE = {}


def made(lib, name, B):
    """B proofs with their right public inputs: the oracle's where there are few, else the library's through the witness program -
    what the verifier must say about them is the mirror's business"""
    if (id(lib), name, B) not in _MADE:
        if B <= 5:
            obs = [oracle_proof(name, j) for j in range(B)]
            P, C = [o["proof"] for o in obs], [o["comms"] for o in obs]
        else:
            P, C = prove(lib, name, Inputs(name, B), program=True)
        _MADE[(id(lib), name, B)] = (P, C)
    return _MADE[(id(lib), name, B)]


def check_verifier(lib, name, B, bad, k):
    """every verifier form over B proofs: right public inputs; coefficient input k of proof `bad` altered (that proof alone gets verdict
    0); the same made non-canonical (that proof malformed, the others judged)"""
    P, C = made(lib, name, B)
    pubs = [publics(name, j) for j in range(B)]
    seeds = [hashlib.sha256(b"pc-vseed %d" % j).digest() for j in range(B)]
    right = b"".join(enc(p) for p in pubs)
    tag = ("%s-%d" % (name, B)).encode()
    bseeds = (bytes(32), hashlib.sha256(b"pc batch seed " + tag).digest())     # a constant batch seed leaves the binding alone
    everyone = [True] * B
    # ---- right public inputs
    assert all(oracle_accepts(name, pubs[j], P[j], C[j], seeds[j]) for j in sorted({0, bad, B - 1}))
    for form in FORMS:
        assert verdicts(lib, name, P, C, seeds, right, form) == everyone, form
    for bs in bseeds:
        assert combined(lib, name, P, C, seeds, right, bs) == (bytes(32), True)
        got = scalars(lib, name, P, C, seeds, right, bs, index_base=5)
        want = expected_scalars(name, pubs, P, C, seeds, bs, 5)
        assert got[2] is True and got[1] == want[1], "%s, B = %d: own-points sum" % (name, B)
        assert got[0] == want[0], "%s, B = %d: combined scalars differ from the mirror's" % (name, B)
    # ---- one coefficient input altered: the oracle's verifier of the baked circuit with that constant rejects the proof
    pubs_bad = list(pubs)
    pubs_bad[bad] = altered(pubs[bad], k)
    wrong = b"".join(enc(p) for p in pubs_bad)
    assert not oracle_accepts(name, pubs_bad[bad], P[bad], C[bad], seeds[bad])
    for form in FORMS:
        assert verdicts(lib, name, P, C, seeds, wrong, form) == [j != bad for j in range(B)], form
    pt, wf = combined(lib, name, P, C, seeds, wrong, bseeds[1])
    assert wf is True and pt != bytes(32)
    got = scalars(lib, name, P, C, seeds, wrong, bseeds[1])
    assert got[:2] == expected_scalars(name, pubs_bad, P, C, seeds, bseeds[1], 0) and got[2] is True
    # ---- a non-canonical public input: that proof is malformed, the rest are judged
    off = 32 * (prog(name).p * bad + k)
    nonc = right[:off] + NONCANONICAL + right[off + 32:]
    for form in FORMS:
        assert verdicts(lib, name, P, C, seeds, nonc, form) == [j != bad for j in range(B)], form
    assert combined(lib, name, P, C, seeds, nonc, bseeds[1])[1] is False
    assert scalars(lib, name, P, C, seeds, nonc, bseeds[1])[2] is False


# ------------------------------------------------------------------ bpr1cs_circuit_create
def _refused(call, why):
    try:
        call()
        assert False, "accepted: %s" % why
    except bp.R1CSError as e:
        assert e.code == -17, why


def check_create(lib):
    """what bpr1cs_circuit_create accepts (and how p is sized) and every refusal of include/bpr1cs.h "Public coefficients", in rows and
    in combinations"""
    v0, w0, one = (bp.VAR_COMMITTED, 0), (bp.VAR_MUL_LEFT, 0), ((bp.VAR_ONE, 0), 1)
    mark = lambda k, s=1: ((bp.VAR_SCALE, k), s)
    zero = (bp.W_LC, 0)                                       # combination 0: empty
    in_row = lambda *terms: bp.Circuit(2, 1, [list(terms)], lib=lib)
    in_lc = lambda *terms, **kw: bp.Circuit(2, 1, [], wops=[zero + zero, kw.get("op", (bp.W_LC, 1)) + zero], lcs=[[], list(terms)], lib=lib)
    # accepted; p = 1 + the highest index over public terms and markers
    assert in_row((v0, 3, 0)).p == 1
    assert in_row((v0, 3, 6), ((bp.VAR_PUBLIC, 2), 1)).p == 7
    assert in_row(mark((1 << 20) - 1, 5), (w0, 2)).p == 1 << 20
    assert in_lc((v0, 3, 4), one).p == 5
    assert in_lc((w0, 3, 1), op=(bp.W_LCBIT, 1 << 8 | 3)).p == 2           # a wire of an EARLIER multiplier
    for kind in (bp.VAR_COMMITTED, bp.VAR_MUL_LEFT, bp.VAR_MUL_RIGHT, bp.VAR_MUL_OUT):
        in_row(((kind, 0), L - 1, 0))
        in_lc(((kind, 0), L - 1, 0))
    for make, where in ((in_row, "row"), (in_lc, "combination")):
        _refused(lambda: make((v0, 1), mark(0)), "a marker that ends its %s" % where)
        _refused(lambda: make(mark(0), one), "a marker in front of One (%s)" % where)
        _refused(lambda: make(mark(0), ((bp.VAR_PUBLIC, 0), 2)), "a marker in front of a public term (%s)" % where)
        _refused(lambda: make(mark(0), mark(1), (v0, 1)), "a marker in front of a marker (%s)" % where)
        _refused(lambda: make(mark(0), ((6, 0), 1)), "a marker in front of kind 6 (%s)" % where)
        _refused(lambda: make(mark(1 << 20), (v0, 1)), "k = 2^20 (%s)" % where)
        _refused(lambda: make(mark(0x0fffffff), (v0, 1)), "k = 2^28 - 1 (%s)" % where)
        _refused(lambda: make(mark(0, 0), (v0, 1)), "s = 0 (%s)" % where)
        _refused(lambda: make(mark(0, NONCANONICAL), (v0, 1)), "s = l (%s)" % where)
        _refused(lambda: make(mark(0, (L + 1).to_bytes(32, "little")), (v0, 1)), "s = l + 1 (%s)" % where)
        _refused(lambda: make((v0, 0, 0)), "c = 0 (%s)" % where)
        _refused(lambda: make((v0, NONCANONICAL, 0)), "c = l (%s)" % where)
        _refused(lambda: make(((bp.VAR_COMMITTED, 1), 1, 0)), "a marked committed index >= m (%s)" % where)
    # a marker at the end of one row does not reach into the next
    _refused(lambda: bp.Circuit(2, 1, [[(v0, 1), mark(0)], [(v0, 1)]], lib=lib), "a marker across a row boundary")
    _refused(lambda: bp.Circuit(2, 1, [], wops=[(bp.W_LC, 0) + (bp.W_LC, 1)], lcs=[[(v0, 1), mark(0)], [(v0, 1)]], lib=lib), "a marker across a combination boundary")
    _refused(lambda: in_row(((bp.VAR_MUL_OUT, 2), 1, 0)), "a marked wire index >= n in a row")
    # a marked term of a combination reads earlier multipliers only
    for vk in (bp.VAR_MUL_LEFT, bp.VAR_MUL_RIGHT, bp.VAR_MUL_OUT):
        _refused(lambda: in_lc(((vk, 1), 1, 0)), "a marked term that reads its own multiplier")
        _refused(lambda: bp.Circuit(2, 1, [], wops=[(bp.W_LC, 1) + zero, zero + zero], lcs=[[], [((vk, 1), 1, 0)]], lib=lib), "a marked term that reads a later multiplier")
        _refused(lambda: in_lc(((vk, 1), 1, 0), op=(bp.W_LCNOTBIT, 1 << 8)), "a marked term under W_LCNOTBIT that reads its own multiplier")


# ------------------------------------------------------------------ the front-end
def _items(k, j):
    return [1 + S.synth_scalar(b"pc-item %d" % j, i) % (1 << 40) for i in range(k)]


def check_set_membership_lean(lib, glib, k, B=3):
    """B membership proofs about B DIFFERENT sets in one call of the device witness program on ONE compiled circuit, each equal to the
    proof the baked front-end path makes for its set (bpr1cs_gadget_prove_on, sp = the items) and accepted by the baked verifier; a
    proof checked against another proof's set is rejected"""
    gname, ip, lab = "set_membership_lean", [k], b"SetMembershipLean"
    sets = [_items(k, j) for j in range(B)]
    sps = [[sc_to_bytes(x) for x in s] for s in sets]
    circ = bp.CompiledGadget(gname, ip, [], lib=lib, glib=glib)
    base = bp.CompiledGadget(gname, ip, sps[0], lib=lib, glib=glib)
    assert circ.p == k and base.p == 0 and circ.has_witness_program
    assert (circ.n, circ.m) == (k, k + 1) == (base.n, base.m) and circ.q == base.q
    m = k + 1
    g = gens(lib, 128)
    pos = [(3 * j + 1) % k for j in range(B)]
    vals = b"".join(enc([1 if i == pos[j] else 0 for i in range(k)] + [sets[j][pos[j]]]) for j in range(B))
    bls = b"".join(enc([S.synth_scalar(b"pc-set-bl%d" % j, i) for i in range(m)]) for j in range(B))
    seeds = b"".join(seed(50 + j) for j in range(B))
    pubs = b"".join(b"".join(sp) for sp in sps)
    P, C = bp.prove_batch(g, circ, lab, vals, bls, seeds, B, wires=None, publics=pubs)
    for j in range(B):
        cut = lambda raw, sz: raw[j * sz:(j + 1) * sz]
        ref, refc, _ = bp.gadget_prove_on(g, gname, ip, sps[j], lab, cut(vals, 32 * m), cut(bls, 32 * m), m, 1, cut(seeds, 32), glib=glib)
        assert P[j] == ref[0], "set_membership_lean, k = %d: proof %d over public items differs from the baked front-end's" % (k, j)
        assert C[j] == refc[0]
        assert bp.gadget_verify_on(g, gname, ip, sps[j], lab, P[j], C[j], glib=glib)[0]
        assert not bp.gadget_verify_on(g, gname, ip, sps[(j + 1) % B], lab, P[j], C[j], glib=glib)[0]
    vs = b"".join(hashlib.sha256(b"pc-set-vseed %d" % j).digest() for j in range(B))
    assert bp.verify_batch(g, circ, lab, P, C, B, seeds=vs, publics=pubs) == [True] * B
    swapped = b"".join(b"".join(sps[j]) for j in ([1, 0] + list(range(2, B))))
    assert bp.verify_batch(g, circ, lab, P, C, B, seeds=vs, publics=swapped) == [False, False] + [True] * (B - 2)


def check_weighted_sum_bound(lib, glib, k, bits, B=3):
    """the same for sum w_i x_i <= budget with per-proof weights and budget: n = bits whatever k is"""
    gname, ip, lab = "weighted_sum_bound", [k, bits], b"WeightedSumBound"
    wbits = max(1, min(16, (bits - 8) // 2))
    ws = [[1 + S.synth_scalar(b"pc-w %d" % j, i) % (1 << wbits) for i in range(k)] for j in range(B)]
    xs = [[S.synth_scalar(b"pc-x %d" % j, i) % (1 << wbits) for i in range(k)] for j in range(B)]
    room = (1 << bits) - 1
    slack = [(0, room, room // 3)[j % 3] for j in range(B)]
    budget = [sum(w * x for w, x in zip(ws[j], xs[j])) + slack[j] for j in range(B)]
    sps = [[sc_to_bytes(w) for w in ws[j]] + [sc_to_bytes(budget[j])] for j in range(B)]
    circ = bp.CompiledGadget(gname, ip, [], lib=lib, glib=glib)
    base = bp.CompiledGadget(gname, ip, sps[0], lib=lib, glib=glib)
    assert circ.p == k + 1 and base.p == 0 and circ.has_witness_program
    assert (circ.n, circ.m) == (bits, k) == (base.n, base.m) and circ.q == base.q
    g = gens(lib, 128)
    vals = b"".join(enc(x) for x in xs)
    bls = b"".join(enc([S.synth_scalar(b"pc-wsb-bl%d" % j, i) for i in range(k)]) for j in range(B))
    seeds = b"".join(seed(70 + j) for j in range(B))
    pubs = b"".join(b"".join(sp) for sp in sps)
    P, C = bp.prove_batch(g, circ, lab, vals, bls, seeds, B, wires=None, publics=pubs)
    for j in range(B):
        cut = lambda raw, sz: raw[j * sz:(j + 1) * sz]
        ref, refc, _ = bp.gadget_prove_on(g, gname, ip, sps[j], lab, cut(vals, 32 * k), cut(bls, 32 * k), k, 1, cut(seeds, 32), glib=glib)
        assert P[j] == ref[0], "weighted_sum_bound (%d, %d): proof %d over public weights differs from the baked front-end's" % (k, bits, j)
        assert C[j] == refc[0]
        assert bp.gadget_verify_on(g, gname, ip, sps[j], lab, P[j], C[j], glib=glib)[0]
        assert not bp.gadget_verify_on(g, gname, ip, sps[(j + 1) % B], lab, P[j], C[j], glib=glib)[0]
    vs = b"".join(hashlib.sha256(b"pc-wsb-vseed %d" % j).digest() for j in range(B))
    assert bp.verify_batch(g, circ, lab, P, C, B, seeds=vs, publics=pubs) == [True] * B
    swapped = b"".join(b"".join(sps[j]) for j in ([1, 0] + list(range(2, B))))
    assert bp.verify_batch(g, circ, lab, P, C, B, seeds=vs, publics=swapped) == [False, False] + [True] * (B - 2)


SET_CASES = [1, 5, 70]
WSB_CASES = [(1, 8), (5, 64), (70, 16)]
