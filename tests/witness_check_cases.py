"""The witness check of the prove calls (BPR1CS_OPT_CHECK_WITNESS, include/bpr1cs.h): circuits, tampering, the expected
refusal records and one driver, shared by the CPU simulator (tests/test_witness_check.py) and the device (tests/test_gpu_witness_check.py).

Expectations never come from the library.  What a slot of `proofs_out` must hold is decided by `violations` below - the gates and the
rows of the oracle's own constraint list (ob["constraints"]) evaluated over big integers mod l on the wires and values that are
actually SUBMITTED: no violation -> the oracle's proof bytes, else the refusal record `record` builds from the header's layout.

Inputs: common.oracle_batch with host wires.  At most 4 witnesses are proved by the oracle; values, blindings, seeds and wires are
tiled to the batch size, so an untampered proof j must equal the oracle's proof j mod 4.  Tampering edits the submitted wires or
values only.  The circuits:
  * "rc3" / "rc2" / "rc1": tests/random_circuits.scenario (n = 13 with m = 3, n = 1 with m = 0, n = 5) - satisfied witnesses;
  * "rc4" / "rc6": its witnesses that VIOLATE their circuit (constant-only rows among them), which the oracle proves all the same: the
    bytes a call with the option off must still produce;
  * "probe" / "probe_long": a circuit made here through the oracle's Prover / Verifier API, because a random circuit gives no handle
    for violating exactly one chosen row: "free" multipliers (x, 0) whose left wire can take any value without breaking the gate, each
    appearing in exactly one row.  Row kinds: a general coefficient, +-1 only, empty, the constant alone; n is not a power of two.
    "probe_long" adds rows of many terms so that the row form has >= 3 chunks of CHECK_CHUNK entries and one row longer than that.
The device witness program is exercised through frontend_cases.case ("is_zero_violated", "poseidon_hash_2" with a wrong claimed image)."""
import os
import re

from pyref import scenarios as S
from pyref.ed import L, sc_to_bytes
from pyref.r1cs import LinearCombination, One
import common
import frontend_cases as fc
import random_circuits as rc

bp = common.bp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_CHUNK = int(re.search(r"#define CHECK_CHUNK (\d+)u", open(os.path.join(ROOT, "bulletproofs-r1cs-gadgets_amd", "csrc", "kernels.hpp")).read()).group(1))
K = 4   # witnesses the oracle proves per circuit
COMMITTED, LEFT, RIGHT, OUT, ONE = 0, 1, 2, 3, 4
NONE = 0xFFFFFFFF


# ------------------------------------------------------------------ the probe circuit
FILL = 100   # terms of a filler row of "probe_long"


def probe_layout(long):
    """-> (rows, n_free): rows = list of (kind, free multiplier or None) in constraint order, without the two rows of the final multiply
    and the last row (appended by the builder)"""
    rows = [("free_general", 0), ("empty", None), ("const_zero", None), ("pm_one", 1), ("general", 2)]
    nf = 5                      # free multipliers 0..2 above, 3 = the last row's, 4 = the second wire of "pm_one"
    if long:
        rows += [("fill", nf + i) for i in range(4)] + [("long", nf + 4)]
        nf += 5
    return rows, nf


def _free_value(i):
    return S.synth_scalar(b"wc-free", i)


def probe(j, long=False, const=0):
    """Multipliers 0..nf-1 are free: (f_i, 0) -> a_O = 0 whatever a_L is.  f_2 = v0 (the only per-proof free value: the rows hold
    no constant that depends on the witness, so every proof has the same circuit).  Then multiply(v0, v1): gate n - 1 and two rows."""
    rows, nf = probe_layout(long)
    v0, v1 = S.synth_scalar(b"wc-v0", j), S.synth_scalar(b"wc-v1", j) or 1
    f = [_free_value(i) for i in range(nf)]
    f[4] = f[1]      # row "pm_one": two wires of equal value, coefficients +1 and -1 only
    f[2] = v0

    def build(cs, cv, prover):
        fl = [cs.allocate_multiplier((f[i], 0) if prover else None)[0] for i in range(nf)]
        for kind, i in rows:
            if kind == "free_general":
                cs.constrain(fl[i] - f[i])                      # +1 and a general constant
            elif kind == "empty":
                cs.constrain(LinearCombination())
            elif kind == "const_zero":
                cs.constrain(One() * const)                     # the constant alone (coefficient 0: it holds)
            elif kind == "pm_one":
                cs.constrain(fl[i] - fl[4])                     # +1 / -1 only
            elif kind == "general":
                cs.constrain(fl[i] * 7 - cv[0] * 7)             # general coefficients, a committed value
            else:
                terms = FILL if kind == "fill" else CHECK_CHUNK + 44
                e = fl[i] - f[i]
                for t in range((terms - 2) // 2):               # pairs that cancel: +-1 for even t, general for odd t
                    c = 1 if t % 2 == 0 else S.synth_scalar(b"wc-c", t)
                    e = e + cv[0] * c - cv[0] * c
                cs.constrain(e)
        cs.multiply(cv[0] + 0, cv[1] * 1)                       # rows: (v0 + 0 * One - l), (v1 - r)
        cs.constrain(fl[3] - f[3])                              # the last row

    def bpv(pr, bl):
        c0, x0 = pr.commit(v0, bl[0])
        c1, x1 = pr.commit(v1, bl[1])
        build(pr, [x0, x1], True)
        return [c0, c1]

    def bv(vr, comms, pc):
        build(vr, [vr.commit(c) for c in comms], False)
    return S.Scenario(b"WitnessCheckProbe", [v0, v1], bpv, bv)


def probe_row(long, kind, which=0):
    """index of the `which`-th row of `kind` in the probe circuit ("mul_left" / "mul_right" / "last": the rows the builder appends)"""
    rows, _ = probe_layout(long)
    if kind in ("mul_left", "mul_right", "last"):
        return len(rows) + ("mul_left", "mul_right", "last").index(kind)
    return [r for r, (k, _) in enumerate(rows) if k == kind][which]


def probe_handle(long, row):
    """a free multiplier whose left wire appears in `row` and nowhere else"""
    rows, _ = probe_layout(long)
    if row == len(rows) + 2:
        return 3
    return rows[row][1]


# ------------------------------------------------------------------ circuits and their oracle batches
def _rc(seed, n_mul, m, rows, cap, sat):
    return dict(fn=lambda j: rc.scenario(seed * 100, n_mul, m, rows, sat), cap=cap, sat=sat)


CIRCUITS = {
    "rc3": _rc(3, 13, 3, 9, 16, True),
    "rc2": _rc(2, 1, 0, 0, 1, True),       # m = 0 (and q = 0 when its one multiplier is an allocate_multiplier)
    "rc1": _rc(1, 5, 2, 4, 8, True),
    "rc4": _rc(4, 7, 1, 6, 8, False),
    "rc6": _rc(6, 3, 5, 11, 4, False),
    "probe": dict(fn=lambda j: probe(j, False), cap=8, sat=True),
    "probe_const": dict(fn=lambda j: probe(j, False, 5), cap=8, sat=False),   # its constant-only row says 5 = 0
    "probe_long": dict(fn=lambda j: probe(j, True), cap=16, sat=True),
}


def oracle(name):
    c = CIRCUITS[name]
    return common.oracle_batch(c["fn"], c["cap"], K, satisfiable=c["sat"], key=("witness_check", name))


# ------------------------------------------------------------------ the checker (big integers, the submitted bytes)
def _scalars(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def violations(ob, wires, values):
    """one proof's submitted wires (a_L | a_R | a_O, 3n x 32 bytes) and values (m x 32 bytes) against the oracle's constraint list
    -> None, or dict(gate, row, gates, rows) as bp.refusal reports it"""
    n = ob["n"]
    w, v = _scalars(wires), _scalars(values)
    aL, aR, aO = w[:n], w[n:2 * n], w[2 * n:]
    bad_g = [i for i in range(n) if (aL[i] * aR[i] - aO[i]) % L]
    bad_r = []
    for j, row in enumerate(ob["constraints"]):
        acc = 0
        for (kind, idx), c in row:
            acc += c * (v[idx] if kind == COMMITTED else aL[idx] if kind == LEFT else aR[idx] if kind == RIGHT else aO[idx] if kind == OUT else 1)
        if acc % L:
            bad_r.append(j)
    if not bad_g and not bad_r:
        return None
    return dict(gate=bad_g[0] if bad_g else None, row=bad_r[0] if bad_r else None, gates=len(bad_g), rows=len(bad_r))


def record(plen, viol):
    """the refusal record of include/bpr1cs.h, from the layout stated there"""
    le = lambda x: (NONE if x is None else x).to_bytes(4, "little")
    return b"\xff\0\0\0" + le(viol["gate"]) + le(viol["row"]) + le(viol["gates"]) + le(viol["rows"]) + bytes(plen - 20)


def chunks(ob):
    """mirror of the chunk list bpr1cs_circuit_create builds: consecutive whole rows, closed when their entries reach CHECK_CHUNK; a
    row of CHECK_CHUNK entries or more is a chunk of its own -> list of (first row, end row)"""
    out, start, cnt = [], 0, 0
    for j, row in enumerate(ob["constraints"]):
        if len(row) >= CHECK_CHUNK and j > start:
            out.append((start, j)); start, cnt = j, 0
        cnt += len(row)
        if cnt >= CHECK_CHUNK:
            out.append((start, j + 1)); start, cnt = j + 1, 0
    if start < len(ob["constraints"]):
        out.append((start, len(ob["constraints"])))
    return out


# ------------------------------------------------------------------ tampering
def _add1(raw, pos):
    x = (int.from_bytes(raw[32 * pos:32 * pos + 32], "little") + 1) % L
    raw[32 * pos:32 * pos + 32] = sc_to_bytes(x)


def tiled(ob, B, tampers=None):
    """-> (values, blindings, seeds, wires) of B proofs, proof j = the oracle's witness j mod K; tampers: {proof: [op, ...]} with
    op = ("wire", side 0 / 1 / 2 = a_L / a_R / a_O, multiplier) or ("value", k): that scalar + 1"""
    n, m = ob["n"], ob["m"]
    per = lambda raw, sz, j: raw[(j % K) * sz:(j % K + 1) * sz]
    vals = bytearray(b"".join(per(ob["values"], 32 * m, j) for j in range(B)))
    bls = b"".join(per(ob["blindings"], 32 * m, j) for j in range(B))
    seeds = b"".join(per(ob["seeds"], 32, j) for j in range(B))
    wires = bytearray(b"".join(per(ob["wires"], 96 * n, j) for j in range(B)))
    for j, ops in (tampers or {}).items():
        for op in ops:
            if op[0] == "wire":
                _add1(wires, 3 * n * j + op[1] * n + op[2])
            else:
                _add1(vals, m * j + op[1])
    return bytes(vals), bls, seeds, bytes(wires)


# ------------------------------------------------------------------ the driver
_CTX = {}


def ctx(lib, name, **gens_opts):
    """one generator handle (window_bits = 8) and one circuit per (library, circuit, creation options)"""
    key = (id(lib), name, tuple(sorted(gens_opts.items())))
    if key not in _CTX:
        ob = oracle(name)
        _CTX[key] = (bp.Gens(CIRCUITS[name]["cap"], lib=lib, window_bits=8, **gens_opts), common.circuit_from_oracle(ob, lib), ob)
    return _CTX[key]


def prove(lib, g, circ, ob, inp, B, entry):
    """the prove entry points over one batch -> (proofs, commitments or None, refused as bpr1cs_prove_stats reports it)"""
    vals, bls, seeds, wires = inp
    m, n = ob["m"], ob["n"]
    if entry == "batch":
        P, C = bp.prove_batch(g, circ, ob["label"], vals, bls, seeds, B, wires=wires)
        return P, C, bp.last_prove_stats(lib)["refused"]
    if entry == "transcripts":
        ts = [bp.Transcript(ob["label"], lib=lib) for _ in range(B)]
        P, C = bp.prove_batch_transcripts(g, circ, ts, vals, bls, seeds, B, wires=wires)
        return P, C, bp.last_prove_stats(lib)["refused"]
    if entry == "draws":
        return prove_draws(lib, g, circ, ob, inp, B), None, bp.last_prove_stats(lib)["refused"]
    assert entry == "begin_end"     # two jobs in flight, ended in order
    h = B // 2
    cut = lambda raw, sz, lo, hi: raw[lo * sz:hi * sz]
    jobs = [bp.ProveJob(g, circ, ob["label"], cut(vals, 32 * m, lo, hi), cut(bls, 32 * m, lo, hi), cut(seeds, 32, lo, hi), hi - lo,
                        wires=cut(wires, 96 * n, lo, hi)) for lo, hi in ((0, h), (h, B))]
    P, C, refused = [], [], 0
    for job in jobs:
        p, c = job.finish()
        P += p; C += c
        refused += bp.last_prove_stats(lib)["refused"]
    return P, C, refused


def prove_draws(lib, g, circ, ob, inp, B):
    """bpr1cs_prove_batch_draws as its caller uses it: per proof a transcript that holds Prover::new's and commit's messages and "m",
    and the 2n + 8 raw 64-byte draws of the proof's TranscriptRng - both made here with the oracle's Merlin (wires may be tampered,
    values may not: the commitments in the transcripts are the oracle's)"""
    import ctypes
    from pyref.merlin import Transcript as OracleTranscript
    vals, bls, seeds, wires = inp
    n, m = ob["n"], ob["m"]
    ts, draws = [], b""
    for j in range(B):
        V = ob["comms"][j % K]
        assert len(V) == m and vals[32 * m * j:32 * m * (j + 1)] == ob["values"][32 * m * (j % K):32 * m * (j % K + 1)]
        ot, t = OracleTranscript(ob["label"]), bp.Transcript(ob["label"], lib=lib)
        ot.append_message(b"dom-sep", b"r1cs v1"); t.append_message(b"dom-sep", b"r1cs v1")
        for c in V:
            ot.append_point(b"V", c); t.append_message(b"V", c)
        ot.append_u64(b"m", m); t.append_message(b"m", m.to_bytes(8, "little"))
        b = ot.build_rng()
        for k in range(m):
            b = b.rekey_with_witness_bytes(b"v_blinding", bls[32 * (m * j + k):32 * (m * j + k + 1)])
        rng = b.finalize(seeds[32 * j:32 * j + 32])
        draws += b"".join(rng.fill_bytes(64) for _ in range(2 * n + 8))
        ts.append(t)
    vp, cp = ctypes.c_void_p, ctypes.c_char_p
    lib.bpr1cs_prove_batch_draws.argtypes = [vp, vp, ctypes.POINTER(vp), cp, cp, cp, cp, ctypes.c_size_t, cp]
    out = ctypes.create_string_buffer(B * circ.proof_len)
    arr = (vp * B)(*[t.h for t in ts])
    rc = lib.bpr1cs_prove_batch_draws(g.h, circ.h, arr, vals or b"\0", bls or b"\0", draws, wires, B, out)
    assert rc == 0, rc
    raw = out.raw
    return [raw[i * circ.proof_len:(i + 1) * circ.proof_len] for i in range(B)]


def check(lib, name, B, tampers=None, entry="batch", on=True, opts=None, gens_opts=None, verify=False):
    """prove B tiled witnesses of circuit `name` with the check on (or off) and compare EVERY slot with what the checker expects;
    -> (the expected violations per proof, proofs, commitments, handle, circuit)"""
    g, circ, ob = ctx(lib, name, **(gens_opts or {}))
    inp = tiled(ob, B, tampers)
    n, m = ob["n"], ob["m"]
    want = [violations(ob, inp[3][96 * n * j:96 * n * (j + 1)], inp[0][32 * m * j:32 * m * (j + 1)]) for j in range(B)]
    opts = dict(opts or {}, check_witness=1 if on else 0)
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        P, C, refused = prove(lib, g, circ, ob, inp, B, entry)
    finally:
        for k in opts:
            g.set_option(k, -1)
    untouched_values = lambda j: not any(op[0] == "value" for op in (tampers or {}).get(j, []))
    for j in range(B):
        if want[j] is None or not on:
            if j not in (tampers or {}):
                assert P[j] == ob["proofs"][j % K], "%s: proof %d of %d differs from the oracle's" % (name, j, B)
            assert bp.refusal(P[j]) is None
        else:
            assert P[j] == record(circ.proof_len, want[j]), "%s: slot %d of %d: %r, expected %r" % (name, j, B, bp.refusal(P[j]), want[j])
            assert bp.refusal(P[j]) == want[j]
        if C is not None and untouched_values(j):
            oc = ob["comms"][j % K]
            assert C[j][:len(oc)] == oc, "%s: commitments of proof %d" % (name, j)
    assert refused == (sum(w is not None for w in want) if on else 0), (refused, want)
    if verify:
        ok = bp.verify_batch(g, circ, ob["label"], P, C, B)
        assert ok == [w is None for w in want], ok
    return want, P, C, g, circ


# ------------------------------------------------------------------ the case table (every entry: callable(lib, glib))
GEOMETRY = {1: [0], 63: [0, 62], 64: [0, 63], 65: [0, 63, 64], 130: [0, 63, 64, 129]}   # B -> bad proofs (0 and 63: one wavefront)


def t_all_good(B):
    def run(lib, glib):
        want, _, _, _, _ = check(lib, "rc3", B)
        assert want == [None] * B
    return run


def t_geometry(B):
    def run(lib, glib):
        n = oracle("rc3")["n"]
        ops = [[("wire", 2, 0)], [("wire", 2, n - 1)], [("wire", 0, 3), ("wire", 2, 5)], [("value", 1)]]
        bad = GEOMETRY[B]
        want, _, _, _, _ = check(lib, "rc3", B, {b: ops[i % 4] for i, b in enumerate(bad)})
        assert [j for j in range(B) if want[j] is not None] == bad
    return run


def t_kinds(lib, glib):
    """one batch of the probe circuit, one kind of violation per proof; the checker's own verdicts are asserted first (the table reaches
    every situation), then every slot"""
    ob = oracle("probe")
    n, q = ob["n"], ob["q"]
    assert n & (n - 1) and q == 8 and [len(r) for r in ob["constraints"]][1] == 0
    row = lambda kind: probe_row(False, kind)
    hand = lambda kind: probe_handle(False, row(kind))
    assert row("free_general") == 0 and row("last") == q - 1
    tampers = {
        0: [("wire", 2, 0)],                       # gate 0 only
        1: [("wire", 2, n - 1)],                   # gate n - 1 only
        2: [("wire", 0, hand("free_general"))],    # the first row only
        3: [("wire", 0, hand("last"))],            # the last row only
        4: [("wire", 0, n - 1)],                   # a gate and a row (the multiply's left wire)
        5: [("value", 0)],                         # a committed value, wires untouched: the rows through slot 3n + 0 (two of them)
        6: [("value", 1)],                         # ... through slot 3n + 1 (one)
        7: [("wire", 0, hand("pm_one"))],          # a row of +-1 coefficients
        8: [("wire", 0, hand("general"))],         # a row of general coefficients
        9: [("wire", 2, 1), ("wire", 2, 3), ("wire", 0, hand("pm_one")), ("wire", 0, hand("last"))],   # counts and minima of both kinds
    }
    B = 12                                         # proofs 10, 11: good
    want, _, _, _, _ = check(lib, "probe", B, tampers)
    V = lambda gate, r, gates, rows: dict(gate=gate, row=r, gates=gates, rows=rows)
    assert want[0] == V(0, None, 1, 0) and want[1] == V(n - 1, None, 1, 0)
    assert want[2] == V(None, 0, 0, 1) and want[3] == V(None, q - 1, 0, 1)
    assert want[4] == V(n - 1, row("mul_left"), 1, 1)
    assert want[5] == V(None, row("general"), 0, 2) and want[6] == V(None, row("mul_right"), 0, 1)
    assert want[7] == V(None, row("pm_one"), 0, 1) and want[8] == V(None, row("general"), 0, 1)
    assert want[9] == V(1, row("pm_one"), 2, 2) and want[10] is None and want[11] is None
    coeffs = lambda kind: {c for _, c in ob["constraints"][row(kind)]}
    assert coeffs("pm_one") == {1, L - 1} and coeffs("general") == {7, L - 7}
    assert [k for (k, _), _ in ob["constraints"][row("const_zero")]] == [ONE]


def t_constant_row(lib, glib):
    """a circuit whose constant-only row does not hold (5 = 0): every witness violates exactly that row; the oracle proves them all
    the same, and those are the bytes of the call with the option off"""
    ob = oracle("probe_const")
    r = probe_row(False, "const_zero")
    assert [(k, c) for (k, _), c in ob["constraints"][r]] == [(ONE, 5)]
    check(lib, "probe_const", 3, on=False)
    want, _, _, _, _ = check(lib, "probe_const", 3)
    assert want == [dict(gate=None, row=r, gates=0, rows=1)] * 3


def t_no_values_no_rows(lib, glib):
    """m = 0 and q = 0: one multiplier, nothing else"""
    ob = oracle("rc2")
    assert (ob["n"], ob["m"], ob["q"]) == (1, 0, 0)
    want, _, _, _, _ = check(lib, "rc2", 3, {1: [("wire", 2, 0)]})
    assert want == [None, dict(gate=0, row=None, gates=1, rows=0), None]


def t_chunking(lib, glib):
    ob = oracle("probe_long")
    ch, lens = chunks(ob), [len(r) for r in ob["constraints"]]
    longs = [j for j, x in enumerate(lens) if x > CHECK_CHUNK]
    assert len(ch) >= 3 and len(longs) == 1
    (lo0, hi0), (lo1, hi1) = ch[0], ch[1]
    assert hi0 - lo0 > 1 and sum(lens[lo0:hi0]) >= CHECK_CHUNK and all(x < CHECK_CHUNK for x in lens[lo0:hi0])   # closed by the count
    assert (longs[0], longs[0] + 1) in ch and ch[-1][1] == ob["q"] and ch[-1][1] - ch[-1][0] > 1                    # the long row alone; a tail
    wire = lambda r: ("wire", 0, probe_handle(True, r))
    tampers = {0: [wire(hi0 - 1)], 1: [wire(lo1)], 2: [wire(longs[0])], 4: [wire(hi0 - 1), wire(lo1), wire(longs[0]), wire(ob["q"] - 1)]}
    want, _, _, _, _ = check(lib, "probe_long", 6, tampers)
    one = lambda r: dict(gate=None, row=r, gates=0, rows=1)
    assert want == [one(hi0 - 1), one(lo1), one(longs[0]), None, dict(gate=None, row=hi0 - 1, gates=0, rows=4), None]


def t_entry(entry):
    def run(lib, glib):
        want, _, _, _, _ = check(lib, "rc1", 6, {1: [("wire", 2, 2)], 3: [("value", 0)], 5: [("wire", 1, 0)]}, entry=entry)
        assert [w is not None for w in want] == [False, True, False, True, False, True]
    return run


def t_three_jobs(lib, glib):
    """a call cut into jobs of 64, 64 and 2 proofs: a bad proof in the second and in the last job"""
    want, _, _, _, _ = check(lib, "rc1", 130, {70: [("wire", 2, 1)], 129: [("value", 1)]}, opts=dict(job_proofs=64))
    assert [j for j in range(130) if want[j] is not None] == [70, 129]


def t_draws(lib, glib):
    """bpr1cs_prove_batch_draws (transcripts and draws made by the caller): the untampered proofs are the oracle's, the others refused"""
    want, _, _, _, _ = check(lib, "rc1", 5, {0: [("wire", 2, 4)], 3: [("wire", 0, 2), ("wire", 1, 1)]}, entry="draws")
    assert [w is not None for w in want] == [True, False, False, True, False]


def t_prover_class(lib, glib):
    """the C++ Prover (bpr1cs_gadget_prove_on, one proof per call) inherits the option through the handle: the record comes back from
    the device call and R1CSProof::from_bytes reports it as a format error - its version check is what refuses it"""
    gname, ip, sp, _, cap = fc.case("is_zero_violated", 0)
    ob = common.oracle_batch(lambda j: fc.case("is_zero_violated", j)[3], cap, 1, satisfiable=False, key="is_zero_violated")
    m = ob["m"]
    g = bp.Gens(cap, lib=lib, window_bits=8)
    P, _, _ = bp.gadget_prove_on(g, gname, ip, sp, ob["label"], ob["values"], ob["blindings"], m, 1, ob["seeds"], glib=glib)
    assert P == ob["proofs"] and bp.last_prove_stats(lib)["refused"] == 0
    g.set_option("check_witness", 1)
    try:
        bp.gadget_prove_on(g, gname, ip, sp, ob["label"], ob["values"], ob["blindings"], m, 1, ob["seeds"], glib=glib)
        assert False, "a refusal record parsed as a proof"
    except bp.R1CSError as e:
        assert e.code == -2
    assert bp.last_prove_stats(lib)["refused"] == 1
    g.close()


def _program_batch(lib, glib, name, circuit_of, pick, sat):
    """the device witness program: a batch whose proof j takes the inputs of the oracle's witness `pick[j]` = (batch name, index);
    circuit and constraint list: those of `circuit_of`.  The wires the checker sees are the oracle's (the program synthesises the same
    ones: tests/test_frontend.py)."""
    gname, ip, sp, _, cap = fc.case(circuit_of, 0)
    obs = {nm: common.oracle_batch(lambda j, nm=nm: fc.case(nm, j)[3], cap, k, satisfiable=sat[nm], key=nm) for nm, k in name.items()}
    ref = common.oracle_batch(lambda j: fc.case(circuit_of, 0)[3], cap, 1, satisfiable=sat[circuit_of], key=circuit_of) if name[circuit_of] != 1 else obs[circuit_of]
    n, m = ref["n"], ref["m"]
    circ = bp.CompiledGadget(gname, ip, sp, lib=lib, glib=glib)
    assert circ.has_witness_program and (circ.n, circ.m, circ.q) == (n, m, ref["q"])
    # (the handle fc.check_compiled keeps per library and capacity: the simulator builds the tables of 256 generators for half a minute)
    cache = fc.check_compiled.__defaults__[-1]
    if (id(lib), cap) not in cache:
        cache[(id(lib), cap)] = bp.Gens(cap, lib=lib, window_bits=8)
    g = cache[(id(lib), cap)]
    cut = lambda raw, sz, j: raw[j * sz:(j + 1) * sz]
    vals = b"".join(cut(obs[nm]["values"], 32 * m, j) for nm, j in pick)
    bls = b"".join(cut(obs[nm]["blindings"], 32 * m, j) for nm, j in pick)
    seeds = b"".join(cut(obs[nm]["seeds"], 32, j) for nm, j in pick)
    want = [violations(ref, cut(obs[nm]["wires"], 96 * n, j), cut(obs[nm]["values"], 32 * m, j)) for nm, j in pick]
    g.set_option("check_witness", 1)
    try:
        P, C = bp.prove_batch(g, circ, ref["label"], vals, bls, seeds, len(pick), wires=None)
    finally:
        g.set_option("check_witness", -1)
    for i, (nm, j) in enumerate(pick):
        assert P[i] == (obs[nm]["proofs"][j] if want[i] is None else record(circ.proof_len, want[i])), (i, bp.refusal(P[i]), want[i])
        assert C[i][:len(obs[nm]["comms"][j])] == obs[nm]["comms"][j]
    assert bp.last_prove_stats(lib)["refused"] == sum(w is not None for w in want)
    return want


def t_program_is_zero(lib, glib):
    pick = [("is_zero", 0), ("is_zero_violated", 1), ("is_zero", 2), ("is_zero_violated", 0), ("is_zero", 1)]
    want = _program_batch(lib, glib, {"is_zero": 3, "is_zero_violated": 2}, "is_zero", pick, {"is_zero": True, "is_zero_violated": False})
    assert [w is None for w in want] == [True, False, True, False, True]
    assert all(w["gates"] == 0 and w["rows"] >= 1 for w in want if w)    # the gates hold by construction: a row fails


def t_program_poseidon(lib, glib):
    """poseidon_hash_2 (Inverse S-box, jointly evaluated permutation) compiled for the image of witness 0: the witnesses 1 and 2 hash
    to other images - every gate holds, the row that pins the image fails"""
    name = "poseidon_hash_2_inverse_pr1"
    assert os.environ.get("BPR1CS_WITNESS_MACRO") is None
    want = _program_batch(lib, glib, {name: 3}, name, [(name, 1), (name, 0), (name, 2)], {name: True})
    assert want[1] is None and all(w and w["gates"] == 0 and w["rows"] >= 1 for w in (want[0], want[2]))


def t_secret_independent(lib, glib):
    want, _, _, _, _ = check(lib, "rc1", 5, {0: [("wire", 2, 4)], 3: [("value", 1)]}, gens_opts=dict(secret_independent=1))
    assert [w is not None for w in want] == [True, False, False, True, False]


def t_verifiers(lib, glib):
    """the outputs go to bpr1cs_verify_batch: verdict 0 exactly at the refused slots, on the per-proof path and on the grouped one"""
    B, bad = 9, {0: [("wire", 2, 3)], 5: [("wire", 0, 1)], 8: [("wire", 2, 0), ("wire", 2, 1)]}
    want, P, C, g, circ = check(lib, "rc3", B, bad, verify=True)
    ob = oracle("rc3")
    for fb in (1, 2):
        g.set_option("verify_group", 4)
        g.set_option("verify_group_fallback", fb)
        try:
            assert bp.verify_batch(g, circ, ob["label"], P, C, B) == [w is None for w in want], fb
        finally:
            g.set_option("verify_group", -1)
            g.set_option("verify_group_fallback", -1)


def t_option_off(lib, glib):
    """the option off: violated inputs give the oracle's bytes, as they always have; on: the same inputs are refused"""
    for name in ("rc4", "rc6"):
        check(lib, name, 5, on=False)
        want, _, _, _, _ = check(lib, name, 5, verify=True)
        assert all(w is not None and w["gates"] == 0 and w["rows"] > 1 for w in want)
    check(lib, "probe", 4, {1: [("wire", 2, 0)], 2: [("value", 0)]}, on=False)


TABLE = {"all_good_1": t_all_good(1), "all_good_64": t_all_good(64), "all_good_130": t_all_good(130)}
TABLE.update({"geometry_%d" % B: t_geometry(B) for B in GEOMETRY})
TABLE.update(kinds=t_kinds, constant_row=t_constant_row, no_values_no_rows=t_no_values_no_rows, chunking=t_chunking,
             transcripts=t_entry("transcripts"), begin_end=t_entry("begin_end"), three_jobs=t_three_jobs, draws=t_draws, prover_class=t_prover_class,
             program_is_zero=t_program_is_zero, program_poseidon=t_program_poseidon, secret_independent=t_secret_independent,
             verifiers=t_verifiers, option_off=t_option_off)
