"""Grouped batch verification (BPR1CS_OPT_VERIFY_GROUP, include/bpr1cs.h): the case table and one checker, shared by
the CPU simulator (tests/test_verify_grouped.py) and the device (tests/test_gpu_verify_grouped.py).

The reference of every case is bp.verify_batch on a handle whose options are at their defaults - the per-proof path, whose parity
with the oracle is the subject of other tests.  With BPR1CS_OPT_VERIFY_GROUP_FALLBACK = 1 the grouped call must return that list; with 0
it returns group verdicts, and that run is the one that shows what the grouped kernels computed (a wrong combined scalar or point
sum makes a VALID group fail, which the fallback would repair silently).

Shapes: the smallest at which the new code can go wrong - a short last group, a lone proof as last group, G >= B (one group),
G = 2 (the smallest group), B <= 8 and B > 8 (the transcripts are replayed on the host / on the device), N = 1 (no inner-product
rounds), N = 4096 (two-level delta sum, several MSM chunks per group) and a group of 70 proofs (a lane of the combining wavefront
takes two)."""
import ctypes

from pyref import scenarios as S
import common
import frontend_cases as fc
import test_batched_verify as tb

bp = common.bp

# name -> (proofs, B, G); proofs: "bound" = tb.make_batch (n = 14, N = 16, m = 3; make_bound_batch below), otherwise a case of frontend_cases
CASES = {
    "b9_g4": ("bound", 9, 4),          # groups 4, 4, 1; device replay
    "b6_g4": ("bound", 6, 4),          # groups 4, 2; host replay
    "b9_g2": ("bound", 9, 2),          # 2, 2, 2, 2, 1
    "b9_g3": ("bound", 9, 3),          # 3, 3, 3: no short group
    "b9_g64": ("bound", 9, 64),        # G >= B: one group
    "factors_b5_g2": ("factors", 5, 2),      # N = 1, lg N = 0
    "vsmt_b3_g2": ("vsmt_4_l4", 3, 2),       # N = 4096 (device only: minutes on the simulator)
    "b141_g70": ("bound", 141, 70),    # groups 70, 70, 1: lanes 0..5 of the combining wavefront take two proofs
}
T_X = 1 + 8 * 32       # offset of the scalar t_x in a proof (tests/test_batched_verify.py tampers the same bytes)
T_XB = 1 + 9 * 32


def seed_sets(B):
    """three different sets of verifier seeds (the first proof's seed is the grouped path's batch seed)"""
    return [b"".join(S.synth_seed(1000 + j) for j in range(B)), bytes(32 * B), b"\x07" * (32 * B)]


def flip(proof, off, mask=1):
    b = bytearray(proof)
    b[off] ^= mask
    return bytes(b)


def group_verdicts(B, G, bad):
    """what BPR1CS_OPT_VERIFY_GROUP_FALLBACK = 0 must return: every proof of a group with a bad proof is rejected, all others accepted"""
    hit = {b // G for b in bad}
    return [b // G not in hit for b in range(B)]


def single_positions(B, G):
    """one tampered proof at a time: the last proof of group 0, the first proof of group 1, the last proof of the batch (the lone proof
    of a short last group where the shape has one)"""
    return sorted({min(G, B) - 1, B - 1} | ({G} if G < B else set()))


def make_bound_batch(lib, glib, batch):
    """tb.make_batch for any batch size: its statement (v = 37 + j in [10, 100]) holds for j < 64 only, so a larger batch is made
    here by the same recipe with the VALUES of proof j % 64 and blindings and seeds of its own - no two proofs are equal"""
    if batch <= 64:
        return tb.make_batch(lib, glib, batch)
    from pyref.ed import sc_to_bytes
    gens, circ, label, _, _ = tb.make_batch(lib, glib, 1)
    vals = b"".join(sc_to_bytes(x) for j in range(batch) for x in (37 + j % 64, 27 + j % 64, 63 - j % 64))
    bls = b"".join(sc_to_bytes(S.synth_scalar(b"bvb%d" % j, i)) for j in range(batch) for i in range(3))
    seeds = b"".join(S.synth_seed(j) for j in range(batch))
    P, C = bp.prove_batch(gens, circ, label, vals, bls, seeds, batch, wires=None)
    return gens, circ, label, P, C


class Env:
    """proofs of one kind made once per library, a default handle (the reference) and a handle created with verify_group"""

    def __init__(self, lib, glib):
        self.lib, self.glib, self._made = lib, glib, {}

    def batch(self, kind, B):
        """-> dict(ref=default handle, grp=handle created with verify_group, circ, label, P, C) with at least B proofs"""
        have = self._made.get(kind)
        if have is None or len(have["P"]) < B:
            if kind == "bound":
                ref, circ, label, P, C = make_bound_batch(self.lib, self.glib, B)
                grp = bp.Gens(16, lib=self.lib, unfold=2, verify_group=4)
            else:
                cache = {}
                ob, P, C = fc.check_compiled(self.lib, self.glib, kind, batch=B, gens_cache=cache)
                gname, ip, sp, _, cap = fc.case(kind, 0)
                circ, label = bp.CompiledGadget(gname, ip, sp, lib=self.lib, glib=self.glib), ob["label"]
                ref = cache[(id(self.lib), cap)]        # window_bits = 8, every other option back at its default
                grp = bp.Gens(cap, lib=self.lib, window_bits=8, verify_group=2)
            have = self._made[kind] = dict(ref=ref, grp=grp, circ=circ, label=label, P=list(P), C=list(C))
        return have

    def reference(self, kind, P, C, seeds):
        e = self.batch(kind, len(P))
        return bp.verify_batch(e["ref"], e["circ"], e["label"], P, C, len(P), seeds)

    def grouped(self, kind, P, C, G, fallback, seeds):
        e = self.batch(kind, len(P))
        e["grp"].set_option("verify_group", G)
        e["grp"].set_option("verify_group_fallback", fallback)
        try:
            return bp.verify_batch(e["grp"], e["circ"], e["label"], P, C, len(P), seeds)
        finally:
            e["grp"].set_option("verify_group", -1)
            e["grp"].set_option("verify_group_fallback", -1)


_ENVS = {}


def env(lib, glib):
    if id(lib) not in _ENVS:
        _ENVS[id(lib)] = Env(lib, glib)
    return _ENVS[id(lib)]


def check(e, name, P, C, bad, seeds=None, reference=True):
    """both fallback settings on the proofs P / commitments C of case `name`, of which the proofs `bad` are wrong"""
    kind, B, G = CASES[name]
    assert len(P) == B
    seeds = seeds if seeds is not None else seed_sets(B)[0]
    want = [b not in bad for b in range(B)]
    if reference:
        assert e.reference(kind, P, C, seeds) == want, "the per-proof path itself"
    got1 = e.grouped(kind, P, C, G, 1, seeds)
    got0 = e.grouped(kind, P, C, G, 0, seeds)
    assert got1 == want, "%s fallback 1: %r" % (name, got1)
    assert got0 == group_verdicts(B, G, bad), "%s fallback 0: %r" % (name, got0)


def check_valid(e, name):
    kind, B, G = CASES[name]
    b = e.batch(kind, B)
    check(e, name, b["P"][:B], b["C"][:B], set())


def check_single_tamper(e, name):
    kind, B, G = CASES[name]
    b = e.batch(kind, B)
    for pos in single_positions(B, G):
        P = b["P"][:B]
        P[pos] = flip(P[pos], T_X + 3)
        check(e, name, P, b["C"][:B], {pos})


def check_two_tampered(e, name, pairs):
    kind, B, G = CASES[name]
    b = e.batch(kind, B)
    for x, y in pairs:
        P = b["P"][:B]
        P[x] = flip(P[x], T_X + 3)
        P[y] = flip(P[y], T_XB + 5, 4)
        for i, seeds in enumerate(seed_sets(B)):
            check(e, name, P, b["C"][:B], {x, y}, seeds=seeds, reference=i == 0)


def malformed_forms(p):
    """proof p with a first point that does not decode (found by K_verify_points, after the transcript stage), with a non-canonical t_x
    and with version byte 1 (both found by the transcript stage)"""
    return [p[:1] + b"\xff" * 32 + p[33:], p[:T_X] + b"\xff" * 32 + p[T_X + 32:], b"\x01" + p[1:]]


def check_malformed_at(e, name, pos, forms=(0, 1, 2), reference=True):
    """proof `pos` malformed among good proofs, in the given forms of malformed_forms: the range sums of modes 0 and 1 leave a
    malformed proof out, so its group must fail by the proof's flag (mode 0 rejects the whole group, mode 1 the proof alone)"""
    kind, B, G = CASES[name]
    b = e.batch(kind, B)
    P = b["P"][:B]
    for f in forms:
        check(e, name, P[:pos] + [malformed_forms(P[pos])[f]] + P[pos + 1:], b["C"][:B], {pos}, reference=reference)


def check_malformed(e, name):
    """in proof 0: a first point that does not decode, a non-canonical t_x, version byte 1; then a commitment swapped between two
    groups (both fail)"""
    kind, B, G = CASES[name]
    b = e.batch(kind, B)
    check_malformed_at(e, name, 0)
    C = [list(c) for c in b["C"][:B]]
    C[0][0], C[G][0] = C[G][0], C[0][0]
    check(e, name, b["P"][:B], C, {0, G})


def verify_null_seeds(e, name, fallback):
    """the C call with verifier_rng_seeds = NULL (the Python wrapper always passes seeds): the batch seed is 32 zero bytes"""
    kind, B, G = CASES[name]
    b = e.batch(kind, B)
    g = b["grp"]
    g.set_option("verify_group", G)
    g.set_option("verify_group_fallback", fallback)
    try:
        ok = (ctypes.c_int * B)()
        rc = e.lib.bpr1cs_verify_batch(g.h, b["circ"].h, b["label"], len(b["label"]), b"".join(b["P"][:B]),
                                       b"".join(b"".join(c) for c in b["C"][:B]), None, B, ok)
        assert rc == 0
        return [bool(x) for x in ok]
    finally:
        g.set_option("verify_group", -1)
        g.set_option("verify_group_fallback", -1)
