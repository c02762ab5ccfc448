#!/usr/bin/env python3
"""What public coefficients are worth for a set membership: one job of one-of-64 membership proofs in two forms,
alternating on one handle of one process - "set_membership" with the items baked (a multiplier pair per item, n = 192, one set for the
whole job) and "set_membership_lean" compiled without items (n = 64: the items are public coefficients of the bit wires, a DIFFERENT set
per proof).  Each form is proved (one bpr1cs_prove_batch call, device witness program), then verified by bpr1cs_verify_batch per proof
and grouped (BPR1CS_OPT_VERIFY_GROUP); every proof is checked by the library's verifier in every timed verify call.  The timed region
is the C call alone.  One JSON line: per form the prove rate, the two verify rates (every timed call, median, min, max) and the bytes
per statement on the wire (proof + commitments; the lean form's k public items travel beside them and are listed separately).

  python tools/public_coeff_probe.py [--proofs 4096] [--k 64] [--rounds 3] [--warm 1] [--group 64] [--tag T]"""
import argparse
import ctypes
import hashlib
import importlib
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--proofs", type=int, default=4096)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3, help="baked / lean pairs of every timed call")
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--group", type=int, default=64)
ap.add_argument("--capacity", type=int, default=256)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
lib = bp.load_library(); bp.load_gadgets_library()
if lib.bpr1cs_device_count() < 1:
    raise SystemExit("public_coeff_probe.py: no device (there is nothing to measure without one)")
B, k = args.proofs, args.k
m = k + 1
sc = lambda x: int(x).to_bytes(32, "little")
L = 2**252 + 27742317777372353535851937790883648493


def scalar(tag, i, bits=40):
    return 1 + int.from_bytes(hashlib.sha256(b"%s %d" % (tag, i)).digest(), "little") % (1 << bits)


base_set = [scalar(b"pcp item", i) for i in range(k)]
ip_baked = [k]
for x in base_set:
    ip_baked += [x & 0xffffffff, x >> 32]
# proof j of the lean form has a set of its own: the base set shifted by j
sets = [[x + j for x in base_set] for j in range(B)]
pos = [(7 * j + 3) % k for j in range(B)]
bits = [[1 if i == pos[j] else 0 for i in range(k)] for j in range(B)]
values = {"baked": b"".join(b"".join(sc(b) for b in bits[j]) + sc(base_set[pos[j]]) for j in range(B)),
          "lean": b"".join(b"".join(sc(b) for b in bits[j]) + sc(sets[j][pos[j]]) for j in range(B))}
publics = {"baked": None, "lean": b"".join(sc(x) for j in range(B) for x in sets[j])}
blindings = b"".join(sc(int.from_bytes(hashlib.sha512(b"pcp bl %d" % t).digest(), "little") % L) for t in range(B * m))
pseeds = b"".join(hashlib.sha256(b"pcp seed %d" % j).digest() for j in range(B))
vseeds = b"".join(hashlib.sha256(b"pcp vseed %d" % j).digest() for j in range(B))
label = b"SetMembershipProbe"
circ = {"baked": bp.CompiledGadget("set_membership", ip_baked, []), "lean": bp.CompiledGadget("set_membership_lean", [k], [])}
assert (circ["baked"].n, circ["baked"].m, circ["baked"].p) == (3 * k, m, 0) and (circ["lean"].n, circ["lean"].m, circ["lean"].p) == (k, m, k)
gens = bp.Gens(args.capacity)


def prove(which):
    c = circ[which]
    t0 = time.perf_counter()
    P, C = bp.prove_batch(gens, c, label, values[which], blindings, pseeds, B, wires=None, publics=publics[which])
    dt = time.perf_counter() - t0
    return B / dt, b"".join(P), b"".join(b"".join(x) for x in C)


def verify(which, P, C, form):
    c = circ[which]
    gens.set_option("verify_group", args.group if form == "grouped" else -1)
    cm = C + (publics[which] or b"")
    ok = (ctypes.c_int * B)()
    t0 = time.perf_counter()
    rc = lib.bpr1cs_verify_batch(gens.h, c.h, label, len(label), P, cm, vseeds, B, ok)
    dt = time.perf_counter() - t0
    assert rc == 0 and all(ok), "%s %s: rc %d, %d of %d proofs rejected" % (which, form, rc, list(ok).count(0), B)
    return B / dt


FORMS = ("per_proof", "grouped")
rates = {w: {f: [] for f in ("prove",) + FORMS} for w in circ}
made = {}
for r in range(args.warm + args.rounds):
    for w in circ:
        rate, P, C = prove(w)
        made[w] = (P, C)
        if r >= args.warm:
            rates[w]["prove"].append(rate)
gens.release_scratch()      # (the prover's arenas: the verifier would hand them back itself, inside its first timed call)
for r in range(args.warm + args.rounds):
    for f in FORMS:
        for w in circ:
            rate = verify(w, made[w][0], made[w][1], f)
            if r >= args.warm:
                rates[w][f].append(rate)
out = {"what": "one-of-%d set membership, %d proofs per call: set_membership (items baked, n = %d) against set_membership_lean (a set per proof, "
               "n = %d), alternating" % (k, B, 3 * k, k), "tag": args.tag, "proofs_per_call": B, "verify_group": args.group}
for w, c in circ.items():
    out[w] = {"n": c.n, "q": c.q, "m": c.m, "p": c.p, "proof_bytes": c.proof_len, "bytes_per_statement": c.proof_len + 32 * c.m, "public_input_bytes": 32 * c.p}
    for f, xs in rates[w].items():
        s = sorted(xs)
        out[w][f] = {"proofs_per_s": [round(x, 1) for x in xs], "median": round(s[len(s) // 2], 1), "min": round(s[0], 1), "max": round(s[-1], 1)}
out["lean_over_baked"] = {f: round(out["lean"][f]["median"] / out["baked"][f]["median"], 4) for f in ("prove",) + FORMS}
print(json.dumps(out), flush=True)
gens.close()
