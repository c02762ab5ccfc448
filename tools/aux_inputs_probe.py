#!/usr/bin/env python3
"""What uncommitted proof nodes are worth: one depth-32 job of 4096 tree proofs in two forms, alternating on one
handle of one process - "vsmt_4" (m = 100: leaf, index, 96 path nodes, 2 statics) and "vsmt_4_aux" (m = 4: the path nodes are auxiliary
inputs of the device witness program).  Each form is proved (one bpr1cs_prove_batch call, device witness program), then verified by
bpr1cs_verify_batch per proof, grouped (BPR1CS_OPT_VERIFY_GROUP = 64) and by bpr1cs_verify_batch_combined; every proof is checked by the
library's verifier in every timed verify call.  The timed region is the C call alone.  One JSON line: per form the prove rate, the
three verify rates (every timed call, median, min, max) and the bytes per statement on the wire (proof + commitments).

  python tools/aux_inputs_probe.py [--proofs 4096] [--rounds 3] [--warm 1] [--group 64] [--tag T]"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--proofs", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=3, help="plain / lean pairs of every timed call")
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--group", type=int, default=64)
ap.add_argument("--depth", type=int, default=32)
ap.add_argument("--capacity", type=int, default=32768)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
wl = importlib.import_module("bulletproofs-r1cs-gadgets_amd.workloads")
lib = bp.load_library(); bp.load_gadgets_library()
if lib.bpr1cs_device_count() < 1:
    raise SystemExit("aux_inputs_probe.py: no device (there is nothing to measure without one)")
B, depth = args.proofs, args.depth
w = wl.vsmt4(bp, None, depth, B, B, 0)
m = w["m"]
assert m == 4 + 3 * depth
nodes = range(2, 2 + 3 * depth)
kept = [i for i in range(m) if i not in nodes]


def pick(raw, idxs):
    """the entries `idxs` of every proof's m x 32 bytes, proof-major"""
    return b"".join(raw[32 * (m * j + i):32 * (m * j + i) + 32] for j in range(B) for i in idxs)


circ = {"plain": bp.CompiledGadget("vsmt_4", w["ip"], w["sp"]), "lean": bp.CompiledGadget("vsmt_4_aux", w["ip"], w["sp"])}
assert (circ["plain"].m, circ["plain"].a) == (m, 0) and (circ["lean"].m, circ["lean"].a) == (4, 3 * depth)
inputs = {"plain": (w["values"], w["blindings"], None), "lean": (pick(w["values"], kept), pick(w["blindings"], kept), pick(w["values"], nodes))}
gens = bp.Gens(args.capacity)
seeds = b"".join((b"vseed%011d" % j).ljust(32, b".") for j in range(B))
bseed = b"aux inputs probe batch seed".ljust(32, b".")


def prove(which):
    vals, bls, aux = inputs[which]
    out = bp.output_buffers(circ[which], B)
    t0 = time.perf_counter()
    P, C = bp.prove_batch_raw(gens, circ[which], w["label"], vals, bls, w["seeds"], B, out=out, aux=aux)
    dt = time.perf_counter() - t0
    return B / dt, bytes(P[:B * circ[which].proof_len]), bytes(C[:B * circ[which].m * 32])


def verify(which, P, C, form):
    c = circ[which]
    gens.set_option("verify_group", args.group if form == "grouped" else -1)
    if form == "combined":
        pt, wf = ctypes.create_string_buffer(32), ctypes.c_int()
        t0 = time.perf_counter()
        rc = lib.bpr1cs_verify_batch_combined(gens.h, c.h, w["label"], len(w["label"]), P, C, seeds, bseed, 0, B, pt, ctypes.byref(wf))
        dt = time.perf_counter() - t0
        assert rc == 0 and wf.value == 1 and pt.raw == bytes(32), "%s combined: rc %d" % (which, rc)
        return B / dt
    ok = (ctypes.c_int * B)()
    t0 = time.perf_counter()
    rc = lib.bpr1cs_verify_batch(gens.h, c.h, w["label"], len(w["label"]), P, C, seeds, B, ok)
    dt = time.perf_counter() - t0
    assert rc == 0 and all(ok), "%s %s: rc %d, %d of %d proofs rejected" % (which, form, rc, list(ok).count(0), B)
    return B / dt


FORMS = ("per_proof", "grouped", "combined")
rates = {k: {f: [] for f in ("prove",) + FORMS} for k in circ}
made = {}
for r in range(args.warm + args.rounds):
    for k in circ:
        rate, P, C = prove(k)
        made[k] = (P, C)
        if r >= args.warm:
            rates[k]["prove"].append(rate)
gens.release_scratch()      # (the prover's arenas: the verifier would hand them back itself, inside its first timed call)
for r in range(args.warm + args.rounds):
    for f in FORMS:
        for k in circ:
            rate = verify(k, made[k][0], made[k][1], f)
            if r >= args.warm:
                rates[k][f].append(rate)
out = {"what": "depth-%d tree membership, %d proofs per call: vsmt_4 (m = %d) against vsmt_4_aux (m = 4, a = %d), alternating" % (depth, B, m, 3 * depth),
       "tag": args.tag, "proofs_per_call": B, "verify_group": args.group}
for k, c in circ.items():
    out[k] = {"n": c.n, "q": c.q, "m": c.m, "a": c.a, "bytes_per_statement": c.proof_len + 32 * c.m}
    for f, xs in rates[k].items():
        s = sorted(xs)
        out[k][f] = {"proofs_per_s": [round(x, 1) for x in xs], "median": round(s[len(s) // 2], 1), "min": round(s[0], 1), "max": round(s[-1], 1)}
out["lean_over_plain"] = {f: round(out["lean"][f]["median"] / out["plain"][f]["median"], 4) for f in ("prove",) + FORMS}
print(json.dumps(out), flush=True)
gens.close()
