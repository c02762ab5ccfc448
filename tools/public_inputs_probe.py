#!/usr/bin/env python3
"""What a public root costs the batched verifier: depth-32 tree proofs (the bench configuration: 4096 proofs, device
witness program) verified by bpr1cs_verify_batch with BPR1CS_OPT_VERIFY_GROUP = 64 through the circuit compiled with the root BAKED into
its last row and through the circuit compiled with the root as public input 0 - the SAME proofs, alternating on one handle of one
process.  The timed region is the C call alone: both `commitments` arrays - the points, and the points with the tail block behind them -
are laid out before it, as a C or Rust caller holds them.  One JSON line with every timed call; the spread of the baked calls is the
box's run-to-run spread that the difference has to be read against.  The proofs are made once by each circuit and asserted equal byte
for byte.

  python tools/public_inputs_probe.py [--proofs 4096] [--rounds 5] [--warm 1] [--group 64] [--tag T]"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--proofs", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=5, help="baked / public pairs of timed verify calls")
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
    raise SystemExit("public_inputs_probe.py: no device (there is nothing to measure without one)")
B = args.proofs
w = wl.vsmt4(bp, None, args.depth, B, B, 0)
m = w["m"]
circ = {"baked": bp.CompiledGadget(w["gadget"], w["ip"], w["sp"]), "public": bp.CompiledGadget(w["gadget"], w["ip"], [])}
assert circ["public"].p == 1 and circ["baked"].p == 0
publics = {"baked": None, "public": w["sp"][0] * B}
gens = bp.Gens(args.capacity)
seeds = b"".join((b"vseed%011d" % j).ljust(32, b".") for j in range(B))


def prove(which):
    return bp.prove_batch_raw(gens, circ[which], w["label"], w["values"], w["blindings"], w["seeds"], B, publics=publics[which])


def verify(which, P, cm):
    ok = (ctypes.c_int * B)()
    t0 = time.perf_counter()
    rc = lib.bpr1cs_verify_batch(gens.h, circ[which].h, w["label"], len(w["label"]), P, cm[which], seeds, B, ok)
    dt = time.perf_counter() - t0
    assert rc == 0 and all(ok), "%s: rc %d, %d of %d proofs rejected" % (which, rc, list(ok).count(0), B)
    return B / dt


def report(what, rates):
    out = {"what": what, "tag": args.tag, "proofs_per_call": B, "n": circ["baked"].n, "q": circ["baked"].q, "m": m}
    for k, r in rates.items():
        s = sorted(r)
        out[k] = {"proofs_per_s": [round(x, 1) for x in r], "median": round(s[len(s) // 2], 1), "min": round(s[0], 1), "max": round(s[-1], 1)}
    out["public_over_baked"] = round(out["public"]["median"] / out["baked"]["median"], 4)
    out["baked_spread"] = round((out["baked"]["max"] - out["baked"]["min"]) / out["baked"]["median"], 4)
    print(json.dumps(out), flush=True)


P, C = prove("baked")
assert prove("public") == (P, C), "the two circuits' proofs differ"
cm = {"baked": C, "public": C + publics["public"]}
gens.release_scratch()      # (the prover's arenas: the verifier would hand them back itself, inside its first timed call)
gens.set_option("verify_group", args.group)
for _ in range(args.warm):
    for k in ("baked", "public"):
        verify(k, P, cm)
rates = {"baked": [], "public": []}
for _ in range(args.rounds):
    for k in rates:
        rates[k].append(verify(k, P, cm))
report("bpr1cs_verify_batch, verify_group=%d, root baked / public alternating" % args.group, rates)
gens.close()
