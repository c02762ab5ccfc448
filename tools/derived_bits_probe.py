#!/usr/bin/env python3
"""What the one-commitment bound check costs or saves: 64-bit bound checks proved in ONE device job by the device
witness program, alternating on one handle of one process between
  m3_baked   the reference gadget (bound_check: v, v - min and max - v committed, the bounds baked; bench configuration c1), and
  m1_public  bound_check_1 (v alone committed; the bits of v - min and max - v are BPR1CS_W_LCBIT operands, the bounds public inputs
             0 and 1 of every proof - a different pair per proof).
Both circuits have n = 128 multipliers.  The timed region is the prove call alone; the input arrays - for m1_public the values with
the tail block of bounds behind them - are laid out before it.  One JSON line with every timed call; the spread of the m3_baked calls
is the box's run-to-run spread that the difference has to be read against.  Before timing, every proof of each kind is verified by
the device verifier.

  python tools/derived_bits_probe.py [--proofs 4096] [--rounds 5] [--warm 1] [--tag T]"""
import argparse
import importlib
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--proofs", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=5, help="m3_baked / m1_public pairs of timed prove calls")
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--capacity", type=int, default=128)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
wl = importlib.import_module("bulletproofs-r1cs-gadgets_amd.workloads")
lib = bp.load_library(); bp.load_gadgets_library()
if lib.bpr1cs_device_count() < 1:
    raise SystemExit("derived_bits_probe.py: no device (there is nothing to measure without one)")
B = args.proofs
w3 = wl.bound_check64(B)
vs, bounds, bl1 = [], [], []
for j in range(B):                          # the same v as proof j of the reference gadget, in a window of its own
    v = int.from_bytes(w3["values"][96 * j:96 * j + 32], "little")
    lo = v - wl.synth_scalar(b"db-probe-lo", j) % min(v + 1, 1 << 64)
    hi = lo + max(v - lo, wl.synth_scalar(b"db-probe-hi", j) % (1 << 64))
    vs.append(wl.sc(v))
    bounds.append(wl.sc(lo) + wl.sc(hi))
    bl1.append(w3["blindings"][96 * j:96 * j + 32])
work = {"m3_baked": dict(circ=bp.CompiledGadget(w3["gadget"], w3["ip"], w3["sp"]), label=w3["label"], values=w3["values"], blindings=w3["blindings"], publics=None),
        "m1_public": dict(circ=bp.CompiledGadget("bound_check_1", [64], []), label=b"BoundCheck1", values=b"".join(vs), blindings=b"".join(bl1), publics=b"".join(bounds))}
assert work["m1_public"]["circ"].p == 2 and work["m3_baked"]["circ"].p == 0
assert all(x["circ"].has_witness_program and x["circ"].n == 128 for x in work.values())
gens = bp.Gens(args.capacity)
gens.set_option("job_proofs", B)           # one job


def prove(which):
    x = work[which]
    t0 = time.perf_counter()
    out = bp.prove_batch_raw(gens, x["circ"], x["label"], x["values"], x["blindings"], w3["seeds"], B, publics=x["publics"])
    return B / (time.perf_counter() - t0), out


for k, x in work.items():
    _, (P, C) = prove(k)
    ok = bp.verify_batch(gens, x["circ"], x["label"], P, C, B, publics=x["publics"])
    assert all(ok), "%s: %d of %d proofs rejected" % (k, ok.count(False), B)
for _ in range(max(0, args.warm - 1)):
    for k in work:
        prove(k)
rates = {k: [] for k in work}
for _ in range(args.rounds):
    for k in rates:
        rates[k].append(prove(k)[0])
out = {"what": "bpr1cs_prove_batch, device witness program, 64-bit bound checks in one job: bound_check (m = 3, baked) / bound_check_1 (m = 1, public bounds) alternating",
       "tag": args.tag, "proofs_per_call": B, "n": 128, "q": {k: x["circ"].q for k, x in work.items()}, "m": {k: x["circ"].m for k, x in work.items()}}
for k, r in rates.items():
    s = sorted(r)
    out[k] = {"proofs_per_s": [round(x, 1) for x in r], "median": round(s[len(s) // 2], 1), "min": round(s[0], 1), "max": round(s[-1], 1)}
out["m1_over_m3"] = round(out["m1_public"]["median"] / out["m3_baked"]["median"], 4)
out["m3_spread"] = round((out["m3_baked"]["max"] - out["m3_baked"]["min"]) / out["m3_baked"]["median"], 4)
print(json.dumps(out), flush=True)
gens.close()
