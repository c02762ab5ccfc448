#!/usr/bin/env python3
"""What BPR1CS_OPT_CHECK_WITNESS costs: proofs/s of one job of depth-32 tree proofs (the bench configuration: 4096
proofs, device witness program) with the option off and on, ALTERNATING on one handle of one process, then the same for one proof per
call.  One JSON line per row with every timed call; the spread of the "off" calls is the box's run-to-run spread that the difference
has to be read against.  All witnesses are good: the check runs, nothing is refused (asserted).

  python tools/witness_check_probe.py [--proofs 4096] [--rounds 5] [--warm 2] [--single 20] [--root DIR] [--tag T]

--root: import the package from another checkout (a build of the parent commit, which has no such option: only the "off" rows run -
the baseline of the "off" rows here; run both in one session, alternating).  The row form's size on the device is read from
bpr1cs_prove_stats: the job-size model charges it while the first checked job has still to upload it."""
import argparse
import importlib
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--proofs", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=5, help="off / on pairs of timed calls")
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--single", type=int, default=20, help="off / on pairs of timed one-proof calls (0: skip)")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
wl = importlib.import_module("bulletproofs-r1cs-gadgets_amd.workloads")
lib = bp.load_library(); bp.load_gadgets_library()
if lib.bpr1cs_device_count() < 1:
    raise SystemExit("witness_check_probe.py: no device (there is nothing to measure without one)")
HAVE = "check_witness" in bp.OPTIONS
B = args.proofs
w = wl.vsmt4(bp, None, 32, B, B, 0)
circ = bp.CompiledGadget(w["gadget"], w["ip"], w["sp"])
m = w["m"]
gens = bp.Gens(32768)


def call(nb, on):
    if HAVE:
        gens.set_option("check_witness", 1 if on else 0)
    t0 = time.perf_counter()
    P, _ = bp.prove_batch(gens, circ, w["label"], w["values"][:32 * m * nb], w["blindings"][:32 * m * nb], w["seeds"][:32 * nb], nb, wires=None)
    dt = time.perf_counter() - t0
    st = bp.last_prove_stats(lib)
    assert st.get("refused", 0) == 0 and P[0][0] == 0 and P[-1][0] == 0
    return nb / dt, st


def report(what, nb, rates):
    out = {"what": what, "tag": args.tag, "proofs_per_call": nb, "n": circ.n, "q": circ.q, "m": m}
    for k, r in rates.items():
        s = sorted(r)
        out[k] = {"proofs_per_s": [round(x, 2) for x in r], "median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}
    if "on" in rates and rates["on"]:
        out["on_over_off"] = round(out["on"]["median"] / out["off"]["median"], 4)
        out["off_spread"] = round((out["off"]["max"] - out["off"]["min"]) / out["off"]["median"], 4)
    print(json.dumps(out), flush=True)


def run(what, nb, warm, rounds):
    fixed = {False: [], True: []}
    for _ in range(warm):
        for on in ((False, True) if HAVE else (False,)):
            fixed[on].append(call(nb, on)[1]["sizing_fixed_bytes"])
    rates = {"off": [], "on": []} if HAVE else {"off": []}
    for _ in range(rounds):
        rates["off"].append(call(nb, False)[0])
        if HAVE:
            rates["on"].append(call(nb, True)[0])
    report(what, nb, rates)
    return fixed


fixed = run("one job, option off / on alternating", B, args.warm, args.rounds)
if HAVE and len(fixed[False]) >= 2:
    # the FIRST call with the option on still has the row form to upload; the second call with it off has nothing pending any more
    # (the first one also had the circuit's merged tables to build)
    print(json.dumps({"what": "row form on the device (36 B per constraint term + row offsets + chunk list)", "bytes": fixed[True][0] - fixed[False][1]}), flush=True)
if args.single:
    run("one proof per call, option off / on alternating", 1, 3, args.single)
gens.close()
