#!/usr/bin/env python3
"""What the start of a prove call costs where it matters most: ONE call of exactly one device job - 4096 depth-32 tree
proofs, the device witness program - so nothing hides the job's TranscriptRng chains.  Median of --calls timed calls after --warm untimed
ones; one JSON line with every call's milliseconds, the host's part of the chains and the multiscalar launches of the call.

  python tools/call_start_probe.py [--proofs 4096] [--calls 5] [--warm 2] [--share -1] [--root DIR] [--tag T]

--root: import the package from another checkout (a build of the parent commit); run the two alternating, one process each."""
import argparse
import importlib
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--proofs", type=int, default=4096)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--share", type=int, default=-1, help="BPR1CS_OPT_HOST_CHAIN_SHARE (-1: the library's choice)")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
wl = importlib.import_module("bulletproofs-r1cs-gadgets_amd.workloads")
lib = bp.load_library(); bp.load_gadgets_library()
if lib.bpr1cs_device_count() < 1:
    raise SystemExit("call_start_probe.py: no device (there is nothing to measure without one)")
B = args.proofs
w = wl.vsmt4(bp, None, 32, B, B, 0)
circ = bp.CompiledGadget(w["gadget"], w["ip"], w["sp"])
m = w["m"]
gens = bp.Gens(32768)
gens.set_option("job_proofs", B)
gens.set_option("host_chain_share", args.share)
ms, st, first = [], None, None
for k in range(args.warm + args.calls):
    t0 = time.perf_counter()
    P, _ = bp.prove_batch(gens, circ, w["label"], w["values"], w["blindings"], w["seeds"], B, wires=None)
    dt = time.perf_counter() - t0
    st = bp.last_prove_stats(lib)
    assert st["jobs"] == 1 and len(P) == B
    if first is None:
        first = P
    assert P == first   # (same witnesses, same seeds: the same bytes every call)
    if k >= args.warm:
        ms.append(1e3 * dt)
s = sorted(ms)
print(json.dumps({"what": "one call = one job", "tag": args.tag, "proofs": B, "n": circ.n, "ms_per_call": [round(x, 2) for x in ms], "median_ms": round(s[len(s) // 2], 2),
                  "min_ms": round(s[0], 2), "max_ms": round(s[-1], 2), "proofs_per_s": round(1e3 * B / s[len(s) // 2], 1), "host_chains": st["host_chains"],
                  "msm_launches": st["msm_launches"], "phase_ms": [round(x, 2) for x in st["phase_ms"]]}), flush=True)
gens.close()
