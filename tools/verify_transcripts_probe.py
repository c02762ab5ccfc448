#!/usr/bin/env python3
"""What the caller's transcripts cost the batched verifiers: depth-32 tree proofs (the bench configuration: 4096 proofs,
device witness program) verified per proof, grouped (BPR1CS_OPT_VERIFY_GROUP = 64) and combined, alternating on one handle of one process

    label   the label form: Transcript::new(label) for every proof
    t0      BPR1CS_LABEL_TRANSCRIPTS, one handle per proof, context of 0 bytes (a fresh transcript: the SAME proofs as `label`)
    t64     the same with 64 bytes of context per proof, different for every proof (proofs made by bpr1cs_prove_batch_transcripts on them)

The timed region is the C call alone; the handles of a transcripts call are made before it (the call advances them, so every call gets
its own).  One JSON line per verifier with every timed call; the spread of the label calls is the box's run-to-run spread that a ratio has to
be read against.  `--forms label` runs on a build without the flag too, and `--lib-dir DIR` takes libbpr1cs_hip.so / libbpr1cs_gadgets.so from
DIR: the parent commit's build and this one, alternating processes on one box, give the cost the new kernel fields have for the label form.

  python tools/verify_transcripts_probe.py [--proofs 4096] [--rounds 5] [--warm 1] [--group 64] [--forms label,t0,t64] [--verifiers per_proof,grouped,combined] [--lib-dir DIR] [--tag T]"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--proofs", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=5, help="timed calls per form and verifier, alternating")
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--group", type=int, default=64)
ap.add_argument("--depth", type=int, default=32)
ap.add_argument("--capacity", type=int, default=32768)
ap.add_argument("--forms", default="label,t0,t64")
ap.add_argument("--verifiers", default="per_proof,grouped,combined")
ap.add_argument("--lib-dir", default=None)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bp = importlib.import_module("bulletproofs-r1cs-gadgets_amd")
wl = importlib.import_module("bulletproofs-r1cs-gadgets_amd.workloads")
if args.lib_dir:
    lib = bp.load_library(os.path.join(args.lib_dir, "libbpr1cs_hip.so"))
    glib = bp.load_gadgets_library(os.path.join(args.lib_dir, "libbpr1cs_gadgets.so"))
else:
    lib, glib = bp.load_library(), bp.load_gadgets_library()
if lib.bpr1cs_device_count() < 1:
    raise SystemExit("verify_transcripts_probe.py: no device (there is nothing to measure without one)")
forms = args.forms.split(",")
assert forms and set(forms) <= {"label", "t0", "t64"}, forms
B = args.proofs
w = wl.vsmt4(bp, glib, args.depth, B, B, 0)
label = w["label"]
circ = bp.CompiledGadget(w["gadget"], w["ip"], w["sp"], lib=lib, glib=glib)
gens = bp.Gens(args.capacity, lib=lib)
seeds = b"".join((b"vseed%011d" % j).ljust(32, b".") for j in range(B))
bseed = b"verify transcripts probe".ljust(32, b".")
FLAG = 1 << (8 * ctypes.sizeof(ctypes.c_size_t) - 1)


def transcripts(form):
    ts = [bp.Transcript(label, lib=lib) for _ in range(B)]
    if form == "t64":
        for j, t in enumerate(ts):
            t.append_message(b"ctx", (b"session %08d " % j).ljust(64, b"#"))
    return ts


def join(P, C):
    return b"".join(P), b"".join(b"".join(c) for c in C)


made = {}
if "label" in forms or "t0" in forms:
    P, C = bp.prove_batch_raw(gens, circ, label, w["values"], w["blindings"], w["seeds"], B)
    made["label"] = made["t0"] = (bytes(P), bytes(C))
if "t64" in forms:
    made["t64"] = join(*bp.prove_batch_transcripts(gens, circ, transcripts("t64"), w["values"], w["blindings"], w["seeds"], B))
if "t0" in forms and args.proofs <= 64:     # (a small run also shows that a fresh handle and the label are the same statement)
    assert join(*bp.prove_batch_transcripts(gens, circ, transcripts("t0"), w["values"], w["blindings"], w["seeds"], B)) == made["t0"]


def timed(verifier, form):
    P, cm = made[form]
    start, start_len, keep = label, len(label), None
    if form != "label":
        keep = transcripts(form)
        arr = (ctypes.c_void_p * B)(*[t.h for t in keep])
        start, start_len = ctypes.cast(arr, ctypes.c_char_p), FLAG | B
    if verifier == "combined":
        out, wf = ctypes.create_string_buffer(32), ctypes.c_int()
        t0 = time.perf_counter()
        rc = lib.bpr1cs_verify_batch_combined(gens.h, circ.h, start, start_len, P, cm, seeds, bseed, 0, B, out, ctypes.byref(wf))
        dt = time.perf_counter() - t0
        assert rc == 0 and wf.value == 1 and out.raw == bytes(32), "%s/%s: rc %d, wellformed %d, point %s" % (verifier, form, rc, wf.value, out.raw.hex())
    else:
        ok = (ctypes.c_int * B)()
        t0 = time.perf_counter()
        rc = lib.bpr1cs_verify_batch(gens.h, circ.h, start, start_len, P, cm, seeds, B, ok)
        dt = time.perf_counter() - t0
        assert rc == 0 and all(ok), "%s/%s: rc %d, %d of %d proofs rejected" % (verifier, form, rc, list(ok).count(0), B)
    return B / dt


def report(verifier, rates):
    out = {"what": "verify, %s" % verifier, "tag": args.tag, "proofs_per_call": B, "n": circ.n, "m": circ.m}
    for k, r in rates.items():
        s = sorted(r)
        out[k] = {"proofs_per_s": [round(x, 1) for x in r], "median": round(s[len(s) // 2], 1), "min": round(s[0], 1), "max": round(s[-1], 1)}
    if "label" in rates:
        out["label_spread"] = round((out["label"]["max"] - out["label"]["min"]) / out["label"]["median"], 4)
        for k in rates:
            if k != "label":
                out[k + "_over_label"] = round(out[k]["median"] / out["label"]["median"], 4)
    print(json.dumps(out), flush=True)


gens.release_scratch()      # (the prover's arenas: the verifier would hand them back itself, inside its first timed call)
for verifier in args.verifiers.split(","):
    assert verifier in ("per_proof", "grouped", "combined"), verifier
    gens.set_option("verify_group", args.group if verifier == "grouped" else -1)
    for _ in range(args.warm):
        for f in forms:
            timed(verifier, f)
    rates = {f: [] for f in forms}
    for _ in range(args.rounds):
        for f in forms:
            rates[f].append(timed(verifier, f))
    report(verifier, rates)
gens.close()
