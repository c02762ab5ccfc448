#!/usr/bin/env python3
"""The start of a prove call from a rocprofv3 --kernel-trace database of `bench.py`: for the first job of the LAST call (the timed one;
JOBS = device jobs of that call, e.g. 4 for --steps 16), on a clock that starts with the job's first kernel - the end of
K_transcript_init, the TranscriptRng chain's launches, the reductions of its draws, and every multiscalar launch of the heavy stream up to
the job's K_transcript_A (the A_I / A_O sums, then S1 in one or two launches) with the idle time in front of it.  Then the steady state
of the jobs that follow: period and k_msm_fixed2 time per job, job by job.
  rocprofv3 --kernel-trace -d DIR -o out -- python bench.py --steps 16 --warmup 4 ; trace_call_start.py DIR 4"""
import collections
import glob
import sqlite3
import sys

db = sorted(glob.glob(sys.argv[1] + "/**/*.db", recursive=True))[-1]
jobs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
con = sqlite3.connect(db)
kt = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')") if r[0].startswith("kernels")][0]


def short(n):
    n = n.split("(")[0]
    for k in ("k_rng_stream", "k_witness_team", "k_msm_fixed2"):
        if k in n:
            return k
    if "k_functor_wave<" in n:
        return n.split("k_functor_wave<")[1].split(">")[0]
    if "k_functor<" in n:
        return n.split("k_functor<")[1].split(">")[0]
    return n[:40]


rows = [(short(n), s, e, q) for n, s, e, q in con.execute("select name, start, end, queue_id from %s order by start" % kt)]
inits = [r for r in rows if r[0] == "K_transcript_init"]
if len(inits) < jobs:
    sys.exit("fewer than %d device jobs in the trace" % jobs)
ti = inits[-jobs]
nxt = inits[-jobs + 1][1] if jobs > 1 else rows[-1][2]
hq = collections.Counter(r[3] for r in rows if r[0] == "k_msm_fixed2").most_common(1)[0][0]
t0 = max(r[1] for r in rows if r[0] == "K_load_inputs" and r[1] <= ti[1])
ms = lambda t: (t - t0) / 1e6
ta = min(r for r in rows if r[0] == "K_transcript_A" and r[1] > ti[1])
print("# first job of the last call (%d jobs); ms after its first kernel" % jobs)
print("K_transcript_init ends              %8.2f" % ms(ti[2]))
for r in rows:
    if r[0] == "k_witness_team" and t0 <= r[1] < min(nxt, ta[1]):
        print("k_witness_team                      %8.2f .. %8.2f" % (ms(r[1]), ms(r[2])))
legs = [r for r in rows if r[0] == "k_rng_stream" and t0 <= r[1] < min(nxt, ta[1])]
for r in legs:
    print("k_rng_stream leg                    %8.2f .. %8.2f   (%.2f ms)" % (ms(r[1]), ms(r[2]), (r[2] - r[1]) / 1e6))
for r in rows:
    if r[0] == "K_rng_reduce" and ti[2] <= r[1] < ta[1]:
        print("K_rng_reduce                        %8.2f .. %8.2f" % (ms(r[1]), ms(r[2])))
heavy = [r for r in rows if r[3] == hq and ti[1] <= r[1] <= ta[1]]
prev = None
for r in heavy:
    if r[0] == "k_msm_fixed2":
        print("k_msm_fixed2                        %8.2f .. %8.2f   (%.2f ms; heavy stream idle for %.2f ms in front of it)" %
              (ms(r[1]), ms(r[2]), (r[2] - r[1]) / 1e6, (r[1] - prev[2]) / 1e6 if prev else 0.0))
    prev = r
print("K_transcript_A starts               %8.2f" % ms(ta[1]))
if legs:
    print("# the chain's last leg ends %.2f ms after the job's first kernel, K_transcript_A starts %.2f ms after that" % (ms(legs[-1][2]), (ta[1] - legs[-1][2]) / 1e6))
# the jobs that follow: from one K_transcript_A to the next
tas = [r for r in rows if r[0] == "K_transcript_A" and r[1] >= ta[1]][:jobs]
print("# jobs 2..%d of the call: period (K_transcript_A to K_transcript_A) and k_msm_fixed2 time inside it, ms" % jobs)
for a, b in zip(tas, tas[1:]):
    inside = [r for r in rows if r[0] == "k_msm_fixed2" and r[3] == hq and a[1] <= r[1] < b[1]]
    print("  period %8.2f   k_msm_fixed2 %8.2f in %d launches" % ((b[1] - a[1]) / 1e6, sum(r[2] - r[1] for r in inside) / 1e6, len(inside)))
