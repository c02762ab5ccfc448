"""The multiscalar-multiplication entry points of the C ABI swept across every launch-geometry boundary: cases and expectations
shared by the CPU simulator (tests/test_msm_geometry.py) and the device (tests/test_gpu_msm_geometry.py).

Three things live here:

  * plan() / plan_msm(): a plain-Python mirror of the host arithmetic that cuts a sum into chunks, picks a kernel by batch size and
    folds the chunk sums (csrc/msm_run.hpp run_msm_multi and pick_chunks, the run / job splitting of bpr1cs_msm_fixed and the
    Straus / Pippenger switch of bpr1cs_msm in csrc/api_lowlevel.hpp).  Its constants are READ from those sources by regular
    expression: a changed threshold moves the plan, and the coverage check of tests/test_msm_geometry.py then says which boundary
    the table no longer straddles.
  * the case table: base lists given as runs of consecutive base indices (0 = B, 1 = B~, 2 + i = G_i, 2 + cap + i = H_i), a batch,
    a scalar recipe and the branch each case exists to reach.
  * the expectations: the C oracle's multiscalar multiplication (oracle/cref.py COracle.msm) - per proof where terms x batch
    <= 2^17, and for larger shapes exact on a few proofs plus ONE random linear combination over all of them.

Nothing here is derived from the library under test except the generators' encodings (bpr1cs_gens_point), which
tests/test_gpu_parity.py::test_generators_match_oracle pins to the oracle."""
import functools
import hashlib
import os
import re
import zlib

from pyref import scenarios as S
from pyref.ed import L, decompress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bulletproofs-r1cs-gadgets_amd", "csrc")
WAVE = 64   # lanes of a wavefront: k_msm_small_wave / k_ge_reduce_wave fold 64 sums, k_msm_fixed2 takes 64 proofs per workgroup


# ------------------------------------------------------------------------------------------------ constants, read from the sources
_PATTERNS = {
    # name: (file, pattern) - every group is an integer
    "LANE_PATH_MAX_PROOFS": ("msm_run.hpp", r"\bMSM_LANE_PATH_MAX_PROOFS\s*=\s*(\d+)\s*;"),
    "WAVE_REDUCE_MAX_CHUNK": ("msm_run.hpp", r"\bMSM_WAVE_REDUCE_MAX_CHUNK\s*=\s*(\d+)\s*;"),
    "REDUCE_GROUP": ("msm_run.hpp", r"\bMSM_REDUCE_GROUP\s*=\s*(\d+)\s*;"),
    # (simulator, device)
    "SMALL_REDUCE_GROUP": ("msm_run.hpp", r"#if defined\(BPR1CS_HOSTSIM\)\s*static const uint32_t SMALL_REDUCE_GROUP\s*=\s*(\d+)\s*;\s*"
                                          r"#else\s*static const uint32_t SMALL_REDUCE_GROUP\s*=\s*(\d+)\s*;"),
    "SMALL_THREADS_LOG2": ("msm_run.hpp", r"pick_chunks\(total, B, 1u << (\d+), q\.plan->chunk\)"),
    "SMALL_MAX_LEVELS": ("msm_run.hpp", r"cnt > MSM_REDUCE_GROUP && S\.nl < (\d+)\)"),
    "IN_WAVE_GROUP": ("msm_run.hpp", r"in_wave \? \(S\.nchunks \+ (\d+)u\) / (\d+)u : S\.nchunks"),
    # (chunk below, total at least) then (chunk set, rounding, divisor)
    "BUMP_IF": ("msm_run.hpp", r"q\.plan->chunk < (\d+) && total >= (\d+)\)"),
    "BUMP_TO": ("msm_run.hpp", r"q\.plan->chunk = (\d+);\s*nchunks = \(total \+ (\d+)\) / (\d+);"),
    "NWG_PAD": ("msm_run.hpp", r"L\.nwg = \(L\.wg_end\[L\.njobs - 1\] \+ (\d+)u\) & ~(\d+)u;"),
    "XCD_REMAP": ("msm_kernel.hpp", r"if \(\(L\.nwg & (\d+)u\) == 0\) wg = \(wg & (\d+)u\) \* \(L\.nwg >> (\d+)\) \+ \(wg >> (\d+)\);"),
    "MAX_JOBS": ("kernels.hpp", r"#define MSM_MAX_JOBS (\d+)\b"),
    "THREADS_LOG2_DEFAULT": ("api_common.hpp", r"msm_threads_log2\{(\d+)\}"),
    # (default, low, low, high, high)
    "THREADS_LOG2_CLAMP": ("api_common.hpp", r"o\.msm_threads_log2 = value < 0 \? (\d+) : \(value < (\d+) \? (\d+) : \(value > (\d+) \? (\d+) : value\)\)"),
    # bpr1cs_msm: (Straus below, its chunk cap), Pippenger from, (chunk cap, terms per chunk)
    "VAR_STRAUS": ("api_lowlevel.hpp", r"VC = N < (\d+) \? \(N \+ 63\) / 64 : (\d+)"),
    "VAR_PIPPENGER_FROM": ("api_lowlevel.hpp", r"if \(N >= (\d+)\) \{\s*// LDS-staged Pippenger"),
    "VAR_PIPPENGER_CHUNKS": ("api_lowlevel.hpp", r"std::min<uint32_t>\((\d+)u, N / (\d+)u\)"),
    # the two-term commitment shape of bpr1cs_msm_fixed: a wavefront per commitment up to this batch
    "COMMIT_WAVE_MAX": ("api_lowlevel.hpp", r"if \(B <= (\d+)\) \{\s*// a handful of commitments"),
}


@functools.lru_cache(None)
def constants():
    """-> dict name -> int or tuple of ints; fails loudly when a pattern no longer matches its source"""
    text, out = {}, {}
    for name, (fn, pat) in _PATTERNS.items():
        if fn not in text:
            with open(os.path.join(CSRC, fn)) as f:
                text[fn] = f.read()
        m = re.search(pat, text[fn])
        assert m, "msm_cases: %s not found in csrc/%s - plan() no longer mirrors the source (pattern %r)" % (name, fn, pat)
        v = tuple(int(x) for x in m.groups())
        out[name] = v[0] if len(v) == 1 else v
    # what the mirror below takes for granted about the shape of those expressions
    assert out["IN_WAVE_GROUP"] == (WAVE - 1, WAVE)
    assert out["BUMP_IF"][0] == out["BUMP_IF"][1] == out["BUMP_TO"][0] == out["BUMP_TO"][2] == out["BUMP_TO"][1] + 1
    assert out["NWG_PAD"][0] == out["NWG_PAD"][1] == out["XCD_REMAP"][0] == out["XCD_REMAP"][1] and out["XCD_REMAP"][2] == out["XCD_REMAP"][3]
    assert out["NWG_PAD"][0] + 1 == 1 << out["XCD_REMAP"][2]
    d, lo, lo2, hi, hi2 = out["THREADS_LOG2_CLAMP"]
    assert d == out["THREADS_LOG2_DEFAULT"] and lo == lo2 and hi == hi2
    assert out["VAR_STRAUS"][0] == out["VAR_PIPPENGER_FROM"]
    return out


def _cdiv(a, b):
    return (a + b - 1) // b


def pick_chunks(items, B, target_threads):
    """csrc/msm_run.hpp pick_chunks -> (chunk, nchunks)"""
    want = max(1, _cdiv(target_threads, B))
    if want > items:
        want = items if items else 1
    chunk = max(1, _cdiv(items, want))
    return chunk, _cdiv(items, chunk)


def split_runs(bases):
    """bpr1cs_msm_fixed: a base list is served as runs of consecutive bases -> [(first term, length)]"""
    runs, t = [], 0
    while t < len(bases):
        e = t + 1
        while e < len(bases) and bases[e] == bases[e - 1] + 1:
            e += 1
        runs.append((t, e - t))
        t = e
    return runs


def _plan_small(reqs, B, K, hostsim):
    group = K["SMALL_REDUCE_GROUP"][0 if hostsim else 1]
    jobs = []
    for a, b in reqs:
        total = a + b
        chunk, nchunks = pick_chunks(total, B, 1 << K["SMALL_THREADS_LOG2"])
        in_wave = (not hostsim) and chunk <= K["WAVE_REDUCE_MAX_CHUNK"]
        groups = _cdiv(nchunks, WAVE) if in_wave else nchunks
        cnt, lv = groups, []
        while cnt > K["REDUCE_GROUP"] and len(lv) < K["SMALL_MAX_LEVELS"]:
            cnt = _cdiv(cnt, group)
            lv.append(cnt)
        jobs.append(dict(path="small", runs=(a, b), lone=b == 0, total=total, chunk=chunk, nchunks=nchunks, last_chunk=total - (nchunks - 1) * chunk,
                         in_wave=in_wave, groups=groups, last_group=(nchunks - (groups - 1) * WAVE) if in_wave else None,
                         lv=tuple(lv), nl=len(lv), first_off=sum(lv), need=(groups + sum(lv)) * B, out_chunks=cnt,
                         launch_paired=False, reduce_paired=False))
    r = 0
    while r < len(jobs):   # the launch loop: two in-wave requests of the same shape share a launch
        if jobs[r]["groups"] == 0 or not jobs[r]["in_wave"]:
            r += 1
            continue
        pair = r + 1 < len(jobs) and jobs[r + 1]["in_wave"] and jobs[r + 1]["groups"] == jobs[r]["groups"]
        if pair:
            jobs[r]["launch_paired"] = jobs[r + 1]["launch_paired"] = True
        r += 2 if pair else 1
    r = 0
    while r < len(jobs):   # the reduction loop: two requests with the same levels share the launches of their levels
        pair = r + 1 < len(jobs) and jobs[r + 1]["groups"] == jobs[r]["groups"] and jobs[r + 1]["nl"] == jobs[r]["nl"] and jobs[r]["nl"] > 0
        if pair:
            jobs[r]["reduce_paired"] = jobs[r + 1]["reduce_paired"] = True
        r += 2 if pair else 1
    return jobs


def _plan_fixed2(reqs, B, K, tl):
    nbk, G = _cdiv(B, WAVE), K["REDUCE_GROUP"]
    jobs, wg = [], 0
    for a, b in reqs:
        total = a + b
        chunk, nchunks = pick_chunks(total, B, 1 << tl)
        bumped = chunk < K["BUMP_IF"][0] and total >= K["BUMP_IF"][1]
        if bumped:
            chunk = K["BUMP_TO"][0]
            nchunks = _cdiv(total, chunk)
        l1 = _cdiv(nchunks, G) if nchunks > G else 0
        l2 = _cdiv(l1, G) if l1 > G else 0
        wg += nchunks * nbk
        jobs.append(dict(path="fixed2", runs=(a, b), lone=b == 0, total=total, chunk=chunk, nchunks=nchunks, last_chunk=total - (nchunks - 1) * chunk,
                         bumped=bumped, below_bump=total < K["BUMP_IF"][1], l1=l1, l2=l2, out_chunks=l2 or l1 or nchunks, nbk=nbk,
                         live_last=B - WAVE * (nbk - 1), wg_end=wg))
    nwg = (wg + K["NWG_PAD"][0]) & ~K["NWG_PAD"][1]
    for j in jobs:
        j.update(nwg_raw=wg, nwg=nwg, padded=nwg != wg)
    return jobs


def plan(runs, B, threads_log2=None, hostsim=False):
    """The launch geometry of bpr1cs_msm_fixed(bases, batch B) on a handle whose BPR1CS_OPT_MSM_THREADS_LOG2 is `threads_log2`
    (None: the default).  `runs`: the run lengths of the base list (or the runs themselves, as lists of indices).  hostsim: what
    the CPU simulator's build of the same host code does (no wavefront kernels, a narrower reduction group).
    -> dict(calls = number of run_msm_multi calls, jobs = [dict per job, in order], nwg = [workgroups per k_msm_fixed2 launch])"""
    K = constants()
    lens = [r if isinstance(r, int) else len(r) for r in runs]
    assert lens and all(n > 0 for n in lens)
    d, lo, _, hi, _ = K["THREADS_LOG2_CLAMP"]
    tl = d if threads_log2 is None or threads_log2 < 0 else min(max(threads_log2, lo), hi)
    reqs = [(lens[i], lens[i + 1] if i + 1 < len(lens) else 0) for i in range(0, len(lens), 2)]
    out = dict(calls=0, jobs=[], nwg=[])
    start = 0
    for j0 in range(0, len(reqs), K["MAX_JOBS"]):
        part = reqs[j0:j0 + K["MAX_JOBS"]]
        jobs = _plan_small(part, B, K, hostsim) if B <= K["LANE_PATH_MAX_PROOFS"] else _plan_fixed2(part, B, K, tl)
        for j in jobs:
            j.update(call=out["calls"], start=start)
            start += j["total"]
        if jobs[0]["path"] == "fixed2":
            out["nwg"].append(jobs[0]["nwg"])
        out["jobs"] += jobs
        out["calls"] += 1
    return out


def plan_msm(n, hostsim=False):
    """bpr1cs_msm on n terms -> dict(path, chunks, per, last): Straus with one chunk per 64 terms below the switch (and in the
    simulator's build at every size), LDS-staged Pippenger buckets over `chunks` slices of ceil(n / chunks) terms from it on"""
    K = constants()
    below, cap = K["VAR_STRAUS"]
    if n < below or hostsim:
        vc = _cdiv(n, 64) if n < below else cap
        return dict(path="straus", chunks=vc, capped=False, last=None)
    ccap, per_chunk = K["VAR_PIPPENGER_CHUNKS"]
    chunks = max(1, min(ccap, n // per_chunk))
    per = _cdiv(n, chunks)
    return dict(path="pippenger", chunks=chunks, capped=n // per_chunk >= ccap, per=per, last=n - (chunks - 1) * per)


# ------------------------------------------------------------------------------------------------ the case table
HANDLES = {
    # name: (window bits, capacity) - "geo": 4098 bases at 64 windows x 9 slots x 128 bytes = 74 KB each (300 MB); the two longest
    # runs (all 4098 bases, twice) make a job of 8196 terms, the smallest that crosses the last threshold of the small path
    "geo": (4, 2048),
    "w8": (8, 64),
    "w11": (11, 64),
    "w15": (15, 4),
}
# The simulator builds its tables on one CPU core (capacity 2048 takes it 100 s): its "geo" handle is a smaller one, and the cases
# flagged `sim` keep to base indices that exist on it.  A base index is a row of the table on either handle, so the geometry of a
# case is the same on both; the points behind the indices differ, and every expectation is made from the points of the handle
# that ran the case.
SIM_HANDLES = dict(HANDLES, geo=(4, 128))
FULL_CHECK_MAX = 1 << 17       # terms x batch up to which every proof gets an oracle sum of its own
SAMPLE_PROOFS = (0, 1, 63, 64, -1)


def _case(name, group, handle, runs, B, branch, tl=None, zeros=(), edges=False, sim=False):
    bases = [i for s, n in runs for i in range(s, s + n)]
    nb = 2 + 2 * HANDLES[handle][1]
    assert all(0 <= i < nb for i in bases), name
    assert [n for _, n in split_runs(bases)] == [n for _, n in runs], "%s: the runs as written are not the runs bpr1cs_msm_fixed will see" % name
    assert not (len(bases) == 2 and bases == [0, 1]), "%s: that is the commitment shape, another code path" % name
    assert not sim or all(i < 2 + 2 * SIM_HANDLES[handle][1] for i in bases), "%s: a base the simulator's handle does not have" % name
    return dict(name=name, group=group, handle=handle, runs=tuple(runs), bases=tuple(bases), terms=len(bases), B=B, tl=tl, zeros=tuple(zeros),
                edges=edges, branch=branch, sim=sim)


# eight runs of unequal length (and a ninth): four jobs - exactly MSM_MAX_JOBS - then a fifth made of a lone run
_RUNS8 = [(2, 12), (130, 8), (100, 17), (0, 3), (180, 11), (129, 9), (257, 1), (50, 130)]   # jobs of 20, 20, 20 and 131 terms
_RUNS9 = _RUNS8 + [(200, 17)]
# 33 terms in chunks of 8 at 70 proofs: chunks [0, 8) [8, 16) [16, 24) [24, 32) and a last chunk of one term
_ZRUNS = [(7, 20), (200, 13)]
_W64 = [(0, 50), (60, 37), (2, 26)]   # capacity 64 (130 bases): 113 terms, runs cycle through the bases (repeats are legal)
_W4 = [(0, 10), (2, 8), (0, 10), (1, 9), (0, 10), (3, 7), (0, 10), (2, 8), (0, 10), (1, 9)]   # capacity 4 (10 bases): 91 terms, five jobs


@functools.lru_cache(None)
def cases():
    c = []
    s = lambda *a, **k: c.append(_case(a[0], "small", "geo", *a[1:], **k))
    f = lambda *a, **k: c.append(_case(a[0], "fixed2", "geo", *a[1:], **k))
    # ---- small path (B <= 64)
    s("b1_t64", [(2, 64)], 1, "one full wavefront; a lone run: the job's second segment is empty", sim=True)
    s("b1_t65", [(2, 65)], 1, "a second wavefront with one live lane", sim=True)
    s("b1_t1024", [(2, 1024)], 1, "16 groups, no level")
    s("b1_t1025", [(2, 1025)], 1, "17 groups: one k_ge_reduce_wave level")
    s("b1_200_191", [(2, 120), (130, 80), (30, 100), (140, 91)], 1, "two jobs, 4 and 3 groups: one group apart, not paired", sim=True)
    s("b1_200_193", [(2, 120), (130, 80), (30, 100), (140, 93)], 1, "two jobs of 4 groups each: the launch is paired", sim=True)
    s("b1_200_60", [(2, 120), (130, 80), (30, 30), (140, 30)], 1, "unequal groups: not paired", sim=True)
    s("b1_1025_1088", [(2, 1000), (2050, 25), (1, 1088)], 1, "two jobs of 17 groups: paired launch AND paired level")
    s("b1_1025_1089", [(2, 1000), (2050, 25), (1, 1089)], 1, "17 and 18 groups, one level each: neither loop pairs them")
    s("b2_t300", [(0, 258), (0, 42)], 2, "5 groups at two proofs; on the simulator 300 sums fold 16 at a time: two levels", sim=True)
    s("b64_t4096", [(0, 4096)], 64, "chunk 1, 64 full groups per proof, one level")
    s("b64_t4097", [(0, 4097)], 64, "chunk 2 in-wave, the last chunk holds one term")
    s("b64_t8192", [(0, 4098), (0, 4094)], 64, "chunk 2 in-wave, every chunk full")
    s("b64_t8193", [(0, 4098), (0, 4095)], 64, "chunk 3: the lane kernel, two levels")
    s("b64_8193_100", [(0, 4098), (0, 4095), (10, 50), (3000, 50)], 64, "a lane-kernel job followed by an in-wave job: the launch loop and the reduction loop step differently")
    s("b3_runs8", _RUNS8, 3, "exactly MSM_MAX_JOBS jobs, the first two paired", sim=True)
    s("b3_runs9", _RUNS9, 3, "five jobs: two run_msm_multi calls, the last job a lone run", sim=True)
    s("b64_runs8", _RUNS8, 64, "exactly MSM_MAX_JOBS jobs at the widest small batch")
    s("b64_runs9", _RUNS9, 64, "five jobs at the widest small batch", sim=True)
    s("b63_t300", [(1, 150), (100, 150)], 63, "below the switch to k_msm_fixed2")
    s("b64_t300", [(1, 150), (100, 150)], 64, "the last batch of the small path", sim=True)
    # ---- k_msm_fixed2 (B >= 65)
    f("b65_t300", [(1, 150), (100, 150)], 65, "the first batch of k_msm_fixed2: a second wavefront with one live lane", sim=True)
    f("b65_t7", [(5, 7)], 65, "no bump: chunk 1, 14 workgroups padded to 16", sim=True)
    f("b65_t8", [(5, 8)], 65, "bumped to chunk 8: 2 workgroups padded to 8", sim=True)
    f("b65_t128", [(5, 100), (150, 28)], 65, "16 chunks, no level", sim=True)
    f("b65_t129", [(5, 100), (150, 29)], 65, "17 chunks: l1 = 2, a last chunk of one term", sim=True)
    f("b129_t2048", [(2, 1024), (2050, 1024)], 129, "three wavefronts per chunk, one live lane in the last; 256 chunks: l1 = 16, l2 = 0")
    f("b129_t2049", [(2, 1025), (2050, 1024)], 129, "257 chunks: l1 = 17, l2 = 2")
    f("b127_t200", [(1, 120), (170, 80)], 127, "a ragged second wavefront", sim=True)
    f("b128_t200", [(1, 120), (170, 80)], 128, "two full wavefronts on the same terms")
    f("b128_tl16_t8196", [(0, 4098), (0, 4098)], 128, "msm_threads_log2 = 16: chunk 17, 483 chunks - the un-bumped chunk", tl=16)
    f("b70_runs8", _RUNS8, 70, "four jobs of unequal length in one launch", sim=True)
    f("b70_runs9", _RUNS9, 70, "4 + 1 jobs: two launches", sim=True)
    # zero patterns at 70 proofs on chunks of 8: 'all' = every proof, 'w0' = proofs 0..63 (the first wavefront), 'not64' = every proof but 64
    f("b70_zero_term", _ZRUNS, 70, "a term that is zero for every proof, one that is zero for all but proof 64", zeros=[(3, "all"), (11, "not64")], sim=True)
    f("b70_zero_chunk_w0", _ZRUNS, 70, "a chunk that is zero for the whole first wavefront: `have` is false from the start, the identity is stored",
      zeros=[(t, "w0") for t in range(16, 24)], sim=True)
    f("b70_zero_edges", _ZRUNS, 70, "the zero term first in a chunk, last in a chunk, the only term of the last chunk (pipeline prologue / epilogue)",
      zeros=[(8, "all"), (23, "all"), (32, "all")], sim=True)
    f("b70_zero_mixed", _ZRUNS, 70, "chunk 0 zero for everyone; the one-term last chunk zero for the first wavefront only; first and last of a chunk zero for one wavefront",
      zeros=[(t, "all") for t in range(8)] + [(32, "w0"), (24, "w0"), (31, "not64")], sim=True)
    # ---- other window widths: edge scalars of the digit recoding on proofs 0, 63, 64, B - 1 at the first and last term of a chunk
    for h, runs, sim in (("w8", _W64, True), ("w11", _W64, False), ("w15", _W4, False)):
        for B in (5, 70):
            c.append(_case("%s_b%d" % (h, B), "widths", h, runs, B, "W = %d, %s" % (HANDLES[h][0], "lane kernel" if B == 5 else "k_msm_fixed2"), edges=True, sim=sim))
    assert len(set(x["name"] for x in c)) == len(c)
    return tuple(c)


def case(name):
    (c,) = [x for x in cases() if x["name"] == name]
    return c


def case_plan(c, hostsim=False):
    return plan([n for _, n in c["runs"]], c["B"], c["tl"], hostsim=hostsim)


VAR_MSM_SIZES = (1, 63, 64, 65, 129, 4095, 6143, 6144, 131073)
# the sizes the simulator's build can afford (Straus at every size there)
VAR_MSM_SIZES_SIM = (1, 63, 64, 65, 129)


# ------------------------------------------------------------------------------------------------ scalars
POOL = 1 << 14


@functools.lru_cache(None)
def _pool():
    """16384 scalars from synth_scalar, as integers and as one byte string: a proof's scalars are a window of it"""
    ints = tuple(S.synth_scalar(b"msm-geometry", i) for i in range(POOL))
    return ints, b"".join(x.to_bytes(32, "little") for x in ints)


def edge_scalars(W):
    """0, 1, l - 1, 2^252, the recoding's carry boundary (every window below the top one holds 2^(W-1): d >= entries), one below it,
    the all-ones carry chain - and the negation mod l of each"""
    nt = (252 + W) // W - 1   # windows below the top one
    half = sum((1 << (W - 1)) << (W * k) for k in range(nt))
    below = sum(((1 << (W - 1)) - 1) << (W * k) for k in range(nt))
    ones = (1 << (W * nt)) - 1
    e = [0, 1, L - 1, 1 << 252, half, below, ones]
    assert all(0 <= x < L for x in e)
    out = []
    for x in e + [(L - x) % L for x in e]:
        if x not in out:
            out.append(x)
    return out


def _zero_proofs(which, B):
    return {"all": range(B), "w0": range(min(B, WAVE)), "not64": [b for b in range(B) if b != 64]}[which]


def chunk_bounds(c):
    """[(first term, last term)] of every chunk of every job of the case, in order (device geometry)"""
    out = []
    for j in case_plan(c)["jobs"]:
        for k in range(j["nchunks"]):
            lo = j["start"] + k * j["chunk"]
            out.append((lo, min(lo + j["chunk"], j["start"] + j["total"]) - 1))
    return out


@functools.lru_cache(None)
def scalars(name):
    """-> (rows, blob): rows[b][t] the scalar of proof b, term t as an integer; blob the proof-major byte string for the call"""
    c = case(name)
    ints, raw = _pool()
    T, B = c["terms"], c["B"]
    seed = zlib.crc32(name.encode())
    offs = [(seed + 61 * b) % (POOL - T) for b in range(B)]
    if not c["zeros"] and not c["edges"]:
        return tuple(ints[o:o + T] for o in offs), b"".join(raw[32 * o:32 * (o + T)] for o in offs)
    rows = [list(ints[o:o + T]) for o in offs]
    for t, which in c["zeros"]:
        for b in _zero_proofs(which, B):
            rows[b][t] = 0
    if c["edges"]:
        E = edge_scalars(HANDLES[c["handle"]][0])
        ch = chunk_bounds(c)
        assert len(ch) >= len(E), "%s: fewer chunks than edge scalars" % name
        for k, b in enumerate(sorted(set(p % B for p in (0, 63, 64, B - 1) if p < B))):
            for i, e in enumerate(E):
                first, last = ch[(i + 5 * k) % len(ch)]
                rows[b][first] = e
                rows[b][last] = E[-1 - i] if last != first else e
    return tuple(tuple(r) for r in rows), b"".join(x.to_bytes(32, "little") for r in rows for x in r)


def weights(label, B):
    """fixed non-zero 128-bit weights of the random-combination check"""
    return [int.from_bytes(hashlib.sha512(b"msm-geometry weight" + label + b.to_bytes(4, "little")).digest()[:16], "little") | 1 for b in range(B)]


# ------------------------------------------------------------------------------------------------ expectations and checks
def handle_points(gens):
    """the compressed generators of a handle in base-index order (0 = B, 1 = B~, 2 + i = G_i, 2 + cap + i = H_i)"""
    cap = gens.capacity
    return tuple([gens.point(0), gens.point(1)] + [gens.point(2, i) for i in range(cap)] + [gens.point(3, i) for i in range(cap)])


def check_outputs(oracle, pts, rows, got, label):
    """`got`: the B encodings the library returned for sum_t rows[b][t] * pts[t].  Every proof is compared with an oracle sum of its
    own while terms x B <= 2^17; above that, proofs {0, 1, 63, 64, B - 1} are, and ALL proofs go through one random linear
    combination: sum_b r_b * got[b] == sum_t (sum_b r_b * rows[b][t]) * pts[t] (two oracle sums; a wrong output passes with
    probability about 2^-128)."""
    B, T = len(rows), len(pts)
    assert len(got) == B and all(len(r) == T for r in rows)
    if T * B <= FULL_CHECK_MAX:
        exact = range(B)
    else:
        exact = sorted(set(p % B for p in SAMPLE_PROOFS if -B <= p < B))
    for b in exact:
        assert got[b] == oracle.msm(rows[b], pts), "%s: proof %d of %d differs from the oracle" % (label, b, B)
    if len(exact) == B:
        return "full"
    for b in range(B):
        assert decompress(got[b]) is not None, "%s: output %d does not decode" % (label, b)
    r = weights(label.encode(), B)
    comb = [0] * T
    for b in range(B):
        rb, row = r[b], rows[b]
        comb = [x + rb * y for x, y in zip(comb, row)]
    assert oracle.msm(r, got) == oracle.msm([x % L for x in comb], pts), "%s: the random combination over all %d proofs differs" % (label, B)
    return "sampled"


def run_case(gens, oracle, pts, c):
    """one case of the table on the handle `gens` (whose points are `pts`); BPR1CS_OPT_MSM_THREADS_LOG2 is set for the call"""
    rows, blob = scalars(c["name"])
    gens.set_option("msm_threads_log2", -1 if c["tl"] is None else c["tl"])
    try:
        got = gens.msm_fixed(list(c["bases"]), blob, c["B"])
    finally:
        gens.set_option("msm_threads_log2", -1)
    return check_outputs(oracle, [pts[i] for i in c["bases"]], rows, got, c["name"])


def var_msm_inputs(n, pool_pts):
    """inputs of bpr1cs_msm at n terms: points cycle through `pool_pts`, edge scalars in front where there is room"""
    ints, _ = _pool()
    off = zlib.crc32(b"var%d" % n) % POOL
    sc = [ints[(off + i) % POOL] for i in range(n)]
    pts = [pool_pts[(7 * i + 3) % len(pool_pts)] for i in range(n)]
    if n >= 8:
        sc[:4] = [0, 1, L - 1, 1 << 252]
    return sc, pts


def check_var_msm(bp, lib, oracle, pool_pts, n):
    """bpr1cs_msm against the C oracle at n terms; all scalars zero must give the identity, 32 zero bytes"""
    sc, pts = var_msm_inputs(n, pool_pts)
    assert bp.msm(sc, pts, lib=lib) == oracle.msm(sc, pts), "bpr1cs_msm, n = %d" % n
    assert bp.msm([0] * n, pts, lib=lib) == bytes(32), "bpr1cs_msm of zero scalars, n = %d" % n


def check_var_msm_special(bp, lib, oracle, pool_pts, pippenger):
    """a whole chunk of zero scalars (Straus: 64 terms per chunk at n = 129) and, where the build has the Pippenger path, a zero slice
    of its three at n = 6144 and one point with one scalar 4096 times (every lane of every step votes for one bucket)"""
    ints, _ = _pool()
    sc, pts = var_msm_inputs(129, pool_pts)
    sc[64:128] = [0] * 64
    assert bp.msm(sc, pts, lib=lib) == oracle.msm(sc, pts), "bpr1cs_msm, n = 129, terms 64..127 zero"
    if not pippenger:
        return
    sc, pts = var_msm_inputs(6144, pool_pts)
    sc[2048:4096] = [0] * 2048
    assert bp.msm(sc, pts, lib=lib) == oracle.msm(sc, pts), "bpr1cs_msm, n = 6144, terms 2048..4095 zero"
    sc, pts = [ints[77]] * 4096, [pool_pts[5]] * 4096
    assert bp.msm(sc, pts, lib=lib) == oracle.msm([ints[77] * 4096 % L], [pool_pts[5]]) == oracle.msm(sc, pts), "bpr1cs_msm, 4096 copies of one term"
    assert bp.msm([0] * 4096, pts, lib=lib) == bytes(32)


def check_points_sum(bp, lib, oracle, pool_pts):
    """bpr1cs_points_sum against the oracle's sum with all-one scalars: 1, 2 and 1000 points, P next to -P, the identity's own
    encoding among the inputs, and a FormatError for an input that does not decode"""
    for n in (1, 2, 1000):
        pts = [pool_pts[(11 * i + 1) % len(pool_pts)] for i in range(n)]
        assert bp.points_sum(pts, lib=lib) == oracle.msm([1] * n, pts), "bpr1cs_points_sum of %d points" % n
    P, Q = pool_pts[9], pool_pts[10]
    negP = oracle.msm([L - 1], [P])
    assert negP != P and decompress(negP) is not None
    assert bp.points_sum([P, negP], lib=lib) == bytes(32)
    assert bp.points_sum([P, Q, negP], lib=lib) == Q
    assert bp.points_sum([bytes(32)], lib=lib) == bytes(32)
    assert bp.points_sum([bytes(32), P, bytes(32), Q], lib=lib) == oracle.msm([1, 1], [P, Q])
    for bad in ([b"\xff" * 32], [P, Q, b"\x01" + bytes(31), P]):   # s >= p; a negative s
        assert decompress(bad[-2 if len(bad) > 1 else 0]) is None
        try:
            bp.points_sum(bad, lib=lib)
        except bp.R1CSError as e:
            assert e.code == -2, e
        else:
            raise AssertionError("bpr1cs_points_sum accepted an input that does not decode")


def check_commit_switch(bp, gens, oracle, pts):
    """the two-term commitment shape of bpr1cs_msm_fixed (bases B, B~) on both sides of the wavefront-per-commitment limit"""
    lim = constants()["COMMIT_WAVE_MAX"]
    ints, _ = _pool()
    edge = [(0, 0), (1, 0), (0, 1), (L - 1, L - 1), (1 << 252, (1 << 252) - 1)]
    pairs = edge + [(ints[2 * i], ints[2 * i + 1]) for i in range(lim + 1 - len(edge))]
    pairs[lim - 1], pairs[lim] = (L - 1, 1), (ints[7], 0)   # the last commitment of either form
    exp = [oracle.msm(list(p), [pts[0], pts[1]]) for p in pairs]
    blob = b"".join(v.to_bytes(32, "little") + r.to_bytes(32, "little") for v, r in pairs)
    for B in (lim, lim + 1):
        assert gens.msm_fixed([0, 1], blob[:64 * B], B) == exp[:B], "commitments, batch %d" % B


# ------------------------------------------------------------------------------------------------ coverage
def coverage():
    """-> (facts, missing): what the case table reaches under plan(), and the branches of the issue's list it does not"""
    K = constants()
    jobs, calls = [], set()
    for c in cases():
        p = case_plan(c)
        calls.add(p["calls"])
        for j in p["jobs"]:
            jobs.append(dict(j, B=c["B"], case=c["name"], njobs_in_call=sum(1 for x in p["jobs"] if x["call"] == j["call"])))
    sm = [j for j in jobs if j["path"] == "small"]
    f2 = [j for j in jobs if j["path"] == "fixed2"]
    G, LP, WC = K["REDUCE_GROUP"], K["LANE_PATH_MAX_PROOFS"], K["WAVE_REDUCE_MAX_CHUNK"]
    want = {
        "path small": bool(sm), "path fixed2": bool(f2),
        "batch on both sides of MSM_LANE_PATH_MAX_PROOFS": {LP, LP + 1} <= {j["B"] for j in jobs},
        "in_wave true": any(j["in_wave"] for j in sm), "in_wave false": any(not j["in_wave"] for j in sm),
        "chunk on both sides of MSM_WAVE_REDUCE_MAX_CHUNK": {WC, WC + 1} <= {j["chunk"] for j in sm},
        "in-wave chunk with a short last chunk": any(j["in_wave"] and j["chunk"] > 1 and j["last_chunk"] < j["chunk"] for j in sm),
        "nl = 0": any(j["nl"] == 0 for j in sm), "nl = 1": any(j["nl"] == 1 for j in sm), "nl = 2": any(j["nl"] == 2 for j in sm),
        "groups on both sides of MSM_REDUCE_GROUP (small)": {G, G + 1} <= {j["groups"] for j in sm},
        "one full wavefront, then one live lane in the next": {(1, WAVE), (2, 1)} <= {(j["groups"], j["last_group"]) for j in sm if j["in_wave"]},
        "ragged last group at a level": any(j["nl"] and j["groups"] % K["SMALL_REDUCE_GROUP"][1] for j in sm),
        "full last group at a level": any(j["nl"] and j["groups"] % K["SMALL_REDUCE_GROUP"][1] == 0 for j in sm),
        "one level folds more than MSM_REDUCE_GROUP sums into one": any(j["lv"] == (1,) and j["groups"] > G for j in sm),
        "launch loop paired": any(j["launch_paired"] for j in sm),
        "launch loop unpaired next to a neighbour": any(not j["launch_paired"] and j["njobs_in_call"] > 1 for j in sm),
        "launch loop unpaired, both in-wave, groups one apart": any(not a["launch_paired"] and a["in_wave"] and b["in_wave"] and abs(a["groups"] - b["groups"]) == 1
                                                                    for a, b in zip(sm, sm[1:]) if a["case"] == b["case"] and a["call"] == b["call"]),
        "lane-kernel job next to an in-wave job": any(not a["in_wave"] and b["in_wave"] for a, b in zip(sm, sm[1:]) if a["case"] == b["case"] and a["call"] == b["call"]),
        "reduction loop paired": any(j["reduce_paired"] for j in sm),
        "reduction loop unpaired with levels": any(not j["reduce_paired"] and j["nl"] > 0 for j in sm),
        "reduction loop unpaired with levels next to a neighbour": any(not j["reduce_paired"] and j["nl"] > 0 and j["njobs_in_call"] > 1 for j in sm),
        "run_msm_multi calls = 1": 1 in calls, "run_msm_multi calls = 2": 2 in calls,
        "exactly MSM_MAX_JOBS jobs in a call (small)": any(j["njobs_in_call"] == K["MAX_JOBS"] for j in sm),
        "exactly MSM_MAX_JOBS jobs in a call (fixed2)": any(j["njobs_in_call"] == K["MAX_JOBS"] for j in f2),
        "lone-run job (small)": any(j["lone"] for j in sm), "lone-run job (fixed2)": any(j["lone"] for j in f2),
        "lone-run job alone in a second call": any(j["lone"] and j["call"] == 1 and j["njobs_in_call"] == 1 for j in jobs),
        "l1 = 0": any(j["l1"] == 0 for j in f2), "l1 > 0": any(j["l1"] > 0 for j in f2),
        "l2 = 0 with l1 > 0": any(j["l2"] == 0 and j["l1"] > 0 for j in f2), "l2 > 0": any(j["l2"] > 0 for j in f2),
        "chunks on both sides of MSM_REDUCE_GROUP (fixed2)": {G, G + 1} <= {j["nchunks"] for j in f2},
        "l1 on both sides of MSM_REDUCE_GROUP": {G, G + 1} <= {j["l1"] for j in f2},
        "bumped chunk": any(j["bumped"] for j in f2),
        "un-bumped chunk above the bump": any(not j["bumped"] and j["chunk"] >= K["BUMP_IF"][0] for j in f2),
        "total below the bump": any(j["below_bump"] and not j["bumped"] for j in f2),
        "total on both sides of the bump": {K["BUMP_IF"][1] - 1, K["BUMP_IF"][1]} <= {j["total"] for j in f2},
        "one-term last chunk (fixed2)": any(j["last_chunk"] == 1 and j["nchunks"] > 1 for j in f2),
        "nwg padded": any(j["padded"] for j in f2), "nwg not padded": any(not j["padded"] for j in f2),
        "nbk = 2 with a ragged last wavefront": any(j["nbk"] == 2 and j["live_last"] < WAVE for j in f2),
        "nbk = 3 with a ragged last wavefront": any(j["nbk"] == 3 and j["live_last"] < WAVE for j in f2),
        "one live lane in the last wavefront": any(j["live_last"] == 1 for j in f2),
        "nbk = 2 with full wavefronts": any(j["nbk"] == 2 and j["live_last"] == WAVE for j in f2),
        "msm_threads_log2 at its lower clamp": any(c["tl"] == K["THREADS_LOG2_CLAMP"][1] for c in cases()),
    }
    vm = {n: plan_msm(n) for n in VAR_MSM_SIZES}
    sw, (ccap, per) = K["VAR_PIPPENGER_FROM"], K["VAR_PIPPENGER_CHUNKS"]
    want.update({
        "bpr1cs_msm: Straus with 1, 2 and 3 chunks": {1, 2, 3} <= {v["chunks"] for v in vm.values() if v["path"] == "straus"},
        "bpr1cs_msm: 64 and 65 terms (one chunk, then two)": vm.get(64, {}).get("chunks") == 1 and vm.get(65, {}).get("chunks") == 2,
        "bpr1cs_msm: the largest Straus size": sw - 1 in vm and vm[sw - 1]["path"] == "straus" and vm[sw - 1]["chunks"] == K["VAR_STRAUS"][1],
        "bpr1cs_msm: Pippenger with 2 chunks, then 3": 3 * per - 1 in vm and 3 * per in vm and vm[3 * per - 1]["chunks"] == 2 and vm[3 * per]["chunks"] == 3,
        "bpr1cs_msm: the chunk cap with a ragged last chunk": any(v["path"] == "pippenger" and v["capped"] and v["last"] < v["per"] for v in vm.values()),
    })
    return jobs, sorted(k for k, v in want.items() if not v)
