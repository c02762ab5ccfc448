"""The launch geometry of the multiscalar-multiplication entry points (tests/msm_cases.py), without a GPU:

  * the plan - a plain-Python mirror of run_msm_multi's arithmetic whose constants are read from the sources - gives the geometry
    worked out by hand for the table's cases, and the table reaches every branch and both sides of every threshold under it;
  * the cases the simulator can afford run against the CPU build of the same host code and of msm_fixed2_body, with the
    expectations of the device file (the C oracle).  For batches above 64 proofs the simulator's recorder (csrc/msm_trace.hpp) also
    pins what outputs cannot show: the workgroups of every launch against the plan, the table loads against the wave votes
    worked out from the scalars (a term that is zero for a whole wavefront is skipped by ALL its lanes, any other by none), and
    for the smallest cases every table slot every lane loads, in order (which proof a spare lane of a ragged wavefront repeats)."""
import ctypes
import os
import subprocess

import pytest

import common
import msm_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bp = common.bp


@pytest.fixture(scope="module")
def oracle():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "c")])
    from cref import COracle
    return COracle()


@pytest.fixture(scope="module")
def handles(sim_lib):
    """one simulator handle per (window bits, capacity), made when a case first asks for it -> (gens, its points)"""
    made = {}

    def get(name):
        if name not in made:
            W, cap = M.SIM_HANDLES[name]
            g = bp.Gens(cap, lib=sim_lib, window_bits=W)
            assert g.table_info()["window_bits"] == W
            made[name] = (g, M.handle_points(g))
        return made[name]
    yield get
    for g, _ in made.values():
        g.close()


# ------------------------------------------------------------------------------------------------ the plan
def test_constants_are_read_from_the_sources():
    K = M.constants()
    assert set(K) == set(M._PATTERNS)
    assert all(isinstance(v, int) or (isinstance(v, tuple) and all(isinstance(x, int) for x in v)) for v in K.values())


def _jobs(name, **kw):
    return M.case_plan(M.case(name), **kw)["jobs"]


def test_plan_gives_the_geometry_worked_out_by_hand():
    """the figures of the case table's descriptions, worked out from csrc/msm_run.hpp at its present constants"""
    has = lambda name, **kv: all(_jobs(name)[0][k] == v for k, v in kv.items()) or pytest.fail("%s: %r, expected %r" % (name, _jobs(name)[0], kv))
    has("b1_t64", path="small", chunk=1, nchunks=64, in_wave=True, groups=1, last_group=64, nl=0, lone=True)
    has("b1_t65", groups=2, last_group=1, nl=0)
    has("b1_t1024", groups=16, nl=0, out_chunks=16)
    has("b1_t1025", groups=17, lv=(1,), first_off=1, out_chunks=1)
    has("b64_t4096", chunk=1, in_wave=True, groups=64, lv=(1,))
    has("b64_t4097", chunk=2, nchunks=2049, in_wave=True, last_chunk=1, groups=33, last_group=1)
    has("b64_t8192", chunk=2, nchunks=4096, in_wave=True, last_chunk=2, groups=64)
    has("b64_t8193", chunk=3, nchunks=2731, in_wave=False, groups=2731, lv=(43, 1), first_off=44, need=(2731 + 44) * 64)
    has("b63_t300", path="small")
    has("b64_t300", path="small")
    has("b65_t300", path="fixed2", nbk=2, live_last=1)
    has("b65_t7", chunk=1, nchunks=7, bumped=False, nwg_raw=14, nwg=16, l1=0)
    has("b65_t8", chunk=8, nchunks=1, bumped=True, nwg_raw=2, nwg=8)
    has("b65_t128", chunk=8, nchunks=16, l1=0, l2=0, padded=False)
    has("b65_t129", nchunks=17, l1=2, l2=0, last_chunk=1, out_chunks=2)
    has("b129_t2048", nbk=3, live_last=1, nchunks=256, l1=16, l2=0)
    has("b129_t2049", nchunks=257, l1=17, l2=2, out_chunks=2)
    has("b127_t200", nbk=2, live_last=63)
    has("b128_t200", nbk=2, live_last=64)
    has("b128_tl16_t8196", chunk=17, nchunks=483, bumped=False, l1=31, l2=2)
    j = _jobs("b1_200_191")
    assert [(x["groups"], x["launch_paired"]) for x in j] == [(4, False), (3, False)]
    j = _jobs("b1_200_193")
    assert [(x["groups"], x["launch_paired"], x["reduce_paired"]) for x in j] == [(4, True, False)] * 2
    j = _jobs("b1_1025_1088")
    assert [(x["groups"], x["launch_paired"], x["reduce_paired"], x["lone"]) for x in j] == [(17, True, True, False), (17, True, True, True)]
    j = _jobs("b64_8193_100")
    assert [(x["in_wave"], x["nl"], x["launch_paired"], x["reduce_paired"]) for x in j] == [(False, 2, False, False), (True, 0, False, False)]
    for b in (3, 64, 70):
        p8, p9 = M.case_plan(M.case("b%d_runs8" % b)), M.case_plan(M.case("b%d_runs9" % b))
        assert (p8["calls"], len(p8["jobs"])) == (1, 4) and (p9["calls"], len(p9["jobs"])) == (2, 5)
        assert p9["jobs"][4]["lone"] and p9["jobs"][4]["call"] == 1 and [x["total"] for x in p9["jobs"]] == [20, 20, 20, 131, 17]
    assert M.case_plan(M.case("b70_runs9"))["nwg"] == [56, 8]   # (3 + 3 + 3 + 17) chunks x 2 wavefronts = 52 -> 56; 3 x 2 = 6 -> 8
    assert [(x["nchunks"], x["l1"]) for x in _jobs("b70_runs8")] == [(3, 0), (3, 0), (3, 0), (17, 2)]
    assert [x["launch_paired"] for x in _jobs("b3_runs8")] == [True, True, False, False]
    # the simulator's build: no wavefront kernels, sixteen sums per level
    assert [(x["in_wave"], x["groups"], x["lv"]) for x in _jobs("b1_t1025", hostsim=True)] == [(False, 1025, (65, 5))]
    assert [(x["groups"], x["lv"]) for x in _jobs("b2_t300", hostsim=True)] == [(300, (19, 2))] and [(x["groups"], x["nl"]) for x in _jobs("b2_t300")] == [(5, 0)]
    # (the same two loops decide there: never a paired launch - no job is in-wave -, a paired level where two neighbours have the same levels)
    assert [(x["groups"], x["lv"], x["launch_paired"], x["reduce_paired"]) for x in _jobs("b3_runs8", hostsim=True)] == \
        [(20, (2,), False, True), (20, (2,), False, True), (20, (2,), False, False), (131, (9,), False, False)]
    assert not any(x["launch_paired"] or x["reduce_paired"] for x in _jobs("b1_1025_1088", hostsim=True))   # (1025 and 1088 sums: not one shape)
    # chunks of 8 at 70 proofs: what the zero patterns are placed on
    assert M.chunk_bounds(M.case("b70_zero_term")) == [(0, 7), (8, 15), (16, 23), (24, 31), (32, 32)]
    assert [M.plan_msm(n)["chunks"] for n in M.VAR_MSM_SIZES] == [1, 1, 1, 2, 3, 64, 2, 3, 64]
    assert M.plan_msm(131073) == dict(path="pippenger", chunks=64, capped=True, per=2049, last=1986)


def test_case_table_reaches_every_branch_and_both_sides_of_every_threshold():
    jobs, missing = M.coverage()
    assert not missing, "no case of tests/msm_cases.py reaches: %s" % "; ".join(missing)
    # every case's scalars obey its recipe (the zero patterns are where the plan's chunks are)
    for c in M.cases():
        if c["zeros"]:
            rows, _ = M.scalars(c["name"])
            for t, which in c["zeros"]:
                zero = set(M._zero_proofs(which, c["B"]))
                assert all((rows[b][t] == 0) == (b in zero) for b in range(c["B"])), (c["name"], t)


@pytest.mark.parametrize("name, value", [("LANE_PATH_MAX_PROOFS", 32), ("WAVE_REDUCE_MAX_CHUNK", 1), ("REDUCE_GROUP", 32), ("SMALL_REDUCE_GROUP", (16, 16)),
                                         ("BUMP_IF", (4, 4)), ("MAX_JOBS", 8), ("THREADS_LOG2_DEFAULT", 12), ("VAR_PIPPENGER_CHUNKS", (64, 1024)),
                                         ("SMALL_THREADS_LOG2", 16)])
def test_a_changed_constant_fails_the_coverage_check(monkeypatch, name, value):
    """the reason the constants are read from the sources: with another threshold the table no longer straddles it, and the
    coverage check says so instead of the sweep going quietly blind"""
    K = dict(M.constants())
    K[name] = value
    if name == "BUMP_IF":
        K["BUMP_TO"] = (4, 3, 4)
    if name == "THREADS_LOG2_DEFAULT":
        K["THREADS_LOG2_CLAMP"] = (12, 10, 10, 26, 26)
    monkeypatch.setattr(M, "constants", lambda: K)
    assert M.coverage()[1], "changing %s left every branch covered: the check does not see that constant" % name


# ------------------------------------------------------------------------------------------------ the simulator
_M64 = (1 << 64) - 1
TABLE, VOTE, GRID = 1, 5, 6   # csrc/msm_trace.hpp


def _trace_hash(values):
    h = 0
    for v in values:
        h = ((h ^ v) * 0x9e3779b97f4a7c15) & _M64
        h ^= h >> 29
    return h


def _recorded(lib, fn):
    lib.bpr1cs_sim_msm_trace.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    lib.bpr1cs_sim_msm_trace.restype = None
    buf = (ctypes.c_uint64 * 16)()
    lib.bpr1cs_sim_msm_trace(1, None)
    try:
        res = fn()
    finally:
        lib.bpr1cs_sim_msm_trace(0, buf)
    return res, list(buf)[:7], list(buf)[7:14]


def _expected_votes(c):
    """-> (terms a lane looks at, terms it walks) summed over the workgroups of the case: a term is walked by a wavefront iff one
    of its proofs has a non-zero scalar for it"""
    rows, _ = M.scalars(c["name"])
    B, seen, live = c["B"], 0, 0
    for j in M.case_plan(c)["jobs"]:
        for k in range(j["nchunks"]):
            lo = j["start"] + k * j["chunk"]
            hi = min(lo + j["chunk"], j["start"] + j["total"])
            for w in range(j["nbk"]):
                proofs = range(64 * w, min(64 * w + 64, B))
                seen += hi - lo
                live += sum(1 for t in range(lo, hi) if any(rows[b][t] for b in proofs))
    return seen, live


def _digits(x, W):
    """csrc/kernels.hpp tab_digit: the signed digits of a canonical scalar, the top window keeps its value"""
    windows, entries, out, carry = (252 + W) // W, 1 << (W - 1), [], 0
    for k in range(windows):
        d = ((x >> (k * W)) & ((1 << W) - 1)) + carry
        carry = 1 if k + 1 < windows and d >= entries else 0
        out.append(d - (carry << W))
    return out


def _expected_table_hash(c, W, stride=128):
    """the table slots the lanes of a k_msm_fixed2 case load, in the simulator's order: launch by launch, workgroup by workgroup as
    launched (the XCD remap decides which chunk a workgroup is), lane by lane - a spare lane of a ragged wavefront repeats the LAST
    proof - and per lane every term its wavefront walks, window by window.  A slot is a byte offset into the table:
    base x base_bytes + window x row bytes + |digit| x stride."""
    rows, _ = M.scalars(c["name"])
    B, windows, row = c["B"], (252 + W) // W, (1 << (W - 1)) + 1
    K = M.constants()
    p = M.case_plan(c)
    ev = []
    for call in range(p["calls"]):
        jobs = [j for j in p["jobs"] if j["call"] == call]
        nwg = jobs[0]["nwg"]
        for raw in range(nwg):
            wg = (raw & K["XCD_REMAP"][1]) * (nwg >> K["XCD_REMAP"][2]) + (raw >> K["XCD_REMAP"][3]) if nwg & K["XCD_REMAP"][0] == 0 else raw
            if wg >= jobs[-1]["wg_end"]:
                continue
            j = [x for x in jobs if wg < x["wg_end"]][0]
            wg -= j["wg_end"] - j["nchunks"] * j["nbk"]
            k, w = wg // j["nbk"], wg % j["nbk"]
            lo = j["start"] + k * j["chunk"]
            terms = range(lo, min(lo + j["chunk"], j["start"] + j["total"]))
            proofs = [min(64 * w + l, B - 1) for l in range(64)]
            live = [t for t in terms if any(rows[b][t] for b in proofs)]
            for b in proofs:
                for t in live:
                    base = c["bases"][t] * windows * row * stride
                    ev += [base + (kk * row + abs(d)) * stride for kk, d in enumerate(_digits(rows[b][t], W))]
    return len(ev), _trace_hash(ev)


SIM_CASES = [c["name"] for c in M.cases() if c["sim"]]
TABLE_HASH_MAX_TERMS = 40   # the cases small enough to restate every table load of in Python


@pytest.mark.parametrize("name", SIM_CASES)
def test_fixed_base_cases_on_the_simulator(sim_lib, oracle, handles, name):
    c = M.case(name)
    gens, pts = handles(c["handle"])
    how, count, hsh = _recorded(sim_lib, lambda: M.run_case(gens, oracle, pts, c))
    assert how == "full" or c["terms"] * c["B"] > M.FULL_CHECK_MAX
    if c["B"] > M.constants()["LANE_PATH_MAX_PROOFS"]:
        p = M.case_plan(c)
        assert count[GRID] == p["calls"] and hsh[GRID] == _trace_hash(p["nwg"]), "the launches are not the plan's: %r" % (p["nwg"],)
        seen, live = _expected_votes(c)
        windows = gens.table_info()["windows"]
        assert count[VOTE] == 64 * seen
        assert count[TABLE] == 64 * windows * live, "table loads: a wavefront walks a term iff one of ITS proofs has a non-zero scalar"
        if c["terms"] <= TABLE_HASH_MAX_TERMS:
            assert (count[TABLE], hsh[TABLE]) == _expected_table_hash(c, gens.table_info()["window_bits"]), \
                "the sequence of table slots loaded: chunk of a workgroup, proof of a lane (spare lanes repeat the last one), digit recoding"


def test_variable_base_points_sum_and_commitments_on_the_simulator(sim_lib, oracle, handles):
    """bpr1cs_msm at the sizes the simulator can afford (Straus there at every size), bpr1cs_points_sum, and the two-term
    commitment shape at 256 and 257 commitments (one functor on the simulator; the device file meets the two kernels)"""
    gens, pts = handles("w8")
    for n in M.VAR_MSM_SIZES_SIM:
        M.check_var_msm(bp, sim_lib, oracle, pts, n)
    M.check_var_msm_special(bp, sim_lib, oracle, pts, pippenger=False)
    M.check_points_sum(bp, sim_lib, oracle, pts)
    M.check_commit_switch(bp, gens, oracle, pts)
