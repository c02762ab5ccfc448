"""Grouped batch verification with BPR1CS_OPT_VERIFY_GROUP_FALLBACK = 2 - bad proofs found by bisection on the device (include/bpr1cs.h;
DESIGN.md §5.53): the case table, a Python mirror of the split rule and one checker, shared by the CPU simulator
(tests/test_verify_bisect.py) and the device (tests/test_gpu_verify_bisect.py).  Built on tests/verify_group_cases.py (proofs made once per
library, the default handle, the handle with the options).

The reference of every case is the per-proof path on a handle whose options are at their defaults; mode 2 must return that list,
and so must mode 1.  A wrong range sum, a wrong subtraction or a malformed proof that is not left out of a sum turns into a wrong
verdict for a good or a bad proof.

Shapes: the smallest at which the new code can go wrong - one group with the odd splits 5/4, 3/2, 2/1 (B = 9, G = 64); groups 4, 4
and a lone proof; G = 3; G = 2 (ranges of one straight away); B <= 8 (transcripts replayed on the host); a group of 70 (a lane of the
combining wavefront takes two proofs); N = 1 (no inner-product rounds); and B = 141, G = 2 with every even proof tampered - 70 ranges
at depth 1, more than the lane / wavefront paths of the MSM and of the range finish take (64)."""
import verify_group_cases as VG

bp = VG.bp
T_X, T_XB, flip, seed_sets = VG.T_X, VG.T_XB, VG.flip, VG.seed_sets
BISECT = 2

# name -> (proofs, B, G)
CASES = {
    "b9_g64": ("bound", 9, 64),        # one group: splits 5/4, 3/2, 2/1
    "b9_g4": ("bound", 9, 4),          # groups 4, 4 and a lone proof
    "b9_g3": ("bound", 9, 3),
    "b9_g2": ("bound", 9, 2),          # ranges of one straight away
    "b6_g4": ("bound", 6, 4),          # host transcript replay
    "b141_g70": ("bound", 141, 70),    # a lane takes two proofs
    "factors_b5_g2": ("factors", 5, 2),      # N = 1
    "b141_g2": ("bound", 141, 2),      # every even proof tampered: 70 ranges at depth 1
}


# ---- the split rule (csrc/api_verify.hpp verify_batch_bisect_once), `bad` = the well-formed but invalid proofs
def cols(lo, hi, bad):
    """MSM columns spent below a range [lo, hi) whose own sum is known"""
    if hi - lo == 1 or not any(lo <= b < hi for b in bad):
        return 0
    mid = lo + (hi - lo + 1) // 2
    return 1 + cols(lo, mid, bad) + cols(mid, hi, bad)


def groups(B, G):
    return [(lo, min(lo + G, B)) for lo in range(0, B, G)]


def columns_per_depth(B, G, bad):
    """[NG, ranges tested at depth 1, at depth 2 ...]: a depth tests the left half of every failing range of more than one proof"""
    out, cur = [len(groups(B, G))], groups(B, G)
    while True:
        cur = [(lo, hi) for lo, hi in cur if hi - lo > 1 and any(lo <= b < hi for b in bad)]
        if not cur:
            break
        out.append(len(cur))
        cur = [r for lo, hi in cur for r in ((lo, lo + (hi - lo + 1) // 2), (lo + (hi - lo + 1) // 2, hi))]
    assert sum(out) == total_columns(B, G, bad)
    return out


def total_columns(B, G, bad):
    return len(groups(B, G)) + sum(cols(lo, hi, bad) for lo, hi in groups(B, G))


def check_mirror():
    """the arithmetic of DESIGN.md §5.53: 4096 proofs, G = 64, 40 bad proofs in 40 groups -> 64 + 40 * 6 columns"""
    assert total_columns(4096, 64, {64 * i + 17 for i in range(40)}) == 64 + 40 * 6
    assert columns_per_depth(9, 64, {4}) == [1, 1, 1, 1]           # [0,9) -> [0,5) -> [3,5) -> 3 | 4
    assert columns_per_depth(9, 64, {0}) == [1, 1, 1, 1, 1]        # [0,9) -> [0,5) -> [0,3) -> [0,2) -> 0 | 1
    assert columns_per_depth(9, 64, set(range(9))) == [1, 1, 2, 4, 1]
    assert columns_per_depth(9, 2, {8}) == [5] and columns_per_depth(9, 2, {0, 3}) == [5, 2]


# ---- the checker
def check(e, name, P, C, rejected, seeds=None, mode1=True):
    """mode 2 (and mode 1) on the proofs P / commitments C of case `name` against the per-proof path on the default handle, which
    itself must reject exactly `rejected`"""
    kind, B, G = CASES[name]
    assert len(P) == B
    seeds = seeds if seeds is not None else seed_sets(B)[0]
    want = e.reference(kind, P, C, seeds)
    assert want == [b not in rejected for b in range(B)], "the per-proof path itself"
    got = e.grouped(kind, P, C, G, BISECT, seeds)
    assert got == want, "%s fallback 2: rejected %r, expected %r" % (name, [b for b in range(B) if not got[b]], sorted(rejected))
    if mode1:
        assert e.grouped(kind, P, C, G, 1, seeds) == want, "%s fallback 1" % name


def tampered(e, name, bad):
    """-> (P, C) of the case with the proofs `bad` tampered (t_x or t_x_blinding, alternating: both stay canonical scalars)"""
    kind, B, G = CASES[name]
    b = e.batch(kind, B)
    P = b["P"][:B]
    for i, pos in enumerate(sorted(bad)):
        P[pos] = flip(P[pos], T_X + 3) if i % 2 == 0 else flip(P[pos], T_XB + 5, 4)
    return P, b["C"][:B]


def check_tampered(e, name, bad, all_seeds=False, mode1=True):
    P, C = tampered(e, name, bad)
    for seeds in seed_sets(CASES[name][1])[:3 if all_seeds else 1]:
        check(e, name, P, C, set(bad), seeds=seeds, mode1=mode1)


def check_every_single_position(e, name):
    for pos in range(CASES[name][1]):
        check_tampered(e, name, {pos}, mode1=False)


malformed_forms = VG.malformed_forms


def check_malformed(e, name, pos, also_tampered=()):
    """proof `pos` malformed in each of the three forms, alone among good proofs or together with tampered proofs"""
    P, C = tampered(e, name, set(also_tampered))
    for broken in malformed_forms(P[pos]):
        check(e, name, P[:pos] + [broken] + P[pos + 1:], C, {pos} | set(also_tampered))


def check_swapped_commitment(e, name):
    """the first commitment of proof 0 and of the first proof of the second group exchanged: one bad proof in each of two groups"""
    kind, B, G = CASES[name]
    b = e.batch(kind, B)
    C = [list(c) for c in b["C"][:B]]
    C[0][0], C[G][0] = C[G][0], C[0][0]
    for seeds in seed_sets(B):
        check(e, name, b["P"][:B], C, {0, G}, seeds=seeds)
