"""Device arithmetic headers (field, scalars, ristretto, Keccak/STROBE/Merlin) compiled for the
host and compared with the oracle's big-integer arithmetic."""
import ctypes
import random

from pyref.ed import P, L, BASEPOINT, from_uniform_bytes
from pyref.merlin import Transcript
from pyref.ed import sc_to_bytes

import prim_cases as pc
from prim_cases import N, FP, val


def _call(f, *ins, n=32):
    o = ctypes.create_string_buffer(n)
    r = f(*ins, o)
    return o.raw, r


def test_field_and_scalar_arithmetic(prim_lib):
    vals = pc.vals()
    for a in vals:
        ia = int.from_bytes(a, "little")
        for b in vals[:20]:
            ib = int.from_bytes(b, "little")
            for f, op, mod in ((prim_lib.hs_fe_mul, ia * ib, P), (prim_lib.hs_fe_add, ia + ib, P), (prim_lib.hs_fe_sub, ia - ib, P),
                               (prim_lib.hs_sc_mul, ia * ib, L), (prim_lib.hs_sc_add, ia + ib, L), (prim_lib.hs_sc_sub, ia - ib, L)):
                assert int.from_bytes(_call(f, a, b)[0], "little") == op % mod
        assert int.from_bytes(_call(prim_lib.hs_fe_inv, a)[0], "little") == pow(ia % P, P - 2, P)
        assert int.from_bytes(_call(prim_lib.hs_fe_sq, a)[0], "little") == ia * ia % P
        inv = pow(ia % L, L - 2, L)
        assert int.from_bytes(_call(prim_lib.hs_sc_inv, a)[0], "little") == inv          # safegcd divsteps
        assert int.from_bytes(_call(prim_lib.hs_sc_inv_fermat, a)[0], "little") == inv   # Fermat ladder
        assert int.from_bytes(_call(prim_lib.hs_sc_inv_var, a)[0], "little") == inv      # variable-time divsteps (public values)


def test_variable_time_inverse_on_many_values(prim_lib):
    for x in pc.inv_var_values():
        got = int.from_bytes(_call(prim_lib.hs_sc_inv_var, x.to_bytes(32, "little"))[0], "little")
        assert got == (pow(x, L - 2, L) if x else 0), hex(x)


def test_group_and_encoding(prim_lib):
    for c in pc.group_cases():
        assert int.from_bytes(_call(prim_lib.hs_sc_wide, c["wide"])[0], "little") == c["wide_mod_l"]
        assert _call(prim_lib.hs_uniform, c["wide"])[0] == c["uniform"]
        assert _call(prim_lib.hs_basemul, c["k"])[0] == c["p"]
        out, ok = _call(prim_lib.hs_decompress_recompress, c["p"])
        assert ok and out == c["p"]
        o4, ok = _call(prim_lib.hs_addsub, c["p"], c["q"], n=128)
        assert ok and o4 == c["addsub"]
    assert _call(prim_lib.hs_decompress_recompress, b"\x01" + bytes(31))[1] == 0


def test_encodings_accepted_and_rejected_as_the_oracle_does(prim_lib):
    """ge_decompress on the directed encodings of prim_cases.encoding_cases (canonicity, sign of s, non-squares, t < 0,
    y = 0): the flag is the oracle's verdict, and an accepted string recompresses to itself."""
    cases = pc.encoding_cases()
    assert sum(ok for _, ok in cases) >= 81 and sum(not ok for _, ok in cases) >= 100
    for e, want in cases:
        out, ok = _call(prim_lib.hs_decompress_recompress, e)
        assert bool(ok) == want, e.hex()
        if want:
            assert out == e, e.hex()


def test_merlin_transcript_and_rng(prim_lib):
    assert _call(prim_lib.hs_merlin_kat)[0].hex() == "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"
    rnd = random.Random(11)
    msgs = bytes(rnd.getrandbits(8) for _ in range(5 * 32))
    seed = bytes(rnd.getrandbits(8) for _ in range(32))
    dr, ch = ctypes.create_string_buffer(32 * 300), ctypes.create_string_buffer(32)
    prim_lib.hs_merlin_script(b"VSMT", 4, msgs, 5, seed, 300, dr, ch)
    t = Transcript(b"VSMT")
    for i in range(5):
        t.append_message(b"V", msgs[32 * i:32 * i + 32])
    t.append_u64(b"m", 5)
    b = t.build_rng()
    for i in range(5):
        b = b.rekey_with_witness_bytes(b"v_blinding", msgs[32 * i:32 * i + 32])
    rng = b.finalize(seed)
    assert dr.raw == b"".join(sc_to_bytes(rng.random_scalar()) for _ in range(300))
    assert ch.raw == sc_to_bytes(t.challenge_scalar(b"y"))


I9, I27, I36 = ctypes.c_int32 * 9, ctypes.c_int32 * 27, ctypes.c_int32 * 36


def _mul_exact_within(f, a, b, lo, hi):
    out, ol = (ctypes.c_uint8 * 32)(), I9()
    f(I9(*a), I9(*b), out, ol)
    assert int.from_bytes(bytes(out), "little") == val(a) * val(b) % P, (a, b)
    assert min(ol) >= lo and max(ol) <= hi, (a, b, list(ol))


def _sq_exact_within_n(prim_lib, a):
    out, ol = (ctypes.c_uint8 * 32)(), I9()
    prim_lib.hs_fe_sq_limbs(I9(*a), out, ol)
    assert int.from_bytes(bytes(out), "little") == val(a) ** 2 % P, a
    assert max(abs(x) for x in ol) <= N, (a, list(ol))


def test_field_limb_bounds(prim_lib):
    """9x29 signed-limb field (csrc/fe.hpp): worst-case limb classes of every product shape used in ge.hpp
    (N*N, 2N*2N, 2N*3N, 3N*3N, 3N*4N, 2N*4N; squares up to 2N) stay exact and return limbs within N."""
    mul, sq, carry = pc.field_limb_cases()
    assert len(mul) == 7 * 44 * 12 and len(sq) == 44 and len(carry) == 5 * 44
    out, ol = (ctypes.c_uint8 * 32)(), I9()
    for a, b in mul:
        _mul_exact_within(prim_lib.hs_fe_mul_limbs, a, b, -N, N)
    for a in sq:
        _sq_exact_within_n(prim_lib, a)
    for a in carry:
        prim_lib.hs_fe_canon_limbs(I9(*a), out)
        assert int.from_bytes(bytes(out), "little") == val(a)
        prim_lib.hs_fe_carry_limbs(I9(*a), ol)
        assert val(list(ol)) == val(a) and max(abs(x) for x in ol) <= N
    # canonical edge values
    for v in pc.CANON_EDGE:
        prim_lib.hs_fe_canon_limbs(I9(*pc.limbs_of(v)), out)
        assert int.from_bytes(bytes(out), "little") == v % P


def test_remainder_word_extremes(prim_lib):
    """Single-limb operands whose one non-zero column sum ends in 0x00000000, 0x7fffffff, 0x80000000 or 0xffffffff, for both
    signs of the sum: the word pass 1 hands to the unsigned multiply-add of pass 2 (and column 8's own remainder)."""
    cases = pc.remainder_word_mul_cases()
    assert len(cases) == 45 * 4 * 2
    for a, b, k, w, sign in cases:
        _mul_exact_within(prim_lib.hs_fe_mul_limbs, a, b, -N, N)
        _mul_exact_within(prim_lib.hs_fe_mul_f_limbs, a, b, -2**24, FP - 1)
    sq = pc.remainder_word_sq_cases()
    assert {(k, w) for _, k, w, _ in sq} >= {(k, w) for k in range(8, 16) for w in pc.REMAINDER_WORDS if not (k % 2 and w % 2)}
    for a, k, w, sign in sq:
        _sq_exact_within_n(prim_lib, a)


def test_column8_carry_wrap(prim_lib):
    """All nine limbs at the end of their class (and the one-limb-off neighbours): the largest column sums and the largest
    carry out of column 8 into limb 0, for every class pair of test_field_limb_bounds and ge_madd_t's floor-carry classes."""
    mul, mul_f, sq = pc.column8_wrap_cases()
    assert len(mul) == 7 * 4 * 19 and len(mul_f) == 4 * 19 and len(sq) == 20
    for a, b in mul:
        _mul_exact_within(prim_lib.hs_fe_mul_limbs, a, b, -N, N)
    for a, b in mul_f:
        _mul_exact_within(prim_lib.hs_fe_mul_f_limbs, a, b, -2**24, FP - 1)
    for a in sq:
        _sq_exact_within_n(prim_lib, a)


def test_table_class_limb_bounds(prim_lib):
    """ge_madd_t (csrc/ge.hpp): the table-addition chain keeps X, Y, T as floor-carry products (limbs in [-2^24, F'),
    F' = 2^29 + 2^24) and Z centred; worst-case limb patterns of that class must multiply exactly and return
    limbs of the same class, for both signs of the digit."""
    mul_f, madd = pc.table_class_cases()
    assert len(mul_f) == 81 and len(madd) == 9 * 4 * 4 * 3 * 5 * 2
    out, ol = (ctypes.c_uint8 * 32)(), I9()
    # the floor-carry multiplier alone, on the largest operand classes ge_madd_t feeds it
    for a2, b3 in mul_f:
        prim_lib.hs_fe_mul_f_limbs(I9(*a2), I9(*b3), out, ol)
        assert int.from_bytes(bytes(out), "little") == val(a2) * val(b3) % P
        assert min(ol) >= -2**24 and max(ol) < FP
    o36, ob = I36(), (ctypes.c_uint8 * 128)()
    for X, Y, Z, T, qq, neg in madd:
        prim_lib.hs_ge_madd_t_limbs(I36(*(X + Y + Z + T)), I27(*qq), neg, o36, ob)
        want = pc.madd_t_expect(X, Y, Z, T, qq, neg)
        got = [int.from_bytes(bytes(ob)[32 * k:32 * k + 32], "little") for k in range(4)]
        assert got == want
        lim = list(o36)
        for k in (0, 1, 3):
            assert min(lim[9 * k:9 * k + 9]) >= -2**24 and max(lim[9 * k:9 * k + 9]) < FP
        assert max(abs(v) for v in lim[18:27]) <= N


def test_table_msm_formats_and_windows(prim_lib):
    """Fixed-base tables of several window widths (W = 11: 23 windows, the top window keeps
    its digit) against the oracle's big-integer MSM, with edge scalars (0, 1, l-1, 2^252, 2^252 - 1, all-ones windows)."""
    import ctypes, random
    from pyref.ed import Point
    rnd = random.Random(37)
    pts = [from_uniform_bytes(bytes(rnd.getrandbits(8) for _ in range(64))) for _ in range(6)]
    edge = [0, 1, L - 1, 2**252, 2**252 - 1, L - 2**121, int("1" * 252, 2), (2**252 // 3)]
    sets = [edge[i:i + 6] for i in (0, 2)] + [[rnd.randrange(L) for _ in range(6)] for _ in range(2)]
    out = ctypes.create_string_buffer(32)
    for W in (11, 8, 5, 4, 12, 10):
        for ss in sets:
            ok = prim_lib.hs_table_msm(b"".join(p.compress() for p in pts), b"".join(sc_to_bytes(s) for s in ss), 6, W, out)
            want = Point.identity()
            for p, s in zip(pts, ss):
                want = want + p * s
            assert ok and out.raw == want.compress(), W


def test_vb_win_workgroup_order_is_a_permutation(prim_lib):
    for B, VC in [(64, 1), (64, 16), (128, 4), (1024, 16), (1000, 16), (3, 2), (192, 2)]:
        assert prim_lib.hs_vb_win_index_is_permutation(B, VC) == 1, (B, VC)
