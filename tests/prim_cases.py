"""Inputs and big-integer expectations for the device arithmetic headers (csrc/fe.hpp, sc.hpp, ge.hpp, fe_wide.hpp), shared by
the CPU build of those headers (tests/test_hostsim_prims.py, the C++ twin of the multipliers) and the device build
(tests/test_gpu_prims.py, the generated gfx950 column chains and the wavefront form).

Every list is built once, in a fixed order from fixed seeds, and returned as a tuple: the tests only read them."""
import functools
import random

from pyref.ed import P, L, BASEPOINT, from_uniform_bytes, decompress

N = 2**28 + 2**23            # bound of a centred product limb (fe.hpp)
FP = 2**29 + 2**24           # F': floor-carry products have limbs in [-2^24, F')
MUL_CLASS_PAIRS = ((1, 1), (2, 2), (2, 3), (3, 3), (3, 4), (2, 4), (4, 1))   # product shapes of ge.hpp, in units of N
CARRY_CLASSES = (1, 2, 3, 4, 7)
CANON_EDGE = (0, 1, 19, P - 1, P, P + 1, 2**255 - 1, 2**255, 2**256 - 1)
# fe_wide.hpp's class: lane 0 in (-2^13, 2^29 + 2^23), lanes 1..8 in (-2^13, 2^29 + 2^13)
FW_LO = -2**13 + 1
FW_HI0 = 2**29 + 2**23 - 1
FW_HI = 2**29 + 2**13 - 1


def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l)) % P


def limbs_of(v):
    """a value below 2^261 as nine limbs in [0, 2^29)"""
    return [(v >> (29 * i)) & (2**29 - 1) for i in range(9)]


@functools.lru_cache(None)
def vals():
    rnd = random.Random(7)
    edge = [0, 1, 2, 19, 38, P - 1, P, P + 1, 2**255 - 1, 2**255, 2**256 - 1, 2**256 - 38, 2**256 - 39, L - 1, L, L + 1, 2**252]
    return tuple([x.to_bytes(32, "little") for x in edge] + [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(120)])


@functools.lru_cache(None)
def inv_var_values():
    rnd = random.Random(77)
    v = [1 << k for k in range(0, 253, 7)] + [L - (1 << k) for k in range(0, 250, 11)] + [(1 << k) - 1 for k in range(1, 253, 9)]
    v += [rnd.getrandbits(rnd.choice((8, 31, 60, 61, 120, 200, 252))) for _ in range(1500)]
    return tuple(x % L for x in v)


def patterns(rnd, bound):
    yield [bound] * 9
    yield [-bound] * 9
    yield [bound if i % 2 else -bound for i in range(9)]
    yield [-bound if i % 2 else bound for i in range(9)]
    for _ in range(40):
        yield [rnd.choice((bound, -bound, rnd.randint(-bound, bound))) for _ in range(9)]


def floor_pat(rnd):
    yield [FP - 1] * 9
    yield [-2**24] * 9
    yield [FP - 1 if i % 2 else -2**24 for i in range(9)]
    for _ in range(6):
        yield [rnd.choice((FP - 1, -2**24, 0, rnd.randint(0, 2**29 - 1))) for _ in range(9)]


def cent_pat(rnd):
    yield [N] * 9
    yield [-N] * 9
    yield [N if i % 2 else -N for i in range(9)]
    for _ in range(4):
        yield [rnd.choice((N, -N, rnd.randint(-N, N))) for _ in range(9)]


def tab_pat(rnd):
    yield [2**29 - 1] * 9
    yield [0] * 9
    for _ in range(3):
        yield [rnd.choice((2**29 - 1, 0, rnd.randint(0, 2**29 - 1))) for _ in range(9)]


def _freeze(x):
    return tuple(_freeze(y) for y in x) if isinstance(x, (list, tuple)) else x


@functools.lru_cache(None)
def field_limb_cases():
    """Worst-case limb classes of every product shape of ge.hpp.  Returns (mul, sq, carry): mul = ((a, b), ...) over
    MUL_CLASS_PAIRS, sq = (a, ...) in class 2N, carry = (a, ...) over CARRY_CLASSES (also the inputs of fe_canon)."""
    rnd = random.Random(29)
    mul, sq, carry = [], [], []
    for ka, kb in MUL_CLASS_PAIRS:
        for a in patterns(rnd, ka * N):
            for b in list(patterns(rnd, kb * N))[:12]:
                mul.append((a, b))
    for a in patterns(rnd, 2 * N):
        sq.append(a)
    for k in CARRY_CLASSES:
        for a in patterns(rnd, k * N):
            carry.append(a)
    return _freeze(mul), _freeze(sq), _freeze(carry)


@functools.lru_cache(None)
def table_class_cases():
    """The accumulator classes of ge_madd_t.  Returns (mul_f, madd): mul_f = ((a, b), ...) with a <= 2F', |b| <= 3N;
    madd = ((X, Y, Z, T, q, negate), ...) with X, Y, T floor-carry, Z centred, q = 27 table limbs in [0, 2^29)."""
    rnd = random.Random(31)
    mul_f, madd = [], []
    for a in floor_pat(rnd):
        for b in floor_pat(rnd):
            a2 = [2 * x for x in a]                      # cY <= 2F'
            b3 = [min(3 * N, max(-3 * N, 3 * x)) for x in b]  # |cZ|, |cT| <= N + F' = 3N in ge_madd_t (T*dxy in floor-carry form)
            mul_f.append((a2, b3))
    for X in floor_pat(rnd):
        for Y in list(floor_pat(rnd))[:4]:
            for Z in list(cent_pat(rnd))[:4]:
                for T in list(floor_pat(rnd))[:3]:
                    for q in tab_pat(rnd):
                        qq = list(q) + list(reversed(q)) + [q[(i * 5) % 9] for i in range(9)]
                        for neg in (0, 1):
                            madd.append((X, Y, Z, T, qq, neg))
    return _freeze(mul_f), _freeze(madd)


def madd_t_expect(X, Y, Z, T, qq, neg):
    """the four coordinates ge_madd_t must return (halved table form: Z, not 2Z)"""
    x, y, z, t = val(X), val(Y), val(Z), val(T)
    ypx, ymx, xy2d = val(qq[:9]), val(qq[9:18]), val(qq[18:])
    if neg:
        ypx, ymx, xy2d = ymx, ypx, -xy2d
    A, B, C, D = (y + x) * ypx, (y - x) * ymx, t * xy2d, z
    cX, cY, cZ, cT = A - B, A + B, D + C, D - C
    return [cX * cT % P, cY * cZ % P, cZ * cT % P, cX * cY % P]


# ---- directed cases ------------------------------------------------------------------------------------------------------------
REMAINDER_WORDS = (0x00000000, 0x7fffffff, 0x80000000, 0xffffffff)


def pass1_columns(a, b):
    """fe.hpp's first pass in big integers: the column sums S_8..S_16 (each with 8 * the high word of the column below)"""
    cols, h = {}, 0
    for k in range(8, 17):
        acc = 8 * h + sum(a[i] * b[k - i] for i in range(9) if 0 <= k - i < 9)
        cols[k] = acc
        h = acc >> 32
    return cols


def _solve(rnd, c, r, want_sign, base):
    """y with c*y = r (mod 2^32), 0 < |y| <= N and sign(base + c*y) == want_sign; None when this c has none"""
    c32 = c % 2**32
    if c32 == 0:
        return None
    v = (c32 & -c32).bit_length() - 1
    if r % (1 << v):
        return None
    m = 1 << (32 - v)
    y0 = (r >> v) * pow(c32 >> v, -1, m) % m
    for _ in range(64):
        y = y0 + m * rnd.randint(-(N // m) - 1, N // m + 1)
        if y and abs(y) <= N and (base + c * y > 0) == (want_sign > 0) and base + c * y != 0:
            return y
    return None


@functools.lru_cache(None)
def remainder_word_mul_cases():
    """a = x e_i, b = y e_j (|x|, |y| <= N): column i + j of the product is x*y alone, and its low 32-bit word - what pass 1
    hands to the UNSIGNED multiply-add of pass 2 (k >= 9), or column 8's own remainder - is one of REMAINDER_WORDS, for
    both signs of x*y.  Every (i, j) with 8 <= i + j <= 16.  Returns ((a, b, k, word, sign), ...)."""
    rnd = random.Random(0x9e37)
    out = []
    for k in range(8, 17):
        for i in range(9):
            j = k - i
            if not 0 <= j < 9:
                continue
            for w in REMAINDER_WORDS:
                for sign in (1, -1):
                    shift = 16 if w == 0 else 15 if w == 0x80000000 else 0   # x = odd * 2^shift, so that x*y can end in w
                    while True:
                        x = ((rnd.randint(1, (N >> shift) - 1) | 1) << shift) * rnd.choice((1, -1))
                        y = _solve(rnd, x, w, sign, 0)
                        if y is not None:
                            break
                    a, b = [0] * 9, [0] * 9
                    a[i], b[j] = x, y
                    assert pass1_columns(a, b)[k] == x * y and (x * y) % 2**32 == w and (x * y > 0) == (sign > 0)
                    out.append((a, b, k, w, sign))
    return _freeze(out)


def sq_pass1_columns(a):
    return pass1_columns(a, a)   # fe_sq forms the same sums (2 a_i a_j for i < j, a_i^2)


@functools.lru_cache(None)
def remainder_word_sq_cases():
    """The same for fe_sq, as far as a square's columns reach: column k of a = x e_i + y e_j (i < j, i + j = k) holds 2xy plus
    what the columns below hand up; with an odd middle limb z e_(k/2) (even k) it becomes odd.  An odd column (k odd) is a sum
    of doubled products and multiples of 8, so the two odd words cannot occur there, and column 16 is a_8^2 alone: of the four
    words only 0 is a square, and only with the positive sign.  Returns ((a, k, word, sign), ...)."""
    rnd = random.Random(0x51ab)
    out = []
    for k in range(8, 16):
        for i in range(9):
            j = k - i
            if not i < j < 9:
                continue
            for w in REMAINDER_WORDS:
                if w % 2 and k % 2:
                    continue
                for sign in (1, -1):
                    while True:
                        a = [0] * 9
                        s = rnd.randrange(17)   # x = odd * 2^s: an even word needs an even x, and 2^(s+1) must divide what is left
                        a[i] = ((rnd.randint(1, (N >> s) - 1) | 1) << s) * rnd.choice((1, -1))
                        if w % 2:
                            a[k // 2] = rnd.randint(-N, N) | 1
                        if max(abs(v) for v in a) > N:
                            continue
                        base = sq_pass1_columns(a)[k]
                        y = _solve(rnd, 2 * a[i], (w - base) % 2**32, sign, base)
                        if y is None:
                            continue
                        a[j] = y
                        col = sq_pass1_columns(a)[k]
                        if col % 2**32 == w and (col > 0) == (sign > 0):
                            break
                    out.append((a, k, w, sign))
    for _ in range(4):
        a = [0] * 9
        a[8] = (rnd.randint(1, N >> 16) << 16) * rnd.choice((1, -1))
        assert sq_pass1_columns(a)[16] % 2**32 == 0
        out.append((a, 16, 0, 1))
    return _freeze(out)


def _one_off(base):
    """the pattern itself and its nine neighbours with one limb one step nearer to zero (still inside the class)"""
    yield list(base)
    for i in range(9):
        v = list(base)
        v[i] -= 1 if v[i] > 0 else -1
        yield v


def _wrap_pairs(a_ends, b_ends):
    for a0 in a_ends:
        for b0 in b_ends:
            yield [a0] * 9, [b0] * 9
            for a in list(_one_off([a0] * 9))[1:]:
                yield a, [b0] * 9
            for b in list(_one_off([b0] * 9))[1:]:
                yield [a0] * 9, b


@functools.lru_cache(None)
def column8_wrap_cases():
    """All nine limbs at the end of their class: every column sum at its largest, and the largest carry out of column 8
    (just under 2^13) wrapping into limb 0.  Returns (mul, mul_f, sq): pairs for fe_mul over MUL_CLASS_PAIRS, pairs for
    fe_mul_f in ge_madd_t's largest classes (a in [-2^25, 2F'), |b| <= 3N), elements for fe_sq at +-2N."""
    mul = [p for ka, kb in MUL_CLASS_PAIRS for p in _wrap_pairs((ka * N, -ka * N), (kb * N, -kb * N))]
    mul_f = list(_wrap_pairs((2 * (FP - 1), -2 * 2**24), (3 * N, -3 * N)))
    sq = [a for e in (2 * N, -2 * N) for a in _one_off([e] * 9)]
    return _freeze(mul), _freeze(mul_f), _freeze(sq)


def fw_in_class(l):
    return FW_LO <= l[0] <= FW_HI0 and all(FW_LO <= x <= FW_HI for x in l[1:9])


@functools.lru_cache(None)
def fw_mul_cases():
    """Operand pairs for fw_mul (limb k on lane k): the ends of the wavefront class, alternating ends, class N against the
    wavefront class (the mixed product fe_pow22523_wave forms: z is a fe_carry result), 40 random members of each."""
    rnd = random.Random(0xf3)
    hi = [FW_HI0] + [FW_HI] * 8
    lo = [FW_LO] * 9
    alt = [hi[i] if i % 2 else lo[i] for i in range(9)]
    alt2 = [lo[i] if i % 2 else hi[i] for i in range(9)]
    ends = [hi, lo, alt, alt2]
    cent = [[N] * 9, [-N] * 9, [N if i % 2 else -N for i in range(9)], [-N if i % 2 else N for i in range(9)]]

    def rw():
        return [rnd.choice((hi[i], lo[i], rnd.randint(lo[i], hi[i]))) for i in range(9)]

    def rn():
        return [rnd.choice((N, -N, rnd.randint(-N, N))) for _ in range(9)]
    out = [(a, b) for a in ends for b in ends]
    out += [(a, b) for a in cent for b in ends] + [(a, b) for a in ends for b in cent] + [(a, b) for a in cent for b in cent]
    out += [(rw(), rw()) for _ in range(40)]
    out += [(rn(), rw()) for _ in range(40)] + [(rw(), rn()) for _ in range(40)]
    out += [(rn(), rn()) for _ in range(40)]
    out += [(a, a) for a in ends + cent] + [(a, a) for a in (rw() for _ in range(40))]   # the squarings of the power chain
    return _freeze(out)


@functools.lru_cache(None)
def pow_inputs():
    """raw limbs for fe_carry / fe_canon / fe_invert / fe_pow22523 (lane and wavefront form): classes 1, 2, 3, 4, 7 N and
    the canonical edge values"""
    return field_limb_cases()[2] + _freeze([limbs_of(v) for v in CANON_EDGE])


@functools.lru_cache(None)
def encoding_cases():
    """32-byte strings for ge_decompress, each with the oracle's verdict: ((bytes, accepted), ...)"""
    rnd = random.Random(0xdec0)
    enc = [bytes.fromhex(h) for h in ("00ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff",   # RFC 9496: non-canonical
                                      "0100000000000000000000000000000000000000000000000000000000000000",   # negative
                                      "edffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f")]  # s = p
    enc += [v.to_bytes(32, "little") for v in (P, P + 1, P + 2, 2**255 - 1)]
    good = [(BASEPOINT * k).compress() for k in range(17)]
    good += [from_uniform_bytes(bytes(rnd.getrandbits(8) for _ in range(64))).compress() for _ in range(64)]
    enc += [(int.from_bytes(g, "little") | 1 << 255).to_bytes(32, "little") for g in good[:4]]   # bit 255 set on a valid s
    enc += [(1 << 255).to_bytes(32, "little"), (2**256 - 1).to_bytes(32, "little")]
    enc += [(int.from_bytes(g, "little") | 1).to_bytes(32, "little") for g in good[1:9]]          # odd canonical s
    enc += [(P - int.from_bytes(g, "little")).to_bytes(32, "little") for g in good[1:9]]          # -s of a valid s (odd, canonical)
    enc += [(2 * k).to_bytes(32, "little") for k in range(1, 24)]                                  # small even s: squares and non-squares
    enc += [(P - 1 - 2 * k).to_bytes(32, "little") for k in range(12)]                             # the largest even canonical s
    enc += [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(200)]
    enc += [(rnd.getrandbits(254) & ~1).to_bytes(32, "little") for _ in range(64)]                 # even, canonical: the curve decides
    enc += good
    return tuple((e, decompress(e) is not None) for e in enc)


@functools.lru_cache(None)
def group_cases():
    """test_group_and_encoding's draws: ((wide64, k32, P = k B compressed, Q compressed), ...) and their expectations"""
    rnd = random.Random(9)
    out = []
    for _ in range(12):
        w = bytes(rnd.getrandbits(8) for _ in range(64))
        k = bytes(rnd.getrandbits(8) for _ in range(32))
        p = BASEPOINT * int.from_bytes(k, "little")
        q = from_uniform_bytes(bytes(rnd.getrandbits(8) for _ in range(64)))
        out.append({"wide": w, "wide_mod_l": int.from_bytes(w, "little") % L, "uniform": from_uniform_bytes(w).compress(),
                    "k": k, "p": p.compress(), "q": q.compress(),
                    "addsub": (p + q).compress() + (p - q).compress() + (p + q).compress() + (p - q).compress()})
    return tuple(out)
