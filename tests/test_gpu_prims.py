"""The device's own field, scalar and group arithmetic against big integers.

On the GPU every field multiplication runs the generated inline-assembly column chains of csrc/fe_asm_gfx950.inc, not the C++
twin the CPU simulator compiles; the lone-wavefront kernels use the limb-per-lane form of csrc/fe_wide.hpp.  tests/devprim/
prim_check.hip puts those bodies behind batch entry points, and these tests feed them the inputs of tests/prim_cases.py: the
worst-case limb classes of tests/test_hostsim_prims.py, the directed remainder-word and column-8 cases, the bounds of the
wavefront class, and encodings judged by the oracle's decoder.  Every comparison is exact."""
import ctypes
import os
import random

import pytest

import __graft_entry__ as entry
import prim_cases as pc
from prim_cases import P, L, N, FP, val

ENTRY_POINTS = ("dp_fe_mul_limbs", "dp_fe_mul_f_limbs", "dp_fe_sq_limbs", "dp_fe_carry_limbs", "dp_fe_canon_limbs", "dp_fe_invert",
                "dp_fe_pow22523", "dp_ge_madd_t_limbs", "dp_sc_mul", "dp_sc_add", "dp_sc_sub", "dp_sc_inv", "dp_sc_inv_var",
                "dp_sc_inv_fermat", "dp_sc_wide", "dp_decompress_recompress", "dp_uniform", "dp_addsub", "dp_basemul",
                "dp_fw_mul_limbs", "dp_fe_pow22523_wave")


@pytest.fixture(scope="module")
def devprim():
    """the harness, rebuilt when its sources are newer (BPR1CS_DEVPRIM_LIB: a prebuilt one instead - a harness compiled against a
    deliberately wrong copy of csrc/ must make these tests fail)"""
    return ctypes.CDLL(os.environ.get("BPR1CS_DEVPRIM_LIB") or entry.build_devprim())


def test_harness_cross_compiles_from_a_clean_build_directory(tmp_path):
    """no GPU needed: hipcc builds the harness for gfx950 into an empty directory, and the library exports every entry point"""
    lib = ctypes.CDLL(entry.build_devprim(str(tmp_path / "_build")))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


# ---- packing ---------------------------------------------------------------------------------------------------------------------
def _i32(rows):
    flat = [x for r in rows for x in r]
    return (ctypes.c_int32 * len(flat))(*flat)


def _rows(arr, width):
    flat = list(arr)
    return [flat[i:i + width] for i in range(0, len(flat), width)]


def _ints(buf, width=32):
    raw = bytes(buf)
    return [int.from_bytes(raw[i:i + width], "little") for i in range(0, len(raw), width)]


def _fe_op(f, a, b=None):
    """a field entry point on a batch: [(value of the canonical bytes, result limbs), ...]"""
    n = len(a)
    ob, ol = ctypes.create_string_buffer(32 * n), (ctypes.c_int32 * (9 * n))()
    args = (_i32(a),) + ((_i32(b),) if b is not None else ()) + (n, ob, ol)
    assert f(*args) == 0, "HIP error in the harness (is a gfx950 device visible?)"
    return list(zip(_ints(ob), _rows(ol, 9)))


def _sc_op(f, a, b=None, width=32):
    n = len(a)
    out = ctypes.create_string_buffer(32 * n)
    args = (b"".join(a),) + ((b"".join(b),) if b is not None else ()) + (n, out)
    assert all(len(x) == width for x in a) and f(*args) == 0, "HIP error in the harness"
    return _ints(out)


def check_products(results, pairs, lo, hi):
    for (got, limbs), (a, b) in zip(results, pairs):
        assert got == val(a) * val(b) % P, (a, b)
        assert lo <= min(limbs) and max(limbs) <= hi, (a, b, limbs)


# ---- field multipliers -----------------------------------------------------------------------------------------------------------
def mul_pairs():
    """every pattern and class pair of the two CPU limb tests (all within 9 |a| |b| < 2^63 and |limb| <= 4N), then the directed cases"""
    rw = [(a, b) for a, b, _, _, _ in pc.remainder_word_mul_cases()]
    wrap_mul, wrap_mul_f, _ = pc.column8_wrap_cases()
    return pc.field_limb_cases()[0] + pc.table_class_cases()[0] + tuple(rw) + wrap_mul + wrap_mul_f


def sq_inputs():
    mul, sq, _ = pc.field_limb_cases()
    small = []                                              # the first operands of the product patterns that fe_sq accepts (<= 2N)
    for a, _ in mul:
        if max(abs(x) for x in a) <= 2 * N and (not small or small[-1] != a):
            small.append(a)
    return sq + tuple(small) + tuple(a for a, _, _, _ in pc.remainder_word_sq_cases()) + pc.column8_wrap_cases()[2]


@pytest.mark.gpu
def test_fe_mul_is_exact_and_centred(devprim):
    pairs = mul_pairs()
    assert len(pairs) == 3696 + 81 + 360 + 532 + 76
    check_products(_fe_op(devprim.dp_fe_mul_limbs, [a for a, _ in pairs], [b for _, b in pairs]), pairs, -N, N)


@pytest.mark.gpu
def test_fe_mul_f_is_exact_and_in_the_floor_carry_class(devprim):
    pairs = mul_pairs()
    check_products(_fe_op(devprim.dp_fe_mul_f_limbs, [a for a, _ in pairs], [b for _, b in pairs]), pairs, -2**24, FP - 1)


@pytest.mark.gpu
def test_fe_sq_is_exact_and_centred(devprim):
    a = sq_inputs()
    assert len(a) >= 44 + 176 + 20
    check_products(_fe_op(devprim.dp_fe_sq_limbs, a), [(x, x) for x in a], -N, N)


# ---- table addition --------------------------------------------------------------------------------------------------------------
def check_madd_t(limbs, coords, cases):
    for lim, got, c in zip(limbs, coords, cases):
        assert got == pc.madd_t_expect(*c), c
        for k in (0, 1, 3):
            assert min(lim[9 * k:9 * k + 9]) >= -2**24 and max(lim[9 * k:9 * k + 9]) < FP, (c, lim)
        assert max(abs(v) for v in lim[18:27]) <= N, (c, lim)


@pytest.mark.gpu
def test_ge_madd_t_on_the_table_class(devprim):
    cases = pc.table_class_cases()[1]
    n = len(cases)
    assert n == 4320
    ol, ob = (ctypes.c_int32 * (36 * n))(), ctypes.create_string_buffer(128 * n)
    rc = devprim.dp_ge_madd_t_limbs(_i32([X + Y + Z + T for X, Y, Z, T, _, _ in cases]), _i32([c[4] for c in cases]),
                                    _i32([[c[5]] for c in cases]), n, ol, ob)
    assert rc == 0, "HIP error in the harness"
    coords = _ints(ob)
    check_madd_t(_rows(ol, 36), [coords[4 * i:4 * i + 4] for i in range(n)], cases)


# ---- carry, canonical form, powers -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fe_carry_canon_invert_pow22523(devprim):
    a = pc.pow_inputs()
    n = len(a)
    assert n == 5 * 44 + 9
    ol = (ctypes.c_int32 * (9 * n))()
    assert devprim.dp_fe_carry_limbs(_i32(a), n, ol) == 0
    for x, r in zip(a, _rows(ol, 9)):
        assert val(r) == val(x) and max(abs(v) for v in r) <= N, (x, r)
    ob = ctypes.create_string_buffer(32 * n)
    assert devprim.dp_fe_canon_limbs(_i32(a), n, ob) == 0
    assert _ints(ob) == [val(x) for x in a]
    for f, e in ((devprim.dp_fe_invert, P - 2), (devprim.dp_fe_pow22523, (P - 5) // 8)):
        for x, (got, limbs) in zip(a, _fe_op(f, a)):
            assert got == pow(val(x), e, P), x
            assert max(abs(v) for v in limbs) <= N, (x, limbs)


# ---- wavefront form --------------------------------------------------------------------------------------------------------------
def check_fw_products(out19, pairs):
    for w, (a, b) in zip(out19, pairs):
        assert val(w[:9]) == val(a) * val(b) % P, (a, b, w)
        assert pc.fw_in_class(w[:9]), (a, b, w)          # lanes 0..8 back inside the documented class
        assert w[9:] == [0] * 10, (a, b, w)              # lanes 9..18 zero


@pytest.mark.gpu
def test_fw_mul_on_the_bounds_of_its_class(devprim):
    pairs = pc.fw_mul_cases()
    n = len(pairs)
    assert n == 272 and all(pc.fw_in_class(x) or max(abs(v) for v in x) <= N for p in pairs for x in p)
    out = (ctypes.c_int32 * (19 * n))()
    assert devprim.dp_fw_mul_limbs(_i32([a for a, _ in pairs]), _i32([b for _, b in pairs]), n, out) == 0, "HIP error in the harness"
    check_fw_products(_rows(out, 19), pairs)


@pytest.mark.gpu
def test_fe_pow22523_wave_against_big_integers(devprim):
    a = pc.pow_inputs()
    for x, (got, limbs) in zip(a, _fe_op(devprim.dp_fe_pow22523_wave, a)):
        assert got == pow(val(x), (P - 5) // 8, P), x
        assert pc.fw_in_class(limbs), (x, limbs)


# ---- scalars ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scalar_mul_add_sub(devprim):
    vals = pc.vals()
    pairs = [(a, b) for a in vals for b in vals[:20]]
    assert len(pairs) == 137 * 20
    ia, ib = [int.from_bytes(a, "little") for a, _ in pairs], [int.from_bytes(b, "little") for _, b in pairs]
    for f, op in ((devprim.dp_sc_mul, lambda x, y: x * y), (devprim.dp_sc_add, lambda x, y: x + y), (devprim.dp_sc_sub, lambda x, y: x - y)):
        assert _sc_op(f, [a for a, _ in pairs], [b for _, b in pairs]) == [op(x, y) % L for x, y in zip(ia, ib)]


@pytest.mark.gpu
def test_scalar_inverses(devprim):
    vals = list(pc.vals())
    want = [pow(int.from_bytes(a, "little") % L, L - 2, L) for a in vals]
    for f in (devprim.dp_sc_inv, devprim.dp_sc_inv_fermat, devprim.dp_sc_inv_var):   # safegcd divsteps, Fermat ladder, variable-time divsteps
        assert _sc_op(f, vals) == want
    many = pc.inv_var_values()
    assert len(many) == 1588
    assert _sc_op(devprim.dp_sc_inv_var, [x.to_bytes(32, "little") for x in many]) == [pow(x, L - 2, L) if x else 0 for x in many]


@pytest.mark.gpu
def test_scalar_wide_reduction(devprim):
    rnd = random.Random(0x51de)
    edge = [2**512 - 1, 0, 1, L - 1, L, L + 1, 2**252, 2**256 - 1, 2**256, L << 256, (L << 256) - 1, L * L, L * L - 1, 2**511, (2**512 - 1) // L * L]
    wide = [x.to_bytes(64, "little") for x in edge] + [c["wide"] for c in pc.group_cases()] + [bytes(rnd.getrandbits(8) for _ in range(64)) for _ in range(37)]
    assert wide[0] == b"\xff" * 64
    assert _sc_op(devprim.dp_sc_wide, wide, width=64) == [int.from_bytes(w, "little") % L for w in wide]


# ---- group -----------------------------------------------------------------------------------------------------------------------
def _decompress_recompress(devprim, enc):
    n = len(enc)
    ok, out = (ctypes.c_int32 * n)(), ctypes.create_string_buffer(32 * n)
    assert devprim.dp_decompress_recompress(b"".join(enc), n, ok, out) == 0, "HIP error in the harness"
    return list(ok), [out.raw[32 * i:32 * i + 32] for i in range(n)]


@pytest.mark.gpu
def test_group_and_encoding_on_the_device(devprim):
    cases = pc.group_cases()
    n = len(cases)
    out = ctypes.create_string_buffer(32 * n)
    assert devprim.dp_uniform(b"".join(c["wide"] for c in cases), n, out) == 0
    assert out.raw == b"".join(c["uniform"] for c in cases)
    assert devprim.dp_basemul(b"".join(c["k"] for c in cases), n, out) == 0
    assert out.raw == b"".join(c["p"] for c in cases)
    ok, rec = _decompress_recompress(devprim, [c["p"] for c in cases] + [b"\x01" + bytes(31)])
    assert ok == [1] * n + [0] and rec[:n] == [c["p"] for c in cases]
    ok4, o4 = (ctypes.c_int32 * n)(), ctypes.create_string_buffer(128 * n)
    assert devprim.dp_addsub(b"".join(c["p"] for c in cases), b"".join(c["q"] for c in cases), n, ok4, o4) == 0
    assert list(ok4) == [1] * n and o4.raw == b"".join(c["addsub"] for c in cases)


@pytest.mark.gpu
def test_decoding_accepts_and_rejects_as_the_oracle_does(devprim):
    cases = pc.encoding_cases()
    ok, rec = _decompress_recompress(devprim, [e for e, _ in cases])
    for (e, want), flag, back in zip(cases, ok, rec):
        assert bool(flag) == want, e.hex()
        if want:
            assert back == e, e.hex()
