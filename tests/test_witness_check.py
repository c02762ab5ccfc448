"""BPR1CS_OPT_CHECK_WITNESS on the CPU simulator (the functor bodies of K_check_gates / K_check_rows, the job plumbing, the refusal
records): the option itself, then the case table of tests/witness_check_cases.py - every expectation is the pure-Python checker's."""
import ctypes
import re

import pytest

import witness_check_cases as wc

bp = wc.bp


def test_option_plumbing(sim_lib):
    """the option exists (BPR1CS_ERR_INVALID_ARGUMENT, -17, before it did), can be given at creation, and -1 restores off"""
    assert bp.OPT_CHECK_WITNESS == 14 and bp.OPTIONS["check_witness"] == 14 and bp.PROOF_REFUSED == 0xFF
    hdr = open(wc.os.path.join(wc.ROOT, "include", "bpr1cs.h")).read()
    for name, val in (("OPT_CHECK_WITNESS", 14), ("PROOF_REFUSED", 0xFF), ("REFUSAL_OFF_GATE", 4), ("REFUSAL_OFF_ROW", 8),
                      ("REFUSAL_OFF_GATE_COUNT", 12), ("REFUSAL_OFF_ROW_COUNT", 16)):
        assert int(re.search(r"#define BPR1CS_%s\s+(\w+)" % name, hdr).group(1), 0) == val == getattr(bp, name)
    g = bp.Gens(8, lib=sim_lib, window_bits=8)
    for v in (1, 0, 7, -1):
        assert sim_lib.bpr1cs_gens_set_option(g.h, 14, v) == 0
    g.close()
    ob = wc.oracle("rc1")
    circ = wc.common.circuit_from_oracle(ob, sim_lib)
    inp = wc.tiled(ob, 2, {1: [("wire", 2, 0)]})
    n, m = ob["n"], ob["m"]
    want = wc.violations(ob, inp[3][96 * n:], inp[0][32 * m:])
    assert want is not None and want["gate"] == 0 and wc.violations(ob, inp[3][:96 * n], inp[0][:32 * m]) is None
    rec = wc.record(circ.proof_len, want)

    def prove(g):
        P, _ = bp.prove_batch(g, circ, ob["label"], inp[0], inp[1], inp[2], 2, wires=inp[3])
        return P[1], bp.last_prove_stats(sim_lib)["refused"]
    g = bp.Gens(8, lib=sim_lib, window_bits=8, check_witness=1)       # at creation
    assert prove(g) == (rec, 1)
    g.set_option("check_witness", -1)                                 # back to the default: off
    p, refused = prove(g)
    assert bp.refusal(p) is None and refused == 0
    g.set_option("check_witness", 5)                                  # any other value means 1
    assert prove(g) == (rec, 1)
    g.close()


def test_refusal_helper():
    rec = wc.record(417, dict(gate=None, row=7, gates=0, rows=3))
    assert bp.refusal(rec) == dict(gate=None, row=7, gates=0, rows=3) and bp.refusal(b"\0" + rec[1:]) is None
    assert rec[0] == 0xFF and rec[1:4] == bytes(3) and rec[20:] == bytes(417 - 20)
    out = ctypes.create_string_buffer(4096)
    lib = bp.load_library() if wc.os.path.exists(bp.LIB_PATH) else None
    if lib is not None:   # the shipped library's parser refuses the record's version byte
        assert lib.bpr1cs_proof_parse(rec, len(rec), ctypes.cast(out, ctypes.POINTER(bp.ProofStruct))) == -2


@pytest.mark.parametrize("case", sorted(wc.TABLE))
def test_case(sim_lib, sim_glib, case):
    wc.TABLE[case](sim_lib, sim_glib)
