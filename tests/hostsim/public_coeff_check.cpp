// The gadgets "set_membership_lean" and "weighted_sum_bound" (host/frontend.cpp run_gadget) through CircuitCompiler with their data baked
// (sp given) and with their data public (no sp), and the two DESCRIPTIONS compared term by term: every constraint row and every witness
// operand is identical, except that a term (var, item_i) / (var, -w_i) of the baked form reads (var x Public i, 1) / (var x Public i, -1)
// and the budget's (One, budget) reads (Public k, 1).  Proof bytes alone cannot show this.  Also: the algebra of a public factor
// (like terms merge only under the same factor; a scaled term whose coefficient came out 0 is dropped from the export; marker + term in
// the exported arrays), and a Prover or a Verifier handed a public factor returns an R1CSError.  Linked against the CPU simulator.
#include <cstdio>
#include "../../bulletproofs-r1cs-gadgets_amd/host/r1cs.hpp"
#include "../../bulletproofs-r1cs-gadgets_amd/host/gadgets.hpp"
using namespace bpr1cs;

static int bad = 0;
static void fail(const char* what, size_t i) { printf("  %s (at %zu)\n", what, i); bad++; }

// the two harnesses of host/frontend.cpp run_gadget, in their commitment order; `sp` empty: the data are public
static void set_lean(CircuitCompiler& cc, size_t k, const std::vector<Scalar>& sp) {
    std::vector<AllocatedQuantity> bits;
    for (size_t i = 0; i < k; i++) {
        AllocatedQuantity q{cc.commit_placeholder(), std::nullopt};
        bit_gadget(cc, q);
        bits.push_back(q);
    }
    vector_sum_gadget(cc, bits, 1);
    AllocatedQuantity val{cc.commit_placeholder(), std::nullopt};
    std::vector<Term> row{{val.variable, -Scalar::one()}};
    for (size_t i = 0; i < k; i++) {
        if (sp.empty()) row.push_back({bits[i].variable.times_public((uint32_t)i), Scalar::one()});
        else row.push_back({bits[i].variable, sp[i]});
    }
    cc.constrain(LinearCombination(row));
}
static void weighted(CircuitCompiler& cc, size_t k, size_t nbits, const std::vector<Scalar>& sp) {
    std::vector<Term> terms;
    if (sp.empty()) terms.push_back({Variable::Public((uint32_t)k), Scalar::one()});
    else terms.push_back({Variable::One(), sp[k]});
    for (size_t i = 0; i < k; i++) {
        const Variable x = cc.commit_placeholder();
        if (sp.empty()) terms.push_back({x.times_public((uint32_t)i), -Scalar::one()});
        else terms.push_back({x, -sp[i]});
    }
    const LinearCombination lc(terms);
    positive_no_gadget_lc(cc, lc, std::nullopt, nbits);
}

// a baked term against its public twin: equal, or (var, c) against (var x Public i, +-1) with c = +-data[i], or (One, c) against (Public k, 1)
static bool twin(const Term& a, const Term& b, const std::vector<Scalar>& data, size_t& scaled, size_t& linear) {
    if (a.first == b.first && a.second == b.second) return true;
    if (b.first.pub) {
        const uint32_t i = b.first.pub - 1;
        Variable plain = b.first;
        plain.pub = 0;
        if (!(a.first == plain) || i >= data.size()) return false;
        scaled++;
        return a.second == b.second * data[i];   // (b's coefficient is +1 or -1)
    }
    if (b.first.kind == VarKind::Public && a.first.kind == VarKind::One && b.first.index < data.size()) {
        linear++;
        return a.second == b.second * data[b.first.index];
    }
    return false;
}
static bool twin_lc(const LinearCombination& a, const LinearCombination& b, const std::vector<Scalar>& data, size_t& scaled, size_t& linear) {
    if (a.terms.size() != b.terms.size()) return false;
    for (size_t i = 0; i < a.terms.size(); i++)
        if (!twin(a.terms[i], b.terms[i], data, scaled, linear)) return false;
    return true;
}
static bool twin_hint(const WitnessHint& a, const WitnessHint& b, const std::vector<Scalar>& data, size_t& scaled, size_t& linear) {
    return a.kind == b.kind && a.committed == b.committed && a.bit == b.bit && twin_lc(a.lc, b.lc, data, scaled, linear);
}

template <class Build>
static void compare(const char* name, const std::vector<Scalar>& data, size_t want_rows_scaled, size_t want_rows_linear, size_t want_n, size_t want_m, const Build& build) {
    Transcript ta(""), tb("");
    CircuitCompiler baked(ta), pub(tb);
    build(baked, data);
    build(pub, std::vector<Scalar>());
    const int before = bad;
    if (baked.num_vars != pub.num_vars || baked.constraints.size() != pub.constraints.size() || !pub.complete || !baked.complete) { fail("shape", 0); return; }
    if (pub.num_vars != want_n || pub.V_.size() != want_m) fail("n / m", pub.num_vars);
    size_t scaled = 0, linear = 0;
    for (size_t j = 0; j < pub.constraints.size(); j++)
        if (!twin_lc(baked.constraints[j], pub.constraints[j], data, scaled, linear)) fail("constraint row", j);
    if (scaled != want_rows_scaled || linear != want_rows_linear) fail("number of public terms in the rows", scaled);
    if (baked.ops.size() != pub.ops.size()) fail("number of witness ops", 0);
    else
        for (size_t i = 0; i < pub.ops.size(); i++) {
            const auto &a = baked.ops[i], &b = pub.ops[i];
            if (a.have_l != b.have_l || a.have_r != b.have_r || !twin_hint(a.l, b.l, data, scaled, linear) || !twin_hint(a.r, b.r, data, scaled, linear)) fail("witness op", i);
        }
    // the exported arrays: a marker (SCALE << 28 | i, 1) in front of every scaled term, nothing else changed in length
    std::vector<uint32_t> ro_a, tv_a, ro_b, tv_b;
    std::vector<uint8_t> tc_a, tc_b;
    baked.export_csr(ro_a, tv_a, tc_a, true);
    pub.export_csr(ro_b, tv_b, tc_b, true);
    size_t markers = 0;
    for (size_t t = 0; t < tv_b.size(); t++)
        if ((tv_b[t] >> 28) == BPR1CS_VAR_SCALE) {
            markers++;
            if (t + 1 >= tv_b.size() || (tv_b[t + 1] >> 28) > BPR1CS_VAR_MUL_OUT || tc_b[32 * t] != 1) fail("exported marker", t);
        }
    if (markers != want_rows_scaled || tv_b.size() != tv_a.size() + markers) fail("exported markers", markers);
    printf("%s: n = %zu, q = %zu, m = %zu, %zu scaled and %zu linear public terms in the rows: %s\n", name, pub.num_vars, pub.constraints.size(), pub.V_.size(),
           want_rows_scaled, want_rows_linear, bad == before ? "same but for the public terms" : "DIFFERENT");
}

static void algebra() {
    const Variable v = Variable::Committed(0);
    LinearCombination lc = LinearCombination(std::vector<Term>{{v, Scalar(2)}, {v.times_public(1), Scalar(3)}, {v, Scalar(5)}, {v.times_public(1), Scalar(4)},
                                                               {v.times_public(2), Scalar(6)}, {v.times_public(2), -Scalar(6)}}).simplify();
    if (lc.terms.size() != 3 || !(lc.terms[0].second == Scalar(7)) || lc.terms[0].first.pub != 0 || !(lc.terms[1].second == Scalar(7)) || lc.terms[1].first.pub != 2 ||
        !lc.terms[2].second.is_zero() || lc.terms[2].first.pub != 3) fail("simplify merges like terms only under the same public factor", lc.terms.size());
    const LinearCombination neg = -(lc * Scalar(2));
    if (neg.terms.size() != 3 || neg.terms[1].first.pub != 2 || !(neg.terms[1].second == -Scalar(14))) fail("the factor rides through the algebra", 0);
    Transcript t("");
    CircuitCompiler cc(t);
    cc.commit_placeholder();
    cc.constrain(lc);
    std::vector<uint32_t> ro, tv;
    std::vector<uint8_t> tc;
    cc.export_csr(ro, tv, tc, true);   // (v, 7), marker 1, (v, 7); the term with coefficient 0 is dropped
    if (tv.size() != 3 || tv[1] != ((BPR1CS_VAR_SCALE << 28) | 1u) || tv[0] != tv[2] || tc[32] != 1 || tc[64] != 7) fail("export: marker + term, zero terms dropped", tv.size());
    for (int which = 0; which < 3; which++) {
        try {
            if (which == 0) (void)Variable::One().times_public(0);
            if (which == 1) (void)Variable::Public(1).times_public(0);
            if (which == 2) (void)v.times_public(0).times_public(1);
            fail("times_public accepted One / Public / a second factor", which);
        } catch (const R1CSError& e) { if (e.code != BPR1CS_ERR_GADGET) fail("error code", which); }
    }
}

// a Prover evaluates, a Prover and a Verifier export: each refuses a public factor
static void refusals() {
    BulletproofGens bp(2, 1);
    PedersenGens pc(bp);
    for (int which = 0; which < 3; which++) {
        Transcript t("public-coefficient-refused");
        try {
            std::vector<uint32_t> ro, tv;
            std::vector<uint8_t> tc;
            if (which == 0) {
                Prover p(pc, t);
                auto cx = p.commit(Scalar(6), Scalar(11));
                p.multiply(LinearCombination(cx.second.times_public(0)), LinearCombination(cx.second));
            } else if (which == 1) {
                Prover p(pc, t);
                auto cx = p.commit(Scalar(6), Scalar(11));
                p.constrain(LinearCombination(cx.second.times_public(0)));
                p.export_csr(ro, tv, tc);
            } else {
                Verifier v(t);
                const Variable x = v.commit(CompressedRistretto{});
                v.constrain(LinearCombination(x.times_public(0)));
                v.export_csr(ro, tv, tc);
            }
            fail("a Prover / Verifier took a public factor", which);
        } catch (const R1CSError& e) { if (e.code != BPR1CS_ERR_GADGET) fail("error code", which); }
    }
}

int main() {
    for (size_t k : {1, 5, 70}) {
        std::vector<Scalar> items;
        for (size_t i = 0; i < k; i++) items.push_back(Scalar(0x1234567887654321ull + 977 * i) * Scalar(0xfedcba9876543210ull) + Scalar(7 + i));
        compare("set_membership_lean", items, k, 0, k, k + 1, [&](CircuitCompiler& cc, const std::vector<Scalar>& sp) { set_lean(cc, k, sp); });
    }
    const size_t shapes[3][2] = {{1, 8}, {5, 64}, {70, 16}};
    for (auto& s : shapes) {
        std::vector<Scalar> data;
        for (size_t i = 0; i <= s[0]; i++) data.push_back(Scalar(3 + 1000003 * i));
        // (the combination appears once as a row - negated - and once per bit operand as the hint; the rows hold k scaled + 1 linear term)
        compare("weighted_sum_bound", data, s[0], 1, s[1], s[0], [&](CircuitCompiler& cc, const std::vector<Scalar>& sp) { weighted(cc, s[0], s[1], sp); });
    }
    algebra();
    refusals();
    printf("%s\n", bad ? "FAIL" : "OK");
    return bad ? 1 : 0;
}
