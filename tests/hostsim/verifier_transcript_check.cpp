// The C++ Verifier (host/r1cs.hpp) on the caller's transcript, whatever it holds (bpr1cs_verify_batch with BPR1CS_LABEL_TRANSCRIPTS):
// (1) Prover and Verifier on Transcripts advanced alike accept, and the two transcripts then draw the same challenge; (2) a differing
// message rejects; (3) two proofs in sequence on ONE pair of transcripts - the second verify on a used transcript is the protocol's next
// proof, not a GadgetError - and in the other order both are rejected.  Linked against the CPU simulator.
#include <cstdio>
#include <cstring>
#include "../../bulletproofs-r1cs-gadgets_amd/host/r1cs.hpp"
using namespace bpr1cs;

struct Made {
    R1CSProof proof;
    std::vector<CompressedRistretto> comms;
};

// x * y = z with (x - 1) * (z - 37) = 25 for x = 6, y = 7, z = 42 (k = 0), and the same shape for other k: x = 6, y = 7 + k
template <class CS>
static void gadget(CS& cs, Variable vx, Variable vy, Variable vz, uint64_t k) {
    MulVars m1 = cs.multiply(LinearCombination(vx), LinearCombination(vy));
    cs.constrain(LinearCombination(m1.out) - LinearCombination(vz));
    MulVars m2 = cs.multiply(LinearCombination(m1.out) - LinearCombination(Scalar(37)), LinearCombination(vx) - LinearCombination(Scalar(1)));
    cs.constrain(LinearCombination(m2.out) - LinearCombination(Scalar(25 + 30 * k)));
}

static Made prove(const BulletproofGens& bp, const PedersenGens& pc, Transcript& t, uint64_t k) {
    Prover p(pc, t);
    std::array<uint8_t, 32> seed;
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(7 * i + 1 + k);
    p.set_rng_seed(seed);
    auto cx = p.commit(Scalar(6), Scalar(11 + k));
    auto cy = p.commit(Scalar(7 + k), Scalar(12 + k));
    auto cz = p.commit(Scalar(6 * (7 + k)), Scalar(13 + k));
    gadget(p, cx.second, cy.second, cz.second, k);
    R1CSProof pf = p.prove(bp);
    return Made{pf, {cx.first, cy.first, cz.first}};
}

// -> 1 accepted, 0 VerificationError, -1 anything else
static int verify(const BulletproofGens& bp, const PedersenGens& pc, Transcript& t, const Made& m, uint64_t k) {
    Verifier v(t);
    Variable vx = v.commit(m.comms[0]), vy = v.commit(m.comms[1]), vz = v.commit(m.comms[2]);
    gadget(v, vx, vy, vz, k);
    try {
        v.verify(m.proof, pc, bp);
        return 1;
    } catch (const R1CSError& e) {
        if (e.code == BPR1CS_ERR_VERIFICATION) return 0;
        printf("  R1CSError %d: %s\n", e.code, e.description.c_str());
        return -1;
    }
}

static bool same_challenge(Transcript& a, Transcript& b) {
    uint8_t x[32], y[32];
    a.challenge_bytes("after", x, 32);
    b.challenge_bytes("after", y, 32);
    return memcmp(x, y, 32) == 0;
}

int main() {
    int bad = 0;
    auto expect = [&](const char* what, bool ok) {
        printf("%s: %s\n", what, ok ? "ok" : "WRONG");
        if (!ok) bad++;
    };
    BulletproofGens bp(8, 1);
    PedersenGens pc(bp);
    {   // (1) fresh and advanced alike
        for (int advanced = 0; advanced < 2; advanced++) {
            Transcript tp("verifier-transcript"), tv("verifier-transcript");
            if (advanced) {
                tp.append_message("ctx", (const uint8_t*)"session 1", 9);
                tv.append_message("ctx", (const uint8_t*)"session 1", 9);
                uint8_t n1[16], n2[16];
                tp.challenge_bytes("nonce", n1, 16);
                tv.challenge_bytes("nonce", n2, 16);
            }
            Made m = prove(bp, pc, tp, 0);
            expect(advanced ? "advanced transcripts accept" : "fresh transcripts accept", verify(bp, pc, tv, m, 0) == 1);
            expect("  prover and verifier draw the same challenge afterwards", same_challenge(tp, tv));
        }
    }
    {   // (2) a differing message
        Transcript tp("verifier-transcript"), tv("verifier-transcript"), bare("verifier-transcript");
        tp.append_message("ctx", (const uint8_t*)"session 1", 9);
        tv.append_message("ctx", (const uint8_t*)"session 2", 9);
        Made m = prove(bp, pc, tp, 0);
        expect("a differing message rejects", verify(bp, pc, tv, m, 0) == 0);
        expect("the bare label rejects", verify(bp, pc, bare, m, 0) == 0);
    }
    {   // (3) two proofs in sequence on one pair of transcripts
        Transcript tp("verifier-transcript"), tv("verifier-transcript"), tw("verifier-transcript");
        for (Transcript* t : {&tp, &tv, &tw}) t->append_u64("round", 7);
        Made a = prove(bp, pc, tp, 0), b = prove(bp, pc, tp, 1);
        expect("first proof on the verifier's transcript", verify(bp, pc, tv, a, 0) == 1);
        expect("second verify on the used transcript is the next proof", verify(bp, pc, tv, b, 1) == 1);
        expect("  prover and verifier draw the same challenge afterwards", same_challenge(tp, tv));
        expect("the other order: the second proof first rejects", verify(bp, pc, tw, b, 1) == 0);
        expect("the other order: then the first rejects", verify(bp, pc, tw, a, 0) == 0);
    }
    printf("%s\n", bad ? "FAIL" : "OK");
    return bad;
}
