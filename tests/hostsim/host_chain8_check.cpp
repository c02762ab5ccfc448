// Test-only (tests/test_host_chain8.py): the eight-way TranscriptRng chain of csrc/host_chain.hpp against the scalar
// host_front_chain, draw by draw.  argv[1] = 1: the AVX-512 path where the CPU has it, 0: the scalar fallback.
#include <random>
#include "host_chain.hpp"

// A proof's transcript and its chain up to the steady state, as host_front_chain makes them, and draw 0 (what K_transcript_init
// hands k_rng_stream and a job's host share).  false: the state after draw 0 is not the steady one.
static bool host_chain_head(const strobe& init, const uint8_t* Vcomp, const uint8_t* v_blindings, const uint8_t seed[32], uint32_t m,
                            strobe* tr_out, uint64_t raw0[8], Chain8& g, unsigned lane) {
    strobe s = init;
    merlin_append(s, "dom-sep", 7, (const uint8_t*)"r1cs v1", 7);
    for (uint32_t j = 0; j < m; j++) merlin_append(s, "V", 1, Vcomp + 32 * (size_t)j, 32);
    merlin_append_u64(s, "m", 1, m);
    *tr_out = s;
    strobe r = s;
    for (uint32_t j = 0; j < m; j++) merlin_rng_rekey(r, "v_blinding", 10, v_blindings + 32 * (size_t)j, 32);
    merlin_rng_finalize(r, seed);
    merlin_rng_raw(r, raw0);
    const bool steady = r.pos == 64 && r.pos_begin == 0;
    for (int k = 0; k < 25; k++) g.st[k][lane] = r.st[k];
    explicit_bzero(r.st, sizeof r.st);
    return steady;
}
static int fail(const char* what, int a, unsigned n, unsigned lanes, unsigned D) {
    printf("MISMATCH %s avx=%d n=%u lanes=%u D=%u\n", what, a, n, lanes, D);
    return 1;
}

int main(int argc, char** argv) {
    const bool avx = argc > 1 && atoi(argv[1]) != 0;
    const chain8_fn fn = chain8_select(avx);
    printf("path %s\n", fn == chain8_advance_scalar ? "scalar" : "avx512");
    std::mt19937_64 rng(20261016);
    // whole proofs from random inputs: the head (transcript, draw 0) on the host, then draws 1 .. 2n+7 eight at a time in chunks of D
    for (uint32_t n : {1u, 2u, 5u, 37u})
        for (unsigned lanes : {1u, 3u, 7u, 8u})
            for (uint32_t D : {1u, 3u, 7u, 13u, 64u}) {
                const uint32_t m = 1 + (uint32_t)(rng() % 3);
                const size_t draws = 2 * (size_t)n + 8;
                strobe init;
                uint8_t label[16];
                for (auto& x : label) x = (uint8_t)rng();
                merlin_new(init, label, 1 + (uint32_t)(rng() % 16));
                std::vector<uint8_t> V(lanes * m * 32), bl(lanes * m * 32), seeds(lanes * 32);
                for (auto& x : V) x = (uint8_t)rng();
                for (size_t i = 0; i < bl.size(); i++) bl[i] = (uint8_t)((i % 32) == 31 ? rng() & 0x0f : rng());   // canonical
                for (auto& x : seeds) x = (uint8_t)rng();
                std::vector<uint64_t> ref(lanes * draws * 8), got(lanes * draws * 8, 0);
                std::vector<strobe> tr(lanes), tr2(lanes);
                for (unsigned p = 0; p < lanes; p++) host_front_chain(init, &V[p * m * 32], &bl[p * m * 32], &seeds[p * 32], m, n, &tr[p], &ref[p * draws * 8]);
                Chain8 g;
                memset(&g, 0, sizeof g);
                for (unsigned p = 0; p < lanes; p++)
                    if (!host_chain_head(init, &V[p * m * 32], &bl[p * m * 32], &seeds[p * 32], m, &tr2[p], &got[p * draws * 8], g, p)) return fail("steady", avx, n, lanes, D);
                for (size_t d = 1; d < draws; d += D) fn(g, lanes, (uint32_t)std::min<size_t>(D, draws - d), &got[d * 8], draws * 8, 8);
                if (ref != got) return fail("draws", avx, n, lanes, D);
                if (memcmp(tr.data(), tr2.data(), lanes * sizeof(strobe))) return fail("transcript", avx, n, lanes, D);
            }
    // the draw-major stream a job uses: random steady states, groups of fewer than 8, chunks that do not divide the draws, small rings
    for (uint32_t P : {1u, 7u, 8u, 9u, 37u})
        for (uint32_t draws : {1u, 9u, 37u, 300u})
            for (uint32_t D : {1u, 5u, 64u})
                for (uint32_t R : {1u, 2u, 4u})
                    for (unsigned T : {1u, 3u}) {
                        std::vector<strobe> st(P);
                        for (auto& s : st) {
                            for (auto& w : s.st) w = rng();
                            s.pos = 64; s.pos_begin = 0; s.cur_flags = SFLAG_I | SFLAG_A | SFLAG_C; s._pad = 0;
                        }
                        std::vector<uint64_t> ref((size_t)draws * P * 8), got((size_t)draws * P * 8, 0), ring((size_t)R * D * P * 8);
                        for (uint32_t p = 0; p < P; p++) {
                            strobe s = st[p];
                            for (uint32_t d = 0; d < draws; d++) merlin_rng_raw(s, &ref[((size_t)d * P + p) * 8]);
                        }
                        const bool ok = host_chains_stream(st.data(), P, draws, D, R, ring.data(), T,
                            [&](uint32_t, uint32_t slot, uint32_t d0, uint32_t nd) { memcpy(&got[(size_t)d0 * P * 8], &ring[(size_t)slot * D * P * 8], (size_t)nd * P * 64); },
                            [&](uint32_t) {}, fn);
                        if (!ok || ref != got) return fail("stream", avx, P, draws, D);
                    }
    // a state that is not the steady one is refused before anything is hashed
    std::vector<strobe> bad(9);
    memset(bad.data(), 0, bad.size() * sizeof(strobe));
    for (auto& s : bad) s.pos = 64;
    bad[8].pos = 12;
    uint64_t ring[8 * 9 * 8];
    if (host_chains_stream(bad.data(), 9, 8, 8, 1, ring, 2, [](uint32_t, uint32_t, uint32_t, uint32_t) {}, [](uint32_t) {}, fn)) return fail("refuse", avx, 9, 8, 8);
    // the default share (host_chain_share_auto): a 4096-proof depth-32 job (37 319 draws) at the box's 0.0287 us per permutation
    if (host_chain_share_auto(true, 4096, 37319, 15, 0.0287, 1076.0) != 100) return fail("share 15 workers", avx, 0, 0, 0);   // 0.3 s of 1.08
    const int s3 = host_chain_share_auto(true, 4096, 37319, 3, 0.0287, 1076.0);                                               // 1.46 s whole
    if (s3 < 50 || s3 > 60) return fail("share 3 workers", avx, s3, 0, 0);
    if (host_chain_share_auto(true, 4096, 37319, 1, 0.0287, 1076.0) != 0) return fail("share 1 worker", avx, 0, 0, 0);
    if (host_chain_share_auto(true, 4096, 37319, 0, 0.0287, 1076.0) != 0) return fail("share 0 workers", avx, 0, 0, 0);
    if (host_chain_share_auto(false, 4096, 37319, 15, 0.0287, 1076.0) != 0) return fail("share scalar", avx, 0, 0, 0);
    const int s1 = host_chain_share_auto(true, 4096, 37319, 15, 0.0287, 37319 * 2.5e-3);                                     // the first job's chain
    if (s1 < 15 || s1 > 30) return fail("share chain deadline", avx, s1, 0, 0);
    if (host_chain_share_auto(true, 4096, 37319, 15, 0.0287, 0.0) != 0) return fail("share no deadline", avx, 0, 0, 0);
    if (!(host_chain_us_per_perm() > 0)) return fail("rate", avx, 0, 0, 0);
    printf("ok\n");
    return 0;
}
