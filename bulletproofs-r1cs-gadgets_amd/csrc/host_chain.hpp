// The front of a SMALL job on host threads: Prover::new's and commit's transcript messages and the proof's TranscriptRng chain
// (reference call site src/gadget_vsmt_4.rs:434 `prover.prove(&bp_gens)` -> bulletproofs r1cs/prover.rs: `transcript.build_rng()
// .rekey_with_witness_bytes("v_blinding", ..) ... .finalize(&mut thread_rng())`, then 3 + 2n + 5 `Scalar::random(&mut rng)`; SURVEY
// 8a P6).  The chain is 2n + 8 Keccak-f[1600] permutations, each keyed by the one before: nothing inside ONE proof runs in parallel,
// and a GPU lane group needs 2.5 us per permutation (two dependent LDS round trips per round, k_rng_stream) where one x86-64 core
// needs 0.15-0.3 us.  A batch hides the device chain behind the sums of the job before it; a call of one or a few proofs - the
// reference's own call shape - has nothing to hide it behind, so there the chains run here, one proof per thread, while the device
// takes the wires and computes the A_I / A_O sums; the raw 64-byte draws are uploaded and reduced mod l by the same kernel
// (K_rng_reduce) that reads the device chain's output.  Same bytes either way (tests: tests/test_hostsim.py, tests/test_gpu_parity.py).
// This is hashing only: no group or field arithmetic runs on the host.
#pragma once
#include <thread>
#include <vector>
#include <atomic>
#include <algorithm>
#include <functional>
#include <mutex>
#include <condition_variable>
#include <chrono>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#if defined(__linux__)
#include <sched.h>
#endif
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#endif
#include "merlin.hpp"

// CPUs this process may actually use: the affinity mask and the cgroup's CPU quota (a container with 256 visible CPUs and a quota
// of 16 runs 16 threads' worth of work, whatever std::thread::hardware_concurrency says)
static unsigned host_cpu_budget() {
    static const unsigned cached = []() -> unsigned {
        unsigned n = std::thread::hardware_concurrency();
        if (n == 0) n = 1;
#if defined(__linux__)
        cpu_set_t set;
        CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof set, &set) == 0) {
            const int c = CPU_COUNT(&set);
            if (c > 0 && (unsigned)c < n) n = (unsigned)c;
        }
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {   // cgroup v2: "<quota> <period>" or "max <period>"
            char q[32];
            long long period = 0;
            if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
                const long long quota = atoll(q);
                if (quota > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, (quota + period - 1) / period));
            }
            fclose(f);
        } else {
            long long quota = -1, period = 0;   // cgroup v1
            if (FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(fq, "%lld", &quota) != 1) quota = -1; fclose(fq); }
            if (FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(fp, "%lld", &period) != 1) period = 0; fclose(fp); }
            if (quota > 0 && period > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, (quota + period - 1) / period));
        }
#endif
        return std::min<unsigned>(std::max<unsigned>(n, 1), 64);
    }();
    return cached;
}

// One proof: what K_transcript_init does (r1cs dom-sep, V x m, "m"; the RNG keyed with the blindings and the outside randomness) and
// then ALL 2n + 8 draws, raw, one after the other: raw[8 d .. 8 d + 8) = draw d (a proof's draws are contiguous: the threads of a
// job never write neighbouring cache lines).
static void host_front_chain(const strobe& init, const uint8_t* Vcomp /* m x 32 */, const uint8_t* v_blindings /* m x 32, canonical */,
                             const uint8_t seed[32], uint32_t m, uint32_t n, strobe* tr_out, uint64_t* raw) {
    strobe s = init;
    merlin_append(s, "dom-sep", 7, (const uint8_t*)"r1cs v1", 7);
    for (uint32_t j = 0; j < m; j++) merlin_append(s, "V", 1, Vcomp + 32 * (size_t)j, 32);
    merlin_append_u64(s, "m", 1, m);
    *tr_out = s;
    strobe r = s;
    for (uint32_t j = 0; j < m; j++) merlin_rng_rekey(r, "v_blinding", 10, v_blindings + 32 * (size_t)j, 32);
    merlin_rng_finalize(r, seed);
    const size_t draws = 2 * (size_t)n + 8;
    for (size_t d = 0; d < draws; d++) merlin_rng_raw(r, raw + 8 * d);
    for (int k = 0; k < 25; k++) ((volatile uint64_t*)r.st)[k] = 0;   // the RNG's key material
}

// ---- Eight chains at once.  Past its first draw every chain is in the same steady state (merlin_rng_raw: pos 64, pos_begin 0 -
// three word XORs and one permutation per draw), so eight proofs' states can share one set of AVX-512 registers: word k of proof p
// in lane p of register k.  Theta's column parities and chi are one vpternlogq each, rho one vprolq; the eight permutations are
// independent, so the core's vector pipes are filled where one scalar chain leaves most of them idle.  CPUs without AVX-512 (and
// the tests' reference) take the scalar merlin_rng_raw per lane, on the same layout.  (tests/hostsim/host_chain8_check.cpp builds a
// proof's steady state itself, from the transcript inputs, and compares every draw with host_front_chain.)
struct Chain8 {
    uint64_t st[25][8];   // [word][lane]: lanes >= the group's proofs are zero and never read
};
// draws [d, d + D) of the group's chains: draw i of lane p to out + p * ps + i * ds (8 words each; p < lanes)
static void chain8_advance_scalar(Chain8& g, unsigned lanes, uint32_t D, uint64_t* out, size_t ps, size_t ds) {
    for (unsigned p = 0; p < lanes; p++) {
        strobe s;
        for (int k = 0; k < 25; k++) s.st[k] = g.st[k][p];
        s.pos = 64; s.pos_begin = 0; s.cur_flags = SFLAG_I | SFLAG_A | SFLAG_C; s._pad = 0;
        for (uint32_t i = 0; i < D; i++) merlin_rng_raw(s, out + p * ps + i * ds);
        for (int k = 0; k < 25; k++) g.st[k][p] = s.st[k];
        explicit_bzero(s.st, sizeof s.st);
    }
}
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define HC8_TARGET __attribute__((target("avx512f")))
HC8_TARGET static void chain8_advance_avx512(Chain8& g, unsigned lanes, uint32_t D, uint64_t* out, size_t ps, size_t ds) {
#define X3(a, b, c) _mm512_ternarylogic_epi64(a, b, c, 0x96)      // a ^ b ^ c
#define CHI(a, b, c) _mm512_ternarylogic_epi64(a, b, c, 0xd2)     // a ^ (~b & c)
#define ROL(a, n) _mm512_rol_epi64(a, n)
    __m512i a00, a01, a02, a03, a04, a05, a06, a07, a08, a09, a10, a11, a12, a13, a14, a15, a16, a17, a18, a19, a20, a21, a22, a23, a24;
#define HC8_ALL(F) F(00) F(01) F(02) F(03) F(04) F(05) F(06) F(07) F(08) F(09) F(10) F(11) F(12) F(13) F(14) F(15) F(16) F(17) F(18) F(19) F(20) F(21) F(22) F(23) F(24)
#define HC8_LD(k) a##k = _mm512_loadu_si512((const void*)g.st[1##k - 100]);
#define HC8_ST(k) _mm512_storeu_si512((void*)g.st[1##k - 100], a##k);
    HC8_ALL(HC8_LD)
    const __m512i f8 = _mm512_set1_epi64((long long)0x0741000000401200ull), f9 = _mm512_set1_epi64(0x447), f20 = _mm512_set1_epi64((long long)0x8000000000000000ull);
    alignas(64) uint64_t w[8][8];
    for (uint32_t i = 0; i < D; i++) {
        a08 = _mm512_xor_si512(a08, f8); a09 = _mm512_xor_si512(a09, f9); a20 = _mm512_xor_si512(a20, f20);   // merlin_rng_raw's framing
        for (int r = 0; r < 24; r++) {
            const __m512i c0 = X3(X3(a00, a05, a10), a15, a20), c1 = X3(X3(a01, a06, a11), a16, a21), c2 = X3(X3(a02, a07, a12), a17, a22);
            const __m512i c3 = X3(X3(a03, a08, a13), a18, a23), c4 = X3(X3(a04, a09, a14), a19, a24);
            const __m512i r0 = ROL(c0, 1), r1 = ROL(c1, 1), r2 = ROL(c2, 1), r3 = ROL(c3, 1), r4 = ROL(c4, 1);
            // theta fused into rho + pi: B[y][2x+3y] = rol(A[x][y] ^ c[x-1] ^ rol(c[x+1], 1), r[x][y])
            const __m512i b00 = X3(a00, c4, r1),          b10 = ROL(X3(a01, c0, r2), 1),  b20 = ROL(X3(a02, c1, r3), 62), b05 = ROL(X3(a03, c2, r4), 28), b15 = ROL(X3(a04, c3, r0), 27);
            const __m512i b16 = ROL(X3(a05, c4, r1), 36), b01 = ROL(X3(a06, c0, r2), 44), b11 = ROL(X3(a07, c1, r3), 6),  b21 = ROL(X3(a08, c2, r4), 55), b06 = ROL(X3(a09, c3, r0), 20);
            const __m512i b07 = ROL(X3(a10, c4, r1), 3),  b17 = ROL(X3(a11, c0, r2), 10), b02 = ROL(X3(a12, c1, r3), 43), b12 = ROL(X3(a13, c2, r4), 25), b22 = ROL(X3(a14, c3, r0), 39);
            const __m512i b23 = ROL(X3(a15, c4, r1), 41), b08 = ROL(X3(a16, c0, r2), 45), b18 = ROL(X3(a17, c1, r3), 15), b03 = ROL(X3(a18, c2, r4), 21), b13 = ROL(X3(a19, c3, r0), 8);
            const __m512i b14 = ROL(X3(a20, c4, r1), 18), b24 = ROL(X3(a21, c0, r2), 2),  b09 = ROL(X3(a22, c1, r3), 61), b19 = ROL(X3(a23, c2, r4), 56), b04 = ROL(X3(a24, c3, r0), 14);
            a00 = CHI(b00, b01, b02); a01 = CHI(b01, b02, b03); a02 = CHI(b02, b03, b04); a03 = CHI(b03, b04, b00); a04 = CHI(b04, b00, b01);
            a05 = CHI(b05, b06, b07); a06 = CHI(b06, b07, b08); a07 = CHI(b07, b08, b09); a08 = CHI(b08, b09, b05); a09 = CHI(b09, b05, b06);
            a10 = CHI(b10, b11, b12); a11 = CHI(b11, b12, b13); a12 = CHI(b12, b13, b14); a13 = CHI(b13, b14, b10); a14 = CHI(b14, b10, b11);
            a15 = CHI(b15, b16, b17); a16 = CHI(b16, b17, b18); a17 = CHI(b17, b18, b19); a18 = CHI(b18, b19, b15); a19 = CHI(b19, b15, b16);
            a20 = CHI(b20, b21, b22); a21 = CHI(b21, b22, b23); a22 = CHI(b22, b23, b24); a23 = CHI(b23, b24, b20); a24 = CHI(b24, b20, b21);
            a00 = _mm512_xor_si512(a00, _mm512_set1_epi64((long long)KECCAK_RC[r]));
        }
        // the draw: words 0..7 (the squeezed bytes), then zeroed in the state; lanes become proofs by a transpose through w
        _mm512_store_si512((void*)w[0], a00); _mm512_store_si512((void*)w[1], a01); _mm512_store_si512((void*)w[2], a02); _mm512_store_si512((void*)w[3], a03);
        _mm512_store_si512((void*)w[4], a04); _mm512_store_si512((void*)w[5], a05); _mm512_store_si512((void*)w[6], a06); _mm512_store_si512((void*)w[7], a07);
        a00 = a01 = a02 = a03 = a04 = a05 = a06 = a07 = _mm512_setzero_si512();
        for (unsigned p = 0; p < lanes; p++) {
            uint64_t* o = out + p * ps + (size_t)i * ds;
            for (int k = 0; k < 8; k++) o[k] = w[k][p];
        }
    }
    HC8_ALL(HC8_ST)
    explicit_bzero(w, sizeof w);
#undef HC8_ALL
#undef HC8_LD
#undef HC8_ST
#undef X3
#undef CHI
#undef ROL
}
#endif
typedef void (*chain8_fn)(Chain8&, unsigned, uint32_t, uint64_t*, size_t, size_t);
static chain8_fn chain8_select(bool allow_avx512 = true) {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    if (allow_avx512 && __builtin_cpu_supports("avx512f")) return chain8_advance_avx512;
#endif
    (void)allow_avx512;
    return chain8_advance_scalar;
}

// How much of a job THAT FOLLOWS ANOTHER JOB OF ITS CALL the host takes by default (BPR1CS_OPT_HOST_CHAIN_SHARE = -1), in percent (the
// call's first job: host_chain_share_first below).  The host's part must be hashed before
// the heavy stream reaches the job's S sum, i.e. while it works through the job before: `deadline_ms`, the heavy stream's time per job
// measured so far in the call (its multiscalar launches, HIP-event timed).  The whole job costs B x draws x us_per_perm / workers of
// wall time on `workers` threads; the share is what fits into 3/4 of the deadline, at most 100.  None without the eight-way chain
// (scalar hashing is ~7x slower per thread) or with fewer than HOST_SHARE_MIN_WORKERS workers (host_cpu_budget() - 1: one CPU stays
// with the calling thread, which hands the chunks to the device).
static const unsigned HOST_SHARE_MIN_WORKERS = 2;
static int host_chain_share_auto(bool eight_way, uint64_t B, uint32_t draws, unsigned workers, double us_per_perm, double deadline_ms) {
    if (!eight_way || workers < HOST_SHARE_MIN_WORKERS || B == 0 || draws == 0 || !(us_per_perm > 0) || !(deadline_ms > 0)) return 0;
    const double whole_ms = (double)B * draws * us_per_perm / workers / 1e3;
    const double share = 100.0 * 0.75 * deadline_ms / whole_ms;
    return share >= 100.0 ? 100 : (int)share;
}
// The FIRST job of a call has no job before it to hide its chains behind: the device chain runs in the open, in front of the job's
// S sum, and the host's workers would idle.  Its default share is what makes both parts end together:
//   T_dev(Bd)  = draws x dev_us_per_perm x max(1, Bd / dev_cap)   k_rng_stream: latency-bound (one chain's own length) up to dev_cap
//                                                                 proofs - one wavefront on every SIMD, two proofs each - and
//                                                                 throughput-bound (LDS) above (profiles/r12a_call_start.txt)
//   T_host(Bh) = Bh x draws x us_per_perm / workers
// -> the Bh that minimises max(T_dev(B - Bh), T_host(Bh)): the balance point of the throughput-bound regime, and no more than
// B - dev_cap (below dev_cap the device part gets no shorter).  None for B <= dev_cap (the device chain is at its latency floor
// already), without the eight-way chain or HOST_SHARE_MIN_WORKERS workers, or when the model saves less than a tenth of T_dev(B).
// dev_us_per_perm on MI355X, for the depth-32 circuit's 37 319 draws (profiles/r12a_call_start.txt): the kernel alone on the chip takes
// 89.0 ms with one wavefront (2.38 us), 108.8 ms at 2048 proofs, 132.6 at 3072 and 154.0 at 4096 (2.06 us x 4096 / 2048); inside a
// call, next to the witness kernel and the A_I / A_O sums, 182 - 207 ms at 4096 (2.44 - 2.77 us x 2).  2.5 us: the model's line
// through the origin then balances at 39 % for 15 workers, where the measured line of the kernel alone (63.7 ms + 0.0220 ms per
// proof) balances at 40 %.
// Nor for a short chain: a split reads the states back, starts the workers and streams through the pinned ring - a millisecond or two
// that a circuit of a few dozen multipliers (a 7-bit bound check: 33 draws, 0.2 ms of chain for 4096 proofs) never earns back.
static const double DEV_CHAIN_US_PER_PERM = 2.5;
static const double HOST_SHARE_FIRST_MIN_SAVED_US = 2000.0;
// What the workers hash also has to reach the device: 64 bytes per draw and proof through the pinned ring and over the link.  In a
// trace of a first job with 1597 host chains (profiles/r12a_call_start.txt) the second half of their draws - 18 659 draws x 1597 proofs
// - took 79.8 ms to arrive: 0.0027 us per permutation and proof (24 GB/s), where 15 workers hash one in 0.0019.  The caller of
// host_chain_share_first counts a worker's rate only down to this floor times the workers.
static const double HOST_CHAIN_STREAM_US_PER_PERM = 0.0027;
static int host_chain_share_first(bool eight_way, uint64_t B, uint32_t draws, unsigned workers, double us_per_perm, uint32_t dev_cap,
                                  double dev_us_per_perm) {
    if (!eight_way || workers < HOST_SHARE_MIN_WORKERS || B == 0 || draws == 0 || !(us_per_perm > 0) || !(dev_us_per_perm > 0) || dev_cap == 0) return 0;
    if (B <= dev_cap) return 0;
    const double dev_rate = dev_us_per_perm / dev_cap, host_rate = us_per_perm / workers;   // us per permutation and proof of each side
    const uint64_t balance = (uint64_t)((double)B * dev_rate / (dev_rate + host_rate));
    const uint64_t Bh = std::min<uint64_t>(balance, B - dev_cap);
    const double t_all = (double)draws * dev_rate * (double)B;
    const double t_dev = (double)draws * dev_rate * (double)(B - Bh), t_host = (double)Bh * draws * host_rate;   // (B - Bh >= dev_cap)
    const double saved = t_all - std::max(t_dev, t_host);
    if (saved < 0.1 * t_all || saved < HOST_SHARE_FIRST_MIN_SAVED_US) return 0;
    return (int)((100 * Bh + B / 2) / B);
}
// Microseconds per permutation and chain of one worker of the eight-way chain: measured once on the calling thread (eight chains, 256
// draws: ~0.1 ms) with a 25 % margin for the workers sharing the package, then replaced by what each streamed job measured.
static std::atomic<double>& host_chain_rate_cell() {
    static std::atomic<double> cell{0.0};
    return cell;
}
static double host_chain_us_per_perm() {
    static const double calibrated = []() {
        Chain8 g;
        for (int k = 0; k < 25; k++)
            for (int p = 0; p < 8; p++) g.st[k][p] = 0x9e3779b97f4a7c15ull * (uint64_t)(25 * p + k + 1);
        std::vector<uint64_t> out((size_t)256 * 64);
        const chain8_fn fn = chain8_select();
        fn(g, 8, 16, out.data(), 8, 64);
        const auto t0 = std::chrono::steady_clock::now();
        fn(g, 8, 256, out.data(), 8, 64);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        return 1.25 * us / (256.0 * 8);
    }();
    const double measured = host_chain_rate_cell().load();
    return measured > 0 ? measured : calibrated;
}

// Draw-major streaming of P chains that start in the steady state (`st`: the RNG states K_transcript_init hands k_rng_stream):
// draws [0, draws) go out in chunks of D draws, chunk c as [D][P][8] words in ring slot c % R (ring: R x D x P x 8 words).  T worker
// threads own groups of 8 proofs (group k on thread k % T) and advance all their groups by one chunk at a time; the calling thread
// hands each finished chunk to upload(c, slot, first draw, draws) and, before a slot is written again, calls slot_free(slot) (blocks
// until the slot's last upload has been read).  -> false (nothing hashed) when a state is not the steady one.  busy_us: the workers'
// time spent hashing, summed over the threads (not their waits for a ring slot).
static bool host_chains_stream(const strobe* st, uint32_t P, uint32_t draws, uint32_t D, uint32_t R, uint64_t* ring, unsigned T,
                               const std::function<void(uint32_t, uint32_t, uint32_t, uint32_t)>& upload, const std::function<void(uint32_t)>& slot_free,
                               chain8_fn fn = chain8_select(), double* busy_us = nullptr) {
    for (uint32_t p = 0; p < P; p++)
        if (st[p].pos != 64 || st[p].pos_begin != 0) return false;
    if (P == 0 || draws == 0) return true;
    const uint32_t G = (P + 7) / 8, C = (draws + D - 1) / D;
    T = std::max(1u, std::min<unsigned>(T, G));
    std::mutex mu;
    std::condition_variable cv;
    uint32_t writable = R;                 // chunks below this may be written
    bool quit = false;                     // the calling thread failed (an upload): the workers stop
    std::vector<unsigned> done(R, 0);      // threads finished with the slot's current chunk
    double busy = 0;
    auto work = [&](unsigned t) {
        std::vector<Chain8> gs;
        for (uint32_t k = t; k < G; k += T) {
            Chain8 g;
            memset(&g, 0, sizeof g);
            for (uint32_t l = 0; l < 8 && 8 * k + l < P; l++)
                for (int w = 0; w < 25; w++) g.st[w][l] = st[8 * k + l].st[w];
            gs.push_back(g);
        }
        for (uint32_t c = 0; c < C; c++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return c < writable || quit; });
                if (quit) break;
            }
            const uint32_t d0 = c * D, nd = std::min(D, draws - d0);
            uint64_t* slot = ring + (size_t)(c % R) * D * P * 8;
            const auto t0 = std::chrono::steady_clock::now();
            for (size_t i = 0; i < gs.size(); i++) {
                const uint32_t k = t + (uint32_t)i * T;
                fn(gs[i], std::min(8u, P - 8 * k), nd, slot + (size_t)8 * 8 * k, 8, (size_t)P * 8);
            }
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            std::lock_guard<std::mutex> lk(mu);
            busy += us;
            done[c % R]++;
            cv.notify_all();
        }
        explicit_bzero(gs.data(), gs.size() * sizeof(Chain8));
    };
    std::vector<std::thread> pool;
    try {
        for (unsigned t = 0; t < T; t++) pool.emplace_back(work, t);
        for (uint32_t c = 0; c < C; c++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return done[c % R] == T; });
                done[c % R] = 0;
            }
            const uint32_t d0 = c * D;
            upload(c, c % R, d0, std::min(D, draws - d0));
            if (c + 1 >= R && c + 1 < C) {   // chunk c + 1 takes the slot of chunk c + 1 - R
                slot_free((c + 1) % R);
                std::lock_guard<std::mutex> lk(mu);
                writable = c + 2;
                cv.notify_all();
            }
        }
    } catch (...) {
        { std::lock_guard<std::mutex> lk(mu); quit = true; cv.notify_all(); }
        for (auto& th : pool) th.join();
        throw;
    }
    for (auto& th : pool) th.join();
    if (busy_us) *busy_us = busy;
    return true;
}

// The chains of a job's B proofs on up to host_cpu_budget() threads (started by the constructor, joined by wait() or the destructor:
// an exception between the two cannot leave a thread writing into released memory).
struct HostChains {
    std::vector<std::thread> pool;
    std::atomic<uint32_t> next{0};
    HostChains() {}
    HostChains(const HostChains&) = delete;
    HostChains& operator=(const HostChains&) = delete;
    // init: n_init = 1 (every proof from init[0]) or B states; raw_out: [B][2n + 8][8] words; tr_out: [B]
    void start(const strobe* init, size_t n_init, const uint8_t* Vcomp, const uint8_t* v_blindings, const uint8_t* seeds, uint32_t B, uint32_t m,
               uint32_t n, strobe* tr_out, uint64_t* raw_out) {
        auto work = [=]() {
            for (;;) {
                const uint32_t b = next.fetch_add(1);
                if (b >= B) return;
                host_front_chain(init[n_init == 1 ? 0 : b], Vcomp + (size_t)b * m * 32, v_blindings + (size_t)b * m * 32, seeds + 32 * (size_t)b, m, n,
                                 tr_out + b, raw_out + (size_t)b * 8 * (2 * (size_t)n + 8));
            }
        };
        const unsigned T = std::min<unsigned>(host_cpu_budget(), B);
        for (unsigned t = 0; t < T; t++) {
            try { pool.emplace_back(work); } catch (...) { break; }   // (no more threads to be had: wait() takes up what is left)
        }
        tail = work;
    }
    std::function<void()> tail;
    void wait() {
        if (tail) { tail(); tail = nullptr; }   // (whatever no thread has claimed - everything, if none could be started)
        for (auto& t : pool) t.join();
        pool.clear();
    }
    ~HostChains() { wait(); }
};
