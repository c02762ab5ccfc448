// The default host share of a call's FIRST job (csrc/host_chain.hpp host_chain_share_first), compiled for the host alone: the rule, not
// the hashing.  Prints "ok" or the first expectation that failed.
#include <stdio.h>
#include <math.h>
#include "host_chain.hpp"

static int fail(const char* what, int got, int want) {
    printf("FAIL %s: %d, expected %d\n", what, got, want);
    return 1;
}

int main() {
    const uint32_t draws = 37319, cap = 2048;     // the depth-32 VSMT-4 circuit's 2n + 7; MI355X: 1024 SIMDs, two proofs per wavefront
    const double host_us = 0.0287;                // profiles/r07b_host_chain_rate.txt
    const double dev_us = DEV_CHAIN_US_PER_PERM;  // profiles/r12a_call_start.txt
    // the balance by hand: device B - Bh proofs at dev_us / cap each, host Bh proofs at host_us / workers each, both ending together
    const double dr = dev_us / cap, hr = host_us / 15;
    const double by_hand = 100.0 * dr / (dr + hr);
    const int s = host_chain_share_first(true, 4096, draws, 15, host_us, cap, dev_us);
    printf("4096 proofs, 15 workers: share %d, balance by hand %.1f\n", s, by_hand);
    if (fabs(s - by_hand) > 5.0) return fail("4096 proofs, 15 workers", s, (int)by_hand);
    if (by_hand < 34.0 || by_hand > 44.0) return fail("the device constant left the measured range (39 % at 2.5 us)", (int)by_hand, 39);
    // at or below one wavefront per SIMD the device chain is at its latency floor: nothing to gain
    for (uint64_t B : {(uint64_t)1, (uint64_t)512, (uint64_t)2047, (uint64_t)cap}) {
        const int z = host_chain_share_first(true, B, draws, 15, host_us, cap, dev_us);
        if (z != 0) return fail("B <= dev_cap", z, 0);
    }
    if (int z = host_chain_share_first(true, 4096, draws, 1, host_us, cap, dev_us)) return fail("1 worker", z, 0);
    if (int z = host_chain_share_first(true, 4096, draws, 0, host_us, cap, dev_us)) return fail("no worker", z, 0);
    if (int z = host_chain_share_first(false, 4096, draws, 15, host_us, cap, dev_us)) return fail("scalar chain", z, 0);
    if (int z = host_chain_share_first(true, 4096, draws, 15, host_us, 0, dev_us)) return fail("unknown device", z, 0);
    // a chain too short to earn the split's set-up back (the 7-bit bound check of tests/test_gpu_parity.py: n = 13; a 64-bit one: n = 128)
    if (int z = host_chain_share_first(true, 4096, 2 * 13 + 7, 15, host_us, cap, dev_us)) return fail("33 draws", z, 0);
    if (int z = host_chain_share_first(true, 4096, 2 * 128 + 7, 15, host_us, cap, dev_us)) return fail("263 draws", z, 0);
    // never more than what leaves the device one wavefront per SIMD, never a split that saves less than a tenth, and monotone in the workers
    for (uint64_t B : {(uint64_t)2049, (uint64_t)2300, (uint64_t)3000, (uint64_t)4096, (uint64_t)8192, (uint64_t)26000}) {
        int prev = 0;
        for (unsigned w = 0; w <= 256; w++) {
            const int p = host_chain_share_first(true, B, draws, w, host_us, cap, dev_us);
            if (p < prev) return fail("the share decreases as workers increase", p, prev);
            if (p < 0 || p > 100) return fail("range", p, 0);
            const uint64_t Bh = (B * (uint64_t)p + 50) / 100;   // as JobDraws::choose rounds it
            if (p && B - Bh + B / 100 + 1 < cap) return fail("the device part fell below its capacity", (int)(B - Bh), (int)cap);
            if (p) {
                const double t_all = draws * dr * B, t_dev = draws * dr * (double)(B - Bh), t_host = (double)Bh * draws * host_us / w;
                if (t_all - (t_dev > t_host ? t_dev : t_host) < 0.08 * t_all) return fail("a split that saves under a tenth", p, 0);
            }
            prev = p;
        }
    }
    // host_chain_share_auto is what it was (a job that follows another): 3/4 of the deadline
    if (host_chain_share_auto(true, 4096, draws, 15, host_us, 1350.0) != 100) return fail("auto", host_chain_share_auto(true, 4096, draws, 15, host_us, 1350.0), 100);
    if (host_chain_share_auto(true, 4096, draws, 15, host_us, 100.0) != (int)(100.0 * 0.75 * 100.0 / (4096.0 * draws * host_us / 15 / 1e3))) return fail("auto, short deadline", 0, 0);
    printf("ok\n");
    return 0;
}
