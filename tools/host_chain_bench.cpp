// Rate of the host-side TranscriptRng chain (csrc/host_chain.hpp) on this machine: microseconds per Keccak-f[1600] permutation of
// a chain of `draws` draws, on 1 .. 2 x budget threads at once, and what host_cpu_budget() reports.
//   g++ -O3 -std=c++17 -DBPR1CS_HOST_ONLY -Ibulletproofs-r1cs-gadgets_amd/csrc tools/host_chain_bench.cpp -o /tmp/hcb -pthread && /tmp/hcb
#include <chrono>
#include <stdio.h>
#include "host_chain.hpp"

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)atoi(argv[1]) : 18656, m = 100;
    printf("host_cpu_budget = %u, hardware_concurrency = %u, bmi path = %d\n", host_cpu_budget(), std::thread::hardware_concurrency(),
           (int)(keccak_host_select() != keccak_f1600_host_generic));
    strobe init;
    merlin_new(init, (const uint8_t*)"bench", 5);
    const size_t draws = 2 * (size_t)n + 8;
    for (unsigned T : {1u, 2u, 4u, 8u, 16u, 32u, 64u}) {
        const uint32_t B = T;
        std::vector<uint8_t> V((size_t)B * m * 32, 7), bl((size_t)B * m * 32, 1), seeds((size_t)B * 32, 3);
        std::vector<uint64_t> raw(draws * B * 8);
        std::vector<strobe> tr(B);
        for (int rep = 0; rep < 2; rep++) {
            auto t0 = std::chrono::steady_clock::now();
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < T; t++)
                pool.emplace_back([&, t]() { host_front_chain(init, V.data() + (size_t)t * m * 32, bl.data() + (size_t)t * m * 32, seeds.data() + 32 * t, m, n, &tr[t], raw.data() + (size_t)t * 8 * draws); });
            for (auto& th : pool) th.join();
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (rep) printf("%2u threads x 1 chain of %zu draws: %.2f ms wall, %.3f us per permutation per chain (%016llx)\n", T, draws, us / 1e3, us / draws, (unsigned long long)raw[8 * 5]);
        }
    }
    // the eight-way chain (csrc/host_chain.hpp chain8_*): one thread, eight steady-state chains, scalar fallback and AVX-512
    for (int avx = 0; avx < 2; avx++) {
        const chain8_fn fn = chain8_select(avx != 0);
        Chain8 g;
        for (int k = 0; k < 25; k++)
            for (int p = 0; p < 8; p++) g.st[k][p] = 0x9e3779b97f4a7c15ull * (uint64_t)(25 * p + k + 1);
        const uint32_t D = 8192;
        std::vector<uint64_t> out((size_t)D * 64);
        fn(g, 8, 512, out.data(), 8, 64);
        auto t0 = std::chrono::steady_clock::now();
        fn(g, 8, D, out.data(), 8, 64);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("1 thread x 8 chains (%s): %.4f us per permutation per chain\n", fn == chain8_advance_scalar ? "scalar fallback" : "avx512", us / D / 8);
    }
    return 0;
}
