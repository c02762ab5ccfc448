// k_rng_stream alone on the chip: milliseconds for `draws` draws (default 37 319: the depth-32 VSMT-4 circuit's 2n + 7) at 1024, 2048,
// 3072 and 4096 proofs, HIP-event timed, second of two launches each - where the TranscriptRng chain stops being latency-bound and
// what it costs per proof above that (csrc/host_chain.hpp host_chain_share_first is fitted to these numbers).  Also checks that a chain
// made in two launches, the second resuming from the states the first wrote back, gives the words of one launch.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Ibulletproofs-r1cs-gadgets_amd/csrc tools/rng_stream_probe.hip -o tools/rng_stream_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "kernels_hip.hpp"
#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
    const uint32_t draws = argc > 1 ? (uint32_t)atoi(argv[1]) : 37319u;
    const uint32_t Bmax = 4096;
    hipDeviceProp_t prop;
    CHK(hipGetDeviceProperties(&prop, 0));
    printf("%s, %d CUs; %u draws per chain\n", prop.name, prop.multiProcessorCount, draws);
    std::vector<strobe> h(Bmax);
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (auto& s : h) {
        for (int k = 0; k < 25; k++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; s.st[k] = x; }
        s.pos = 64; s.pos_begin = 0; s.cur_flags = 0; s._pad = 0;
    }
    strobe *st, *st2;
    uint64_t *raw, *raw2;
    int* err;
    const size_t raw_bytes = (size_t)draws * Bmax * 64;
    CHK(hipMalloc(&st, Bmax * sizeof(strobe))); CHK(hipMalloc(&st2, Bmax * sizeof(strobe)));
    CHK(hipMalloc(&raw, raw_bytes)); CHK(hipMalloc(&err, sizeof(int)));
    CHK(hipMemcpy(st, h.data(), Bmax * sizeof(strobe), hipMemcpyHostToDevice));
    CHK(hipMemset(err, 0, sizeof(int)));
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    const uint32_t sizes[] = {2, 1024, 2048, 3072, 4096};
    for (uint32_t B : sizes) {
        float ms = 0;
        for (int rep = 0; rep < 2; rep++) {
            CHK(hipEventRecord(e0));
            hipLaunchKernelGGL(k_rng_stream, dim3((B + 1) / 2), dim3(64), 0, 0, (const strobe*)st, raw, err, B, draws, (strobe*)nullptr);
            CHK(hipGetLastError());
            CHK(hipEventRecord(e1));
            CHK(hipEventSynchronize(e1));
            CHK(hipEventElapsedTime(&ms, e0, e1));
        }
        printf("B = %4u: %8.2f ms   %.3f us per permutation of a chain   %.4f us per permutation and proof\n", B, ms, 1e3 * ms / draws, 1e3 * ms / draws / B);
    }
    // two legs against one launch: 131 proofs (the last wavefront carries one), a short chain cut at an odd draw
    {
        const uint32_t B = 131, D = 523, cut = 258;
        const size_t words = (size_t)D * B * 8;
        CHK(hipMalloc(&raw2, words * 8));
        std::vector<uint64_t> one(words), two(words);
        hipLaunchKernelGGL(k_rng_stream, dim3((B + 1) / 2), dim3(64), 0, 0, (const strobe*)st, raw, err, B, D, (strobe*)nullptr);
        CHK(hipMemcpy(one.data(), raw, words * 8, hipMemcpyDeviceToHost));
        CHK(hipMemset(raw2, 0, words * 8));
        hipLaunchKernelGGL(k_rng_stream, dim3((B + 1) / 2), dim3(64), 0, 0, (const strobe*)st, raw2, err, B, cut, st2);
        hipLaunchKernelGGL(k_rng_stream, dim3((B + 1) / 2), dim3(64), 0, 0, (const strobe*)st2, raw2 + (size_t)cut * B * 8, err, B, D - cut, st2);
        CHK(hipMemcpy(two.data(), raw2, words * 8, hipMemcpyDeviceToHost));
        int e = 0;
        CHK(hipMemcpy(&e, err, sizeof(int), hipMemcpyDeviceToHost));
        const bool same = memcmp(one.data(), two.data(), words * 8) == 0;
        printf("two legs (%u + %u draws, %u proofs) %s one launch; refused states: %d\n", cut, D - cut, B, same ? "==" : "DIFFER FROM", e);
        if (!same || e) return 1;
    }
    return 0;
}
