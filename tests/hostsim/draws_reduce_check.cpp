// The K_rng_reduce launches a prove job describes for its TranscriptRng draws (csrc/prove_draws.hpp DrawsLayout), run on the CPU: the
// functor's operator() for every thread index of each described launch.  For every source the union of its ranges must write every
// slot of blind[1..8), s_L and s_R exactly once, with the value ONE whole-batch launch writes from the same draws.  The raw buffer is
// laid out as the job lays it out: the host part [draws][Bh][8] first, then the device part [draws][B - Bh][8].  Prints "ok" or the
// first expectation that failed.  No device, no job: the Bc / b0 / d0 arithmetic only.
#include <stdio.h>
#include <string.h>
#include <vector>
#define BPR1CS_DRAWS_LAYOUT_ONLY
#include "prove_draws.hpp"

struct Out {
    std::vector<sc> blind, sL, sR;   // [8][B], [n][B], [n][B]
    Out(uint32_t B, uint32_t n) : blind((size_t)8 * B), sL((size_t)n * B), sR((size_t)n * B) {}
    void fill(int byte) {
        if (!blind.empty()) memset(blind.data(), byte, blind.size() * sizeof(sc));
        if (!sL.empty()) memset(sL.data(), byte, sL.size() * sizeof(sc));
        if (!sR.empty()) memset(sR.data(), byte, sR.size() * sizeof(sc));
    }
    size_t slots() const { return blind.size() + sL.size() + sR.size(); }
    sc& at(size_t i) { return i < blind.size() ? blind[i] : i < blind.size() + sL.size() ? sL[i - blind.size()] : sR[i - blind.size() - sL.size()]; }
};
static bool untouched(const sc& x) {   // (a reduced scalar is below 2^253: never all ones)
    for (int k = 0; k < 8; k++) if (x.v[k] != 0xffffffffu) return false;
    return true;
}
static uint64_t rnd(uint64_t& s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s * 0x2545f4914f6cdd1dull; }

// run the launches one by one into a scratch, count the writes per slot, keep the values
struct Run {
    Out scratch, got;
    std::vector<uint32_t> writes;
    Run(uint32_t B, uint32_t n) : scratch(B, n), got(B, n), writes(scratch.slots(), 0) { got.fill(0xff); }
    DrawsLayout over(DrawsLayout l) { l.blind = scratch.blind.data(); l.sL = scratch.sL.data(); l.sR = scratch.sR.data(); return l; }
    bool launch(const DrawsReduce& r) {
        scratch.fill(0xff);
        for (uint64_t t = 0; t < r.threads; t++) r.k((uint32_t)t);
        uint64_t written = 0;
        for (size_t i = 0; i < scratch.slots(); i++)
            if (!untouched(scratch.at(i))) { written++; writes[i]++; got.at(i) = scratch.at(i); }
        return written == r.threads;   // (a thread writes one slot: fewer slots than threads = two threads on one slot)
    }
};

static int check(const char* what, uint32_t n, uint32_t B, uint32_t Bh, Run& run, Out& want, bool lead) {
    for (size_t i = 0; i < want.slots(); i++) {
        const bool i_bl = i < B;   // blind[0]: the lead form's own first draw, not one of the stream's
        const uint32_t w = i_bl && !lead ? 0u : 1u;
        if (run.writes[i] != w) { printf("FAIL %s n=%u B=%u Bh=%u: slot %zu written %u times, expected %u\n", what, n, B, Bh, i, run.writes[i], w); return 1; }
        if (!i_bl && memcmp(&run.got.at(i), &want.at(i), sizeof(sc))) { printf("FAIL %s n=%u B=%u Bh=%u: slot %zu differs from the whole-batch launch\n", what, n, B, Bh, i); return 1; }
    }
    return 0;
}

int main() {
    uint64_t seed = 0x9e3779b97f4a7c15ull;
    int cases = 0;
    for (uint32_t n : {0u, 1u, 128u, 254u})
        for (uint32_t B : {1u, 2u, 65u, 130u}) {
            const uint32_t draws = 2 * n + 7, d_half = n + 2;
            // the draws, [draws][B][8]: what one whole-batch launch reads
            std::vector<uint64_t> whole((size_t)draws * B * 8);
            for (auto& w : whole) w = rnd(seed);
            Out want(B, n);
            want.fill(0xff);
            {
                const DrawsReduce r = DrawsLayout{B, 0, n, draws, whole.data(), want.blind.data(), want.sL.data(), want.sR.data()}.reduce(DrawsPart::Whole, 0, draws);
                if (r.threads != (uint64_t)draws * B) { printf("FAIL whole n=%u B=%u: %llu threads\n", n, B, (unsigned long long)r.threads); return 1; }
                for (uint64_t t = 0; t < r.threads; t++) r.k((uint32_t)t);
            }
            // the lead form (the caller's draws, the chains of a small job): [B][2n + 8][8], one more draw in front
            {
                std::vector<uint64_t> raw((size_t)(draws + 1) * B * 8);
                for (uint32_t b = 0; b < B; b++)
                    for (uint32_t d = 0; d <= draws; d++)
                        for (int k = 0; k < 8; k++) raw[((size_t)b * (draws + 1) + d) * 8 + k] = d ? whole[((size_t)(d - 1) * B + b) * 8 + k] : rnd(seed);
                Run run(B, n);
                if (!run.launch(run.over(DrawsLayout{B, 0, n, draws, raw.data()}).reduce_lead())) { printf("FAIL lead n=%u B=%u: two threads on one slot\n", n, B); return 1; }
                if (check("lead", n, B, 0, run, want, true)) return 1;
                cases++;
            }
            const uint32_t shares[5] = {0, 1, (uint32_t)(((uint64_t)B * 50 + 50) / 100) /* as the job rounds a share of 50 % */, B - 1, B};
            for (uint32_t Bh : shares) {
                if (Bh > B) continue;
                // as the job lays it out: the host part first, then the device part, each contiguous per draw
                std::vector<uint64_t> raw((size_t)draws * B * 8);
                for (uint32_t d = 0; d < draws; d++)
                    for (uint32_t b = 0; b < B; b++) {
                        uint64_t* dst = b < Bh ? &raw[((size_t)d * Bh + b) * 8] : &raw[(size_t)draws * Bh * 8 + ((size_t)d * (B - Bh) + (b - Bh)) * 8];
                        memcpy(dst, &whole[((size_t)d * B + b) * 8], 64);
                    }
                for (int cut = 0; cut < 2; cut++) {
                    Run run(B, n);
                    const DrawsLayout lay = run.over(DrawsLayout{B, Bh, n, draws, raw.data()});
                    bool ok = true;
                    const uint32_t ends[3] = {0, cut ? d_half : draws, draws};
                    for (int leg = 0; leg < (cut ? 2 : 1); leg++) {
                        // a job reduces the parts it has: the host's if Bh > 0, the device's if Bh < B (with Bh = 0 that is the whole batch)
                        if (Bh) ok = ok && run.launch(lay.reduce(DrawsPart::Host, ends[leg], ends[leg + 1]));
                        if (Bh < B) ok = ok && run.launch(lay.reduce(DrawsPart::Device, ends[leg], ends[leg + 1]));
                    }
                    if (!ok) { printf("FAIL parts n=%u B=%u Bh=%u cut=%d: two threads on one slot\n", n, B, Bh, cut); return 1; }
                    if (check(cut ? "parts, cut" : "parts, uncut", n, B, Bh, run, want, false)) return 1;
                    cases++;
                    if (!Bh) {   // what a job without a host part launches: the second range, and an uncut chain, as whole-batch launches
                        Run run2(B, n);
                        const DrawsLayout lay2 = run2.over(DrawsLayout{B, 0, n, draws, raw.data()});
                        bool ok2 = true;
                        if (cut) ok2 = run2.launch(lay2.reduce(DrawsPart::Device, 0, d_half)) && run2.launch(lay2.reduce(DrawsPart::Whole, d_half, draws));
                        else ok2 = run2.launch(lay2.reduce(DrawsPart::Whole, 0, draws));
                        if (!ok2) { printf("FAIL whole n=%u B=%u cut=%d: two threads on one slot\n", n, B, cut); return 1; }
                        if (check(cut ? "whole, cut" : "whole, uncut", n, B, 0, run2, want, false)) return 1;
                        cases++;
                    }
                }
            }
        }
    printf("%d cases\nok\n", cases);
    return 0;
}
