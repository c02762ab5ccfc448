// Simulator-only recorder of what the multiscalar kernels' bodies DO with memory and control flow: every global / LDS
// address they form (relative to its buffer), every wave vote, every loop trip count and every launched grid goes through
// MSM_TRACE(kind, value) into one running (count, hash) pair per kind.  tests/test_secret_independent.py proves a circuit twice with
// different secrets and compares the recordings: equal for k_msm_fixed_ct's body (the contract of BPR1CS_OPT_SECRET_INDEPENDENT), different for
// msm_fixed2_body (the control: its gathers and votes follow the digits).  The lane-per-(chunk, proof) functor of jobs of <= 64 proofs
// (kernels.hpp K_msm_fixed_small) records its scalar loads too (MSM_TR_SCALAR, through the MSM_TRACE_F2 form: silent under f2_mute):
// tests/test_verify_grouped.py counts them to tell the grouped verifier's path from the per-proof one.  In the device build the macro
// expands to nothing: the shipped library has no recorder, no export for it, and k_msm_fixed2's instructions are what they were without it.
#pragma once
#include <stdint.h>

#define MSM_TR_SCALAR 0u   // global load of a scalar: element offset into its segment's array
#define MSM_TR_TABLE 1u    // global load of a table slot: byte offset into the job's table
#define MSM_TR_LDS 2u      // LDS access: uint16 index into the digit buffer
#define MSM_TR_STORE 3u    // global store of a chunk sum: element offset into the job's partial sums
#define MSM_TR_TRIP 4u     // loop trip count
#define MSM_TR_VOTE 5u     // outcome of a wave vote
#define MSM_TR_GRID 6u     // workgroups of a launch
#define MSM_TR_KINDS 7u

#if defined(BPR1CS_HOSTSIM)
struct MsmTrace {
    int on = 0;
    uint64_t count[MSM_TR_KINDS] = {}, hash[MSM_TR_KINDS] = {};
    uint64_t ct_launches = 0, fixed2_launches = 0;   // counted whether or not the recorder is on
    int f2_mute = 0;   // msm_fixed2_body's hooks (and K_msm_fixed_small's) are silent while set: a prove job sets it where its inner-product argument begins (outside
                       // the contract: l and r differ from batch to batch in either mode), so that the control recording is of the commit phase
};
inline MsmTrace& msm_trace() {
    static MsmTrace t;
    return t;
}
inline void msm_trace_put(uint32_t kind, uint64_t v) {
    MsmTrace& t = msm_trace();
    if (!t.on) return;
    t.count[kind]++;
    uint64_t h = (t.hash[kind] ^ v) * 0x9e3779b97f4a7c15ull;   // order-sensitive: the SEQUENCE is what is compared
    t.hash[kind] = h ^ (h >> 29);
}
#define MSM_TRACE(kind, v) msm_trace_put((kind), (uint64_t)(v))
#define MSM_TRACE_F2(kind, v) do { if (!msm_trace().f2_mute) msm_trace_put((kind), (uint64_t)(v)); } while (0)
#define MSM_TRACE_F2_MUTE(x) do { msm_trace().f2_mute = (x); } while (0)
#else
#define MSM_TRACE(kind, v) do { } while (0)
#define MSM_TRACE_F2(kind, v) do { } while (0)
#define MSM_TRACE_F2_MUTE(x) do { } while (0)
#endif
