// The secret-independent twin of the dominant kernel (BPR1CS_OPT_SECRET_INDEPENDENT): batched fixed-base multiscalar
// multiplication over the NARROW table set (MSM_CT_W-bit signed windows) whose sequence of memory addresses, branch outcomes and
// trip counts is a function of the launch geometry alone - never of a scalar.  ONE body (msm_fixed_ct_body) serves the gfx950 kernel
// and the CPU simulator, as msm_fixed2_body does; the simulator's build reports every address it forms to the recorder of
// msm_trace.hpp, which is how the property is tested.
//
//   * Same geometry as k_msm_fixed2: one wavefront per workgroup = 64 consecutive proofs of one chunk of the term list.  All 64
//     lanes walk the SAME row of the same base, so the row address is wave-uniform and public.
//   * Per window the wavefront reads the WHOLE row - identity slot and the 2^(W-1) multiples, 27 limbs each - at wave-uniform
//     addresses through the constant address space: scalar loads (s_load_dwordx8 / x4 / x2 / x1 into scalar registers), slot by slot
//     (27 limbs in, 27 selects, next slot: a row of 9 slots is 243 limbs, a wavefront has ~100 scalar registers).  Each lane keeps
//     its entry with a full scan of compare + bit-select (v_bfi_b32 under an all-ones / zero mask) over the slots; digit 0 keeps slot 0, the identity, by the same scan.
//     No per-lane table address exists anywhere in the kernel: its only vector loads from global memory are the scalars, whose
//     addresses are given by the proof index.
//   * Every term of every chunk is processed: no vote, no zero-term skipping, no (wire - 1) form, no produced (MsmGeo) scalars.
//   * Recoding as msm_recode (branch-free), digits through LDS at lane-fixed addresses ([windows][64] uint16, one buffer: a lane
//     reads back only what it wrote itself, so the wavefront needs no barrier).
//   * Sign of a digit by the polarity of the accumulator (as k_msm_fixed2: branch-free).
//   * Vector stores only; no scratch.
#pragma once
#include "msm_kernel.hpp"

#define MSM_CT_W 4u   // window bits of the narrow table set: 64 windows x 9 slots x 128 B = 73.7 KB per base
#define MSM_CT_WINDOWS ((252u + MSM_CT_W) / MSM_CT_W)

#if defined(BPR1CS_HOSTSIM)
typedef const uint32_t* msm_ct_slot_t;
#else
typedef const __attribute__((address_space(4))) uint32_t* msm_ct_slot_t;   // constant address space: a wave-uniform load from it is a scalar load
#endif

// lane `lane` of logical workgroup `wg_raw`; msm_dig: [windows][64] uint16 (LDS on the device)
MSM_FN void msm_fixed_ct_body(const MsmLaunch& L, uint32_t wg_raw, const uint32_t lane, uint16_t* msm_dig) {
    uint32_t wg = wg_raw;
    if ((L.nwg & 7u) == 0) wg = (wg & 7u) * (L.nwg >> 3) + (wg >> 3);  // XCD-aware, as k_msm_fixed2
    uint32_t j = 0, w0 = 0;
#pragma unroll
    for (uint32_t t = 0; t + 1 < MSM_MAX_JOBS; t++)
        if (t + 1 < L.njobs && wg >= L.wg_end[t]) { j = t + 1; w0 = L.wg_end[t]; }
    if (wg >= L.wg_end[L.njobs - 1]) return;  // padding up to a multiple of 8
    j = MsmWave::uniform(j);
    const MsmJob& J = L.job[j];
    const TabCfg tc = J.tc;
    wg -= w0;
    const uint32_t B = L.B, c = wg / L.nbk, b0 = (wg % L.nbk) * 64u;
    uint32_t b = b0 + lane;
    const bool active = b < B;
    if (!active) b = B - 1;  // ragged batch: the spare lanes repeat the last proof and do not store
    const uint32_t total = J.seg[0].count + J.seg[1].count;
    const uint32_t lo = c * J.chunk;
    const uint32_t hi = lo + J.chunk < total ? lo + J.chunk : total;
    const size_t row_bytes = (size_t)tc.row * tc.stride;
    MSM_TRACE(MSM_TR_TRIP, hi - lo);

    ge acc = ge_identity();
    int32_t pol = 0;  // 0: acc = +S, -1: acc = -S
    for (uint32_t o = lo; o < hi; o++) {
        const MsmTerm T = msm_term(J, o, B, tc, L.geo);   // (plain segments only: the host never gives this kernel a produced scalar)
        MSM_TRACE(MSM_TR_SCALAR, (T.scal - (o < J.seg[0].count ? J.seg[0].scal : J.seg[1].scal)) + b);
        sc x = T.scal[b];
        if (T.mont) x = sc_from_mont(x);   // (the form is the segment's: wave-uniform and public)
        msm_recode(x, msm_dig + lane, tc);
        MSM_TRACE(MSM_TR_TRIP, tc.windows);
        for (uint32_t k = 0; k < tc.windows; k++) {
            MSM_TRACE(MSM_TR_LDS, k * 64u + lane);
            const uint32_t d = msm_dig[k * 64u + lane];
            const uint32_t mag = d & 0x7fffu;
            // ---- the lane's entry: a scan over the whole row at wave-uniform addresses
            const uint8_t* rowp = T.tab + (size_t)k * row_bytes;
            MsmEntry E;
            {
                MSM_TRACE(MSM_TR_TABLE, rowp - J.tab);
                msm_ct_slot_t s0 = (msm_ct_slot_t)(uintptr_t)rowp;
#pragma unroll
                for (int i = 0; i < 27; i++) E.w[i] = s0[i];   // slot 0: the identity (digit 0)
            }
            MSM_TRACE(MSM_TR_TRIP, tc.entries);
            for (uint32_t s = 1; s <= tc.entries; s++) {
                MSM_TRACE(MSM_TR_TABLE, rowp + (size_t)s * tc.stride - J.tab);
                msm_ct_slot_t sp = (msm_ct_slot_t)(uintptr_t)(rowp + (size_t)s * tc.stride);
                // the select as mask arithmetic, (v & m) | (E & ~m): every limb of every slot is loaded and used unconditionally.  Written
                // as `take ? v : E` the compiler moved the loads of a slot under a branch on "any lane of the wavefront takes it" - a vote
                // on digits.
                const uint32_t m = 0u - (uint32_t)(mag == s);
#pragma unroll
                for (int i = 0; i < 27; i++) {
                    const uint32_t v = sp[i];
                    E.w[i] = (v & m) | (E.w[i] & ~m);
                }
            }
            // ---- the mixed addition (as k_msm_fixed2's two layers; the sign enters through the accumulator's polarity)
            const int32_t sgn = -(int32_t)(d >> 15);   // -1: negative digit
            const int32_t flip = sgn ^ pol;
            const uint32_t fadd = (uint32_t)flip & 1u;
            pol = sgn;
#pragma unroll
            for (int i = 0; i < 9; i++) {
                acc.X.v[i] = (int32_t)(((uint32_t)acc.X.v[i] ^ (uint32_t)flip) + fadd);
                acc.T.v[i] = (int32_t)(((uint32_t)acc.T.v[i] ^ (uint32_t)flip) + fadd);
            }
            ge_niels q = msm_entry_unpack(E);
            fe PP = fe_mul_f(fe_add(acc.Y, acc.X), q.yplusx);
            fe MM = fe_mul_f(fe_sub(acc.Y, acc.X), q.yminusx);
            fe Txy2d = fe_mul_f(acc.T, q.xy2d);
            fe cX = fe_sub(PP, MM), cY = fe_add(PP, MM);
            fe cZ = fe_add(acc.Z, Txy2d), cT = fe_sub(acc.Z, Txy2d);
            acc.X = fe_mul_f(cX, cT); acc.Y = fe_mul_f(cY, cZ); acc.Z = fe_mul(cZ, cT); acc.T = fe_mul_f(cX, cY);
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
        acc.X.v[i] = (acc.X.v[i] ^ pol) - pol;
        acc.T.v[i] = (acc.T.v[i] ^ pol) - pol;
    }
    if (active) {
        MSM_TRACE(MSM_TR_STORE, (size_t)c * B + b);
        J.partial[(size_t)c * B + b] = ge_from_table_class(acc);
    }
}

#if defined(BPR1CS_HOSTSIM)
inline void msm_fixed_ct_sim(const MsmLaunch& L) {
    std::vector<uint16_t> dig((size_t)L.max_windows * 64u);
    for (uint32_t wg = 0; wg < L.nwg; wg++)
        for (uint32_t lane = 0; lane < 64; lane++) msm_fixed_ct_body(L, wg, lane, dig.data());
}
#else
// 3 wavefronts per SIMD (<= 168 VGPRs), 8 KB of LDS per workgroup (64 windows x 64 lanes x 2 B): LDS would allow 5 per SIMD, the
// registers of the field arithmetic decide - as for k_msm_fixed2
__global__ void __launch_bounds__(64, 3) k_msm_fixed_ct(const MsmLaunch L) {
    __shared__ uint16_t msm_ct_dig[MSM_CT_WINDOWS * 64u];  // [windows][64]
    msm_fixed_ct_body(L, blockIdx.x, threadIdx.x, msm_ct_dig);
}
#endif
