// C ABI: the verifier: per proof, cross-proof batched, split for several GPUs.
#pragma once
#include "msm_run.hpp"
// ---------------------------------------------------------------- verifier
static const uint32_t VERIFY_HOST_TRANSCRIPT_MAX_PROOFS = 8;
struct VerifyCtx {  // device state shared by the per-proof and the cross-proof verifier
    uint32_t B, n, m, N, lgN, H, P;
    uint32_t p = 0;                 // public inputs per proof
    const uint8_t* d_pub = nullptr; // [B][p][32] canonical bytes: the tail block of `commitments`, behind the points in d_vc
    size_t plen;
    DevBuf<uint8_t> d_pf, d_vc, d_seed, d_label, bind;
    DevBuf<sc> chal, uk, plo, phi, wvec, gh, dpart, delta, bsc;
    DevBuf<int> fail;
    DevBuf<strobe> d_init, d_after;   // caller transcripts (VerifyStart): the starting states and, read back, the states afterwards
};
// Where the proofs' transcripts start: Transcript::new(label), or - BPR1CS_LABEL_TRANSCRIPTS in label_len - the caller's own transcripts.
// `init` is a snapshot taken once per call (a retry after OUT_OF_MEMORY replays from the same states); `after`, when set, receives
// the state of every proof after its last inner-product challenge from the call's FIRST replay, and the extern "C" wrapper writes it
// to the handles once the call has succeeded.
struct VerifyStart {
    const uint8_t* label = nullptr;
    size_t label_len = 0;
    const strobe* init = nullptr;
    size_t n_init = 0;           // 0: the label form; 1: every proof from init[0]; batch: proof b from init[b]
    strobe* after = nullptr;     // [batch] host memory, only with n_init == batch
    VerifyStart sub(const std::vector<strobe>& gathered) const {   // a sub-batch of the same call: its own starting states, nothing written back
        VerifyStart s = *this;
        s.after = nullptr;
        if (n_init > 1) { s.init = gathered.data(); s.n_init = gathered.size(); }
        return s;
    }
};
struct VerifyHandles {   // the parsed (label, label_len) of an entry point
    VerifyStart ts;
    std::vector<strobe> init, after;
    bpr1cs_transcript* const* handles = nullptr;
    int parse(const uint8_t* label, size_t label_len, size_t batch) {
        ts.label = label; ts.label_len = label_len;
        if (!(label_len & BPR1CS_LABEL_TRANSCRIPTS)) return BPR1CS_OK;
        const size_t count = label_len & ~BPR1CS_LABEL_TRANSCRIPTS;
        if (!label || batch == 0 || (count != 1 && count != batch)) return BPR1CS_ERR_INVALID_ARGUMENT;
        handles = (bpr1cs_transcript* const*)(const void*)label;
        for (size_t i = 0; i < count; i++)
            if (!handles[i]) return BPR1CS_ERR_INVALID_ARGUMENT;
        try {
            if (count == batch && batch > 1) {   // the same handle twice: which state would it be left in?
                std::vector<const bpr1cs_transcript*> sorted(handles, handles + count);
                std::sort(sorted.begin(), sorted.end());
                if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return BPR1CS_ERR_INVALID_ARGUMENT;
            }
            init.resize(count);
            for (size_t i = 0; i < count; i++) init[i] = handles[i]->s;
            if (count == batch) { after.resize(batch); ts.after = after.data(); }
        } catch (const std::bad_alloc&) { return BPR1CS_ERR_OUT_OF_MEMORY; }
        ts.label = (const uint8_t*)"";   // never read
        ts.label_len = 0;
        ts.init = init.data();
        ts.n_init = count;
        return BPR1CS_OK;
    }
    int finish(int rc) {   // the handles of a call that succeeded: where upstream's &mut transcript is when verify() returns
        if (rc == BPR1CS_OK && ts.after)
            for (size_t i = 0; i < after.size(); i++) handles[i]->s = after[i];
        return rc;
    }
};
static int verify_args_ok(const bpr1cs_gens* g, const bpr1cs_circuit* c, const uint8_t* label, const uint8_t* proofs, const uint8_t* commitments, size_t batch) {
    if (!g || !c || !label || !proofs || batch == 0 || batch > (1u << 20)) return BPR1CS_ERR_INVALID_ARGUMENT;
    if ((c->m || c->p) && !commitments) return BPR1CS_ERR_INVALID_ARGUMENT;
    if (!have_device()) return BPR1CS_ERR_NO_DEVICE;
    if (g->cap < c->N) return BPR1CS_ERR_INVALID_GENERATORS_LENGTH;
    if (((uint64_t)4 * c->N + 3ull * c->n + c->m + c->p + 64) * batch > 0xffffffffull) return BPR1CS_ERR_INVALID_ARGUMENT;
    return BPR1CS_OK;
}
// transcript replay, flattened constraints, mega-check scalars of the shared bases: gh = g_i | h_i (canonical), bsc (Montgomery)
static void verify_front(VerifyCtx& v, const bpr1cs_gens* g, const bpr1cs_circuit* c, const VerifyStart& ts, const uint8_t* proofs,
                         const uint8_t* commitments, const uint8_t* verifier_rng_seeds, size_t batch, bool want_bind, dev_stream_t st) {
    const uint32_t B = v.B = (uint32_t)batch, n = v.n = c->n, m = v.m = c->m, N = v.N = c->N, lgN = v.lgN = c->lgN;
    const uint32_t p = v.p = c->p;
    v.plen = bpr1cs_proof_len(c);
    const uint8_t* label = ts.label;
    const size_t label_len = ts.label_len;
    v.d_pf.alloc((size_t)B * v.plen); v.d_vc.alloc((size_t)B * (m + p) * 32 + 1); v.d_seed.alloc((size_t)B * 32); v.d_label.alloc(label_len ? label_len : 1);
    dev_h2d(v.d_pf.p, proofs, (size_t)B * v.plen, st);
    if (m + p) dev_h2d(v.d_vc.p, commitments, (size_t)B * (m + p) * 32, st);   // the points and, behind them, the public inputs: one block
    v.d_pub = v.d_vc.p + (size_t)B * m * 32;
    if (verifier_rng_seeds) dev_h2d(v.d_seed.p, verifier_rng_seeds, (size_t)B * 32, st);
    else dev_zero(v.d_seed.p, (size_t)B * 32, st);
    if (label_len) dev_h2d(v.d_label.p, label, label_len, st);
    v.chal.alloc((size_t)VCH_COUNT * B); v.uk.alloc((size_t)(lgN ? lgN : 1) * 2 * B);
    v.fail.alloc(B);
    dev_zero(v.fail.p, sizeof(int) * B, st);
    K_verify_transcript kt{v.d_label.p, (uint32_t)label_len, v.d_pf.p, v.d_vc.p, v.d_seed.p, v.chal.p, v.uk.p, v.fail.p, B, m, lgN, (uint32_t)v.plen, (uint64_t)N};
    if (want_bind) { v.bind.alloc((size_t)B * 32); kt.bind = v.bind.p; }
    const uint32_t init_stride = ts.n_init > 1 ? 1 : 0;
    bool after_on_device = false;
#if !defined(BPR1CS_HOSTSIM)
    const bool host_replay = B <= VERIFY_HOST_TRANSCRIPT_MAX_PROOFS && g->opts.host_chain.load() != 0;
#else
    const bool host_replay = false;
#endif
    if (ts.init && !host_replay) {   // 216 bytes per state up and, where the handles follow their proofs, down again
        v.d_init.alloc(ts.n_init);
        dev_h2d(v.d_init.p, ts.init, ts.n_init * sizeof(strobe), st);
        kt.init = v.d_init.p; kt.init_stride = init_stride;
        if (ts.after) { v.d_after.alloc(B); kt.tr_out = v.d_after.p; after_on_device = true; }
    }
#if !defined(BPR1CS_HOSTSIM)
    // A handful of proofs: the transcript replay - every byte it hashes is public and in the caller's memory - runs on the calling
    // thread (the same functor, host STROBE: ~150 appends and 20 challenges of a depth-32 proof in ~50 us) and its challenges go up;
    // on the device it is one lane per proof walking the appends a state word at a time: 1.2 of a depth-32 verification's 3.3 ms.
    // (BPR1CS_OPT_HOST_CHAIN_PROOFS = 0 keeps every transcript on the device, as for the prover.)
    if (host_replay) {
        std::vector<sc> h_chal((size_t)VCH_COUNT * B), h_uk((size_t)(lgN ? lgN : 1) * 2 * B);
        std::vector<int> h_fail(B, 0);
        std::vector<uint8_t> h_bind(want_bind ? (size_t)B * 32 : 0), zero_seeds;
        const uint8_t* seeds = verifier_rng_seeds;
        if (!seeds) { zero_seeds.assign((size_t)B * 32, 0); seeds = zero_seeds.data(); }
        K_verify_transcript kh{label, (uint32_t)label_len, proofs, commitments, seeds, h_chal.data(), h_uk.data(), h_fail.data(), B, m, lgN, (uint32_t)v.plen, (uint64_t)N};
        if (want_bind) kh.bind = h_bind.data();
        if (ts.init) { kh.init = ts.init; kh.init_stride = init_stride; kh.tr_out = ts.after; }
        for (uint32_t b = 0; b < B; b++) kh(b);
        dev_h2d(v.chal.p, h_chal.data(), h_chal.size() * sizeof(sc), st);
        dev_h2d(v.uk.p, h_uk.data(), h_uk.size() * sizeof(sc), st);
        dev_h2d(v.fail.p, h_fail.data(), sizeof(int) * B, st);
        if (want_bind) dev_h2d(v.bind.p, h_bind.data(), h_bind.size(), st);
    } else
#endif
    launch_transcript(B, kt, st);
    uint32_t maxe = std::max<uint32_t>(N, c->q + 1);
    v.H = (maxe >> 8) + 1;
    v.plo.alloc((size_t)3 * 256 * B); v.phi.alloc((size_t)3 * v.H * B);
    launch_pow_tables(K_pow_tables{v.chal.p, v.plo.p, v.phi.p, B, v.H}, B, st);
    const uint32_t nslots = 3 * n + m + p + 1;
    v.wvec.alloc((size_t)nslots * B);
    // public coefficients (BPR1CS_VAR_SCALE): the flattening multiplies by the public inputs, which lie here as the caller's canonical
    // bytes, proof-major - converted once (a non-canonical one reads as 0; K_verify_public below marks its proof malformed)
    DevBuf<sc> pub_m;
    if (c->n_sc_chunks) {
        pub_m.alloc((size_t)p * B);
        launch((uint64_t)p * B, K_public_mont{v.d_pub, pub_m.p, B, p}, st);
    }
    run_flatten(c, nslots, v.plo.p, v.phi.p, v.wvec.p, B, v.H, st, pub_m.p);
    v.gh.alloc((size_t)2 * N * B); v.dpart.alloc((size_t)N * B); v.delta.alloc(B); v.bsc.alloc((size_t)2 * B);
    launch((uint64_t)N * B, K_verify_gh{v.wvec.p, v.plo.p, v.phi.p, v.chal.p, v.uk.p, v.gh.p, v.gh.p + (size_t)N * B, v.dpart.p, B, v.H, n, N, lgN}, st);
    if (N >= 1024) {  // delta = sum_i y^-i wR_i wL_i in two levels (one thread per proof walking N values alone takes ~12 ms)
        DevBuf<sc> dsum((size_t)(N / 256) * B);
        launch_sum_partials((uint64_t)(N / 256) * B, K_sum_partials{v.dpart.p, dsum.p, B, 256}, st);
        launch_sum_partials(B, K_sum_partials{dsum.p, v.delta.p, B, N / 256}, st);
    } else {
        launch_sum_partials(B, K_sum_partials{v.dpart.p, v.delta.p, B, N}, st);
    }
    sc* wc = v.wvec.p + (size_t)(3 * n + m + p) * B;
    // w_c += sum_k (column of public input k) x p_k; a non-canonical public input makes its proof malformed
    const K_verify_public kpub{v.wvec.p + (size_t)(3 * n + m) * B, v.d_pub, wc, v.fail.p, B, p};
    if (p && !LAUNCH_WAVE_FORM(B <= FINISH_WAVE_MAX_PROOFS, B, st, k_verify_public_wave, kpub)) launch(B, kpub, st);
    launch(B, K_verify_bscalars{v.chal.p, wc, v.delta.p, v.bsc.p, B}, st);
    v.P = 8 + m + 2 * lgN;
    if (after_on_device) dev_d2h(ts.after, v.d_after.p, (size_t)B * sizeof(strobe), st);   // (behind the front's launches: the copy waits for the stream)
}

static int verify_batch_once(const bpr1cs_gens* g, const bpr1cs_circuit* c, const VerifyStart& ts,
                                   const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds, size_t batch,
                                   int* ok_out) {
    if (!ok_out) return BPR1CS_ERR_INVALID_ARGUMENT;
    int rc = verify_args_ok(g, c, ts.label, proofs, commitments, batch);
    if (rc) return rc;
    API_TRY
    dev_stream_t st = g->stream;
    CallScope scope(st);
    MsmStats stats;
    VerifyCtx v;
    verify_front(v, g, c, ts, proofs, commitments, verifier_rng_seeds, batch, false, st);
    const uint32_t B = v.B, N = v.N, baseG = 2, baseH = 2 + g->cap;
    DevBuf<ge> partial;
    MsmPlan plan;
    MsmSeg sg{v.gh.p, N, N, N, 0, baseG, 0}, sh{v.gh.p + (size_t)N * B, N, N, N, 0, baseH, 0};
    run_msm(g, sg, sh, B, partial, plan, st, &stats);
    DevBuf<ge> pts;
    DevBuf<int> ok(B);
    uint32_t n_pts = v.P;
    K_verify_points kp{v.d_pf.p, v.d_vc.p, v.chal.p, v.uk.p, v.wvec.p + (size_t)3 * v.n * B, nullptr, v.fail.p, B, v.m, v.lgN, (uint32_t)v.plen};
#if !defined(BPR1CS_HOSTSIM)
    DevBuf<ge_cached> vtab;
    DevBuf<uint32_t> vdig;
    DevBuf<ge> vpart;
    if (B <= FINISH_WAVE_MAX_PROOFS) {
        // one proof per verify() (the reference's own call shape, src/gadget_vsmt_4.rs:442-479): the proof's own points summed by Straus
        // with shared doublings - a thread per term prepares multiples and digits, a wavefront per (window, proof) adds, one chain of
        // doublings per proof - instead of a 255-doubling scalar multiplication per term and a lane adding the results one by one
        const size_t T = (size_t)v.P * B;
        vtab.alloc((size_t)VB_MULT * T); vdig.alloc((size_t)VB_WORDS * T); vpart.alloc((size_t)VB_WINDOWS * B); pts.alloc(B);
        kp.vtab = vtab.p; kp.vdig = vdig.p;
        launch((uint64_t)T, kp, st);
        launch_kernel(k_verify_win_wave, dim3(VB_WINDOWS * B), dim3(64), 0, st, vtab.p, vdig.p, vpart.p, B, v.P);
        launch(B, K_ipa_vb_horner{vpart.p, pts.p, B, 1}, st);
        n_pts = 1;
    } else
#endif
    {
        pts.alloc((size_t)v.P * B);
        kp.out = pts.p;
        launch((uint64_t)v.P * B, kp, st);
    }
    const K_verify_finish kf{g->tab.p, g->tc, partial.p, pts.p, v.bsc.p, v.fail.p, ok.p, B, plan.nchunks, n_pts};
    if (!LAUNCH_WAVE_FORM(B <= FINISH_WAVE_MAX_PROOFS, B, st, k_verify_finish_wave, kf)) launch(B, kf, st);
    dev_d2h(ok_out, ok.p, sizeof(int) * B, st);
    stats.collect();
    return BPR1CS_OK;
    API_CATCH
}

// Cross-proof batching, first half (shared by the two entry points below): weights, ONE combined scalar per shared
// base (cgh: G | H canonical; cb: B, B~ Montgomery), and the weighted sum of the proofs' own points reduced to <= 64 points.
struct CombinedCtx {
    DevBuf<uint8_t> d_bseed, digest;
    DevBuf<sc> rho, cgh, cb;
    DevBuf<ge> pts, red[2];
    const ge* own = nullptr;
    uint32_t own_cnt = 0;
};
// the weights rho_b (Montgomery) of a batch whose transcripts were replayed with binding values (verify_front, want_bind)
static void verify_weights(CombinedCtx& k, VerifyCtx& v, const uint8_t* batch_seed, uint64_t index_base, dev_stream_t st) {
    const uint32_t B = v.B;
    k.d_bseed.alloc(32); k.digest.alloc(32); k.rho.alloc(B);
    dev_h2d(k.d_bseed.p, batch_seed, 32, st);
    const uint32_t leaves = (B + BATCH_LEAF - 1) / BATCH_LEAF;
    DevBuf<uint8_t> leaf((size_t)leaves * 32);
    launch(leaves, K_batch_leaf{v.bind.p, leaf.p, B, v.d_pub, v.p}, st);
    launch(1, K_batch_digest{k.d_bseed.p, leaf.p, k.digest.p, index_base, B}, st);
    launch(B, K_batch_weights{k.digest.p, k.rho.p, index_base}, st);
}
// every proof's own points times its weight: k.pts[P][B]; a point that does not decode sets its proof's flag
static void verify_weighted_points(CombinedCtx& k, VerifyCtx& v, dev_stream_t st) {
    const uint32_t B = v.B;
    k.pts.alloc((size_t)v.P * B);
    K_verify_points kp{v.d_pf.p, v.d_vc.p, v.chal.p, v.uk.p, v.wvec.p + (size_t)3 * v.n * B, k.pts.p, v.fail.p, B, v.m, v.lgN, (uint32_t)v.plen};
    kp.rho = k.rho.p;
    launch((uint64_t)v.P * B, kp, st);
}
// sums of 64 points, level after level, until at most 64 points are left: -> where they sit (cur itself or one of red[]), cnt updated
static const ge* reduce_to_64_points(const ge* cur, uint32_t& cnt, DevBuf<ge> red[2], dev_stream_t st) {
    for (int flip = 0; cnt > 64; flip ^= 1) {
        const uint32_t outc = (cnt + 63) / 64;
        red[flip].alloc(outc);
        launch(outc, K_ge_reduce{cur, red[flip].p, 1, cnt, 64}, st);
        cur = red[flip].p;
        cnt = outc;
    }
    return cur;
}
static void verify_combine(CombinedCtx& k, VerifyCtx& v, const uint8_t* batch_seed, uint64_t index_base, dev_stream_t st) {
    const uint32_t B = v.B, N = v.N;
    verify_weights(k, v, batch_seed, index_base, st);
    k.cgh.alloc((size_t)2 * N); k.cb.alloc(2);
    launch((uint64_t)2 * N, K_combine_scalars{v.gh.p, k.rho.p, k.cgh.p, B}, st);
    launch(2, K_combine_scalars{v.bsc.p, k.rho.p, k.cb.p, B}, st);
    verify_weighted_points(k, v, st);
    k.own_cnt = v.P * B;
    k.own = reduce_to_64_points(k.pts.p, k.own_cnt, k.red, st);
}

// Cross-proof batched verification: one identity test for the whole batch (and, summed over ranks, for the whole job).
// Returns this rank's partial point; the caller adds the ranks' points (bpr1cs_points_sum) and accepts iff the sum
// is the identity (32 zero bytes) and every rank reported `wellformed`.
static int verify_batch_combined_once(const bpr1cs_gens* g, const bpr1cs_circuit* c, const VerifyStart& ts,
                                            const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds,
                                            const uint8_t* batch_seed, uint64_t index_base, size_t batch, uint8_t* partial_point_out,
                                            int* wellformed_out) {
    if (!batch_seed || !partial_point_out || !wellformed_out) return BPR1CS_ERR_INVALID_ARGUMENT;
    int rc = verify_args_ok(g, c, ts.label, proofs, commitments, batch);
    if (rc) return rc;
    API_TRY
    dev_stream_t st = g->stream;
    CallScope scope(st);
    MsmStats stats;
    VerifyCtx v;
    verify_front(v, g, c, ts, proofs, commitments, verifier_rng_seeds, batch, true, st);
    CombinedCtx k;
    verify_combine(k, v, batch_seed, index_base, st);
    const uint32_t N = v.N, baseG = 2, baseH = 2 + g->cap;
    DevBuf<ge> partial;
    MsmPlan plan;
    MsmSeg sg{k.cgh.p, N, N, N, 0, baseG, 0}, sh{k.cgh.p + N, N, N, N, 0, baseH, 0};
    run_msm(g, sg, sh, 1, partial, plan, st, &stats);
    uint32_t mcnt = plan.nchunks;
    DevBuf<ge> mred[2];
    const ge* mcur = reduce_to_64_points(partial.p, mcnt, mred, st);
    DevBuf<uint8_t> d_out(32);
    DevBuf<int> d_wf(1);
    launch(1, K_batch_finish{g->tab.p, g->tc, mcur, k.own, k.cb.p, v.fail.p, d_out.p, d_wf.p, mcnt, k.own_cnt, v.B}, st);
    dev_d2h(partial_point_out, d_out.p, 32, st);
    dev_d2h(wellformed_out, d_wf.p, sizeof(int), st);
    stats.collect();
    return BPR1CS_OK;
    API_CATCH
}

// Grouped verification (BPR1CS_OPT_VERIFY_GROUP): the batch in NG = ceil(B / G) groups of G consecutive proofs, one combined
// identity test per group - the shared-base sum is one fixed-base MSM of batch NG over the segmented combination cgh[2N][NG] of the
// proofs' scalar vectors.  What happens to a group that fails is BPR1CS_OPT_VERIFY_GROUP_FALLBACK: nothing more (0: its proofs are rejected),
// the per-proof path for its well-formed proofs (1, verify_batch_grouped_once) or bisection on the device (2).  One routine,
// verify_batch_bisect_once, serves all three: the groups are the ranges of its depth 0, and modes 0 and 1 stop there.
// Workgroups (one wavefront each) of k_combine_scalars_range_wave for rows x R outputs.  A launch must stay below 2^32 threads in
// all, and the depth-32 circuit (2N = 65536 rows) passes 2^26 outputs at R = 1024 - 4096 proofs in groups of 4: the grid is capped and
// a wavefront walks outputs a grid apart (2^20 wavefronts are 128 times what the chip holds at once; a 4096-proof job with G = 64 is
// four outputs per wavefront).  The output index itself must fit 32 bits (verify_args_ok bounds 4N x batch, and R <= (batch + 1) / 2).
static const uint32_t GROUP_COMBINE_MAX_WGS = 1u << 20;
static uint32_t combine_grouped_wgs(uint64_t rows, uint64_t NG) {
    const uint64_t outputs = rows * NG;
    if (rows > 0xffffffffull || NG > 0xffffffffull || outputs > 0xffffffffull) throw DevError{BPR1CS_ERR_INVALID_ARGUMENT};
    return (uint32_t)std::min<uint64_t>(outputs, GROUP_COMBINE_MAX_WGS);
}
static void launch_combine_ranges(uint32_t rows, const K_combine_scalars_ranges& f, dev_stream_t st) {
    const uint32_t wgs = combine_grouped_wgs(rows, f.R);
    if (wgs) LAUNCH_WAVE_ALWAYS(wgs, st, k_combine_scalars_range_wave, (uint64_t)rows * f.R, f, f, rows * f.R);
}
#if defined(BPR1CS_HOSTSIM)
// Simulator only (never part of libbpr1cs_hip.so): the launch geometry above for a shape no test can afford to run - *wgs = workgroups
// of 64 threads for rows x NG outputs; returns BPR1CS_ERR_INVALID_ARGUMENT where the output index does not fit 32 bits.
extern "C" int bpr1cs_sim_group_combine_grid(uint64_t rows, uint64_t NG, uint32_t* wgs) {
    if (!wgs) return BPR1CS_ERR_INVALID_ARGUMENT;
    API_TRY
    *wgs = combine_grouped_wgs(rows, NG);
    return BPR1CS_OK;
    API_CATCH
}
#endif
// The device part of all three modes.  S(R) = sum_{b in R, fail[b] = 0} rho_b E_b is additive over the proofs of a range R, and
// everything it is made of - gh, bsc, the weights, the weighted own points - stays on the device.  Depth 0 tests the groups: one
// range combination, one run_msm of batch NG and one range finish.  `descend` = false (modes 0 and 1) ends there with group
// verdicts: a group holds iff its S is the identity and none of its proofs is malformed.  `descend` = true (mode 2) is
// level-synchronous bisection: every later depth takes the failing ranges of more than one proof of ALL groups, computes S of their
// left halves (ceil(s / 2) proofs) with one range combination, one run_msm whose batch is the number of ranges and one range finish -
// which also forms S(right) = S(parent) - S(left) - and reads the identity flags back.  A passing range accepts its well-formed
// proofs, a failing range of one proof rejects it.  Nothing is uploaded again and the per-proof path is not taken.
// -> ok_out[B], pfail[B] (proof is malformed)
struct BisectRange { uint32_t lo, hi, pt; };   // a failing range of more than one proof; pt: where its S sits among the depth's points
static int verify_batch_bisect_once(const bpr1cs_gens* g, const bpr1cs_circuit* c, const VerifyStart& ts,
                                    const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds, size_t batch,
                                    uint32_t G, bool descend, int* ok_out, std::vector<int>& pfail) {
    API_TRY
    dev_stream_t st = g->stream;
    CallScope scope(st);
    MsmStats stats;
    VerifyCtx v;
    verify_front(v, g, c, ts, proofs, commitments, verifier_rng_seeds, batch, true, st);
    const uint32_t B = v.B, N = v.N, NG = (B + G - 1) / G, baseG = 2, baseH = 2 + g->cap;
    // the entry point has no batch seed of its own: the first proof's verifier seed (zeros with none), bound to the whole batch by the digest
    uint8_t bseed[32] = {0};
    if (verifier_rng_seeds) memcpy(bseed, verifier_rng_seeds, 32);
    CombinedCtx k;
    verify_weights(k, v, bseed, 0, st);
    // the own points first: a point that does not decode sets its proof's flag, and the sums below leave such a proof out
    verify_weighted_points(k, v, st);
    // scratch of a slice of at most NG ranges - what depth 0 needs - shared by all depths
    k.cgh.alloc((size_t)2 * N * NG); k.cb.alloc((size_t)2 * NG);
    DevBuf<ge> rpts(NG), partial, spts[2];   // spts: S of the ranges of this depth and of the one before (the parents)
    std::vector<BisectRange> cur(NG), next;
    for (uint32_t grp = 0; grp < NG; grp++) cur[grp] = BisectRange{grp * G, std::min(B, (grp + 1) * G), 0};
    std::vector<int> zero;
    std::vector<uint32_t> h_rng;
    pfail.resize(B);
    for (uint32_t depth = 0; !cur.empty(); depth++) {
        const uint32_t R = (uint32_t)cur.size();
        h_rng.resize((size_t)3 * R);   // lo | hi | parent of the tested ranges: the groups at depth 0, the left halves below
        for (uint32_t i = 0; i < R; i++) {
            const uint32_t s = cur[i].hi - cur[i].lo;
            h_rng[i] = cur[i].lo;
            h_rng[R + i] = depth ? cur[i].lo + (s + 1) / 2 : cur[i].hi;
            h_rng[2 * R + i] = cur[i].pt;
        }
        DevBuf<uint32_t> d_rng((size_t)3 * R);
        dev_h2d(d_rng.p, h_rng.data(), h_rng.size() * sizeof(uint32_t), st);
        DevBuf<ge>& out = spts[depth & 1];
        const ge* parent = depth ? spts[(depth & 1) ^ 1].p : nullptr;
        out.alloc((size_t)2 * R);   // left | right
        DevBuf<int> d_zero((size_t)2 * R);
        for (uint32_t off = 0; off < R; off += NG) {
            const uint32_t cnt = std::min(NG, R - off);
            const uint32_t *lo = d_rng.p + off, *hi = d_rng.p + R + off, *par = d_rng.p + 2 * (size_t)R + off;
            launch_combine_ranges(2 * N, K_combine_scalars_ranges{v.gh.p, k.rho.p, v.fail.p, lo, hi, k.cgh.p, B, cnt}, st);
            launch_combine_ranges(2, K_combine_scalars_ranges{v.bsc.p, k.rho.p, v.fail.p, lo, hi, k.cb.p, B, cnt}, st);
            const K_range_points krp{k.pts.p, v.fail.p, lo, hi, rpts.p, B, v.P};   // (a wavefront per range whatever their number: a range is up to G x P points)
            LAUNCH_WAVE_ALWAYS(cnt, st, k_range_points_wave, cnt, krp, krp);
            MsmPlan plan;
            MsmSeg sg{k.cgh.p, N, N, N, 0, baseG, 0}, sh{k.cgh.p + (size_t)N * cnt, N, N, N, 0, baseH, 0};
            run_msm(g, sg, sh, cnt, partial, plan, st, &stats);
            const K_range_finish krf{g->tab.p, g->tc, partial.p, rpts.p, k.cb.p, parent, par, out.p + off, out.p + R + off,
                                     d_zero.p + off, d_zero.p + R + off, cnt, plan.nchunks};
            if (!LAUNCH_WAVE_FORM(cnt <= FINISH_WAVE_MAX_PROOFS, cnt, st, k_range_finish_wave, krf)) launch(cnt, krf, st);
        }
        zero.resize((size_t)2 * R);
        dev_d2h(zero.data(), d_zero.p, sizeof(int) * (depth ? 2 * (size_t)R : R), st);
        if (depth == 0) {
            dev_d2h(pfail.data(), v.fail.p, sizeof(int) * B, st);
            for (uint32_t b = 0; b < B; b++) ok_out[b] = !pfail[b];   // a malformed proof is rejected and is part of no sum
            if (!descend) {   // group verdicts (a group's S leaves its malformed proofs out: their flags fail the group here)
                for (uint32_t i = 0; i < R; i++) {
                    int good = zero[i];
                    for (uint32_t b = cur[i].lo; b < cur[i].hi; b++) good &= !pfail[b];
                    for (uint32_t b = cur[i].lo; b < cur[i].hi; b++) ok_out[b] = good;
                }
                break;
            }
        }
        next.clear();
        auto classify = [&](uint32_t lo, uint32_t hi, uint32_t pt, int is_zero) {
            if (is_zero) return;                        // every well-formed proof of the range is accepted
            if (hi - lo == 1) ok_out[lo] = 0;           // (a range of one malformed proof sums to the identity: it never gets here)
            else next.push_back(BisectRange{lo, hi, pt});
        };
        for (uint32_t i = 0; i < R; i++) {
            if (depth == 0) { classify(cur[i].lo, cur[i].hi, i, zero[i]); continue; }
            const uint32_t mid = h_rng[R + i];
            classify(cur[i].lo, mid, i, zero[i]);
            classify(mid, cur[i].hi, R + i, zero[R + i]);
        }
        cur.swap(next);
    }
    stats.collect();
    return BPR1CS_OK;
    API_CATCH
}
static int verify_batch_grouped_once(const bpr1cs_gens* g, const bpr1cs_circuit* c, const VerifyStart& ts,
                                     const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds, size_t batch,
                                     uint32_t G, int mode, int* ok_out) {
    if (!ok_out) return BPR1CS_ERR_INVALID_ARGUMENT;
    int rc = verify_args_ok(g, c, ts.label, proofs, commitments, batch);
    if (rc) return rc;
    std::vector<int> pfail;
    rc = verify_batch_bisect_once(g, c, ts, proofs, commitments, verifier_rng_seeds, batch, G,
                                  mode == BPR1CS_VERIFY_GROUP_FALLBACK_BISECT, ok_out, pfail);
    if (rc || mode != BPR1CS_VERIFY_GROUP_FALLBACK_RECHECK) return rc;
    API_TRY
    std::vector<size_t> redo;   // well-formed proofs of the groups that failed
    for (size_t b = 0; b < batch; b++)
        if (!ok_out[b] && !pfail[b]) redo.push_back(b);
    if (redo.empty()) return BPR1CS_OK;
    // the inputs are host memory: the sub-batch is gathered here and takes the per-proof path as a batch of its own
    const size_t plen = bpr1cs_proof_len(c), clen = (size_t)c->m * 32, ulen = (size_t)c->p * 32;   // (public inputs: the tail block of both arrays)
    const uint8_t* pub = commitments ? commitments + batch * clen : nullptr;
    std::vector<uint8_t> sp(redo.size() * plen), sc_(redo.size() * (clen + ulen) + 1), ss(verifier_rng_seeds ? redo.size() * 32 : 0);
    std::vector<int> sok(redo.size(), 0);
    for (size_t i = 0; i < redo.size(); i++) {
        memcpy(sp.data() + i * plen, proofs + redo[i] * plen, plen);
        if (clen) memcpy(sc_.data() + i * clen, commitments + redo[i] * clen, clen);
        if (ulen) memcpy(sc_.data() + redo.size() * clen + i * ulen, pub + redo[i] * ulen, ulen);
        if (verifier_rng_seeds) memcpy(ss.data() + i * 32, verifier_rng_seeds + redo[i] * 32, 32);
    }
    std::vector<strobe> st0(ts.n_init > 1 ? redo.size() : 0);   // per-proof starting states travel with their proofs
    for (size_t i = 0; i < st0.size(); i++) st0[i] = ts.init[redo[i]];
    rc = verify_batch_once(g, c, ts.sub(st0), sp.data(), sc_.data(), verifier_rng_seeds ? ss.data() : nullptr, redo.size(), sok.data());
    if (rc) return rc;
    for (size_t i = 0; i < redo.size(); i++) ok_out[redo[i]] = sok[i];
    return BPR1CS_OK;
    API_CATCH
}

// Multi-GPU form of the batched verifier: instead of evaluating the shared-base MSM itself, a rank
// returns its combined scalar vector; the ranks add their vectors (all_gather / all_reduce of 2N+2 scalars, ~2 MB at
// N = 32768), each evaluates 1/world of the bases with bpr1cs_msm_fixed, and the points are gathered and summed.
static int verify_batch_scalars_once(const bpr1cs_gens* g, const bpr1cs_circuit* c, const VerifyStart& ts,
                                           const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds,
                                           const uint8_t* batch_seed, uint64_t index_base, size_t batch, uint8_t* combined_scalars_out,
                                           uint8_t* own_points_sum_out, int* wellformed_out) {
    if (!batch_seed || !combined_scalars_out || !own_points_sum_out || !wellformed_out) return BPR1CS_ERR_INVALID_ARGUMENT;
    int rc = verify_args_ok(g, c, ts.label, proofs, commitments, batch);
    if (rc) return rc;
    API_TRY
    dev_stream_t st = g->stream;
    CallScope scope(st);
    VerifyCtx v;
    verify_front(v, g, c, ts, proofs, commitments, verifier_rng_seeds, batch, true, st);
    CombinedCtx k;
    verify_combine(k, v, batch_seed, index_base, st);
    const uint32_t N = v.N;
    // own points only (no shared-base part, no B / B~ terms): K_batch_finish with zero scalars for B, B~
    DevBuf<sc> zero2(2);
    dev_zero(zero2.p, 2 * sizeof(sc), st);
    DevBuf<uint8_t> d_out(32);
    DevBuf<int> d_wf(1);
    launch(1, K_batch_finish{g->tab.p, g->tc, nullptr, k.own, zero2.p, v.fail.p, d_out.p, d_wf.p, 0, k.own_cnt, v.B}, st);
    dev_d2h(own_points_sum_out, d_out.p, 32, st);
    dev_d2h(wellformed_out, d_wf.p, sizeof(int), st);
    // scalars in base order B, B~, G[0..N), H[0..N), canonical bytes
    std::vector<sc> hb(2), hgh((size_t)2 * N);
    dev_d2h(hb.data(), k.cb.p, 2 * sizeof(sc), st);
    dev_d2h(hgh.data(), k.cgh.p, (size_t)2 * N * sizeof(sc), st);
    sc_mont_tobytes(hb[0], combined_scalars_out);
    sc_mont_tobytes(hb[1], combined_scalars_out + 32);
    for (size_t i = 0; i < (size_t)2 * N; i++) sc_store_raw(hgh[i], combined_scalars_out + 64 + 32 * i);
    return BPR1CS_OK;
    API_CATCH
}
// out = sum of `count` scalar vectors of `len` canonical scalars each (mod l): the reduction step between the two halves
// of the multi-GPU batched verifier when the host gathers instead of all-reducing
extern "C" int bpr1cs_scalars_sum(const uint8_t* vectors, size_t count, size_t len, uint8_t* out) {
    if (!vectors || !out || count == 0 || len == 0) return BPR1CS_ERR_INVALID_ARGUMENT;
    if (!host_scalars_canonical(vectors, count * len)) return BPR1CS_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < len; i++) {
        sc acc = sc_load_raw(vectors + 32 * i);
        for (size_t r = 1; r < count; r++) acc = sc_add(acc, sc_load_raw(vectors + 32 * (r * len + i)));
        sc_store_raw(acc, out + 32 * i);
    }
    return BPR1CS_OK;
}

// The prover keeps its scratch (the handle's arenas) between calls; a verifier call that finds no memory next to it hands that
// scratch - and the allocator's cache - back and tries once more (only while no prove job of the handle is in flight).
template <class F>
static int with_scratch_retry(const bpr1cs_gens* g, F&& once) {
    int rc = once();
    if (rc == BPR1CS_ERR_OUT_OF_MEMORY && g && g->in_flight.load() == 0) {
        g->arena.release(); g->front[0].release(); g->front[1].release(); g->shared_front.release();
        dev_release_cache();
        rc = once();
    }
    return rc;
}
// The entry points parse (label, label_len) ONCE (VerifyHandles), run - and possibly re-run - on the snapshot, and write the handles
// of a transcripts call back only when the call has succeeded.
extern "C" int bpr1cs_verify_batch(const bpr1cs_gens* g, const bpr1cs_circuit* c, const uint8_t* label, size_t label_len,
                                   const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds, size_t batch,
                                   int* ok_out) {
    VerifyHandles h;
    if (int rc = h.parse(label, label_len, batch)) return rc;
    const VerifyStart& ts = h.ts;
    const int G = g ? g->opts.verify_group.load() : 0;
    if (G >= 2 && batch >= 2) {
        const int mode = g->opts.verify_group_fallback.load();
        return h.finish(with_scratch_retry(g, [&] { return verify_batch_grouped_once(g, c, ts, proofs, commitments, verifier_rng_seeds, batch, (uint32_t)G, mode, ok_out); }));
    }
    return h.finish(with_scratch_retry(g, [&] { return verify_batch_once(g, c, ts, proofs, commitments, verifier_rng_seeds, batch, ok_out); }));
}
extern "C" int bpr1cs_verify_batch_combined(const bpr1cs_gens* g, const bpr1cs_circuit* c, const uint8_t* label, size_t label_len,
                                            const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds,
                                            const uint8_t* batch_seed, uint64_t index_base, size_t batch, uint8_t* partial_point_out,
                                            int* wellformed_out) {
    VerifyHandles h;
    if (int rc = h.parse(label, label_len, batch)) return rc;
    const VerifyStart& ts = h.ts;
    return h.finish(with_scratch_retry(g, [&] { return verify_batch_combined_once(g, c, ts, proofs, commitments, verifier_rng_seeds, batch_seed, index_base, batch, partial_point_out, wellformed_out); }));
}
// (the sharded form parses for itself: its handles are written when the whole exchange has succeeded, not when this step has)
static int verify_batch_scalars_parsed(const bpr1cs_gens* g, const bpr1cs_circuit* c, const VerifyStart& ts,
                                       const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds,
                                       const uint8_t* batch_seed, uint64_t index_base, size_t batch, uint8_t* combined_scalars_out,
                                       uint8_t* own_points_sum_out, int* wellformed_out) {
    return with_scratch_retry(g, [&] { return verify_batch_scalars_once(g, c, ts, proofs, commitments, verifier_rng_seeds, batch_seed, index_base, batch, combined_scalars_out, own_points_sum_out, wellformed_out); });
}
extern "C" int bpr1cs_verify_batch_scalars(const bpr1cs_gens* g, const bpr1cs_circuit* c, const uint8_t* label, size_t label_len,
                                           const uint8_t* proofs, const uint8_t* commitments, const uint8_t* verifier_rng_seeds,
                                           const uint8_t* batch_seed, uint64_t index_base, size_t batch, uint8_t* combined_scalars_out,
                                           uint8_t* own_points_sum_out, int* wellformed_out) {
    VerifyHandles h;
    if (int rc = h.parse(label, label_len, batch)) return rc;
    return h.finish(verify_batch_scalars_parsed(g, c, h.ts, proofs, commitments, verifier_rng_seeds, batch_seed, index_base, batch, combined_scalars_out, own_points_sum_out, wellformed_out));
}
