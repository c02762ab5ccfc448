// The way a prove job's TranscriptRng draws take to blind / s_L / s_R: one unit (JobDraws), three entry points called by prove_job_begin
// (csrc/api_prove.hpp).  Nothing else knows where the draws come from.
//
// A proof's chain gives 2n + 7 raw 64-byte draws behind its first one (i_bl): o_bl, s_bl, s_L[n], s_R[n], the five t blindings.  Five sources, the last in two forms:
//   Caller          the caller's own draws (bpr1cs_prove_batch_draws)                    lead form: 2n + 8 draws, proof-major [B][2n + 8][8]
//   HostThreads     a small job: every chain on host threads (HostChains)                lead form
//   Device          k_rng_stream, one launch                                             [2n + 7][B][8]
//   DeviceTwoLegs   k_rng_stream in two legs, cut behind draw n + 1 (d_half = n + 2)      [2n + 7][B][8]
//   Split           the first Bh proofs on host threads through a pinned ring, the       [2n + 7][Bh][8], then [2n + 7][B - Bh][8]
//   SplitTwoLegs    rest in k_rng_stream; one leg or two                                 (each part contiguous per draw)
// The two-leg sources are those of a call's first job: S1's first half, <s_L, G>, needs draws [0, n + 2) only, so these
// are reduced as soon as they are there and the caller's `sum_first_half` is enqueued on the heavy stream behind them.
//
// Streams: front (sl: the job's own), witness (su: the job's own; a copy engine's work, the heavy stream never waits for a copy),
// heavy (st: shared by the handle's jobs).  Events of the handle, waited for only when its jobs share W / rng_raw (`shared`):
//   rng_free_ev   recorded by close() of the job before: its raw draws are reduced and wiped.  Waited for by whatever writes rng_raw
//                 first on a stream (the upload of the lead form, k_rng_stream, the ring's copies).
//   w_free_ev     recorded on the heavy stream by the job before, behind its l(x), r(x).  s_L / s_R live in W: waited for in front of
//                 the first K_rng_reduce on every stream that launches one.
// Per source, in stream order ([..]: only when shared):
//   Caller         enqueue_front   front: [rng_free_ev] upload, [w_free_ev] reduce_lead, close
//   HostThreads    enqueue_front   nothing on the device (the caller has queued the V commitments' read-back on the front stream)
//                  start_host_chains  the host waits for the front stream, the threads start
//                  deliver         the host joins the threads; front: transcripts up, then as Caller
//   Device         enqueue_front   front: [rng_free_ev] k_rng_stream, [w_free_ev] reduce whole [0, draws), close
//   DeviceTwoLegs  enqueue_front   front: [rng_free_ev] leg 1 (leaves its states where it found them), record ev_rng_half, leg 2
//                  deliver         heavy: wait ev_rng_half, [w_free_ev] reduce whole [0, d_half), record ev_rng_red; sum_first_half
//                                  front: [w_free_ev] reduce whole [d_half, draws), wait ev_rng_red, close
//                                  (leg 1 is reduced on the heavy stream, in front of the sum that needs it: between the legs it had to find
//                                  room on a GPU full of the A_I / A_O sum's waves and held leg 2 back by 42 ms in a trace; the wipe in close
//                                  must not overtake that reduction: ev_rng_red)
//   Split*         enqueue_front   front: the host part's RNG states back (h_tr0), record ev_head - before the device chain is queued on
//                                  this stream -, [rng_free_ev] k_rng_stream of the device part in one leg, or two as above
//                  deliver         the host waits for ev_head; witness: [rng_free_ev], then per chunk of 256 draws (ring of 4 pinned slots,
//                                  64 MiB each at 4096 proofs) its copy and the slot's event, which the host waits for before the workers
//                                  write the slot again.  Two legs, in the hand-over of the chunk that holds draw n + 1, while the workers
//                                  hash on: witness: [w_free_ev] reduce host [0, d_half), record ev_rng_half_h; heavy: the device part's
//                                  first leg as above (if there is a device part), wait ev_rng_half_h; sum_first_half.
//                                  Behind the last chunk: witness: record ev_head (again); front: wait ev_head, [w_free_ev] reduce host
//                                  [r0, draws), reduce device [r0, draws) (r0 = d_half with two legs, else 0), wait ev_rng_red, close
// close(): front: zero rng_raw, zero rng, [record rng_free_ev], record ev_rng - which the heavy stream waits for in front of the rest of
// S1.  The CPU simulator (BPR1CS_HOSTSIM) runs the whole device chain inside K_transcript_init: it knows Caller, HostThreads and Device.
#pragma once
#include "kernels.hpp"

// ---- the raw draws' layout and the K_rng_reduce launches over it: plain arithmetic (tests/hostsim/draws_reduce_check.cpp runs the
// described launches on the CPU)
enum class DrawsPart { Whole, Host, Device };   // every proof; the host's [0, Bh); the device's [Bh, B)
struct DrawsReduce { uint64_t threads; K_rng_reduce k; };
struct DrawsLayout {
    uint32_t B, Bh, n, draws;
    const uint64_t* raw;
    sc* blind; sc* sL; sc* sR;
    // draws [d0, d1) of a part: a thread per draw and proof of the part
    DrawsReduce reduce(DrawsPart part, uint32_t d0, uint32_t d1) const {
        if (part == DrawsPart::Device && !Bh) part = DrawsPart::Whole;   // (no host part: the device's is the whole batch)
        const uint32_t nd = d1 - d0;
        switch (part) {
        case DrawsPart::Host: return {(uint64_t)nd * Bh, K_rng_reduce{raw, blind, sL, sR, B, n, 0u, /*Bc*/ Bh, /*b0*/ 0u, d0}};
        case DrawsPart::Device: return {(uint64_t)nd * (B - Bh), K_rng_reduce{raw + (size_t)draws * Bh * 8, blind, sL, sR, B, n, 0u, /*Bc*/ B - Bh, /*b0*/ Bh, d0}};
        default: return {(uint64_t)nd * B, K_rng_reduce{raw, blind, sL, sR, B, n, 0u, /*Bc*/ 0u, /*b0*/ 0u, d0}};
        }
    }
    // the lead form: all 2n + 8 draws of every proof, i_bl first, one proof's after the other's
    DrawsReduce reduce_lead() const { return {(uint64_t)(draws + 1) * B, K_rng_reduce{raw, blind, sL, sR, B, n, 1u}}; }
};

#if !defined(BPR1CS_DRAWS_LAYOUT_ONLY)
enum class DrawsSource { Caller, HostThreads, Device, DeviceTwoLegs, Split, SplitTwoLegs };
struct JobDraws {
    DrawsSource src = DrawsSource::Device;
    uint32_t B = 0, Bh = 0, n = 0, draws = 0, d_half = 0;
    unsigned chain_workers = 0;
    bpr1cs_job* job = nullptr;
    const bpr1cs_gens* g = nullptr;
    bool shared = false;
    dev_stream_t st{}, sl{}, su{};   // heavy, front, witness
    DevBuf<uint64_t>* rng_raw = nullptr;
    DevBuf<strobe>* rng = nullptr;   // the chains' states (device sources; allocated by the caller in front of K_transcript_init)
    strobe* tr = nullptr;
    int* rng_err = nullptr;
    sc* blind = nullptr; sc* sL = nullptr; sc* sR = nullptr;
    HostChains chains;   // (joined by its destructor on every path out of prove_job_begin)

    bool lead() const { return src == DrawsSource::Caller || src == DrawsSource::HostThreads; }
    bool two_legs() const { return src == DrawsSource::DeviceTwoLegs || src == DrawsSource::SplitTwoLegs; }

    void choose(const bpr1cs_gens* g_, uint32_t B_, uint32_t n_, bool ext, bool first_of_call, int auto_share) {
        g = g_; B = B_; n = n_;
        draws = 2 * n + 7;
        d_half = n + 2;
        chain_workers = host_cpu_budget() - 1;
        if (ext) { src = DrawsSource::Caller; return; }
        // A small job's TranscriptRng chains run on host threads (csrc/host_chain.hpp): BPR1CS_OPT_HOST_CHAIN_PROOFS, default = jobs of up
        // to 4 proofs per usable CPU.  One more draw travels then: the chain's first (i_bl), which the device path makes in K_transcript_init.
        const int o_hc = g->opts.host_chain.load();
        if (o_hc < 0 ? B <= 4u * host_cpu_budget() : B <= (uint32_t)o_hc) { src = DrawsSource::HostThreads; return; }
#if defined(BPR1CS_HOSTSIM)
        (void)first_of_call; (void)auto_share;
#else
        // The split (BPR1CS_OPT_HOST_CHAIN_SHARE): in a job that follows another job of its call, the chains run beside that job's
        // sums - k_rng_stream took ~9 % of the GPU's kernel time beside them and slowed the A_I / S launches by 80 ms a job -
        // while the host's cores sit idle.  auto_share: what bpr1cs_prove_batch chose for this job (host_chain_share_auto: the part the
        // host's budget - 1 workers hash within the heavy stream's time per job; for the first job of a call, whose chains nothing hides,
        // host_chain_share_first: the part that lets the host and the device end together).  No split without a worker: the calling
        // thread only hands the chunks over.
        if (chain_workers > 0) {
            const int o_share = g->opts.host_chain_share.load();
            const int share = o_share >= 0 ? o_share : std::max(0, std::min(100, auto_share));
            Bh = (uint32_t)(((uint64_t)B * (uint32_t)share + 50) / 100);
        }
        // The first job of a call is the only one whose heavy stream waits for the chain (a later job's chain ends while the job before it
        // is summed), and S1's first half, <s_L, G>, needs only the first n + 2 draws: the chain runs in two legs, cut behind draw n + 1,
        // each reduced when it ends, and S1 is summed in two launches, the first behind the chain's second leg.  Point
        // addition is exact: the same S1.  Not for a job of a few proofs (one launch for the three finishes), a secret-independent handle
        // (S1 shares its launch with the blinding terms) or the caller's own draws.
        const bool two = first_of_call && n > 0 && B > SMALL_JOB_PROOFS && !g->ct();
        src = Bh ? (two ? DrawsSource::SplitTwoLegs : DrawsSource::Split) : (two ? DrawsSource::DeviceTwoLegs : DrawsSource::Device);
#endif
    }

    // ---- the two helpers every source goes through
    DrawsLayout layout() const { return DrawsLayout{B, Bh, n, draws, rng_raw->p, blind, sL, sR}; }
    void reduce(DrawsPart part, uint32_t d0, uint32_t d1, dev_stream_t s) const {
        const DrawsReduce r = layout().reduce(part, d0, d1);
        launch(r.threads, r.k, s);
    }
    void reduce_lead(dev_stream_t s) const {
        const DrawsReduce r = layout().reduce_lead();
        launch(r.threads, r.k, s);
    }
    // the chain's end, on the front stream: the raw draws (blinding material) and the states are wiped, the next job may write rng_raw, the
    // heavy stream may read blind / s_L / s_R
    void close() const {
        if (job->ev_rng_red) dev_stream_wait(sl, job->ev_rng_red);   // (two legs: the first leg's draws are reduced on the heavy stream - before the wipe)
        dev_zero(rng_raw->p, rng_raw->bytes(), sl);
        if (rng->p) dev_zero(rng->p, rng->bytes(), sl);   // (the lead form has no states on the device)
        if (shared) dev_event_record(g->rng_free_ev, sl);
        dev_event_record(job->ev_rng, sl);
    }
    // the lead form goes up from job->h_raw and is reduced at once
    void upload_lead() const {
        if (shared) dev_stream_wait(sl, g->rng_free_ev);   // the job before has reduced (and wiped) its raw output
        dev_h2d_async(rng_raw->p, job->h_raw, job->h_raw_bytes, sl);
        if (shared) dev_stream_wait(sl, g->w_free_ev);     // s_L / s_R live in W: the job before is past its l(x), r(x)
        reduce_lead(sl);
        close();
    }
    // two legs, heavy stream: what is there of draws [0, d_half) is reduced (the device part) or waited for (the host part)
    void first_half_to_heavy() const {
        if (job->ev_rng_half) {   // the device chain's first leg has ended: o_bl, s_bl and s_L of its proofs
            dev_stream_wait(st, job->ev_rng_half);
            if (shared) dev_stream_wait(st, g->w_free_ev);
            reduce(DrawsPart::Device, 0, d_half, st);
            dev_event_create(&job->ev_rng_red);
            dev_event_record(job->ev_rng_red, st);   // (the front stream wipes the raw draws only behind it)
        }
        if (job->ev_rng_half_h) dev_stream_wait(st, job->ev_rng_half_h);
    }

    // ---- entry 1: behind K_transcript_init (device sources), the V commitments' read-back (HostThreads) or the transcripts' copy (Caller)
    void enqueue_front(const uint8_t* ext_draws) {
        if (lead()) {
            job->h_raw_bytes = (size_t)(draws + 1) * B * 64;
            job->h_raw = (uint64_t*)host_stage_alloc(job->h_raw_bytes);
            if (src == DrawsSource::Caller) {   // nothing to hash and nothing to wait for: the draws go up and are reduced at once
                memcpy(job->h_raw, ext_draws, job->h_raw_bytes);
                upload_lead();
            } else job->h_tr0 = (strobe*)host_stage_alloc((size_t)B * sizeof(strobe));
            return;
        }
#if defined(BPR1CS_HOSTSIM)
        dev_event_record(job->ev_rng, sl);   // (the simulator runs a kernel's functor proof by proof: the whole chain inside K_transcript_init)
#else
        // TranscriptRng on the device: the sequential STROBE chain of a proof (2n + 7 draws, one Keccak-f[1600] each) runs lane-parallel -
        // one state on 25 lanes, two proofs per wavefront (k_rng_stream) -, the wide reductions mod l of its outputs afterwards in
        // parallel.  Hidden behind the sums of the job before this one when a batch is cut into jobs.
        if (Bh) {   // the host's share: its RNG states go back now (before the device chain is queued on this stream)
            job->h_tr0 = (strobe*)host_stage_alloc((size_t)Bh * sizeof(strobe));
            dev_d2h_async(job->h_tr0, rng->p, (size_t)Bh * sizeof(strobe), sl);
            dev_event_create(&job->ev_head);
            dev_event_record(job->ev_head, sl);
        }
        if (shared) dev_stream_wait(sl, g->rng_free_ev);   // the job before has reduced (and wiped) its raw output
        const uint32_t Bd = B - Bh;
        uint64_t* raw_d = rng_raw->p + (size_t)draws * Bh * 8;
        strobe* rng_d = rng->p + Bh;
        const dim3 wgs((Bd + 1) / 2);
        if (Bd && two_legs()) {
            launch_kernel(k_rng_stream, wgs, dim3(64), 0, sl, rng_d, raw_d, rng_err, Bd, d_half, rng_d);
            dev_event_create(&job->ev_rng_half);
            dev_event_record(job->ev_rng_half, sl);
            launch_kernel(k_rng_stream, wgs, dim3(64), 0, sl, rng_d, raw_d + (size_t)d_half * Bd * 8, rng_err, Bd, draws - d_half, nullptr);
        } else if (Bd) {
            launch_kernel(k_rng_stream, wgs, dim3(64), 0, sl, rng_d, raw_d, rng_err, Bd, draws, nullptr);
        }
        if (src == DrawsSource::Device) {
            if (shared) dev_stream_wait(sl, g->w_free_ev);
            reduce(DrawsPart::Whole, 0, draws, sl);
            close();
        }
#endif
    }

    // ---- entry 2 (HostThreads): the chains start once the V commitments are on the host (their compressed encodings are transcript
    // messages); the wires go in and the A_I / A_O sums run on the device while the host hashes
    void start_host_chains(const strobe* init, size_t n_init, const uint8_t* v_blindings, const uint8_t* rng_seeds, uint32_t m) {
        if (src != DrawsSource::HostThreads) return;
        dev_sync(sl);
        DBG_JOB("begin: %u host chain(s) start", B);
        chains.start(init, n_init, job->h_V, v_blindings, rng_seeds, B, m, n, job->h_tr0, job->h_raw);
        if ((uint64_t)B * (draws + 1) <= 4096) chains.wait();   // (a few thousand permutations - a bound check's 264 - are done before a thread has started)
    }

    // ---- entry 3: where the heavy stream is about to wait for the draws (in front of S1's wait for ev_rng).  sum_first_half (two legs): called
    // once, when draws [0, d_half) of every proof are on their way to blind / s_L
    template <class F>
    void deliver(F&& sum_first_half) {
        switch (src) {
        case DrawsSource::Caller:
        case DrawsSource::Device: return;
        case DrawsSource::HostThreads:
            chains.wait();
            DBG_JOB("begin: host chain(s) done");
            dev_h2d_async(tr, job->h_tr0, (size_t)B * sizeof(strobe), sl);
            upload_lead();
            return;
        case DrawsSource::DeviceTwoLegs:
            first_half_to_heavy();
            sum_first_half();
            if (shared) dev_stream_wait(sl, g->w_free_ev);
            reduce(DrawsPart::Whole, d_half, draws, sl);
            close();
            return;
        case DrawsSource::Split:
        case DrawsSource::SplitTwoLegs: break;
        }
        const uint32_t Dc = 256, R = 4;
        if (!dev_event_sync(job->ev_head)) throw DevError{BPR1CS_ERR_DEVICE};
        job->h_raw_bytes = (size_t)R * Dc * Bh * 64;
        job->h_raw = (uint64_t*)host_stage_alloc(job->h_raw_bytes);
        if (shared) dev_stream_wait(su, g->rng_free_ev);
        dev_event_t ev_slot[R] = {};
        for (uint32_t r = 0; r < R; r++) dev_event_create(&ev_slot[r]);
        struct Events { dev_event_t* e; uint32_t n; ~Events() { for (uint32_t r = 0; r < n; r++) dev_event_destroy(&e[r]); } } evs_guard{ev_slot, R};
        DBG_JOB("begin: %u host chain(s) of %u streamed (%.4f us per permutation and worker)", Bh, B, host_chain_us_per_perm());
        double busy_us = 0;
        const bool ok = host_chains_stream(job->h_tr0, Bh, draws, Dc, R, job->h_raw, chain_workers,
            [&](uint32_t, uint32_t slot, uint32_t d0, uint32_t nd) {
                dev_h2d_async(rng_raw->p + (size_t)d0 * Bh * 8, job->h_raw + (size_t)slot * Dc * Bh * 8, (size_t)nd * Bh * 64, su);
                dev_event_record(ev_slot[slot], su);
                if (two_legs() && d0 <= d_half - 1 && d_half - 1 < d0 + nd) {   // draws [0, n + 2) of the host's chains are up: o_bl, s_bl, all of s_L
                    if (shared) dev_stream_wait(su, g->w_free_ev);
                    reduce(DrawsPart::Host, 0, d_half, su);
                    dev_event_create(&job->ev_rng_half_h);
                    dev_event_record(job->ev_rng_half_h, su);
                    first_half_to_heavy();
                    sum_first_half();
                }
            },
            [&](uint32_t slot) { if (!dev_event_sync(ev_slot[slot])) throw DevError{BPR1CS_ERR_DEVICE}; }, chain8_select(), &busy_us);
        if (ok && busy_us > 0) host_chain_rate_cell().store(busy_us / ((double)Bh * draws));   // (the next jobs' share is sized from it)
        host_wipe(job->h_tr0, (size_t)Bh * sizeof(strobe));   // (the RNG states: key material)
        if (!ok) throw DevError{BPR1CS_ERR_INVALID_ARGUMENT};   // (not the steady STROBE state - k_rng_stream refuses it alike)
        DBG_JOB("begin: host chain(s) hashed");
        dev_event_record(job->ev_head, su);
        dev_stream_wait(sl, job->ev_head);
        if (shared) dev_stream_wait(sl, g->w_free_ev);
        const uint32_t r0 = two_legs() ? d_half : 0u;   // (two legs: the first range of either part is reduced already)
        reduce(DrawsPart::Host, r0, draws, sl);
        if (Bh < B) reduce(DrawsPart::Device, r0, draws, sl);
        close();
    }
};
#endif
