// C ABI: sustained integer rates of the device (bench.py's ceilings).
#pragma once
#include "api_common.hpp"
// Sustained instruction / primitive rates of the device this process runs on (bench.py's integer ceilings)
extern "C" int bpr1cs_device_rates(double seconds_each, double* mad_lane_ops_per_s, double* table_adds_per_s) {
    if (!mad_lane_ops_per_s || !table_adds_per_s || !(seconds_each > 0) || seconds_each > 2.0) return BPR1CS_ERR_INVALID_ARGUMENT;
    if (!have_device()) return BPR1CS_ERR_NO_DEVICE;
#if defined(BPR1CS_HOSTSIM)
    *mad_lane_ops_per_s = 0; *table_adds_per_s = 0;
    return BPR1CS_OK;
#else
    API_TRY
    const uint32_t blocks = dev_cu_count() * 8u, threads = 256;  // 8 wavefronts per SIMD
    if (!blocks) throw DevError{DEV_ERR_DEVICE};
    dev_stream_t st{};
    CallScope scope(st);
    DevBuf<uint32_t> out((size_t)blocks * threads);
    struct Events {
        dev_event_t e0{}, e1{};
        ~Events() { dev_event_destroy(&e0); dev_event_destroy(&e1); }
    } ev;
    dev_event_create(&ev.e0, true);
    dev_event_create(&ev.e1, true);
    auto timed = [&](int which, uint32_t iters) {
        dev_event_record(ev.e0, st);
        launch_kernel(which == 0 ? k_probe_mad : k_probe_madd, dim3(blocks), dim3(threads), 0, st, out.p, iters);
        dev_event_record(ev.e1, st);
        if (!dev_event_sync(ev.e1)) throw DevError{DEV_ERR_DEVICE};
        return (double)dev_event_ms(ev.e0, ev.e1) * 1e-3;
    };
    double rate[2];
    for (int which = 0; which < 2; which++) {
        uint32_t iters = which == 0 ? 4096u : 64u;
        double t = timed(which, iters);                       // calibration (also warms the clocks up)
        double scale = seconds_each / (t > 1e-6 ? t : 1e-6);
        uint64_t want = (uint64_t)((double)iters * (scale < 1 ? 1 : scale));
        if (want > 0x7fffffffull) want = 0x7fffffffull;
        t = timed(which, (uint32_t)want);
        rate[which] = (double)blocks * threads * (double)want * (which == 0 ? 8.0 : 1.0) / t;
    }
    *mad_lane_ops_per_s = rate[0];
    *table_adds_per_s = rate[1];
    return BPR1CS_OK;
    API_CATCH
#endif
}
