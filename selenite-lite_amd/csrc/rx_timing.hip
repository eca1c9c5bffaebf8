// rx_timing.hip -- the timing entry points (selenite_rx_time_*): process calls and the two no-DSP roofs between HIP events on the
// instance's stream.  What bench.py and the tools measure with.
#include "rx_host.h"

using namespace srx;

static int time_process(selenite_rx_instance *S, const void *src, void *dst, bool q15, uint32_t blockSize,
                        uint32_t iters, float *ms_per_call, const char *who)
{
    if (!S || !ms_per_call || iters == 0) return SELENITE_RX_ARGUMENT_ERROR;
    if (!block_size_ok(S, blockSize, who)) return S->status;
    HIPCHK(S, hipSetDevice(S->device));
    return timed_loop(S, iters, ms_per_call, [&] { return run_call(S, src, q15, dst, q15, blockSize, kAll, nullptr); });
}

extern "C" int selenite_rx_time_process_device(selenite_rx_instance *S, const float *dSrcIQ, float *dDstAudio,
                                               uint32_t blockSize, uint32_t iters, float *ms_per_call)
{
    return time_process(S, dSrcIQ, dDstAudio, false, blockSize, iters, ms_per_call, "selenite_rx_time_process_device");
}

extern "C" int selenite_rx_time_process_q15_device(selenite_rx_instance *S, const int16_t *dSrcIQ, int16_t *dDstAudio,
                                                   uint32_t blockSize, uint32_t iters, float *ms_per_call)
{
    return time_process(S, dSrcIQ, dDstAudio, true, blockSize, iters, ms_per_call, "selenite_rx_time_process_q15_device");
}

extern "C" int selenite_rx_time_process_each_device(selenite_rx_instance *S, const void *dSrcIQ, void *dDstAudio, uint32_t blockSize,
                                                    uint32_t iters, float *ms_each, int q15)
{
    if (!S || !ms_each || iters == 0) return SELENITE_RX_ARGUMENT_ERROR;
    if (!block_size_ok(S, blockSize, "selenite_rx_time_process_each_device")) return S->status;
    HIPCHK(S, hipSetDevice(S->device));
    struct Events {                                        // destroyed on every exit path
        std::vector<hipEvent_t> e;
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    ev.e.assign((size_t)iters + 1, nullptr);
    for (auto &x : ev.e) HIPCHK(S, hipEventCreate(&x));
    HIPCHK(S, hipEventRecord(ev.e[0], S->stream));
    for (uint32_t i = 0; i < iters; ++i) {
        int rc = run_call(S, dSrcIQ, q15 != 0, dDstAudio, q15 != 0, blockSize, kAll, nullptr);
        if (rc) return rc;
        HIPCHK(S, hipEventRecord(ev.e[i + 1], S->stream));
    }
    HIPCHK(S, hipEventSynchronize(ev.e[iters]));
    for (uint32_t i = 0; i < iters; ++i) HIPCHK(S, hipEventElapsedTime(&ms_each[i], ev.e[i], ev.e[i + 1]));
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_time_streaming_roof_device(selenite_rx_instance *S, const void *dSrcIQ, void *dDstAudio, uint32_t blockSize,
                                                      uint32_t iters, float *ms_each, int q15)
{
    if (!S || !ms_each || iters == 0 || !dSrcIQ || !dDstAudio) return SELENITE_RX_ARGUMENT_ERROR;
    if (!block_size_ok(S, blockSize, "selenite_rx_time_streaming_roof_device")) return S->status;
    const selenite_rx_config &g = S->cfg;
    HIPCHK(S, hipSetDevice(S->device));
    // the per-channel state of SURVEY.md 8d (what selenite_rx_algorithmic_bytes counts), in a scratch buffer: the instance's own stays untouched
    uint32_t words = 0;
    if (g.nd_taps > 1) words += 2 * (g.nd_taps - 1);
    if (g.nh_taps > 1) words += 2 * (g.nh_taps - 1);
    words += 4 * g.n_biquad + (g.agc_enable ? 1 : 0) + (g.nco_enable ? 1 : 0);
    if (words > 1024) return fail(S, SELENITE_RX_LENGTH_ERROR, "selenite_rx_time_streaming_roof_device: state larger than the roof kernel handles");
    struct Scratch {
        float *p = nullptr; std::vector<hipEvent_t> e;
        ~Scratch() { if (p) (void)hipFree(p); for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } sc;
    const size_t nst = (size_t)g.channels * (words ? words : 1);
    HIPCHK(S, hipMalloc((void **)&sc.p, nst * sizeof(float)));
    HIPCHK(S, hipMemsetAsync(sc.p, 0, nst * sizeof(float), S->stream));
    sc.e.assign((size_t)iters + 1, nullptr);
    for (auto &x : sc.e) HIPCHK(S, hipEventCreate(&x));
    const uint32_t in_bytes = blockSize * (q15 ? 4u : 8u), out_bytes = (blockSize / g.decim) * (q15 ? 2u : 4u);
    for (int w = 0; w < 3; ++w) HIPCHK(S, launch_stream_roof(dSrcIQ, dDstAudio, sc.p, g.channels, in_bytes, out_bytes, words, S->stream));
    HIPCHK(S, hipEventRecord(sc.e[0], S->stream));
    for (uint32_t i = 0; i < iters; ++i) {
        HIPCHK(S, launch_stream_roof(dSrcIQ, dDstAudio, sc.p, g.channels, in_bytes, out_bytes, words, S->stream));
        HIPCHK(S, hipEventRecord(sc.e[i + 1], S->stream));
    }
    HIPCHK(S, hipEventSynchronize(sc.e[iters]));
    for (uint32_t i = 0; i < iters; ++i) HIPCHK(S, hipEventElapsedTime(&ms_each[i], sc.e[i], sc.e[i + 1]));
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_time_pattern_roof_device(selenite_rx_instance *S, const void *dSrcIQ, void *dDstAudio, uint32_t blockSize,
                                                    uint32_t iters, float *ms_each, int q15, uint32_t work)
{
    if (!S || !ms_each || iters == 0 || !dSrcIQ || !dDstAudio) return SELENITE_RX_ARGUMENT_ERROR;
    if (!block_size_ok(S, blockSize, "selenite_rx_time_pattern_roof_device")) return S->status;
    const selenite_rx_config &g = S->cfg;
    if (!cw_fused_ok(g, blockSize) || (g.block != 128 && g.block != 256 && g.block != 512) || (g.block == 512 && g.n_biquad == 2))
        return fail(S, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_time_pattern_roof_device: only the shapes of the systolic CW kernel (DSP blocks of 128 / 256 / 512) have a pattern of their own");
    HIPCHK(S, hipSetDevice(S->device));
    struct Scratch {
        float4 *p = nullptr; std::vector<hipEvent_t> e;
        ~Scratch() { if (p) (void)hipFree(p); for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } sc;
    const uint32_t ch_per_wg = 64u / g.n_biquad;
    const size_t nst = (size_t)((g.channels + ch_per_wg - 1) / ch_per_wg) * 64u;
    HIPCHK(S, hipMalloc((void **)&sc.p, nst * sizeof(float4)));
    HIPCHK(S, hipMemsetAsync(sc.p, 0, nst * sizeof(float4), S->stream));
    sc.e.assign((size_t)iters + 1, nullptr);
    for (auto &x : sc.e) HIPCHK(S, hipEventCreate(&x));
    const RxParams p = make_params(S, all_channels(S), blockSize);
    for (int w = 0; w < 3; ++w) HIPCHK(S, launch_cw_roof(p, dSrcIQ, q15 != 0, dDstAudio, sc.p, work, S->stream));
    HIPCHK(S, hipEventRecord(sc.e[0], S->stream));
    for (uint32_t i = 0; i < iters; ++i) {
        HIPCHK(S, launch_cw_roof(p, dSrcIQ, q15 != 0, dDstAudio, sc.p, work, S->stream));
        HIPCHK(S, hipEventRecord(sc.e[i + 1], S->stream));
    }
    HIPCHK(S, hipEventSynchronize(sc.e[iters]));
    for (uint32_t i = 0; i < iters; ++i) HIPCHK(S, hipEventElapsedTime(&ms_each[i], sc.e[i], sc.e[i + 1]));
    return SELENITE_RX_SUCCESS;
}
