// rx_api.hip -- the C-ABI of include/selenite_rx.h over the HIP kernels: instance setup and teardown, the accessors, and the
// device-pointer process entry points.  The dispatcher behind them is rx_dispatch.hip, the host-pointer calls rx_hostpipe.hip, the timing
// calls rx_timing.hip; each stage's host side sits next to its kernels (rx_tones.hip, rx_cwdec.hip, rx_fskdec.hip, rx_afilt.hip, rx_nlms.hip, rx_meter.hip, rx_out.hip, rx_spectrum.hip, rx_iqc.hip, rx_nb.hip).
//
// Host side of the drop-in boundary: mirrors the CMSIS-DSP init/process convention
// (arm_fir_decimate_init_f32.c:63-101 validation and state clearing; process calls return void)
// and the firmware's DSP_Set_Mode hook (Core/Src/dsp_if.c:367-370).  No CPU compute path exists
// here: without a usable HIP device init fails with SELENITE_RX_DEVICE_ERROR.
#include "rx_host.h"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

using namespace srx;

std::string &srx::last_error()
{
    static thread_local std::string msg = "";
    return msg;
}

// sinTable_f32[513] (CommonTables/arm_common_tables.c:21895) regenerated from the generator the
// reference documents (:21881-21891): the source holds every entry as an 8-decimal literal, so
// entry n = float("%.8f" % sin(2*pi*n/512)), sign of the (tiny negative) last entry included.
const float *srx::host_sin_table()
{
    static float table[513];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int n = 0; n <= 512; ++n) {
            const double s = std::sin(2.0 * 3.14159265358979323846 * (double)n / 512.0);
            char buf[32];
            std::snprintf(buf, sizeof buf, "%.8f", s);
            table[n] = std::strtof(buf, nullptr);
        }
    });
    return table;
}

static bool mode_valid(uint8_t m, uint32_t nh_taps)
{
    if (m == SELENITE_MODE_FM) return nh_taps >= 2;        // the discriminator's one-sample memory lives in the FIR pair's delay lines
    return m == SELENITE_MODE_LSB || m == SELENITE_MODE_USB || m == SELENITE_MODE_CW ||
           m == SELENITE_MODE_CWR || m == SELENITE_MODE_AM || m == SELENITE_MODE_DIG ||
           m == SELENITE_MODE_PKT;
}

static void classify_coeffs(selenite_rx_instance *S)
{
    const TapClass t = classify_taps(S->h_delay.data(), S->h_hilb.data(), S->cfg.nh_taps);
    S->delay_is_impulse = t.delay_is_impulse;
    S->hilb_odd_only = t.hilb_odd_only;
    if (t.delay_is_impulse) S->delay_index = t.delay_index;
}

static void free_device(selenite_rx_instance *S)
{
    dev_free(S->d_flags, S->d_guard_ch, S->d_rerun_flag, S->d_rerun_list, S->d_hist_ext, S->d_conv_in, S->d_dec_c, S->d_hilb_c, S->d_delay_c, S->d_biq_c, S->d_sintab, S->d_step, S->d_phase,
             S->d_dec_state, S->d_fir_state, S->d_biq_state, S->d_gain, S->d_scratch, S->d_env, S->d_env_part,
             S->d_io_in, S->d_io_out, S->d_lo, S->pipe.d_in[0], S->pipe.d_in[1], S->pipe.d_out[0], S->pipe.d_out[1]);
    S->tones.release();
    S->cwdec.release();
    S->fskdec.release();
    S->afilt.release();
    S->nr.release();
    S->meter.release();
    S->out.release();
    S->spec.release();
    S->iqc.release();
    S->nb.release();
    if (S->h_rerun_seen) (void)hipHostFree(S->h_rerun_seen);
    S->h_rerun_seen = nullptr;
    for (int i = 0; i < 2; ++i) {
        if (S->pipe.h_in[i]) (void)hipHostFree(S->pipe.h_in[i]);
        if (S->pipe.h_out[i]) (void)hipHostFree(S->pipe.h_out[i]);
        if (S->pipe.ev_in[i]) (void)hipEventDestroy(S->pipe.ev_in[i]);
        if (S->pipe.ev_done[i]) (void)hipEventDestroy(S->pipe.ev_done[i]);
        if (S->pipe.ev_out[i]) (void)hipEventDestroy(S->pipe.ev_out[i]);
    }
    if (S->pipe.h2d) (void)hipStreamDestroy(S->pipe.h2d);
    if (S->pipe.d2h) (void)hipStreamDestroy(S->pipe.d2h);
    free_fused(S->plan);
    if (S->own_stream) (void)hipStreamDestroy(S->own_stream);
}

static int reset_state(selenite_rx_instance *S)
{
    const selenite_rx_config &g = S->cfg;
    const size_t C = g.channels;
    if (g.nd_taps > 1) HIPCHK(S, hipMemsetAsync(S->d_dec_state, 0, C * 2 * (g.nd_taps - 1) * sizeof(float), S->stream));
    if (g.nh_taps > 1) HIPCHK(S, hipMemsetAsync(S->d_fir_state, 0, C * 2 * (g.nh_taps - 1) * sizeof(float), S->stream));
    if (g.n_biquad) HIPCHK(S, hipMemsetAsync(S->d_biq_state, 0, C * 4 * g.n_biquad * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(S->d_phase, 0, C * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(S->d_flags, 0, kFlagWords * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(S->d_guard_ch, 0, 3 * C * sizeof(uint32_t), S->stream));
    // (0 = no rerun pending, the channel's state is in exact arithmetic (kProvExact): what a cleared state is)
    if (S->d_rerun_flag) HIPCHK(S, hipMemsetAsync(S->d_rerun_flag, 0, C * sizeof(uint32_t), S->stream));
    if (S->d_rerun_list) HIPCHK(S, hipMemsetAsync(S->d_rerun_list, 0, 2 * sizeof(uint32_t), S->stream));      // both counters
    S->rerun_par = 0;
    if (int rc = fill_rows(S, S->d_gain, C, &g.agc_gain_init)) return rc;      // (drains the stream)
    S->phase_uniform = true;
    S->phase_host = 0;
    if (int rc = S->tones.init_state(S)) return rc;
    if (int rc = S->cwdec.init_state(S)) return rc;
    if (int rc = S->fskdec.init_state(S)) return rc;
    if (int rc = S->afilt.init_state(S)) return rc;
    if (int rc = S->nr.init_state(S)) return rc;
    if (int rc = S->meter.init_state(S)) return rc;
    if (int rc = S->out.init_state(S)) return rc;
    if (int rc = S->spec.init_state(S)) return rc;
    if (int rc = S->iqc.init_state(S)) return rc;
    return S->nb.init_state(S);
}

// the kernels' flag word (non-finite audio: ARM_MATH_NANINF), read after the stream has drained; latches the status
int srx::check_device_flags(selenite_rx_instance *S)
{
    uint32_t f = 0;
    HIPCHK(S, hipMemcpy(&f, S->d_flags, sizeof f, hipMemcpyDeviceToHost));
    if (f & 1u) fail(S, SELENITE_RX_NANINF, "a process call produced NaN / Inf audio (non-finite input samples?)");
    return S->status;
}

extern "C" int selenite_rx_abi_version(void) { return SELENITE_RX_ABI_VERSION; }

// ---- plan options (rx_diag.h) ----
namespace { uint32_t g_plan_opt[SELENITE_RX_OPT_COUNT] = { 0u, 0u, 0u, 0u, 0u, 0u }; }
namespace srx {
uint32_t plan_option(int option)
{
    return option >= 0 && option < SELENITE_RX_OPT_COUNT ? __atomic_load_n(&g_plan_opt[option], __ATOMIC_RELAXED) : 0u;
}
}  // namespace srx
extern "C" int selenite_rx_set_plan_option(int option, uint32_t value)
{
    if (option < 0 || option >= SELENITE_RX_OPT_COUNT) return SELENITE_RX_ARGUMENT_ERROR;
    if (option == SELENITE_RX_OPT_RERUN_GRID || option == SELENITE_RX_OPT_CW_GRID ? value > (1u << 20) : value > 1u) return SELENITE_RX_ARGUMENT_ERROR;
    __atomic_store_n(&g_plan_opt[option], value, __ATOMIC_RELAXED);
    return SELENITE_RX_SUCCESS;
}
extern "C" uint32_t selenite_rx_get_plan_option(int option) { return srx::plan_option(option); }

extern "C" int selenite_rx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int selenite_rx_set_device(int ordinal)
{
    HIPCHK(nullptr, hipSetDevice(ordinal));
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_init(selenite_rx_instance **out, const selenite_rx_config *caller_cfg)
{
    if (!out) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: S is NULL");
    *out = nullptr;
    if (!caller_cfg) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: cfg is NULL");
    // The caller owns the struct and says, through struct_size, which header it was built against (include/selenite_rx.h: ABI versions).
    // Version 1 ends with agc_gain_init: nothing behind it is read (it is padding of the caller's), int16 output truncates.
    static_assert(offsetof(selenite_rx_config, q15_rounding) == 108 && sizeof(selenite_rx_config) == 120, "selenite_rx_config layout (LP64)");
    selenite_rx_config own{};
    if (caller_cfg->struct_size == SELENITE_RX_CONFIG_SIZE_V1) {
        std::memcpy(&own, caller_cfg, offsetof(selenite_rx_config, q15_rounding));
        own.abi_version = 1;
    } else if (caller_cfg->struct_size == sizeof(selenite_rx_config)) {
        own = *caller_cfg;
        if (own.abi_version != SELENITE_RX_ABI_VERSION || own.reserved != 0)
            return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: abi_version must be SELENITE_RX_ABI_VERSION (2) and reserved 0 with this struct_size");
        if (own.q15_rounding > 1u)
            return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: q15_rounding is 0 or 1");
    } else {
        return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: struct_size matches neither this header's selenite_rx_config nor version 1's");
    }
    own.struct_size = (uint32_t)sizeof(selenite_rx_config);
    const selenite_rx_config *cfg = &own;
    if (cfg->channels == 0 || cfg->block == 0 || cfg->decim == 0)
        return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: channels, block, decim must be non-zero");
    if (!mode_valid(cfg->mode, cfg->nh_taps))
        return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: unsupported mode (FM needs the FIR pair's delay lines: nh_taps >= 2)");
    if (cfg->arith != SELENITE_ARITH_CMSIS && cfg->arith != SELENITE_ARITH_FMA && cfg->arith != SELENITE_ARITH_SPLIT16 &&
        cfg->arith != SELENITE_ARITH_AUTO)
        return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: bad arith");
    if (cfg->nd_taps == 0 && cfg->decim != 1)
        return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: decim > 1 needs a decimator (nd_taps)");
    if (cfg->nd_taps && !cfg->dec_coeffs)
        return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: dec_coeffs is NULL");
    if (cfg->nh_taps && (!cfg->hilb_coeffs || !cfg->delay_coeffs))
        return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: hilb_coeffs / delay_coeffs is NULL");
    if (cfg->n_biquad && !cfg->biquad_coeffs)
        return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: biquad_coeffs is NULL");
    if (cfg->nd_taps > 65535 || cfg->nh_taps > 65535 || cfg->decim > 255)   // CMSIS field widths
        return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_init: taps > 65535 or decim > 255");
    // arm_fir_decimate_init_f32.c:74-97
    if (cfg->block % cfg->decim != 0)
        return fail(nullptr, SELENITE_RX_LENGTH_ERROR, "selenite_rx_init: block is not a multiple of decim");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, SELENITE_RX_DEVICE_ERROR,
                    "selenite_rx_init: no HIP device (this library has no CPU fallback)");

    selenite_rx_instance *S = new selenite_rx_instance();
    S->cfg = *cfg;
    const size_t C = cfg->channels;
    if (cfg->nd_taps) S->h_dec.assign(cfg->dec_coeffs, cfg->dec_coeffs + cfg->nd_taps);
    if (cfg->nh_taps) {
        S->h_hilb.assign(cfg->hilb_coeffs, cfg->hilb_coeffs + cfg->nh_taps);
        S->h_delay.assign(cfg->delay_coeffs, cfg->delay_coeffs + cfg->nh_taps);
    }
    if (cfg->n_biquad) S->h_biq.assign(cfg->biquad_coeffs, cfg->biquad_coeffs + 5 * cfg->n_biquad);
    S->h_step.resize(C);
    for (size_t c = 0; c < C; ++c) S->h_step[c] = cfg->nco_step ? cfg->nco_step[c] : cfg->nco_step_all;
    S->cfg.dec_coeffs = S->h_dec.data(); S->cfg.hilb_coeffs = S->h_hilb.data();
    S->cfg.delay_coeffs = S->h_delay.data(); S->cfg.biquad_coeffs = S->h_biq.data();
    S->cfg.nco_step = S->h_step.data();
    S->steps_uniform = true;
    for (size_t c = 1; c < C; ++c) S->steps_uniform = S->steps_uniform && S->h_step[c] == S->h_step[0];
    S->steps_grid256 = true;
    for (size_t c = 0; c < C; ++c) S->steps_grid256 = S->steps_grid256 && (S->h_step[c] & 0x00FFFFFFu) == 0;
    // kernel-selection overrides of the tests (selenite_rx_set_plan_option): taken over at init, results do not depend on them
    S->force_generic = plan_option(SELENITE_RX_OPT_FORCE_GENERIC) ? 1 : 0;
    S->no_shared_lo = plan_option(SELENITE_RX_OPT_NO_SHARED_LO) ? 1 : 0;
    S->no_periodic_lo = plan_option(SELENITE_RX_OPT_NO_PERIODIC_LO) ? 1 : 0;

#define INITCHK(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            int rc_ = fail(nullptr, SELENITE_RX_DEVICE_ERROR,                                \
                           std::string("selenite_rx_init: " #call ": ") + hipGetErrorString(e_)); \
            free_device(S);                                                                  \
            delete S;                                                                        \
            return rc_;                                                                      \
        }                                                                                    \
    } while (0)

    INITCHK(hipGetDevice(&S->device));
    INITCHK(hipStreamCreateWithFlags(&S->own_stream, hipStreamNonBlocking));
    S->stream = S->own_stream;
    INITCHK(dev_upload(&S->d_dec_c, S->h_dec.data(), S->h_dec.size()));
    INITCHK(dev_upload(&S->d_hilb_c, S->h_hilb.data(), S->h_hilb.size()));
    INITCHK(dev_upload(&S->d_delay_c, S->h_delay.data(), S->h_delay.size()));
    INITCHK(dev_upload(&S->d_biq_c, S->h_biq.data(), S->h_biq.size()));
    INITCHK(dev_upload(&S->d_sintab, host_sin_table(), (size_t)513));
    INITCHK(dev_upload(&S->d_step, S->h_step.data(), C));
    INITCHK(dev_alloc(&S->d_phase, C));
    INITCHK(dev_alloc(&S->d_dec_state, cfg->nd_taps > 1 ? C * 2 * (cfg->nd_taps - 1) : 0));
    INITCHK(dev_alloc(&S->d_fir_state, cfg->nh_taps > 1 ? C * 2 * (cfg->nh_taps - 1) : 0));
    INITCHK(dev_alloc(&S->d_biq_state, C * 4 * cfg->n_biquad));
    INITCHK(dev_alloc(&S->d_gain, C));
    INITCHK(dev_alloc(&S->d_flags, (size_t)kFlagWords));
    INITCHK(dev_alloc(&S->d_guard_ch, 3 * C));
    INITCHK(dev_alloc(&S->d_rerun_flag, cfg->arith == SELENITE_ARITH_AUTO ? C : 0));
    INITCHK(dev_alloc(&S->d_rerun_list, cfg->arith == SELENITE_ARITH_AUTO ? C + 2 : 0));
    if (cfg->arith == SELENITE_ARITH_AUTO) {
        INITCHK(hipHostMalloc(reinterpret_cast<void **>(&S->h_rerun_seen), sizeof(uint32_t), hipHostMallocMapped));
        *S->h_rerun_seen = 0u;
    }
    // k_ssb_split16 leaves the mixed samples in front of the decimator state in rows of ext_len samples (two buffers: the one a channel's
    // state points at stays intact while the next call fills the other), for k_hist_exact
    // (round 4: allocated by the first call that needs it -- 2 x channels x ext_len x 8 bytes, 4 KB per channel for the cfg3 chain --
    // and released when the repair is switched off: ensure_hist_ext / selenite_rx_set_handover_repair)
    if (!diag_env("SELENITE_RX_NO_HIST_EXT")) S->ext_len = hist_ext_len(*cfg);
#undef INITCHK
    classify_coeffs(S);
    if (plan_fused(S->cfg, S->delay_is_impulse, S->hilb_odd_only, S->plan) != hipSuccess) {
        int rc_ = fail(nullptr, SELENITE_RX_DEVICE_ERROR, "selenite_rx_init: building fused-kernel tables failed");
        free_device(S);
        delete S;
        return rc_;
    }
    int rc = reset_state(S);
    if (rc != SELENITE_RX_SUCCESS) { free_device(S); delete S; return rc; }
    *out = S;
    return SELENITE_RX_SUCCESS;
}

extern "C" void selenite_rx_free(selenite_rx_instance *S)
{
    if (!S) return;
    (void)hipSetDevice(S->device);
    if (S->stream) (void)hipStreamSynchronize(S->stream);
    free_device(S);
    delete S;
}

extern "C" int selenite_rx_set_mode(selenite_rx_instance *S, uint8_t mode)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_mode: S is NULL");
    if (!mode_valid(mode, S->cfg.nh_taps)) return refuse("selenite_rx_set_mode", "unsupported mode");      // instance stays usable in its old mode
    S->cfg.mode = mode;
    HIPCHK(S, plan_fused(S->cfg, S->delay_is_impulse, S->hilb_odd_only, S->plan));
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_status(const selenite_rx_instance *S) { return S ? S->status : SELENITE_RX_ARGUMENT_ERROR; }
extern "C" const char *selenite_rx_error_string(const selenite_rx_instance *S)
{
    return S ? S->err.c_str() : last_error().c_str();
}
extern "C" const char *selenite_rx_kernel_name(const selenite_rx_instance *S)
{
    if (!S) return "";
    if (on_ssb_fused(S)) return S->plan.name;
    if (S->force_generic) return "generic";
    if (cw_fused_ok(S->cfg, S->cfg.block)) {
        static thread_local std::string name;
        name = "k_cw_fused<" + std::to_string(S->cfg.n_biquad) + "," + std::to_string(S->cfg.block) + ">";
        return name.c_str();
    }
    return "generic";
}

extern "C" int selenite_rx_set_stream(selenite_rx_instance *S, void *hip_stream)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : S->own_stream;
    if (next != S->stream) {
        // calls already queued on the old stream and calls on the new one share the streaming state (filter
        // histories, gains, phases, the LO table, scratch): drain the old stream before switching
        HIPCHK(S, hipSetDevice(S->device));
        HIPCHK(S, hipStreamSynchronize(S->stream));
        S->stream = next;
    }
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_sync(selenite_rx_instance *S)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    HIPCHK(S, hipStreamSynchronize(S->stream));
    return check_device_flags(S);
}

extern "C" int selenite_rx_set_guard_ratio(selenite_rx_instance *S, float ratio)
{
    if (!S || !(ratio >= 0.0f)) return SELENITE_RX_ARGUMENT_ERROR;      // (NaN rejected)
    S->guard_ratio = ratio;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_guard_stats(selenite_rx_instance *S, uint64_t *guard_blocks, uint64_t *guard_channel_calls,
                                       uint64_t *rerun_channel_calls)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    HIPCHK(S, hipSetDevice(S->device));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    // the kernels keep two words per channel (no atomics on shared counters); summed here, on the host
    const size_t C = S->cfg.channels;
    std::vector<uint32_t> w(2 * C);
    HIPCHK(S, hipMemcpy(w.data(), S->d_guard_ch, 2 * C * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t blocks = 0, calls = 0;
    for (size_t c = 0; c < C; ++c) { blocks += w[c]; calls += w[C + c]; }
    if (guard_blocks) *guard_blocks = blocks;
    if (guard_channel_calls) *guard_channel_calls = calls;
    // SELENITE_ARITH_AUTO recomputes every guarded channel-call (the counts only ever come from the split-precision kernels)
    if (rerun_channel_calls) *rerun_channel_calls = S->cfg.arith == SELENITE_ARITH_AUTO ? calls : 0;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_guard_channels(selenite_rx_instance *S, uint32_t *per_channel)
{
    if (!S || !per_channel) return SELENITE_RX_ARGUMENT_ERROR;
    HIPCHK(S, hipSetDevice(S->device));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    HIPCHK(S, hipMemcpy(per_channel, S->d_guard_ch, (size_t)S->cfg.channels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SELENITE_RX_SUCCESS;
}

// diagnostic (tests, tools): the per-channel words of SELENITE_ARITH_AUTO (rx_internal.h: rerun / provenance / hold bits, level)
extern "C" int selenite_rx_auto_words(selenite_rx_instance *S, uint32_t *per_channel)
{
    if (!S || !per_channel) return SELENITE_RX_ARGUMENT_ERROR;
    HIPCHK(S, hipSetDevice(S->device));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    if (!S->d_rerun_flag) { std::memset(per_channel, 0, (size_t)S->cfg.channels * sizeof(uint32_t)); return SELENITE_RX_SUCCESS; }
    HIPCHK(S, hipMemcpy(per_channel, S->d_rerun_flag, (size_t)S->cfg.channels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_guard_clear(selenite_rx_instance *S)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    HIPCHK(S, hipSetDevice(S->device));
    HIPCHK(S, hipMemsetAsync(S->d_guard_ch, 0, 3 * (size_t)S->cfg.channels * sizeof(uint32_t), S->stream));
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_set_auto_launches(selenite_rx_instance *S, int launches)
{
    if (!S || !(launches == 1 || launches == 3)) return SELENITE_RX_ARGUMENT_ERROR;
    S->auto_launches = launches;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_auto_launches_last(const selenite_rx_instance *S)
{
    return S ? (int)S->auto_form_last : 0;
}

extern "C" int selenite_rx_set_handover_repair(selenite_rx_instance *S, int on)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    S->handover_repair = on != 0;
    if (!S->handover_repair && S->d_hist_ext) {
        // the rows go (0.27 GB at 65 536 channels of the cfg3 chain); a state that pointed at them is "matrix kernel, no samples" from now on
        HIPCHK(S, hipSetDevice(S->device));
        HIPCHK(S, hipStreamSynchronize(S->stream));
        const size_t C = S->cfg.channels;
        std::vector<uint32_t> w(C);
        HIPCHK(S, hipMemcpy(w.data(), S->d_rerun_flag, C * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < C; ++c)
            if (((w[c] >> kProvShift) & kProvMask) == kProvSplitExt)
                w[c] = (w[c] & ~((kProvMask << kProvShift) | kExtQ15)) | (kProvSplit << kProvShift);
        HIPCHK(S, hipMemcpy(S->d_rerun_flag, w.data(), C * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCHK(S, hipFree(S->d_hist_ext));
        S->d_hist_ext = nullptr;
    }
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_guard_handover(selenite_rx_instance *S, uint64_t *handover_blocks)
{
    if (!S || !handover_blocks) return SELENITE_RX_ARGUMENT_ERROR;
    HIPCHK(S, hipSetDevice(S->device));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    const size_t C = S->cfg.channels;
    std::vector<uint32_t> w(C);
    HIPCHK(S, hipMemcpy(w.data(), S->d_guard_ch + 2 * C, C * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t n = 0;
    for (size_t c = 0; c < C; ++c) n += w[c];
    *handover_blocks = n;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_reset(selenite_rx_instance *S)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    return reset_state(S);
}

// ---- device-pointer process calls (rx_dispatch.hip) ----
extern "C" void selenite_rx_process_f32_device(selenite_rx_instance *S, const float *dSrcIQ,
                                               float *dDstAudio, uint32_t blockSize)
{
    if (!S || !block_size_ok(S, blockSize, "selenite_rx_process_f32_device")) return;
    run_call(S, dSrcIQ, false, dDstAudio, false, blockSize, kAll, nullptr);
}

extern "C" void selenite_rx_process_q15_device(selenite_rx_instance *S, const int16_t *dSrcIQ,
                                               int16_t *dDstAudio, uint32_t blockSize)
{
    if (!S || !block_size_ok(S, blockSize, "selenite_rx_process_q15_device")) return;
    run_call(S, dSrcIQ, true, dDstAudio, true, blockSize, kAll, nullptr);
}

extern "C" void selenite_rx_global_phase1_device(selenite_rx_instance *S, const float *dSrcIQ,
                                                 float *dDstAudio, float *dEnv, uint32_t blockSize)
{
    if (!S || !block_size_ok(S, blockSize, "selenite_rx_global_phase1_device")) return;
    if (!(S->cfg.agc_enable && S->cfg.agc_global)) {
        fail(S, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_global_phase1_device: instance is not agc_global");
        return;
    }
    if (S->out.on) {
        fail(S, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_global_phase1_device: the split calls exchange audio at the decimated rate: not with an output stage (selenite_rx_set_out)");
        return;
    }
    run_call(S, dSrcIQ, false, dDstAudio, false, blockSize, kPhase1, dEnv);
}

extern "C" void selenite_rx_global_phase2_device(selenite_rx_instance *S, float *dDstAudio,
                                                 const float *dEnv, uint32_t blockSize)
{
    if (!S || !block_size_ok(S, blockSize, "selenite_rx_global_phase2_device")) return;
    if (!(S->cfg.agc_enable && S->cfg.agc_global)) {
        fail(S, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_global_phase2_device: instance is not agc_global");
        return;
    }
    if (S->out.on) {
        fail(S, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_global_phase2_device: the split calls exchange audio at the decimated rate: not with an output stage (selenite_rx_set_out)");
        return;
    }
    run_call(S, nullptr, false, dDstAudio, false, blockSize, kPhase2, const_cast<float *>(dEnv));
}

// ------------------------------------------------------------------------------------------
// the five arrays of selenite_rx_state_view copied out of the device (to_host) or into it; a row the configuration does not have is skipped
static int chain_state_copy(selenite_rx_instance *S, const selenite_rx_state_view *v, bool to_host)
{
    const selenite_rx_config &g = S->cfg;
    const size_t b = g.channels * sizeof(float);            // bytes of one word per channel
    return copy_rows(S, to_host, { { S->d_dec_state, g.nd_taps > 1 ? v->dec_state : nullptr, b * 2 * (g.nd_taps - 1) },
                                   { S->d_fir_state, g.nh_taps > 1 ? v->fir_state : nullptr, b * 2 * (g.nh_taps - 1) },
                                   { S->d_biq_state, g.n_biquad ? v->biq_state : nullptr, b * 4 * g.n_biquad },
                                   { S->d_gain, v->agc_gain, b }, { S->d_phase, v->nco_phase, b } });
}

extern "C" int selenite_rx_get_state(selenite_rx_instance *S, const selenite_rx_state_view *v)
{
    if (!S || !v) return SELENITE_RX_ARGUMENT_ERROR;
    return chain_state_copy(S, v, true);
}

extern "C" int selenite_rx_set_state(selenite_rx_instance *S, const selenite_rx_state_view *v)
{
    if (!S || !v) return SELENITE_RX_ARGUMENT_ERROR;
    const size_t C = S->cfg.channels;
    if (int rc = chain_state_copy(S, v, false)) return rc;
    if (v->nco_phase) {
        S->phase_uniform = true;
        for (size_t c = 1; c < C; ++c) S->phase_uniform = S->phase_uniform && v->nco_phase[c] == v->nco_phase[0];
        S->phase_host = v->nco_phase[0];
    }
    if (S->d_rerun_flag) HIPCHK(S, hipMemsetAsync(S->d_rerun_flag, 0, C * sizeof(uint32_t), S->stream));      // a given state counts as exact
    return SELENITE_RX_SUCCESS;
}

extern "C" void *selenite_rx_device_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { last_error() = "hipMalloc failed"; return nullptr; }
    return p;
}
extern "C" void selenite_rx_device_free(void *dptr) { if (dptr) (void)hipFree(dptr); }
extern "C" int selenite_rx_memcpy_h2d(void *dptr, const void *hptr, size_t bytes)
{
    HIPCHK(nullptr, hipMemcpy(dptr, hptr, bytes, hipMemcpyHostToDevice));
    return SELENITE_RX_SUCCESS;
}
extern "C" int selenite_rx_memcpy_d2h(void *hptr, const void *dptr, size_t bytes)
{
    HIPCHK(nullptr, hipMemcpy(hptr, dptr, bytes, hipMemcpyDeviceToHost));
    return SELENITE_RX_SUCCESS;
}

// ------------------------------------------------------------------------------------------
extern "C" void selenite_rx_synth_iq_host(float *iq, uint32_t first_channel, uint32_t nch,
                                          uint64_t first_sample, uint32_t nsamp, uint64_t seed)
{
    synth_host(iq, host_sin_table(), first_channel, nch, first_sample, nsamp, seed);
}

extern "C" int selenite_rx_synth_iq_device(selenite_rx_instance *S, float *dIQ, uint32_t first_channel,
                                           uint32_t nch, uint64_t first_sample, uint32_t nsamp, uint64_t seed)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    HIPCHK(S, hipSetDevice(S->device));
    HIPCHK(S, launch_synth(dIQ, S->d_sintab, first_channel, nch, first_sample, nsamp, seed, S->stream));
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_device_pci_bus_id(int ordinal, char *buf, size_t len)
{
    if (!buf || len < 13) return SELENITE_RX_ARGUMENT_ERROR;
    HIPCHK(nullptr, hipDeviceGetPCIBusId(buf, (int)len, ordinal));
    return SELENITE_RX_SUCCESS;
}

extern "C" uint64_t selenite_rx_algorithmic_bytes(const selenite_rx_config *g, uint32_t blockSize, uint64_t *read_bytes)
{
    if (!g || g->decim == 0) return 0;
    // state = FIR histories (both rails) + 16 B per biquad stage + AGC/NCO scalars,
    // read once and written once per channel-block.
    uint64_t state = 0;
    if (g->nd_taps > 1) state += 4ull * 2 * (g->nd_taps - 1);
    if (g->nh_taps > 1) state += 4ull * 2 * (g->nh_taps - 1);
    state += 16ull * g->n_biquad;
    state += 4ull * ((g->agc_enable ? 1 : 0) + (g->nco_enable ? 1 : 0));
    const uint64_t rd = 8ull * blockSize + state;
    const uint64_t wr = 4ull * (blockSize / g->decim) + state;
    if (read_bytes) *read_bytes = rd * g->channels;
    return (rd + wr) * g->channels;
}
