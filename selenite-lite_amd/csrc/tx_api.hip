// tx_api.hip -- the TX instance and its chain on the host side (include/selenite_tx.h): init / free, mode, status, stream, reset, the
// chain's state accessors, run() executing the decision of tx_select.h, the audio entries and their timing entry.  The kernels are in
// tx_generic.hip and tx_fused.hip; FM, keyed CW and the input stage have their host sides in their own files (tx_host.h).
#include <cmath>
#include <cstddef>
#include <cstring>

#include "tx_host.h"

namespace srx {

static bool tx_mode_ok(uint8_t m)
{
    return m == SELENITE_MODE_LSB || m == SELENITE_MODE_USB || m == SELENITE_MODE_CW || m == SELENITE_MODE_CWR ||
           m == SELENITE_MODE_AM || m == SELENITE_MODE_DIG || m == SELENITE_MODE_PKT;
}

TxParams make_params(const selenite_tx_instance *S, uint32_t block_size)
{
    const selenite_tx_config &g = S->cfg;
    TxParams p{};
    p.channels = g.channels; p.block = g.block; p.L = g.interp; p.ni = g.ni_taps;
    p.P = g.ni_taps ? g.ni_taps / g.interp : 1; p.nh = g.nh_taps; p.mode = g.mode;
    p.nco = g.nco_enable ? 1 : 0; p.alc = g.alc_enable ? 1 : 0; p.block_size = block_size; p.q15_round = g.q15_rounding ? 1u : 0u;
    p.ic = S->d_ic; p.hc = S->d_hc; p.dc = S->d_dc; p.sintab = S->d_sintab;
    p.step = S->d_step; p.phase = S->d_phase;
    p.fir_state = S->d_fir_state; p.int_state = S->d_int_state; p.gain = S->d_gain;
    p.alcp = AgcParams{ g.alc_target, g.alc_attack, g.alc_decay, g.alc_gain_min, g.alc_gain_max, g.alc_env_floor };
    return p;
}

bool block_size_ok(selenite_tx_instance *S, uint32_t bs, const char *who)
{
    if (!S) return false;
    if (bs == 0 || bs % S->cfg.block != 0) {
        fail(S, SELENITE_RX_LENGTH_ERROR, std::string(who) + ": blockSize is not a non-zero multiple of cfg.block");
        return false;
    }
    return true;
}

TxDecision decide(const selenite_tx_instance *S, const TxParams &p, bool key)
{
    TxSelCall c;
    c.block_size = p.block_size; c.key = key; c.phase_uniform = S->phase_uniform;
    c.lds_generic = tx_lds_bytes(p); c.lds_fm = tx_fm_lds_bytes(p); c.lds_cw = key ? tx_cw_lds_bytes(p, S->cw.p) : 0;
    return tx_select(S->cfg, S->sel, c);
}

int run(selenite_tx_instance *S, const void *src, void *dst, bool q15, uint32_t bs)
{
    HIPCHK(S, hipSetDevice(S->device));
    const selenite_tx_config &g = S->cfg;
    TxParams p = make_params(S, bs);
    const TxDecision d = decide(S, p, false);
    if (d.refused) return fail(S, SELENITE_RX_LENGTH_ERROR, "filter lengths exceed the LDS budget of the TX kernel");
    // decided: from here on the host's state moves
    if (d.clears_uniform) S->phase_uniform = false;         // no shared LO until reset or set_state say otherwise
    if (d.kernel == kTxFm) {
        HIPCHK(S, launch_tx_fm(p, S->fm.p, (int)g.arith, src, q15, dst, S->stream));
        return 0;
    }
    const uint32_t phase_now = S->phase_host;
    if (g.nco_enable) S->phase_host += bs * g.interp * S->h_step[0];
    if (d.kernel == kTxGeneric) {
        HIPCHK(S, launch_tx_generic(p, (int)g.arith, src, q15, dst, S->stream));
        return 0;
    }
    if (d.lo_n && !(S->lo_valid && S->lo_phase == phase_now && S->lo_step == S->h_step[0] && S->lo_n >= d.lo_n)) {
        // the table is a pure function of (start phase, step, length): reused when the call starts where it starts
        // (every call for an LO on the fs / 256 grid: the phase advance of a call is then a multiple of 2^32)
        S->lo_valid = false;
        if (ensure(S, (void **)&S->d_lo, &S->lo_bytes, (size_t)d.lo_n * sizeof(float2))) return S->status;
        HIPCHK(S, launch_lo_table(S->d_lo, S->d_sintab, phase_now, S->h_step[0], d.lo_n, S->stream));
        S->lo_valid = true; S->lo_phase = phase_now; S->lo_step = S->h_step[0]; S->lo_n = d.lo_n;
    }
    const float2 *lo = d.lo_n ? S->d_lo : nullptr;
    p.lo_period = d.nco == 3u ? 256u : 0u;                  // k_tx_split16 keeps the period in registers
    if (d.kernel == kTxSplit16)
        HIPCHK(S, launch_tx_split16(p, d.nco, S->delay_index, lo, S->d_ttab16, S->tpost, src, q15, dst, S->stream));
    else
        HIPCHK(S, launch_tx_fused(p, (int)g.arith, d.nco, S->delay_index, lo, src, q15, dst, S->stream));
    return 0;
}

static int reset_state(selenite_tx_instance *S)
{
    const selenite_tx_config &g = S->cfg;
    const size_t C = g.channels, nh1 = g.nh_taps ? g.nh_taps - 1 : 0, p1 = g.ni_taps ? g.ni_taps / g.interp - 1 : 0;
    if (nh1) HIPCHK(S, hipMemsetAsync(S->d_fir_state, 0, C * 2 * nh1 * sizeof(float), S->stream));
    if (p1) HIPCHK(S, hipMemsetAsync(S->d_int_state, 0, C * 2 * p1 * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(S->d_phase, 0, C * sizeof(uint32_t), S->stream));
    if (tx_fm_reset(S) || tx_cw_reset(S) || tx_in_reset(S) || tx_keyer_reset(S)) return S->status;
    if (int rc = fill_rows(S, S->d_gain, C, &g.alc_gain_init)) return rc;      // (drains the stream)
    S->phase_host = 0;
    S->phase_uniform = S->sel.steps_same;
    return 0;
}

// the chain's rows of a state view, out of the device or into it
static int state_copy(selenite_tx_instance *S, const selenite_tx_state_view *v, bool to_host)
{
    const selenite_tx_config &g = S->cfg;
    const size_t C = g.channels, nh1 = g.nh_taps ? g.nh_taps - 1 : 0, p1 = g.ni_taps ? g.ni_taps / g.interp - 1 : 0;
    return copy_rows(S, to_host, { { S->d_fir_state, v->fir_state, C * 2 * nh1 * sizeof(float) }, { S->d_int_state, v->interp_state, C * 2 * p1 * sizeof(float) },
                                   { S->d_gain, v->alc_gain, C * sizeof(float) }, { S->d_phase, v->nco_phase, C * sizeof(uint32_t) } });
}

static void process_host(selenite_tx_instance *S, const void *src, void *dst, uint32_t bs, bool q15, const char *who)
{
    if (!block_size_ok(S, bs, who)) return;
    const size_t nin = (size_t)S->cfg.channels * bs * sample_bytes(q15), nout = nin * S->cfg.interp * 2;
    (void)staged_call(S, { { src, nin, kToDevice, &S->d_io_in, &S->io_in_bytes }, { dst, nout, kToHost, &S->d_io_out, &S->io_out_bytes } },
                      [&] { return run(S, S->d_io_in, S->d_io_out, q15, bs); });
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_tx_init(selenite_tx_instance **out, const selenite_tx_config *caller_cfg)
{
    if (!out) return SELENITE_RX_ARGUMENT_ERROR;
    *out = nullptr;
    if (!caller_cfg) return SELENITE_RX_ARGUMENT_ERROR;
    // struct_size says which header the caller was built against (include/selenite_rx.h: ABI versions); version 1 ends with alc_gain_init
    static_assert(offsetof(selenite_tx_config, q15_rounding) == 92 && sizeof(selenite_tx_config) == 104, "selenite_tx_config layout (LP64)");
    selenite_tx_config own{};
    if (caller_cfg->struct_size == SELENITE_TX_CONFIG_SIZE_V1) {
        std::memcpy(&own, caller_cfg, offsetof(selenite_tx_config, q15_rounding));
        own.abi_version = 1;
    } else if (caller_cfg->struct_size == sizeof(selenite_tx_config)) {
        own = *caller_cfg;
        if (own.abi_version != SELENITE_RX_ABI_VERSION || own.reserved != 0) return SELENITE_RX_ARGUMENT_ERROR;
    } else {
        return SELENITE_RX_ARGUMENT_ERROR;
    }
    own.struct_size = (uint32_t)sizeof(selenite_tx_config);
    const selenite_tx_config *g = &own;
    if (g->q15_rounding > 1u || !g->channels || !g->block || !g->interp || !tx_mode_ok(g->mode) ||
        g->arith > SELENITE_ARITH_SPLIT16)
        return SELENITE_RX_ARGUMENT_ERROR;
    if ((g->interp > 1) != (g->ni_taps > 0)) return SELENITE_RX_ARGUMENT_ERROR;
    if (g->ni_taps && !g->interp_coeffs) return SELENITE_RX_ARGUMENT_ERROR;
    if (g->nh_taps && (!g->hilb_coeffs || !g->delay_coeffs)) return SELENITE_RX_ARGUMENT_ERROR;
    if (g->ni_taps % g->interp) return SELENITE_RX_LENGTH_ERROR;        // arm_fir_interpolate_init_f32.c:91-96
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return SELENITE_RX_DEVICE_ERROR;   // no CPU fallback
    selenite_tx_instance *S = new selenite_tx_instance;
    S->cfg = *g;
    S->cfg.interp_coeffs = S->cfg.hilb_coeffs = S->cfg.delay_coeffs = nullptr;
    S->cfg.nco_step = nullptr;
    auto bail = [&](int code) { selenite_tx_free(S); return code; };
    if (hipGetDevice(&S->device) != hipSuccess) return bail(SELENITE_RX_DEVICE_ERROR);
    if (hipStreamCreateWithFlags(&S->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(SELENITE_RX_DEVICE_ERROR);
    S->stream = S->own_stream;
    const size_t C = g->channels, nh1 = g->nh_taps ? g->nh_taps - 1 : 0, p1 = g->ni_taps ? g->ni_taps / g->interp - 1 : 0;
    TxSelPlan &sel = S->sel;
    S->h_step.resize(C);
    for (size_t c = 0; c < C; ++c) S->h_step[c] = g->nco_step ? g->nco_step[c] : g->nco_step_all;
    sel.step0 = S->h_step[0];
    for (size_t c = 1; c < C; ++c) sel.steps_same = sel.steps_same && S->h_step[c] == sel.step0;
    // what tx_fused.hip relies on: a unit-impulse delay FIR and a type-III Hilbert, classified as on the RX side
    const TapClass t = classify_taps(g->delay_coeffs, g->hilb_coeffs, g->nh_taps);
    sel.delay_is_impulse = t.delay_is_impulse; sel.hilb_odd_only = t.hilb_odd_only;
    if (t.delay_is_impulse) S->delay_index = (uint32_t)t.delay_index;
    // kernel-selection overrides of the tests (selenite_rx_set_plan_option)
    sel.force_generic = plan_option(SELENITE_RX_OPT_TX_FORCE_GENERIC) != 0;
    sel.no_periodic_lo = plan_option(SELENITE_RX_OPT_NO_PERIODIC_LO) != 0;
    if (tx_wants_table(*g, sel)) {
        if (build_tx_split16_table(g->interp_coeffs, &S->d_ttab16, &S->tpost) != hipSuccess) return bail(SELENITE_RX_DEVICE_ERROR);
        sel.table = true;
    }
    if (dev_upload(&S->d_ic, g->interp_coeffs, (size_t)g->ni_taps) || dev_upload(&S->d_hc, g->hilb_coeffs, (size_t)g->nh_taps) ||
        dev_upload(&S->d_dc, g->delay_coeffs, (size_t)g->nh_taps) || dev_upload(&S->d_sintab, host_sin_table(), (size_t)513) ||
        dev_upload(&S->d_step, (const uint32_t *)S->h_step.data(), C) || dev_alloc(&S->d_phase, C) ||
        dev_alloc(&S->d_fir_state, C * 2 * nh1) || dev_alloc(&S->d_int_state, C * 2 * p1) || dev_alloc(&S->d_gain, C))
        return bail(SELENITE_RX_DEVICE_ERROR);
    if (reset_state(S)) return bail(SELENITE_RX_DEVICE_ERROR);
    *out = S;
    return SELENITE_RX_SUCCESS;
}

extern "C" void selenite_tx_free(selenite_tx_instance *S)
{
    if (!S) return;
    tx_fm_free(S); tx_cw_free(S); tx_in_free(S); tx_keyer_free(S);
    dev_free(S->d_ic, S->d_hc, S->d_dc, S->d_sintab, S->d_step, S->d_phase, S->d_fir_state, S->d_int_state, S->d_gain, S->d_io_in, S->d_io_out,
             S->d_lo, S->d_ttab16);
    if (S->own_stream) (void)hipStreamDestroy(S->own_stream);
    delete S;
}

extern "C" int selenite_tx_set_mode(selenite_tx_instance *S, uint8_t mode)
{
    // instance stays usable in its old mode; FM exists once selenite_tx_set_fm has configured it
    if (!S || !(tx_mode_ok(mode) || (mode == SELENITE_MODE_FM && S->fm.set))) return SELENITE_RX_ARGUMENT_ERROR;
    S->cfg.mode = mode;
    return SELENITE_RX_SUCCESS;
}

extern "C" const char *selenite_tx_kernel_name(const selenite_tx_instance *S)
{
    return S ? tx_kernel_name(tx_select(S->cfg, S->sel, tx_whole_pass_call())) : "";
}

extern "C" int selenite_tx_status(const selenite_tx_instance *S) { return S ? S->status : SELENITE_RX_ARGUMENT_ERROR; }
extern "C" const char *selenite_tx_error_string(const selenite_tx_instance *S) { return S ? S->err.c_str() : "null instance"; }

extern "C" void selenite_tx_process_f32(selenite_tx_instance *S, const float *src, float *dst, uint32_t bs) { process_host(S, src, dst, bs, false, "selenite_tx_process_f32"); }
extern "C" void selenite_tx_process_q15(selenite_tx_instance *S, const int16_t *src, int16_t *dst, uint32_t bs) { process_host(S, src, dst, bs, true, "selenite_tx_process_q15"); }
extern "C" void selenite_tx_process_f32_device(selenite_tx_instance *S, const float *src, float *dst, uint32_t bs) { if (block_size_ok(S, bs, "selenite_tx_process_f32_device")) run(S, src, dst, false, bs); }
extern "C" void selenite_tx_process_q15_device(selenite_tx_instance *S, const int16_t *src, int16_t *dst, uint32_t bs) { if (block_size_ok(S, bs, "selenite_tx_process_q15_device")) run(S, src, dst, true, bs); }

extern "C" int selenite_tx_set_stream(selenite_tx_instance *S, void *hip_stream)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : S->own_stream;
    if (next != S->stream) {                                // the streaming state is shared: drain the old stream first
        HIPCHK(S, hipStreamSynchronize(S->stream));
        S->stream = next;
    }
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_tx_sync(selenite_tx_instance *S)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    HIPCHK(S, hipStreamSynchronize(S->stream));
    return S->status;
}

extern "C" int selenite_tx_get_state(selenite_tx_instance *S, const selenite_tx_state_view *v) { return S && v ? state_copy(S, v, true) : SELENITE_RX_ARGUMENT_ERROR; }

extern "C" int selenite_tx_set_state(selenite_tx_instance *S, const selenite_tx_state_view *v)
{
    if (!S || !v) return SELENITE_RX_ARGUMENT_ERROR;
    if (int rc = state_copy(S, v, false)) return rc;
    if (v->nco_phase) {
        bool same = S->sel.steps_same;
        for (size_t c = 1; c < S->cfg.channels; ++c) same = same && v->nco_phase[c] == v->nco_phase[0];
        S->phase_uniform = same;
        S->phase_host = v->nco_phase[0];
    }
    return 0;
}

extern "C" int selenite_tx_reset(selenite_tx_instance *S) { return S ? reset_state(S) : SELENITE_RX_ARGUMENT_ERROR; }

extern "C" int selenite_tx_time_process_device(selenite_tx_instance *S, const float *src, float *dst, uint32_t bs,
                                               uint32_t iters, float *ms_per_call)
{
    if (!S || !ms_per_call || iters == 0) return SELENITE_RX_ARGUMENT_ERROR;
    if (!block_size_ok(S, bs, "selenite_tx_time_process_device")) return S->status;
    return timed_loop(S, iters, ms_per_call, [&] { return run(S, src, dst, false, bs) ? S->status : 0; });
}
