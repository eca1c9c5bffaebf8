// rx_dispatch.hip -- the one dispatcher behind every process entry point: which kernels serve a call, over which channels
// (ChanRange), from which stream positions (CallStart).  Two host-side functions decide, the launchers here execute: select() (rx_select.h)
// names the kernel of a launch, route() (rx_route.h) its way through the stages -- which of them run, on which buffer, what finishes it.
// The ten stages hook in here and nowhere else:
//   run_front        the spectrum tap, the I/Q correction and the noise blanker in front of the chain;
//   run_part         the tone detector, the Morse decoder, the FSK decoder, the audio filter, NLMS and the level meter in front of the AGC, the meter's gate behind it;
//   with_out_stage   the output stage behind the chain.
// A new stage in front of the AGC is one line in the route (its flag in StagesOn: it then counts in `unscaled`, and in what select() is told)
// and one in the executor (its launch in run_part, at its place among the others); one in front of the chain is one line in run_front.
#include "rx_host.h"

#include <dlfcn.h>

using namespace srx;

// the stages in front of the AGC this instance has switched on
static StagesOn stages_on(const selenite_rx_instance *S)
{
    StagesOn on;
    on.tones = S->tones.on; on.afilt = S->afilt.on; on.nr = S->nr.kind != SELENITE_RX_NR_OFF; on.meter = S->meter.on;
    on.cwdec = S->cwdec.on; on.fskdec = S->fskdec.on;
    return on;
}

// the facts select() (rx_select.h) wants of a call of block_size samples on this instance
static SelCall call_facts(const selenite_rx_instance *S, uint32_t block_size, bool q15)
{
    SelCall c;
    c.block_size = block_size; c.q15 = q15;
    c.global_gain = S->cfg.agc_enable && S->cfg.agc_global;
    c.unscaled_stage = stages_on(S).any();
    c.hist_ext = S->handover_repair && S->d_hist_ext;
    c.steps_uniform = S->steps_uniform; c.phase_uniform = S->phase_uniform; c.steps_grid256 = S->steps_grid256;
    c.no_shared_lo = S->no_shared_lo; c.no_periodic_lo = S->no_periodic_lo;
    c.auto_launches = S->auto_launches; c.rerun_words = S->d_rerun_flag != nullptr;
    return c;
}

// the LO fields of the decision, in words (the call length does not move them)
extern "C" const char *selenite_rx_nco_path(const selenite_rx_instance *S)
{
    if (!S) return "";
    if (!S->cfg.nco_enable) return "off";
    const bool ssb = on_ssb_fused(S);
    if (!ssb && (S->force_generic || !cw_fused_ok(S->cfg, S->cfg.block))) return "per-channel arm_sin/cos_f32 in the kernel";
    const Decision d = select(S->cfg, ssb ? S->plan.sel : SelPlan{}, call_facts(S, S->cfg.block, false));
    if (d.nco_rx == 2) return d.lo_period ? "shared LO, period 256 samples, held in registers" : "shared LO table per call";
    return d.lo_period ? "per-channel LO, period 256 samples (arm_sin/cos_f32 once per channel and call), held in registers"
                       : "per-channel arm_sin/cos_f32 in the kernel";
}

// SELENITE_ARITH_AUTO on a shape with a split-precision decimator: the rows k_ssb_split16 leaves for k_hist_exact, allocated by the
// first call that can use them
static int ensure_hist_ext(selenite_rx_instance *S)
{
    if (S->d_hist_ext || !S->ext_len || !S->handover_repair || !S->d_rerun_flag) return SELENITE_RX_SUCCESS;
    const size_t n = 2 * (size_t)S->cfg.channels * S->ext_len;
    HIPCHK(S, hipMalloc((void **)&S->d_hist_ext, n * sizeof(float2)));
    HIPCHK(S, hipMemsetAsync(S->d_hist_ext, 0, n * sizeof(float2), S->stream));
    return SELENITE_RX_SUCCESS;
}

// ------------------------------------------------------------------------------------------
RxParams srx::make_params(selenite_rx_instance *S, ChanRange r, uint32_t block_size)
{
    const selenite_rx_config &g = S->cfg;
    RxParams p{};
    p.channels = r.count; p.block = g.block; p.decim = g.decim;
    p.nd = g.nd_taps; p.nh = g.nh_taps; p.nbiq = g.n_biquad; p.mode = g.mode; p.q15_round = g.q15_rounding ? 1u : 0u;
    p.nco = g.nco_enable ? 1 : 0; p.agc = g.agc_enable ? 1 : 0;
    p.block_size = block_size; p.nout = block_size / g.decim;
    p.in_stride = p.block_size; p.out_stride = p.nout;
    p.dec_c = S->d_dec_c; p.hilb_c = S->d_hilb_c; p.delay_c = S->d_delay_c; p.biq_c = S->d_biq_c;
    p.sintab = S->d_sintab; p.step = S->d_step; p.phase = S->d_phase;
    p.dec_state = S->d_dec_state; p.fir_state = S->d_fir_state; p.biq_state = S->d_biq_state;
    p.gain = S->d_gain;
    p.flags = S->d_flags;
    p.guard_ratio = S->guard_ratio;
    p.guard_ch = S->d_guard_ch;
    p.guard_calls = S->d_guard_ch + g.channels;
    p.guard_hand = S->d_guard_ch + 2 * (size_t)g.channels;
    p.hist_ext = S->handover_repair ? S->d_hist_ext : nullptr; p.ext_len = S->ext_len; p.ext_buf_stride = (size_t)g.channels * S->ext_len;
    const size_t c0 = r.first;                              // every per-channel array moves with the range
    p.step += c0; p.phase += c0; p.gain += c0; p.guard_ch += c0; p.guard_calls += c0; p.guard_hand += c0;
    if (p.hist_ext) p.hist_ext += c0 * p.ext_len;
    if (p.dec_state) p.dec_state += c0 * 2 * (g.nd_taps - 1);
    if (p.fir_state) p.fir_state += c0 * 2 * (g.nh_taps - 1);
    if (p.biq_state) p.biq_state += c0 * 4 * g.n_biquad;
    p.agcp = AgcParams{ g.agc_target, g.agc_attack, g.agc_decay, g.agc_gain_min, g.agc_gain_max, g.agc_env_floor };
    // generic front kernel: largest pass (<= 256 outputs) whose LDS image fits 64 KiB
    uint32_t P = 256;
    for (;;) {
        p.pass_out = P;
        if (front_generic_lds_bytes(p) <= 64 * 1024 || P == 1) break;
        P >>= 1;
    }
    return p;
}

bool srx::block_size_ok(selenite_rx_instance *S, uint32_t block_size, const char *who)
{
    if (block_size == 0 || block_size % S->cfg.block != 0) {
        fail(S, SELENITE_RX_LENGTH_ERROR, std::string(who) + ": blockSize is not a non-zero multiple of cfg.block");
        return false;
    }
    return true;
}

// Where a launch sits in its call: the samples of the call in front of it, and the whole call's length (what the caller's rows are apart).
// An uncut call is the part { 0, block_size }.
struct CallPart { uint32_t offset, total; };

// what route() (rx_route.h) wants of a launch on this instance
static RouteFacts route_facts(const selenite_rx_instance *S, Phase phase, bool src_q15, bool dst_q15, bool cw_kernel)
{
    const selenite_rx_config &g = S->cfg;
    RouteFacts f;
    f.phase = phase; f.src_q15 = src_q15; f.dst_q15 = dst_q15;
    f.agc_enable = g.agc_enable; f.global = g.agc_enable && g.agc_global;
    f.on = stages_on(S); f.gate = S->meter.on && S->meter.gate;
    f.force_generic = S->force_generic; f.ssb_kernels = on_ssb_fused(S); f.cw_kernel = cw_kernel;
    f.cw_biquads = mode_is_cw(g.mode) && g.n_biquad; f.words = S->d_rerun_flag != nullptr;
    return f;
}

// The one executor behind every process entry point: one launch of block_size samples, the part `at` of a call whose buffers are src and
// dst and whose first sample has the common NCO phase phase0.  d: select() for this launch; the route is decided here, once, and run top to
// bottom.
static int run_part(selenite_rx_instance *S, ChanRange r, const Decision &d, CallPart at, uint32_t phase0, const void *src, bool src_q15, void *dst, bool dst_q15,
                    uint32_t block_size, Phase phase, float *ext_env)
{
    const selenite_rx_config &g = S->cfg;
    HIPCHK(S, hipSetDevice(S->device));
    RxParams p = make_params(S, r, block_size);
    // both buffers are addressed with the whole call's per-channel stride, from this part's first sample
    p.in_stride = at.total; p.out_stride = at.total / g.decim;
    src = static_cast<const char *>(src) + (size_t)at.offset * 2 * (src_q15 ? sizeof(int16_t) : sizeof(float));
    dst = static_cast<char *>(dst) + (size_t)(at.offset / g.decim) * (dst_q15 ? sizeof(int16_t) : sizeof(float));
    const uint32_t phase_now = phase0 + at.offset * S->h_step[0];
    if (front_generic_lds_bytes(p) > 64 * 1024 && !on_ssb_fused(S))
        return fail(S, SELENITE_RX_LENGTH_ERROR, "filter lengths exceed the LDS budget of the generic kernel");
    const int arith = (int)g.arith;
    const int garith = arith == SELENITE_ARITH_AUTO ? SELENITE_ARITH_CMSIS : arith;      // the generic kernels: AUTO is bit-exact there
    hipStream_t st = S->stream;
    // (the fused CW kernel: not with wider strides, which the generic kernels take)
    const bool cw_kernel = phase != kPhase2 && !S->force_generic && cw_fused_ok(g, block_size) && cw_strides_ok(p.in_stride, p.out_stride);
    const Route t = route(route_facts(S, phase, src_q15, dst_q15, cw_kernel));

    // Un-scaled audio (Route::unscaled): the fused kernels serve such a launch with their own AGC off, and the stages, the envelope
    // reduction and the gain pass below finish it.  They convert in and out symmetrically, and the audio between them and the tail is f32:
    // int16 input is converted once, up front -- arm_q15_to_float over the whole buffer, the very operation the fused int16 load performs
    // -- and the launch runs as an f32-input call whose gain pass stores int16.  (f32 in, int16 out -- behind the I/Q correction, whose
    // copy is f32 -- the same way: into the f32 scratch, k_agc_generic applies the AGC and stores int16.)
    if (t.convert_in) {
        // int16 values of the call (block_size % 4 == 0 for every fused shape), up to the end of the last channel's block_size samples: the
        // second part of a cut call starts inside the rows (= p.channels * p.in_stride * 2 when the call is not cut)
        const size_t nval = ((size_t)(p.channels - 1) * p.in_stride + block_size) * 2;
        if (nval % 8 == 0) {
            int rc = ensure(S, (void **)&S->d_conv_in, &S->conv_in_bytes, nval * sizeof(float));
            if (rc) return rc;
            HIPCHK(S, launch_q15_to_f32(static_cast<const int16_t *>(src), S->d_conv_in, nval, S->stream));
            src = S->d_conv_in;
            src_q15 = false;
        }
    }
    float *audio = (float *)dst;      // un-scaled audio: dst itself when dst is f32, else scratch
    if (t.audio_in_scratch) {
        const size_t need = (size_t)g.channels * p.out_stride * sizeof(float);
        int rc = ensure(S, (void **)&S->d_scratch, &S->scratch_bytes, need);
        if (rc) return rc;
        audio = S->d_scratch;
    }
    // step 4c: the gate bytes of this launch, [cfg.channels][blocks], indexed by absolute channel; phase 2 reads the ones its phase 1 left
    MeterParams mq{};
    if (t.run.meter || t.gate) {
        const size_t need = (size_t)g.channels * (block_size / g.block);
        if (t.run.meter) {
            int rc = ensure(S, (void **)&S->meter.d_bits, &S->meter.bits_bytes, need);
            if (rc) return rc;
        } else if (S->meter.bits_bytes < need) {
            return fail(S, SELENITE_RX_ARGUMENT_ERROR, "global phase 2: no phase 1 of this length has left the squelch gate of its blocks");
        }
        mq = S->meter.params(r, p);
    }
    // (SELENITE_ARITH_AUTO outside the SSB fused kernels -- CW, generic: every channel's state stays in exact arithmetic, and the
    // provenance words k_ssb_split16 reads at its next call say so)
    // (a channel the matrix kernel left with its samples gets its Hilbert-pair history recomputed in exact arithmetic first: the
    // generic / CW kernels read it -- advisor finding, round 3)
    if (t.clear_words) {
        uint32_t *words = S->d_rerun_flag + r.first;
        if (p.hist_ext) {
            RxParams ph = p;
            ph.chan_flags = words;
            HIPCHK(S, launch_hist_exact(ph, true, st));
        }
        HIPCHK(S, hipMemsetAsync(words, 0, p.channels * sizeof(uint32_t), st));
    }
    bool env_emitted = false;      // global gain: the fused kernel wrote the per-channel block maxima
    if (t.fused) {
        RxParams pf = p;
        pf.nco = d.nco_rx; pf.lo_period = d.lo_period;
        if (d.lo_n) {
            // one LO for all channels: computed once per call, read from L2 by every wavefront
            // the table is a pure function of (start phase, step, length): a call that starts where the table in d_lo
            // starts reuses it -- every chunk of a pipelined host call, and EVERY call when the phase advance of a call
            // is a multiple of 2^32 (an LO on the fs / 256 grid with calls of whole DSP blocks)
            if (!(S->lo_valid && S->lo_phase == phase_now && S->lo_step == S->h_step[0] && S->lo_n >= d.lo_n)) {
                S->lo_valid = false;
                int rc = ensure(S, (void **)&S->d_lo, &S->lo_bytes, (size_t)d.lo_n * sizeof(float2));
                if (rc) return rc;
                HIPCHK(S, launch_lo_table(S->d_lo, S->d_sintab, phase_now, S->h_step[0], d.lo_n, st));
                S->lo_valid = true; S->lo_phase = phase_now; S->lo_step = S->h_step[0]; S->lo_n = d.lo_n;
            }
            pf.lo = S->d_lo;
        }
        if (arith == SELENITE_ARITH_AUTO && t.ssb_fused) {
            // the split16 kernel raises the rerun flag of the channels it guards and leaves their state alone; the bit-exact
            // kernel then recomputes the flagged channels (launch_fused)
            pf.rerun_flag = S->d_rerun_flag + r.first;
            pf.chan_list = S->d_rerun_list + 2;
            pf.chan_count = S->d_rerun_list;              // the two counters; launch_fused picks by *rerun_par_host where it launches the prepare kernel
            pf.rerun_par_host = &S->rerun_par;
            pf.rerun_seen = S->h_rerun_seen;
            pf.auto_inline = S->auto_launches == 1 ? 1u : 0u;
            pf.form_host = &S->auto_form_last;
        }
        void *fdst = dst;
        bool fq15 = dst_q15;
        if (t.fused_agc_off) {
            pf.agc = 0; fdst = audio; fq15 = false;
            pf.out_cached = 1;                            // phase 2 (and, without block maxima from the kernel, the envelope fold) reads this audio back
            if (d.env_part) {                             // the kernel leaves the block maxima of every channel behind: folded below
                const size_t need = sizeof(float) * env_fold_scratch_floats(p.channels, block_size / g.block);
                int rc = ensure(S, (void **)&S->d_env_part, &S->env_part_cap, need);
                if (rc) return rc;
                pf.env_part = S->d_env_part;
                env_emitted = true;
            }
        }
        if (t.ssb_fused) HIPCHK(S, launch_fused(S->plan, pf, d, src, src_q15, fdst, fq15, S->delay_index, st));
        else HIPCHK(S, launch_cw_fused(pf, src, src_q15, fdst, fq15, st));
        if (t.done_after_fused) return SELENITE_RX_SUCCESS;
    }

    // generic path: front -> [biquad] -> AGC / convert
    if (t.generic_front) HIPCHK(S, launch_front_generic(p, garith, src, src_q15, audio, st));
    if (t.biquad) HIPCHK(S, launch_biquad_generic(p, garith, audio, st));
    // step 4-t: the tone detector reads the un-scaled audio of this launch.  Its frames are counted in DSP blocks of the stream: the second
    // part of a cut call starts behind the blocks of the first
    if (t.run.tones) HIPCHK(S, launch_tones(S->tones.params(r, p, at.offset / g.block), audio, st));
    // step 4-d: the Morse decoder reads the same audio, one tick per DSP block of this launch
    if (t.run.cwdec) HIPCHK(S, launch_cwdec(S->cwdec.params(r, p), audio, st));
    // step 4-r: the FSK decoder reads the same audio, n / T ticks per DSP block of this launch
    if (t.run.fskdec) HIPCHK(S, launch_fskdec(S->fskdec.params(r, p), audio, st));
    // step 4a: the audio filter in place on the un-scaled audio of this launch (a part of a cut call: its dst offset, the full stride)
    if (t.run.afilt) HIPCHK(S, launch_afilt(S->afilt.params(r, p), audio, st));
    // step 4b: NLMS in place on the un-scaled audio (phase 1 of a global gain: before the envelope)
    if (t.run.nr) HIPCHK(S, launch_nlms(S->nr.params(r, p), S->nr.taps, audio, st));
    // step 4c: the level meter reads the same audio and leaves the gate of every block of this launch
    if (t.run.meter) HIPCHK(S, launch_meter(mq, audio, st));
    if (t.env || t.apply) {
        float *env = ext_env;
        if (!env) {
            const size_t need = sizeof(float) * (block_size / g.block);
            int rc = ensure(S, (void **)&S->d_env, &S->env_cap, need);
            if (rc) return rc;
            env = S->d_env;
        }
        if (t.env) {
            if (env_emitted) {
                HIPCHK(S, launch_env_fold(S->d_env_part, env, p.channels, block_size / g.block, st));
            } else {
                const size_t need = sizeof(float) * env_global_rows(p) * (block_size / g.block);
                int rc = ensure(S, (void **)&S->d_env_part, &S->env_part_cap, need);
                if (rc) return rc;
                HIPCHK(S, launch_env_global(p, audio, S->d_env_part, env, st));
            }
        }
        if (t.apply) HIPCHK(S, launch_agc_apply_global(p, garith, audio, env, dst, dst_q15, st));
    }
    if (t.agc_generic) HIPCHK(S, launch_agc_generic(p, garith, audio, dst, dst_q15, st));
    // the gate, behind the AGC: zeros over the closed blocks of whatever this launch's dst is (with an output stage: its input)
    if (t.gate) HIPCHK(S, launch_gate(mq, dst, dst_q15, st));
    return SELENITE_RX_SUCCESS;
}

// Entry of every process call: decides once which kernel serves it (rx_select.h) and runs that.  A split-precision call that ends in a
// partial pass too short for the matrix kernel is cut in two launches on the same streaming state, each decided as a call of its own and
// told where it sits in the call (CallPart).  The tail is shorter than a pass, which k_ssb_split16
// takes: under SELENITE_ARITH_SPLIT16 it runs there; under SELENITE_ARITH_AUTO it is too short to leave the repair rows behind and runs
// on the bit-exact k_ssb_fused, from a history k_hist_exact repairs first.
static int run_chain_core(selenite_rx_instance *S, ChanRange r, uint32_t phase0, const void *src, bool src_q15, void *dst, bool dst_q15,
                          uint32_t block_size, Phase phase, float *ext_env)
{
    const selenite_rx_config &g = S->cfg;
    const bool ssb = phase != kPhase2 && on_ssb_fused(S);
    if (ssb && S->plan.sel.btab16)
        if (int rc = ensure_hist_ext(S)) return rc;
    SelCall c = call_facts(S, block_size, src_q15 && dst_q15);      // (f32 in, int16 out -- behind the I/Q correction -- is decided as the f32 call it runs as)
    const Decision d = select(g, ssb ? S->plan.sel : SelPlan{}, c);
    if (!d.first) return run_part(S, r, d, CallPart{ 0u, block_size }, phase0, src, src_q15, dst, dst_q15, block_size, phase, ext_env);
    if (int rc = run_part(S, r, d, CallPart{ 0u, block_size }, phase0, src, src_q15, dst, dst_q15, d.first, kAll, nullptr)) return rc;
    c.block_size = block_size - d.first;
    return run_part(S, r, select(g, S->plan.sel, c), CallPart{ d.first, block_size }, phase0, src, src_q15, dst, dst_q15, c.block_size, kAll, nullptr);
}

// The taps and copies in front of the chain, in this order on the stream: the spectrum tap reads the caller's own input, the I/Q
// correction (step 0b2) writes a corrected f32 copy of it, the noise blanker (step 0c) a blanked copy of that; from here on the call reads
// *src, in the format *src_q15 says.  A new stage in front of the chain is one line here.
static int run_front(selenite_rx_instance *S, ChanRange r, uint64_t spec_pos, const void **src, bool *src_q15, uint32_t block_size)
{
    if (S->spec.len)
        if (int rc = S->spec.run(S, r, spec_pos, *src, *src_q15, block_size)) return rc;
    if (S->iqc.frame) {
        if (int rc = S->iqc.run(S, r, *src, *src_q15, block_size, src)) return rc;
        *src_q15 = false;
    }
    if (S->nb.frame)
        if (int rc = S->nb.run(S, r, *src, *src_q15, block_size, src)) return rc;
    return SELENITE_RX_SUCCESS;
}

// The output stage's side of a call, around `chain(src, src_q15, dst, dst_q15)`.  Without a stage that is the chain on the caller's dst.
// With one the chain runs exactly as without, into the instance's f32 audio buffer, and the stage kernel writes the caller's dst.
// int16 slots: the fused kernels convert in and out symmetrically, so the input is converted up front (arm_q15_to_float over the whole
// buffer, the operation the fused int16 load performs) and the call runs as an f32 call whose stage stores int16.
template <typename Chain>
static int with_out_stage(selenite_rx_instance *S, ChanRange r, const void *src, bool src_q15, void *dst, bool dst_q15, uint32_t block_size, Chain chain)
{
    if (!S->out.on) return chain(src, src_q15, dst, dst_q15);
    HIPCHK(S, hipSetDevice(S->device));
    float *audio = nullptr;
    if (int rc = S->out.audio_buffer(S, r, block_size, &audio)) return rc;
    if (src_q15) {
        const size_t nval = (size_t)r.count * block_size * 2;
        if (int rc = ensure(S, (void **)&S->d_conv_in, &S->conv_in_bytes, nval * sizeof(float))) return rc;
        HIPCHK(S, launch_q15_to_f32(static_cast<const int16_t *>(src), S->d_conv_in, nval, S->stream));
        src = S->d_conv_in;
    }
    if (int rc = chain(src, false, audio, false)) return rc;
    return S->out.run(S, r, audio, dst, dst_q15, block_size);
}

int srx::run_chain(selenite_rx_instance *S, ChanRange r, CallStart at, const void *src, bool src_q15, void *dst, bool dst_q15,
                   uint32_t block_size, Phase phase, float *ext_env)
{
    // an invariant, checked before anything is launched: both split entry points (rx_api.hip) refuse such an instance themselves, with
    // their own message, so no C-ABI call gets here
    if (S->out.on && phase != kAll) return fail(S, SELENITE_RX_ARGUMENT_ERROR, "the split global-gain calls exchange audio at the decimated rate: not with an output stage");
    if (phase != kPhase2)
        if (int rc = run_front(S, r, at.spec_pos, &src, &src_q15, block_size)) return rc;
    return with_out_stage(S, r, src, src_q15, dst, dst_q15, block_size, [&](const void *in, bool in_q15, void *out, bool out_q15) {
        return run_chain_core(S, r, at.phase, in, in_q15, out, out_q15, block_size, phase, ext_env);
    });
}

// global_phase2 advances nothing (its phase 1 did); the NCO phase moves only when the NCO runs
void srx::advance_streams(selenite_rx_instance *S, uint32_t block_size, Phase phase)
{
    if (phase == kPhase2) return;
    if (S->cfg.nco_enable) S->phase_host += block_size * S->h_step[0];
    if (S->spec.len) S->spec.pos += block_size;
    if (S->tones.on) S->tones.pos += block_size / S->cfg.block;
}

int srx::run_call(selenite_rx_instance *S, const void *src, bool src_q15, void *dst, bool dst_q15, uint32_t block_size, Phase phase, float *ext_env)
{
    if (int rc = run_chain(S, all_channels(S), call_start(S), src, src_q15, dst, dst_q15, block_size, phase, ext_env)) return rc;
    advance_streams(S, block_size, phase);
    return SELENITE_RX_SUCCESS;
}

// ---- global-gain call with the exchange done HERE, for a plain C host: phase 1, ncclAllReduce(MAX) of the
// per-block envelopes over RCCL / xGMI, phase 2 -- all on the instance's stream.  RCCL is bound at run time
// (the process's already loaded librccl -- e.g. the one torch ships -- or librccl.so.1), so the library carries no
// link-time dependency on it and a host that never uses global gain never loads it.
typedef int (*nccl_allreduce_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
static nccl_allreduce_fn rccl_allreduce()
{
    static nccl_allreduce_fn fn = [] {
        void *sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
        if (!sym) {
            void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (h) sym = dlsym(h, "ncclAllReduce");
        }
        return reinterpret_cast<nccl_allreduce_fn>(sym);
    }();
    return fn;
}

extern "C" int selenite_rx_global_process_f32_device(selenite_rx_instance *S, const float *dSrcIQ, float *dDstAudio,
                                                     uint32_t blockSize, void *rccl_comm)
{
    if (!S || !block_size_ok(S, blockSize, "selenite_rx_global_process_f32_device")) return S ? S->status : SELENITE_RX_ARGUMENT_ERROR;
    if (!(S->cfg.agc_enable && S->cfg.agc_global))
        return fail(S, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_global_process_f32_device: instance is not agc_global");
    const size_t nblk = blockSize / S->cfg.block;
    int rc = ensure(S, (void **)&S->d_env, &S->env_cap, sizeof(float) * nblk);
    if (rc) return rc;
    // (an output stage sits behind phase 2: both phases work on the instance's audio buffer, the stage writes dDstAudio)
    const ChanRange r = all_channels(S);
    const CallStart at = call_start(S);
    const void *in = dSrcIQ;
    bool in_q15 = false;
    if ((rc = run_front(S, r, at.spec_pos, &in, &in_q15, blockSize))) return rc;
    rc = with_out_stage(S, r, in, in_q15, dDstAudio, false, blockSize, [&](const void *src, bool, void *audio, bool) {
        if (int e = run_chain_core(S, r, at.phase, src, false, audio, false, blockSize, kPhase1, S->d_env)) return e;
        if (rccl_comm) {                                    // NULL: single rank, nothing to exchange
            nccl_allreduce_fn ar = rccl_allreduce();
            if (!ar) return fail(S, SELENITE_RX_DEVICE_ERROR, "selenite_rx_global_process_f32_device: RCCL (ncclAllReduce) is not available");
            const int nccl_float = 7, nccl_max = 2;         // ncclFloat32, ncclMax (rccl.h)
            const int e = ar(S->d_env, S->d_env, nblk, nccl_float, nccl_max, rccl_comm, S->stream);
            if (e != 0) return fail(S, SELENITE_RX_DEVICE_ERROR, "selenite_rx_global_process_f32_device: ncclAllReduce failed (" + std::to_string(e) + ")");
        }
        return run_chain_core(S, r, at.phase, nullptr, false, audio, false, blockSize, kPhase2, S->d_env);
    });
    if (rc) return rc;
    advance_streams(S, blockSize, kAll);
    return SELENITE_RX_SUCCESS;
}
