/*
 * selenite_rx.h -- C-ABI of the MI355X-native Selenite Lite RX DSP block path.
 *
 * Drop-in boundary.  Every entry point mirrors the CMSIS-DSP
 * "instance / init / process(S, pSrc, pDst, blockSize)" convention that the
 * reference vendors (Drivers/CMSIS/DSP/Include/arm_math.h:1175-1195 arm_fir_f32,
 * :1326-1344 arm_biquad_cascade_df1_f32, :3288-3312 arm_fir_decimate_f32) and sits
 * in the per-block callback slot of the firmware
 * (Core/Src/dsp_if.c:50-54,63-67 HAL_I2SEx_TxRx{Half,}CpltCallback, between the
 * int16 I/Q that DSP_In_Buff_Write (dsp_if.c:250-301) receives and the int16
 * audio DSP_Out_Buff_Read (dsp_if.c:204-219) hands back).
 *
 * Plain C: pointers and sizes only, no C++/torch types.  The library behind it
 * (libselenite_rx.so) is hand-written HIP for gfx950; there is NO CPU fallback:
 * selenite_rx_init() fails with SELENITE_RX_DEVICE_ERROR when no HIP device is
 * usable.
 *
 * Data layout (device and host views are the same):
 *   pSrcIQ    float  [channels][blockSize][2]   I,Q adjacent  (dsp_if.c:286-289 interleave)
 *   pDstAudio float  [channels][blockSize/decim]
 *   q15 variants: int16_t with the same shapes (arm_q15_to_float / arm_float_to_q15
 *   semantics, SupportFunctions/arm_q15_to_float.c:65-113, arm_float_to_q15.c:64-122).
 *
 * The chain that runs per channel and per DSP block is specified in DESIGN.md
 * ("Chain specification"); every step is one CMSIS-DSP primitive:
 *   NCO (arm_sin_f32/arm_cos_f32 + arm_cmplx_mult_cmplx_f32)
 *   -> arm_fir_decimate_f32 on the I and the Q rail
 *   -> arm_fir_f32 (delay taps) on I, arm_fir_f32 (Hilbert taps) on Q
 *   -> arm_sub_f32 / arm_add_f32 (USB / LSB)   [AM: arm_cmplx_mag_f32]
 *   -> arm_biquad_cascade_df1_f32 (CW narrow filter)
 *   -> [optional tap: Goertzel tone-detector bank (CTCSS, DTMF, selcall), selenite_rx_set_tones]
 *   -> [optional tap: arm_power_f32 per DSP block -> Morse decoder (CW skimmer), selenite_rx_set_cwdec]
 *   -> [optional tap: two arm_biquad_cascade_df1_f32 + arm_power_f32 per tick -> FSK teleprinter decoder (RTTY skimmer), selenite_rx_set_fskdec]
 *   -> [optional: arm_biquad_cascade_df1_f32 audio filter (notch, de-emphasis, EQ), selenite_rx_set_afilt]
 *   -> [optional: arm_lms_norm_f32 noise reduction / automatic notch, selenite_rx_set_nr]
 *   -> [optional: arm_power_f32 per DSP block -> level meter -> squelch decision, selenite_rx_set_meter]
 *   -> arm_abs_f32 + arm_max_f32 -> gain law -> arm_scale_f32 (AGC)
 *   -> [optional: the squelch gate: closed DSP blocks leave as zeros, selenite_rx_set_meter with gate = 1]
 *   -> [optional: arm_fir_interpolate_f32 back to the slot rate, mono / stereo frames, selenite_rx_set_out]
 */
#ifndef SELENITE_RX_H
#define SELENITE_RX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header (selenite_rx_abi_version() returns the library's).
 *   1  rounds 1-4: selenite_rx_config ends with agc_gain_init (112 bytes on LP64, the last 4 of them tail padding).
 *   2  selenite_rx_config grows to 120 bytes: q15_rounding (in the former padding), abi_version, reserved -- same for selenite_tx_config
 *      (96 -> 104 bytes).  selenite_rx_init / selenite_tx_init tell the two layouts apart by struct_size, CMSIS-style (the caller owns
 *      the struct, the library reads only what that caller's header declared, cf. arm_math.h:3272-3312): a version-1 caller
 *      (struct_size = SELENITE_RX_CONFIG_SIZE_V1) keeps working unchanged -- the bytes behind agc_gain_init are NOT read, whatever
 *      they hold, and int16 output truncates as it always did; a version-2 caller (struct_size = sizeof) must set abi_version = 2. */
#define SELENITE_RX_ABI_VERSION 2
#define SELENITE_RX_CONFIG_SIZE_V1 112u

/* Status codes: numerically identical to arm_status (arm_math.h:399-408). */
#define SELENITE_RX_SUCCESS          0   /* ARM_MATH_SUCCESS          */
#define SELENITE_RX_ARGUMENT_ERROR (-1)  /* ARM_MATH_ARGUMENT_ERROR   */
#define SELENITE_RX_LENGTH_ERROR   (-2)  /* ARM_MATH_LENGTH_ERROR     */
#define SELENITE_RX_NANINF         (-4)  /* ARM_MATH_NANINF (arm_math.h:405): a process call produced NaN / Inf audio -- latched by
                                           * selenite_rx_sync() and the host-pointer process calls (every fused kernel) */
#define SELENITE_RX_DEVICE_ERROR   (-7)  /* outside arm_status: HIP device/runtime failure */

/* Demodulator modes: the values of the firmware's Mode enum (Core/Inc/rxtx_if.h:33-43),
 * i.e. the byte DSP_Set_Mode() (Core/Src/dsp_if.c:367-370) receives from the CAT parser. */
#define SELENITE_MODE_LSB 0x00
#define SELENITE_MODE_USB 0x01
#define SELENITE_MODE_CW  0x02
#define SELENITE_MODE_CWR 0x03
#define SELENITE_MODE_AM  0x04
#define SELENITE_MODE_FM  0x08   /* Build-defined (the reference has no FM demodulator, CMSIS-DSP 1.5.3 no arctangent):
                                  * audio[n] = angle(z[n] * conj(z[n-1])) / pi on the decimated I/Q -- arm_cmplx_conj_f32,
                                  * arm_cmplx_mult_cmplx_f32, a stated arctangent, arm_scale_f32.  The
                                  * sample in front of a block comes from the delay lines of the FIR pair, which this mode keeps
                                  * running without evaluating the taps: needs nh_taps >= 2 (ARGUMENT_ERROR otherwise).
                                  * SELENITE_ARITH_SPLIT16 runs FM as _FMA; _AUTO guards it on min|z| x max|audio|. */
#define SELENITE_MODE_DIG 0x0A   /* = USB */
#define SELENITE_MODE_PKT 0x0C   /* = LSB */

/* Arithmetic contract of the MAC loops (DESIGN.md "Arithmetic modes"). */
#define SELENITE_ARITH_CMSIS 0   /* product rounded, then sum rounded: bit-exact vs CMSIS-DSP 1.5.3 C code */
#define SELENITE_ARITH_FMA   1   /* same operation order, the multiply-add of the FIR tap loops fused (fmaf);
                                    NCO, biquad recurrence and AGC keep the reference rounding.  Bit-exact
                                    vs the oracle's fmaf restatement, <=1e-5 relative vs CMSIS */
#define SELENITE_ARITH_SPLIT16 2 /* the many-tap FIR of the shape as a split-precision matrix product on the 16-bit matrix
                                    cores (decimator of the /2, /4 and /8 shapes; Hilbert FIR of the no-decimator shapes; TX
                                    interpolator): samples and taps split into f16 hi + lo parts, the three significant
                                    products (hi*hi, hi*lo, lo*hi) accumulated in f32 by MFMA, with a block exponent taken
                                    from the data of every pass (any amplitude a float can hold).  NOT bit-exact against any
                                    CPU order.  Guarantee: per DSP block max|out - ref| <= 1e-5 max|ref| against the CMSIS
                                    chain wherever the block's audio is within 12 dB of the largest sample its matrix product
                                    saw; every DSP block outside that zone is COUNTED (selenite_rx_guard_stats), and there the
                                    figure is the split product's error against the INPUT level (~1e-6 of it).  Everything
                                    else in the chain, and every configuration without such a kernel, runs as _FMA.
                                    Streaming filter state stays exact f32. */
#define SELENITE_ARITH_AUTO 3    /* _SPLIT16 with the conditional zone closed -- the default of the benchmarks.  A channel with
                                    a guarded DSP block in a call (selenite_rx_set_guard_ratio) is recomputed for that call,
                                    from its pre-call streaming state, by the bit-exact _CMSIS kernel, on the device, inside
                                    the same process call.  Guarantee: per DSP block max|out - ref| <= 1e-5 max|ref| against
                                    the CMSIS chain on EVERY block of every call, for any input, call length and mode switch
                                    (unguarded blocks by the split product's accuracy, recomputed channels with 0 ULP;
                                    selenite_rx_set_handover_repair keeps the recomputation exact across call boundaries).
                                    int16 slots: the bar holds for the float audio in front of arm_float_to_q15; the int16
                                    words are within 1 LSB + 1e-5 x (block maximum of that float audio) x 32768 of the
                                    reference's (a float inside the bar can still flip the truncation; only _CMSIS / _FMA
                                    are bit-exact there).
                                    Split-precision kernels exist for every decimator of 2 .. 256 taps (even count) by 2 or
                                    by 4 in front of a 31- / 63- / 127-tap type-III pair, by 8 in front of a 63-tap one, and
                                    for those pairs alone; other configurations run as _CMSIS. */

typedef struct selenite_rx_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_config) (a caller built against the version-1 header passes SELENITE_RX_CONFIG_SIZE_V1) */
    uint32_t channels;        /* C: independent I/Q channels handled by this instance */
    uint32_t block;           /* DSP block: complex input samples per CMSIS call / AGC update */
    uint32_t decim;           /* M (arm_fir_decimate_instance_f32.M); 1 = no decimator */
    uint32_t nd_taps;         /* decimator taps (numTaps); 0 = decimator bypassed (requires decim==1) */
    uint32_t nh_taps;         /* taps of the Hilbert / delay FIR pair; 0 = no FIR pair */
    uint32_t n_biquad;        /* DF1 biquad stages applied in CW/CWR; 0 = none */
    uint32_t arith;           /* SELENITE_ARITH_* */
    uint8_t  mode;            /* SELENITE_MODE_* */
    uint8_t  nco_enable;      /* 1 = quadrature NCO mix in front of the chain */
    uint8_t  agc_enable;      /* 1 = AGC at the end of the chain */
    uint8_t  agc_global;      /* 1 = one gain from the envelope maximum over ALL channels (and ranks) */
    uint32_t nco_step_all;    /* phase step per input sample (2^32 = one turn) when nco_step == NULL */
    const float    *dec_coeffs;    /* [nd_taps]  CMSIS order {b[N-1] .. b[0]} (arm_fir_decimate_f32.c:64-69) */
    const float    *hilb_coeffs;   /* [nh_taps]  arm_fir_f32 taps applied to the Q rail */
    const float    *delay_coeffs;  /* [nh_taps]  arm_fir_f32 taps applied to the I rail */
    const float    *biquad_coeffs; /* [5*n_biquad] {b0,b1,b2,a1,a2} per stage, feedback ADDED
                                      (arm_biquad_cascade_df1_f32.c:52-63) */
    const uint32_t *nco_step;      /* [channels] per-channel phase step, or NULL */
    float agc_target;         /* wanted peak level of the audio block */
    float agc_attack;         /* one-pole rate when the gain has to fall */
    float agc_decay;          /* one-pole rate when the gain may rise */
    float agc_gain_min;
    float agc_gain_max;
    float agc_env_floor;      /* envelope is clamped from below to this before target/env */
    float agc_gain_init;      /* gain before the first block */
    uint32_t q15_rounding;    /* int16 output (arm_float_to_q15): 0 = truncate -- the reference's code as the firmware builds it
                                 (ARM_MATH_ROUNDING undefined, arm_float_to_q15.c:117) --, 1 = the ARM_MATH_ROUNDING variant
                                 (arm_float_to_q15.c:90-101: +-0.5 in float before the truncation); any other value is an ARGUMENT_ERROR.
                                 ABI version 2: read only when struct_size == sizeof(selenite_rx_config) (it sits where version 1 had padding). */
    uint32_t abi_version;     /* ABI version 2: = SELENITE_RX_ABI_VERSION (anything else with the version-2 struct_size: ARGUMENT_ERROR) */
    uint32_t reserved;        /* 0 */
} selenite_rx_config;

/* Host-side view of the per-channel streaming state (what CMSIS keeps in pState).
 * Any pointer may be NULL (skipped).  Layouts:
 *   dec_state  [channels][2][nd_taps-1]   rail 0 = I, rail 1 = Q; oldest sample first
 *                                         (arm_fir_decimate_f32.c:396-426 copy-back order)
 *   fir_state  [channels][2][nh_taps-1]   rail 0 = delay FIR (I), rail 1 = Hilbert FIR (Q)
 *                                         (arm_fir_f32.c:947-978)
 *   biq_state  [channels][n_biquad][4]    {x[n-1], x[n-2], y[n-1], y[n-2]}
 *                                         (arm_biquad_cascade_df1_f32.c:319-322)
 *   agc_gain   [channels]
 *   nco_phase  [channels]                 uint32 phase accumulator
 */
typedef struct selenite_rx_state_view {
    float    *dec_state;
    float    *fir_state;
    float    *biq_state;
    float    *agc_gain;
    uint32_t *nco_phase;
} selenite_rx_state_view;

/* ---- NLMS noise reduction / automatic notch (step 4b of DESIGN.md section 2, between the CW filter and the AGC) -------------
 * Per channel, on the un-scaled audio x of the demodulator (every mode), at the audio rate:
 *   u[n] = x[n - delay]                                   decorrelation delay line (zeros after selenite_rx_set_nr)
 *   arm_lms_norm_f32(S, pSrc = u, pRef = x, pOut = y, pErr = e, n)   (FilteringFunctions/arm_lms_norm_f32.c:161-348, the
 *                                                         ARM_MATH_DSP branch the firmware's -DARM_MATH_CM4 selects)
 *   SELENITE_RX_NR_DENOISE passes y (what the input predicts from `delay` samples back: tones, voiced speech; broadband noise falls),
 *   SELENITE_RX_NR_NOTCH   passes e = x - y (the predictable part removed: carriers, heterodynes);
 * the AGC then runs on the stage's output.  The stage keeps the reference's rounding in every arith mode (products then sums in
 * tap order, energy -= x0*x0; energy += in*in, a correctly rounded division, no contraction): given its input it is bit-exact
 * against arm_lms_norm_f32.  Non-finite stage output raises SELENITE_RX_NANINF like any other. */
#define SELENITE_RX_NR_OFF     0
#define SELENITE_RX_NR_DENOISE 1
#define SELENITE_RX_NR_NOTCH   2

typedef struct selenite_rx_nr_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_nr_config) (this struct's own growth path, as selenite_rx_config's) */
    uint32_t kind;            /* SELENITE_RX_NR_* */
    uint32_t num_taps;        /* arm_lms_norm_instance_f32.numTaps: 8, 16, 32 or 64 */
    uint32_t delay;           /* decorrelation delay D in audio samples, 1 .. 64 */
    float    mu;              /* step size, finite, 0 < mu < 2 */
    const float *coeffs_init; /* [num_taps] initial weights in pCoeffs order (shared by every channel), or NULL = zeros; copied */
} selenite_rx_nr_config;

/* Host-side view of the stage's per-channel state; any pointer may be NULL (skipped).  N = num_taps, D = delay:
 *   coeffs [channels][N]      pCoeffs
 *   window [channels][N-1]    the last N-1 samples of u, oldest first (arm_lms_norm_f32.c:315-346 copy-back order)
 *   delay  [channels][D]      the last D samples of x, oldest first
 *   energy [channels]         arm_lms_norm_instance_f32.energy
 *   x0     [channels]         arm_lms_norm_instance_f32.x0 */
typedef struct selenite_rx_nr_state_view {
    float *coeffs;
    float *window;
    float *delay;
    float *energy;
    float *x0;
} selenite_rx_nr_state_view;

/* ---- audio output stage (step 7 of DESIGN.md section 2, behind the AGC; off by default) ---------------------------------------
 * What DSP_Out_Buff_Read (Core/Src/dsp_if.c:204-219) hands the codec: the audio back at the slot rate, as left / right frames.
 * Per channel and DSP block of n = block / decim audio samples:
 *   arm_fir_interpolate_f32(L, coeffs, ni_taps)   n in, n * L out (FilteringFunctions/arm_fir_interpolate_f32.c:136-563)
 *   int16 slots: arm_float_to_q15 on the interpolated samples (cfg.q15_rounding)
 *   SELENITE_RX_OUT_MONO one value per sample; SELENITE_RX_OUT_STEREO each value twice, left then right (pbuf[k] = i, pbuf[k + 1] = q)
 * With the stage on, pDstAudio of every process entry point is [channels][blockSize / decim * L * (STEREO ? 2 : 1)]
 * (selenite_rx_out_values per channel).  The stage keeps the reference's rounding in every arith mode (one accumulator per output from
 * +0.0f, taps ascending, product rounded, then sum rounded): given its input it is bit-exact against arm_fir_interpolate_f32.
 * Non-finite stage output raises SELENITE_RX_NANINF like any other. */
#define SELENITE_RX_OUT_MONO   0
#define SELENITE_RX_OUT_STEREO 1

typedef struct selenite_rx_out_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_out_config) (this struct's own growth path) */
    uint32_t interp;          /* L: 1, 2, 4 or 8 (need not equal cfg.decim) */
    uint32_t ni_taps;         /* L * P, P = phaseLength 1 .. 64; interp == 1 && ni_taps == 0: no FIR, frames only */
    uint32_t frames;          /* SELENITE_RX_OUT_* */
    const float *coeffs;      /* [ni_taps] pCoeffs order {b[numTaps-1] .. b[0]} (arm_fir_interpolate_f32.c:63-72); finite; copied */
} selenite_rx_out_config;

/* ---- spectrum tap (step 0b of DESIGN.md section 2, on the raw input I/Q in front of the NCO; off by default) -----------------------
 * What the PC side of the reference draws: the power spectrum of the band, per channel.  The input stream (int16 slots through
 * arm_q15_to_float) is cut into frames of fft_len consecutive complex samples -- frames of the STREAM, counted from set_spectrum / reset,
 * not of the call: a partial frame waits in the instance.  Frame f is transformed iff f % stride == 0 (the others are never read):
 *   arm_cmplx_mult_real_f32(frame, window)            ComplexMathFunctions/arm_cmplx_mult_real_f32.c (absent when window == NULL)
 *   arm_cfft_f32(&arm_cfft_sR_f32_lenN, frame, 0, 1)  TransformFunctions/arm_cfft_f32.c:562-616, arm_cfft_radix8_f32.c:45-285: forward,
 *                                                     natural-order output; fft_len 64 or 512, the pure radix-8 lengths
 *   p = arm_cmplx_mag_squared_f32(frame)              ComplexMathFunctions/arm_cmplx_mag_squared_f32.c: re * re + im * im
 *   average == 0: row[k] = p[k];  average == 1: row[k] = row[k] + alpha * (p[k] - row[k]) from row = +0.0f, every operation rounded
 * The row is stored display-ordered: bin k at index (k + fft_len / 2) mod fft_len, DC in the middle.  Bit-exact against that composition
 * in every arith mode (no contraction, no flushed denormals).  Non-finite power is stored as it comes and does NOT raise
 * SELENITE_RX_NANINF: that status keeps meaning audio.  No dB: CMSIS-DSP 1.5.3 has no logarithm, the conversion is the display's. */
#define SELENITE_RX_WINDOW_HANN            0
#define SELENITE_RX_WINDOW_BLACKMAN_HARRIS 1

typedef struct selenite_rx_spec_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_spec_config) (this struct's own growth path) */
    uint32_t fft_len;         /* N: 64 or 512; any other length is a SELENITE_RX_LENGTH_ERROR (arm_cfft_f32.c:582-599: radix8by2 / by4) */
    uint32_t stride;          /* 1 .. 65535: every stride-th frame is transformed */
    uint32_t average;         /* 0: the row is the last transformed frame's power; 1: exponential averaging with alpha */
    float alpha;              /* 0 < alpha <= 1, finite */
    const float *window;      /* [fft_len], finite, copied; NULL = none */
} selenite_rx_spec_config;

/* The tap's whole state.  rows [channels][fft_len] display order; pending [channels][fft_len][2]: the first position % fft_len samples
 * of the frame the stream stands in (kept only for a frame that will be transformed); position: ONE value, input samples per channel
 * since set_spectrum / reset.  NULL members are skipped. */
typedef struct selenite_rx_spec_state_view {
    float *rows;
    float *pending;
    uint64_t *position;
} selenite_rx_spec_state_view;

/* ---- impulse noise blanker (step 0c of DESIGN.md section 2, on the raw input I/Q behind the spectrum tap and in front of the NCO; off by
 * default) ---------------------------------------------------------------------------------------------------------------------------
 * The third of the classic NR / ANF / NB set, and the one that belongs at the input rate: one sample far above the band level rings through
 * the decimator and the Hilbert pair and pumps the AGC; behind the demodulator nothing undoes that.  Every mode, every arith mode.  The
 * call's input (int16 slots seen through arm_q15_to_float) is cut into frames of `frame` consecutive complex samples; frame divides
 * cfg.block and every call is a whole number of DSP blocks, so nothing is left pending.  Per channel one float of state, level (+0.0f after
 * set_nb and reset), and two counters.  Per frame, every operation rounded to f32, no contraction, denormals kept:
 *   p[n] = arm_cmplx_mag_squared_f32(frame)           ComplexMathFunctions/arm_cmplx_mag_squared_f32.c: re * re + im * im
 *   m    = arm_mean_f32(p, frame)                     StatisticsFunctions/arm_mean_f32.c:67-120: s = 0; s = s + p[n], n ascending; s / frame
 *   !(level > 0) (not primed: zero, negative, NaN):   nothing is blanked; level = m
 *   level > 0:  hit[n] = p[n] > threshold * level; k = the number of hits
 *               1 <= k <= max_hits: sample n is blanked iff a hit lies within `guard` samples of it, inside the frame
 *               k > max_hits: a signal that came up, not impulse noise: nothing is blanked, bursts += 1
 *               level = level + alpha * (min(m, clamp * level) - level)     (the AGC's form; m < c ? m : c)
 * The level does not depend on what was blanked: an impulse raises it by at most `clamp` per frame.  A blanked sample becomes (+0.0f, +0.0f)
 * or (0, 0) and counts in `blanked`; every other sample is passed on as the bits it is (-0.0f, NaN payloads, -32768).  The chain then runs
 * on that copy in place of the caller's input, in the caller's format; the spectrum tap keeps reading the caller's own.  Bit-exact against
 * that composition.  The stage never raises SELENITE_RX_NANINF: that status keeps meaning audio (a NaN power is not a hit). */
typedef struct selenite_rx_nb_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_nb_config) (this struct's own growth path) */
    uint32_t frame;           /* F: 32, 64 or 128, and a divisor of cfg.block; anything else is a SELENITE_RX_LENGTH_ERROR */
    uint32_t guard;           /* 0 .. 8 samples on either side of a hit */
    uint32_t max_hits;        /* 1 .. F / 4 */
    float threshold;          /* finite, >= 1: sample power over level */
    float alpha;              /* 0 < alpha <= 1 */
    float clamp;              /* finite, >= 1 */
} selenite_rx_nb_config;

/* The blanker's whole state, each [channels]: level; blanked: samples blanked since set_nb / reset; bursts: frames with more than max_hits
 * hits since then.  NULL members are skipped. */
typedef struct selenite_rx_nb_state_view {
    float *level;
    uint64_t *blanked;
    uint64_t *bursts;
} selenite_rx_nb_state_view;

/* ---- I/Q correction: DC offset, gain and phase imbalance (on the raw input I/Q behind the
 * spectrum tap and in front of the noise blanker; off by default) ---------------------------------------------------------------------
 * A quadrature sampling detector in front of a stereo codec leaves a DC offset on each rail (a carrier in the passband) and a gain and
 * phase mismatch between the rails (a mirror image of every signal on the other sideband) that no Hilbert pair behind it removes.  Every
 * mode, every arith mode.  The call's input (int16 slots seen through arm_q15_to_float) is cut into frames of `frame` consecutive complex
 * samples, I[n] = x[2n], Q[n] = x[2n + 1]; frame divides cfg.block and every call is a whole number of DSP blocks, so nothing is left
 * pending.  Per channel four floats of state, dc_i, dc_q, p, g (dc_i_init, dc_q_init, p_init, g_init after set_iqc and reset), and one
 * counter, held (0).  Per frame, every operation rounded to f32, no contraction, denormals kept:
 *   correct, with the coefficients in front of the frame:
 *     i[n] = I[n] - dc_i, q[n] = Q[n] - dc_q            BasicMathFunctions/arm_offset_f32.c:145 with the negated offset: the same bits
 *     t[n] = i[n] * p                                   BasicMathFunctions/arm_scale_f32.c:148
 *     u[n] = q[n] - t[n]                                BasicMathFunctions/arm_sub_f32.c:129
 *     Iout[n] = i[n], Qout[n] = u[n] * g                arm_scale_f32
 *   DC estimate (dc_alpha > 0):
 *     mi = arm_mean_f32(I, frame), mq likewise          StatisticsFunctions/arm_mean_f32.c:67-120: s = 0; s = s + I[n], n ascending; s / frame
 *     dc_i = dc_i + dc_alpha * (mi - dc_i)              difference, product, sum each rounded (the AGC's form); a rail whose mean is not
 *                                                       finite keeps its dc
 *   imbalance estimate (alpha > 0), on the i, q above:
 *     pii = arm_power_f32(i), pqq = arm_power_f32(q)    StatisticsFunctions/arm_power_f32.c:86-117: sum = sum + in * in, n ascending
 *     piq = arm_dot_prod_f32(i, q)                      BasicMathFunctions/arm_dot_prod_f32.c:85-112: sum = sum + a * b, n ascending
 *     a = piq / pii; r = pqq - a * piq; b = arm_sqrt_f32(pii / r)        Include/arm_math.h:5726-5742: sqrtf, correctly rounded
 *     valid: pii > min_power && pii <= FLT_MAX && r > min_power && r <= FLT_MAX          (a NaN anywhere: not valid)
 *     valid:     a = a < -p_max ? -p_max : (a > p_max ? p_max : a);  b = b < g_min ? g_min : (b > g_max ? g_max : b), g_min = 1.0f / g_max
 *                p = p + alpha * (a - p);  g = g + alpha * (b - g)
 *     not valid: p and g stay, held += 1
 *   alpha == 0: no estimate, held does not move (manual calibration: p_init / g_init, or selenite_rx_set_iqc_state).
 * The estimates read the raw input and the dc in front of the frame, never the corrected output.  The corrected samples are always f32, in
 * a buffer of the instance; the rest of the call (the noise blanker, then the chain) reads that in place of the caller's input, and the
 * spectrum tap keeps reading the caller's own.  int16 slots become f32 in, int16 out: the audio words are arm_float_to_q15 of the f32
 * call's audio, bit for bit in SELENITE_ARITH_CMSIS and _FMA and within the int16 bar of the arith mode otherwise.  Bit-exact against that
 * composition.  The stage never raises SELENITE_RX_NANINF. */
typedef struct selenite_rx_iqc_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_iqc_config) (this struct's own growth path) */
    uint32_t frame;           /* F: 32, 64 or 128, and a divisor of cfg.block; anything else is a SELENITE_RX_LENGTH_ERROR */
    float alpha;              /* 0 .. 1; 0: p and g are not estimated */
    float dc_alpha;           /* 0 .. 1; 0: dc_i and dc_q are not estimated */
    float p_max;              /* finite, 0 < p_max <= 1 */
    float g_max;              /* finite, >= 1 */
    float min_power;          /* finite, >= 0 */
    float p_init;             /* -p_max .. p_max */
    float g_init;             /* 1 / g_max .. g_max */
    float dc_i_init;          /* finite */
    float dc_q_init;          /* finite */
} selenite_rx_iqc_config;

/* The stage's whole state, each [channels]: dc_i, dc_q, p, g; held: frames whose imbalance estimate was not valid since set_iqc / reset.
 * NULL members are skipped. */
typedef struct selenite_rx_iqc_state_view {
    float *dc_i;
    float *dc_q;
    float *p;
    float *g;
    uint64_t *held;
} selenite_rx_iqc_state_view;

/* ---- signal-level meter and squelch (on the un-scaled audio in front of the AGC, the gate
 * behind it; off by default) -----------------------------------------------------------------------------------------------------------
 * How strong is the signal in a channel's passband, and is there one at all: agc_gain is the AGC's control variable, not a measurement, and
 * the spectrum tap shows the band in front of the NCO.  Every mode, every arith mode.  Per channel and per DSP block of n = block / decim
 * UN-SCALED audio samples x -- the demodulator's output, behind the CW filter and behind NLMS when that is on, in front of the AGC.  Per
 * channel: level (f32; level_init after set_meter and reset), open (u32, 0 / 1; 0), hold (u32; 0), opens (u64; 0), open_blocks (u64; 0).
 * Per block, every operation rounded to f32, no contraction, denormals kept:
 *   pw = arm_power_f32(x, n)            StatisticsFunctions/arm_power_f32.c:64-125: sum = +0.0f; sum = sum + in * in, ascending (product
 *                                       rounded, then the sum)
 *   ms = pw / (float)n                  correctly rounded division (n is any block / decim, e.g. 24: not always a power of two)
 *   ms <= FLT_MAX (false for NaN):      r = ms > level ? attack : decay;  d = ms - level;  level = level + r * d      (the AGC's form)
 *   otherwise:                          level stays
 *   v = level
 *   want_open  = sense == ABOVE ? v > open_level  : v < open_level
 *   want_close = sense == ABOVE ? v < close_level : v > close_level
 *   if (!open)           { if (want_open) { open = 1; hold = hang; opens += 1; } }
 *   else if (want_close) { if (hold == 0) open = 0; else hold -= 1; }
 *   else                   hold = hang;
 *   open_blocks += open
 * SELENITE_RX_SQ_ABOVE is a carrier / level squelch; SELENITE_RX_SQ_BELOW a noise squelch, which FM needs (a quieted discriminator means a
 * signal).  The hysteresis is close_level against open_level; hang is the number of consecutive closing blocks the gate survives.
 * gate == 1: a block whose open is 0 AFTER its update leaves the call as +0.0f (int16 slots: 0), BEHIND the AGC: the AGC itself runs on the
 * un-scaled audio of every block as it does without the stage -- gain, the agc_global envelope and all chain state are bit for bit those
 * of the same call without the stage.  gate == 0: meter only, the audio is untouched.  With an output stage the gate sits in front of the
 * interpolator, whose FIR rings the edge out.  The level is a mean square, linear: CMSIS-DSP 1.5.3 has no logarithm (the spectrum tap's
 * rule).  Bit-exact given its input in every arith mode.  The stage never raises or clears SELENITE_RX_NANINF. */
#define SELENITE_RX_SQ_ABOVE 0
#define SELENITE_RX_SQ_BELOW 1
typedef struct selenite_rx_meter_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_meter_config) (this struct's own growth path) */
    uint32_t sense;           /* SELENITE_RX_SQ_* */
    uint32_t gate;            /* 0: meter only; 1: closed blocks leave as zeros */
    uint32_t hang;            /* 0 .. 65535 */
    float attack;             /* 0 < attack <= 1 */
    float decay;              /* 0 < decay <= 1 */
    float open_level;         /* finite, >= 0 */
    float close_level;        /* finite, >= 0; ABOVE: close_level <= open_level; BELOW: close_level >= open_level */
    float level_init;         /* finite, >= 0 */
} selenite_rx_meter_config;

/* The stage's whole state, each [channels].  NULL members are skipped. */
typedef struct selenite_rx_meter_state_view {
    float *level;
    uint32_t *open;
    uint32_t *hold;
    uint64_t *opens;          /* closed -> open transitions since set_meter / reset */
    uint64_t *open_blocks;    /* DSP blocks that ended open since set_meter / reset */
} selenite_rx_meter_state_view;

/* ---- audio biquad filter (on the un-scaled audio behind the demodulator and the CW filter, in
 * front of NLMS, the level meter and the AGC; off by default) ----------------------------------------------------------------------------
 * A manual notch, FM de-emphasis, tone control, an audio high-pass or low-pass: NLMS adapts on the filtered audio and the meter sees what
 * the listener hears.  Every mode, every arith mode.  The un-scaled audio of a channel is one stream, a call contributes
 * nout = blockSize / decim samples; per channel
 *   arm_biquad_cascade_df1_f32(S, x, x, nout)     FilteringFunctions/arm_biquad_cascade_df1_f32.c:165-407, in place, stage-outer
 *     per stage s = 0 .. n_stages-1, coefficients {b0, b1, b2, a1, a2} (CMSIS sign: the a's are ADDED), state {x1, x2, y1, y2}:
 *     acc = b0 * x[n];  acc = acc + b1 * x1;  acc = acc + b2 * x2;  acc = acc + a1 * y1;  acc = acc + a2 * y2
 *     x2 = x1; x1 = x[n]; y2 = y1; y1 = acc; x[n] = acc
 * every product rounded to f32, then every sum; no contraction, denormals kept, in SELENITE_ARITH_CMSIS, _FMA, _SPLIT16 and _AUTO alike:
 * bit-exact given its input, and the bits do not depend on how the stream is cut into calls.  Coefficients are one set [n_stages][5] for
 * all channels, or with per_channel = 1 one set per channel, [channels][n_stages][5] (a notch where each channel's heterodyne is); they
 * must be finite and are copied.  Stability is the caller's business: the stage neither raises nor clears SELENITE_RX_NANINF, and a state
 * that became NaN stays NaN until selenite_rx_reset or selenite_rx_set_afilt_state, as with CMSIS.  State: [channels][n_stages][4] in
 * CMSIS pState order, +0.0f after set_afilt and reset. */
#define SELENITE_RX_AFILT_MAX_STAGES 8
typedef struct selenite_rx_afilt_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_afilt_config) (this struct's own growth path) */
    uint32_t n_stages;        /* 1 .. 8 */
    uint32_t per_channel;     /* 0: coeffs [n_stages][5]; 1: coeffs [channels][n_stages][5] */
    uint32_t reserved;        /* 0 */
    const float *coeffs;      /* finite, copied */
} selenite_rx_afilt_config;

/* The stage's state and, for get only, its coefficients as configured.  NULL members are skipped. */
typedef struct selenite_rx_afilt_state_view {
    float *state;             /* [channels][n_stages][4] {x1, x2, y1, y2} */
    float *coeffs;            /* [n_stages][5] or [channels][n_stages][5], as configured; get only */
} selenite_rx_afilt_state_view;

/* ---- tone-detector bank (a TAP on the un-scaled audio behind the demodulator and the CW
 * filter, in front of the audio filter, NLMS, the level meter and the AGC; off by default) -----------------------------------------------
 * Which of K known tones is in the channel: CTCSS tone squelch, DTMF, selective calling, a 1750 Hz burst, a CW pitch indicator.  The
 * stage reads the audio and changes none of it (a CTCSS tone is seen in front of the high-pass that removes it).  Every mode, every arith
 * mode.  The un-scaled audio of a channel is one stream; n = block / decim; a frame is frame_blocks consecutive DSP blocks of it,
 * N = frame_blocks * n samples, counted from selenite_rx_set_tones / selenite_rx_reset, not per call: one `position` (uint64, in DSP
 * blocks) says where the stream stands, a frame may straddle calls and a call may end several frames.  One table of K tones for all
 * channels, three floats each: {c, cw, sw} = {2 cos w, cos w, sin w}, w = 2 pi f, 0 < f < 0.5 cycles per audio sample
 * (selenite_rx_design_tones); finite, copied.  Every operation below is rounded to f32; no contraction, denormals kept.
 *   per sample x and tone k, state s1, s2 (+0.0f at a frame's start):
 *     t = c * s1;  s0 = x + t;  s0 = s0 - s2;  s2 = s1;  s1 = s0
 *   per sample, once per channel (arm_power_f32's sum, +0.0f at a frame's start):
 *     e = x * x;  E = E + e
 *   at the frame's last sample, per tone (arm_cmplx_mag_squared_f32's form):
 *     u = cw * s2;  re = s1 - u;  im = sw * s2;  a = re * re;  b = im * im;  p[k] = a + b
 *   then per channel (arm_max_f32, StatisticsFunctions/arm_max_f32.c: the first index of the maximum; a NaN wins only at index 0):
 *     (p_best, best) = arm_max_f32(p, K)
 *     t = ratio * E;  t = t * (float)N
 *     hit = p_best > t && p_best > min_power && p_best <= FLT_MAX
 *     w = hit ? best : SELENITE_RX_TONE_NONE
 *     if (w == cand) run = min(run + 1, 65535); else { cand = w; run = 1; }
 *     if (cand != tone && run >= (cand == NONE ? release : confirm)) { tone = cand; changes += 1; }
 *     power[k] = p[k];  frame_energy = E;  last_best = best           (the rows a reader sees)
 *     s1 = s2 = +0.0f for every tone;  E = +0.0f
 * The recurrence is arm_biquad_cascade_df1_f32 with the one section {1, 0, 0, c, -1} (s1 = y1, s2 = y2) less its two dead products
 * 0 * x1 and 0 * x2: the same bits on finite input that holds no -0.0f.  The three-operation form is the specification: a -0.0f sample can
 * give a zero of the other sign (c < 0, zero state, x = -0.0f: -0.0f here, +0.0f there) and an Inf sample becomes NaN one step later here.
 * The stage neither raises nor clears SELENITE_RX_NANINF; a non-finite sample poisons its own frame only (the state is cleared at the
 * frame's end).  State after set_tones and reset: s, E, power, frame_energy +0.0f; last_best, run, changes, position 0; tone, cand NONE. */
#define SELENITE_RX_TONES_MAX  64
#define SELENITE_RX_TONE_NONE  0xFFFFFFFFu
typedef struct selenite_rx_tones_config {
    uint32_t struct_size;    /* = sizeof(selenite_rx_tones_config) (this struct's own growth path) */
    uint32_t n_tones;        /* K: 1 .. 64 */
    uint32_t frame_blocks;   /* 1 .. 65535 DSP blocks per frame (frame_blocks * block / decim < 2^31) */
    uint32_t confirm;        /* 1 .. 65535 consecutive frames before a tone is reported */
    uint32_t release;        /* 1 .. 65535 consecutive frames without a hit before NONE is reported */
    uint32_t reserved;       /* 0 */
    float ratio;             /* finite, 0 <= ratio <= 1: p_best against E * N (a pure tone alone gives 0.5) */
    float min_power;         /* finite, >= 0 */
    const float *coeffs;     /* [n_tones][3] {2 cos w, cos w, sin w}, finite, copied */
} selenite_rx_tones_config;

/* The stage's state.  NULL members are skipped. */
typedef struct selenite_rx_tones_state_view {
    float *s;                 /* [channels][n_tones][2] {s1, s2} of the running frame */
    float *energy;            /* [channels] E of the running frame */
    float *power;             /* [channels][n_tones] p of the last whole frame */
    float *frame_energy;      /* [channels] E of the last whole frame */
    uint32_t *last_best;      /* [channels] best of the last whole frame */
    uint32_t *tone;           /* [channels] the reported tone, or SELENITE_RX_TONE_NONE */
    uint32_t *cand;           /* [channels] the candidate */
    uint32_t *run;            /* [channels] consecutive frames of the candidate, saturating at 65535 */
    uint64_t *changes;        /* [channels] changes of `tone` since set_tones / reset */
    uint64_t *position;       /* ONE value: DSP blocks per channel since set_tones / reset */
} selenite_rx_tones_state_view;

/* ---- Morse decoder, a CW skimmer (a TAP on the un-scaled audio behind the demodulator and
 * the CW filter, in front of the audio filter, NLMS, the level meter and the AGC; off by default) ------------------------------------------
 * The stage is a tap, off by default, available in every mode and every `arith` mode.  It reads the un-scaled audio behind the
 * demodulator and behind the CW filter (step 4).  That is the tone bank's position, in front of 4a / 4b / 4c / the AGC.  It changes none
 * of the audio.  One tick is one DSP block of n = block / decim samples x.
 * Every float operation is rounded to f32, with no contraction and denormals kept.  The division is correctly rounded.  These are the
 * meter's rules.
 * State per channel, with its value after set_cwdec / reset in brackets: peak, floor (f32; +0.0f); primed, key, flip, run (u32; 0);
 * unit (u32, Q8 blocks; unit_init); code (u32; 1); word (u32; 0); count (u64; 0); text[ring] (u8; 0).
 *   pw = arm_power_f32(x, n);  ms = pw / (float)n
 *   raw = 0
 *   if (ms <= FLT_MAX) {                                   (false for NaN: peak, floor stay, raw = 0)
 *       if (!primed) { peak = ms; floor = ms; primed = 1; }
 *       else {
 *           r = ms > peak  ? peak_attack  : peak_decay;   d = ms - peak;   t = r * d;  peak  = peak  + t;
 *           r = ms < floor ? floor_attack : floor_decay;  d = ms - floor;  t = r * d;  floor = floor + t;
 *       }
 *       span = peak - floor;  f = key ? off_frac : on_frac;  t = f * span;  thr = floor + t;
 *       q = snr * floor;  active = peak > q && peak > min_power;
 *       raw = active && ms > thr;
 *   }
 *   edge = 0
 *   if (raw == key) { run = min(run + flip + 1, 65535); flip = 0; }
 *   else { flip += 1;  if (flip >= debounce) { ended = run; key = raw; run = flip; flip = 0; edge = 1; } }
 *   if (edge && key == 0) {                                (a mark of `ended` blocks is over)
 *       m = ended << 8;  dah = m >= 2 * unit;              (unit as it stood before this update)
 *       if (adapt) { g = dah ? m / 3 : m;
 *                    if (g >= unit) unit += (g - unit) >> track; else unit -= (unit - g) >> track;
 *                    unit = min(max(unit, unit_min), unit_max); }
 *       code = (code == 0 || code >= 128) ? 0 : (code << 1) | dah;       (0: more than 7 elements)
 *   }
 *   if (key == 0) {
 *       s = run << 8;
 *       if (code != 1 && s >= 2 * unit) { emit(table[code]); code = 1; word = 1; }
 *       if (word && s >= 5 * unit)      { emit(' ');         word = 0; }
 *   }
 *   emit(c):  text[count % ring] = c;  count += 1
 * `table` is 256 bytes, copied, indexed by the element pattern behind a leading 1.  `.-` is 0b101.  Index 0 is the overflow character.
 * The stage neither raises nor clears SELENITE_RX_NANINF.  One set of parameters and one table for all channels. */
typedef struct selenite_rx_cwdec_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_cwdec_config) (this struct's own growth path) */
    float peak_attack;        /* the four follower rates: finite, in (0, 1] */
    float peak_decay;
    float floor_attack;
    float floor_decay;
    float on_frac;            /* 0 < off_frac <= on_frac < 1 */
    float off_frac;
    float snr;                /* finite, >= 1 */
    float min_power;          /* finite, >= 0 */
    uint32_t debounce;        /* 1 .. 255 */
    uint32_t adapt;           /* 0 / 1 */
    uint32_t track;           /* 0 .. 8 */
    uint32_t unit_min;        /* Q8 blocks: 256 <= unit_min <= unit_init <= unit_max <= 8192 * 256 */
    uint32_t unit_init;
    uint32_t unit_max;
    uint32_t ring;            /* a power of two, 16 .. 65536: characters kept per channel */
    const uint8_t *table;     /* [256], copied; NULL selects the built-in table (selenite_rx_design_morse with unknown = '#') */
} selenite_rx_cwdec_config;

/* The stage's whole state.  NULL members are skipped. */
typedef struct selenite_rx_cwdec_state_view {
    float *peak;              /* [channels] */
    float *floor;             /* [channels] */
    uint32_t *primed;         /* [channels] 0 / 1 */
    uint32_t *key;            /* [channels] 0 / 1: the debounced key */
    uint32_t *flip;           /* [channels] consecutive blocks against `key` */
    uint32_t *run;            /* [channels] blocks of the running mark or space, saturating at 65535 */
    uint32_t *unit;           /* [channels] the dit length, Q8 blocks */
    uint32_t *code;           /* [channels] the elements of the running character behind a leading 1; 0: overflow */
    uint32_t *word;           /* [channels] 0 / 1: a character is out and its word space is not */
    uint64_t *count;          /* [channels] characters emitted since set_cwdec / reset */
    uint8_t *text;            /* [channels][ring] */
} selenite_rx_cwdec_state_view;

/* ---- FSK teleprinter decoder, an RTTY skimmer (a TAP on the un-scaled audio behind the
 * demodulator and the CW filter, in front of the audio filter, NLMS, the level meter and the AGC; off by default) -----------------------
 * The stage is a tap, off by default, on the un-scaled audio behind the demodulator and the CW filter (step 4).  That is the tone bank's and
 * the Morse decoder's position, in front of 4a / 4b / 4c / the AGC.  It works in every mode and every `arith` mode, and it changes none of
 * the audio.  It neither raises nor clears SELENITE_RX_NANINF.
 * One tick is T = tick consecutive audio samples, 4 <= T <= 256.  T must divide n = block / decim, otherwise the call returns
 * SELENITE_RX_LENGTH_ERROR, as the noise blanker's frame does.  So ticks never straddle DSP blocks or calls, and nothing is left pending.
 * Every float operation is rounded to f32, with no contraction and denormals kept.  These are the meter's rules.
 * Per channel and tick, with x the tick's samples:
 *   two arm_biquad_cascade_df1_f32 instances of ONE section each, coefficients {b0,b1,b2,a1,a2} = mark[5] / space[5] (one set for all channels),
 *   state {x1,x2,y1,y2} each, running on across ticks, blocks and calls:
 *       per sample:  acc = b0*x; acc = acc + b1*x1; acc = acc + b2*x2; acc = acc + a1*y1; acc = acc + a2*y2;  (each product rounded, then the sum)
 *                    x2 = x1; x1 = x; y2 = y1; y1 = acc
 *   pm = arm_power_f32(ym, T);  ps = arm_power_f32(ys, T);  pw = arm_power_f32(x, T)        (from +0.0f, ascending; no division)
 *   if (reverse) swap(pm, ps)
 *   if (pm <= FLT_MAX && ps <= FLT_MAX && pw <= FLT_MAX) {           (false for NaN: the followers stay)
 *       d = pm - em; t = alpha*d; em = em + t;      es, ew likewise from ps, pw          (the AGC's form)
 *   }
 *   tot = em + es;  dd = em - es;  th = hyst*tot;  q = frac*ew
 *   present = tot > q && tot > min_power && tot <= FLT_MAX
 *   prev = lvl
 *   if (!present) lvl = 1;  else if (dd > th) lvl = 1;  else if (-dd > th) lvl = 0;      (else lvl stays; 1 = mark = idle)
 *   if (k == 0) { if (prev == 1 && lvl == 0) { k = 1; t_q8 = 0; shift = 0; } }            (start edge; nothing is sampled in this tick)
 *   else {
 *       t_q8 += 256
 *       if (t_q8 >= (k-1)*bit + (bit >> 1)) {                                             (centre of bit k-1; bit: this channel's, Q8 ticks)
 *           if (k == 1)      { k = lvl ? 0 : 2; }                                         (a start bit that did not last: false start)
 *           else if (k <= 6) { shift |= lvl << (k-2); k += 1; }                           (five data bits, LSB first)
 *           else { if (lvl) { c = shift;
 *                             if (c == 31) figs = 0; else if (c == 27) figs = 1;
 *                             else { b = table[figs*32 + c]; if (b) emit(b); if (usos && c == 4) figs = 0; } }
 *                  else ferr += 1;                                                         (framing error: nothing is emitted)
 *                  k = 0; }
 *       }
 *   }
 *   emit(b):  text[count % ring] = b;  count += 1
 * State per channel after set_fskdec / selenite_rx_reset: filt[2][4], em, es, ew: +0.0f; lvl: 1; k, t_q8, shift, figs, ferr: 0; bit: the
 * config's bit_q8; count: 0 (u64); text[ring]: 0.  `bit` is a state row: through set_fskdec_state every channel can run at its own speed,
 * the way `unit` does for the Morse decoder.  A non-finite sample poisons that channel's filters until reset or set_fskdec_state: the three
 * followers stay where they stood.  The state moves with ChanRange.first.  set_mode and the other setters leave it alone.
 * `table` is 64 bytes, copied: letters then figures, indexed by the 5-bit code; a 0 byte emits nothing.
 * One set of parameters, one coefficient pair and one table for all channels. */
typedef struct selenite_rx_fskdec_config {
    uint32_t struct_size;     /* = sizeof(selenite_rx_fskdec_config) (this struct's own growth path) */
    uint32_t tick;            /* T: 4 .. 256 audio samples; must divide cfg.block / cfg.decim (SELENITE_RX_LENGTH_ERROR) */
    uint32_t bit_q8;          /* a bit in Q8 ticks, 8 * 256 .. 1024 * 256: every channel's `bit` after set_fskdec / reset */
    uint32_t reverse;         /* 0 / 1: the tones swapped (mark is the `space` filter) */
    uint32_t usos;            /* 0 / 1: unshift on space */
    uint32_t ring;            /* a power of two, 16 .. 65536: characters kept per channel */
    float mark[5];            /* {b0, b1, b2, a1, a2} in CMSIS's sign convention (selenite_rx_design_fsk); finite */
    float space[5];
    float alpha;              /* the followers' rate: finite, in (0, 1] */
    float hyst;               /* finite, in [0, 1) */
    float frac;               /* finite, in [0, 1] */
    float min_power;          /* finite, >= 0 */
    const uint8_t *table;     /* [64], copied; NULL selects the built-in ITA2 / US-TTY table (selenite_rx_design_ita2) */
} selenite_rx_fskdec_config;

/* The stage's whole state.  NULL members are skipped. */
typedef struct selenite_rx_fskdec_state_view {
    float *filt;              /* [channels][2][4]: mark then space, {x1, x2, y1, y2} each */
    float *em;                /* [channels] the three followers: mark, space (behind `reverse`), the whole band */
    float *es;
    float *ew;
    uint32_t *lvl;            /* [channels] 1 = mark = idle */
    uint32_t *k;              /* [channels] 0: idle; 1: in the start bit; 2 .. 6: before data bit k - 2; 7: before the stop bit */
    uint32_t *t_q8;           /* [channels] Q8 ticks since the start edge */
    uint32_t *shift;          /* [channels] the data bits so far, LSB first */
    uint32_t *figs;           /* [channels] 0 / 1: letters / figures */
    uint32_t *ferr;           /* [channels] framing errors since set_fskdec / reset */
    uint32_t *bit;            /* [channels] this channel's bit length, Q8 ticks */
    uint64_t *count;          /* [channels] characters emitted since set_fskdec / reset */
    uint8_t *text;            /* [channels][ring] */
} selenite_rx_fskdec_state_view;

typedef struct selenite_rx_instance selenite_rx_instance;  /* opaque; state lives in HBM */

/* ---- instance life cycle ------------------------------------------------------------- */

/* Mirrors arm_fir_decimate_init_f32 (FilteringFunctions/arm_fir_decimate_init_f32.c:63-101):
 * validates (block % decim != 0 -> SELENITE_RX_LENGTH_ERROR), clears all state.  Coefficient
 * arrays are copied to the device; the caller may free them afterwards.  Uses the calling
 * thread's current HIP device.  On failure *S is set to NULL. */
int  selenite_rx_init(selenite_rx_instance **S, const selenite_rx_config *cfg);
void selenite_rx_free(selenite_rx_instance *S);

/* Mirrors DSP_Set_Mode(uint8_t) (Core/Src/dsp_if.c:367-370).  Filter state is kept. */
int  selenite_rx_set_mode(selenite_rx_instance *S, uint8_t mode);

/* Sticky status of the instance: first error raised by a process call (they return void, as
 * their CMSIS counterparts do), or SELENITE_RX_SUCCESS. */
int  selenite_rx_status(const selenite_rx_instance *S);
/* Human-readable text for the last error of this thread / instance (never NULL). */
const char *selenite_rx_error_string(const selenite_rx_instance *S);

/* ---- the per-block process call ------------------------------------------------------- */

/* Host buffers, synchronous: the literal "float* I/Q in, float* audio out, blockSize" call of the slot.
 * blockSize = complex input samples per channel in this call; it must be a non-zero multiple of cfg.block
 * (several DSP blocks are processed back to back exactly as successive CMSIS calls would).  The call is cut into
 * channel chunks and pipelined over PCIe (H2D of chunk k+1 || kernels of chunk k || D2H of chunk k-1, two
 * device buffers each way, no allocation per call).  Page-locked caller memory (selenite_rx_host_alloc,
 * selenite_rx_host_register) is the DMA source / target itself; pageable memory is staged through the
 * library's pinned buffers by a few host threads.  Same bits as the _device call on the same data. */
void selenite_rx_process_f32(selenite_rx_instance *S, const float *pSrcIQ,
                             float *pDstAudio, uint32_t blockSize);

/* Page-locked host memory for the buffers of the host-pointer calls: allocate it, or register memory the caller
 * already owns (the firmware-side analogue is a DMA-capable buffer).  Optional: unregistered memory works, slower. */
void *selenite_rx_host_alloc(size_t bytes);
void  selenite_rx_host_free(void *hptr);
int   selenite_rx_host_register(void *hptr, size_t bytes);
int   selenite_rx_host_unregister(void *hptr);

/* Device buffers (HBM-resident), asynchronous on the instance's stream. */
void selenite_rx_process_f32_device(selenite_rx_instance *S, const float *dSrcIQ,
                                    float *dDstAudio, uint32_t blockSize);

/* int16 wire format of the slot (dsp_if.c:286-289): q15 in, q15 out; conversion is fused into
 * the kernels' load and store (arm_q15_to_float: /32768.0f; arm_float_to_q15: *32768.0f,
 * truncate, saturate). */
void selenite_rx_process_q15(selenite_rx_instance *S, const int16_t *pSrcIQ,
                             int16_t *pDstAudio, uint32_t blockSize);
void selenite_rx_process_q15_device(selenite_rx_instance *S, const int16_t *dSrcIQ,
                                    int16_t *dDstAudio, uint32_t blockSize);

/* Global-gain AGC (cfg.agc_global) split at the only cross-GPU exchange point:
 *   phase 1 runs the chain up to the un-scaled audio and leaves, per DSP block of this call,
 *           max|audio| over this instance's channels in dEnv[blockSize/cfg.block] (device);
 *   the caller all-reduces dEnv with MAX across ranks (RCCL) -- or not, single GPU;
 *   phase 2 runs the gain law on dEnv and scales dDstAudio in place.
 * selenite_rx_process_f32_device() on an agc_global instance = phase 1 + phase 2. */
void selenite_rx_global_phase1_device(selenite_rx_instance *S, const float *dSrcIQ,
                                      float *dDstAudio, float *dEnv, uint32_t blockSize);
void selenite_rx_global_phase2_device(selenite_rx_instance *S, float *dDstAudio,
                                      const float *dEnv, uint32_t blockSize);

/* The same in one call for a plain C host: phase 1, ncclAllReduce(ncclMax) of the blockSize / cfg.block envelopes
 * over `rccl_comm` (an ncclComm_t whose rank runs on this instance's device; NULL = single rank), phase 2, all
 * enqueued on the instance's stream.  RCCL is resolved at run time (no link dependency).  Returns the status. */
int selenite_rx_global_process_f32_device(selenite_rx_instance *S, const float *dSrcIQ, float *dDstAudio,
                                          uint32_t blockSize, void *rccl_comm);

/* ---- parity guard of the split-precision arithmetic (SELENITE_ARITH_SPLIT16 / _AUTO) -------------------------- */

/* A DSP block is GUARDED when max |audio| of the block (before the AGC) is below `ratio` x the largest |component| of the mixed
 * samples whose split-precision error can reach it: those its pass of the matrix product held (new samples and FIR history); for
 * the blocks that still read FIR-pair history of the pass before (the first nh_taps - 1 audio samples of a pass) also that pass's;
 * at a call's start also the level the call before left.  FM: guarded when min|z| x max|audio| is below `ratio` x that maximum (the
 * discriminator's error is |dz| / (pi |z|)).  Default ratio 0.25 (-12 dB); 0 disables the guard, +inf guards every block with
 * non-zero input (SELENITE_ARITH_AUTO then recomputes every channel bit-exactly: a test hook).  Takes effect with the next call.
 * SELENITE_ARITH_AUTO recomputes a channel that owns a guarded block with the bit-exact kernel, inside the same call, and then HOLDS
 * it there: the matrix kernel skips the channel in the following calls (a channel whose pass band is empty call after call costs
 * the bit-exact kernel's time, not both kernels') until two calls in a row show no block under 1.25 x ratio. */
int selenite_rx_set_guard_ratio(selenite_rx_instance *S, float ratio);
/* Counters since init / the last selenite_rx_guard_clear (any pointer may be NULL); drains the instance's stream:
 *   guard_blocks         DSP blocks guarded
 *   guard_channel_calls  (channel, process call) pairs with at least one guarded block
 *                        (SELENITE_ARITH_AUTO: plus every call of a channel the bit-exact kernel holds)
 *   rerun_channel_calls  (channel, call) pairs SELENITE_ARITH_AUTO computed with the bit-exact kernel (0 for _SPLIT16) */
int selenite_rx_guard_stats(selenite_rx_instance *S, uint64_t *guard_blocks, uint64_t *guard_channel_calls,
                            uint64_t *rerun_channel_calls);
/* per_channel[channels]: guarded DSP blocks of every channel since init / the last clear (sticky per-channel view). */
int selenite_rx_guard_channels(selenite_rx_instance *S, uint32_t *per_channel);
/* Diagnostic: per_channel[channels] = the word SELENITE_ARITH_AUTO keeps per channel (bit 0: recompute pending; bits 1-2: what the
 * call before left the streaming state as -- 0 exact, 1 matrix kernel with the samples for the repair, 2 without; bit 5: the channel is
 * HELD by the bit-exact kernel, bit 6: its last call there was clean; bits 8-31: level of the last pass).  Zeros in the other modes. */
int selenite_rx_auto_words(selenite_rx_instance *S, uint32_t *per_channel);
/* SELENITE_ARITH_AUTO across calls.  A channel the previous call left on the matrix kernel carries a FIR-pair history (the last
 * nh_taps - 1 decimated samples) of split16 precision; if THIS call has to be recomputed for it, its first blocks would start from
 * that history.  Handover repair (default ON): the matrix kernel also leaves the exact mixed samples in front of the decimator state
 * behind (decim * (nh_taps - 1) samples per channel and call, rounded up to whole quads of audio samples: 2 KB for the cfg3 chain;
 * two buffers -- 4 KB of device memory per channel, allocated by the first call that needs them and released when the repair is
 * switched off), and the recomputation derives the FIR-pair history from them in exact arithmetic first: a recomputed call is CMSIS
 * bit for bit from its first sample (apart from the gain the previous call's AGC left: ~1e-6 relative).  A call too short to hold
 * those samples (under nd_taps + decim * (nh_taps - 1) per channel: the firmware's literal one-slot callback) runs on the bit-exact
 * kernel in _AUTO, and the history is repaired in front of an AM call and in front of the CW / generic kernels -- so with the repair
 * ON no block ever starts from a history of split16 precision: selenite_rx_guard_handover stays 0 and the _AUTO guarantee is
 * unconditional.  Cost: those bytes (2 % of the headline at 4096 samples per call).
 * OFF (a diagnostic: what the repair is worth): nothing is kept; guarded blocks inside the reach of the history behind a call that
 * stayed on the matrix kernel carry the error of a guarded block of raw _SPLIT16 and are COUNTED (selenite_rx_guard_handover): */
int selenite_rx_set_handover_repair(selenite_rx_instance *S, int on);
/* SELENITE_ARITH_AUTO, where the recomputation runs.  launches = 1 (default): on the no-decimator shapes (k_hilb_split16: one channel per
 * workgroup) the workgroup that guarded a channel recomputes it itself, with the body of the bit-exact kernel -- one launch per call.
 * launches = 3: always in two launches behind the matrix kernel (a dense list of the channels; what the decimating shapes do anyway).
 * The RESULT does not depend on the choice: which arithmetic serves a channel is decided by the channel's word alone; both forms run
 * the same code on it and give the same bits (tests/test_gpu_auto_forms.py). */
int selenite_rx_set_auto_launches(selenite_rx_instance *S, int launches);
/* Diagnostic: the form the last SELENITE_ARITH_AUTO call on a matrix kernel took, 1 or 3 (0: none yet). */
int selenite_rx_auto_launches_last(const selenite_rx_instance *S);
int selenite_rx_guard_handover(selenite_rx_instance *S, uint64_t *handover_blocks);
int selenite_rx_guard_clear(selenite_rx_instance *S);

/* ---- streams, state, memory ----------------------------------------------------------- */

/* hipStream_t passed as void*; NULL = the library-owned stream created at init. */
int  selenite_rx_set_stream(selenite_rx_instance *S, void *hip_stream);
int  selenite_rx_sync(selenite_rx_instance *S);

int  selenite_rx_get_state(selenite_rx_instance *S, const selenite_rx_state_view *dst);
int  selenite_rx_set_state(selenite_rx_instance *S, const selenite_rx_state_view *src);
int  selenite_rx_reset(selenite_rx_instance *S);      /* state back to the post-init values (an NLMS stage: to its post-set_nr values) */

/* ---- NLMS noise reduction / automatic notch --------------------------------------------- */

/* Mirrors arm_lms_norm_init_f32 (FilteringFunctions/arm_lms_norm_init_f32.c:60-89) for every channel: weights = coeffs_init (or 0),
 * window, delay line, energy and x0 = 0.  nr == NULL or kind == SELENITE_RX_NR_OFF removes the stage.  A field out of range:
 * SELENITE_RX_ARGUMENT_ERROR, and the instance is left as it was.  selenite_rx_set_mode leaves the stage's state alone; every
 * process entry point (f32 and int16 slots, device and host pointers, the timing calls, global phase 1) runs it. */
int  selenite_rx_set_nr(selenite_rx_instance *S, const selenite_rx_nr_config *nr);
/* The stage's state (layouts: selenite_rx_nr_state_view).  SELENITE_RX_ARGUMENT_ERROR while the stage is off. */
int  selenite_rx_get_nr_state(selenite_rx_instance *S, const selenite_rx_nr_state_view *dst);
int  selenite_rx_set_nr_state(selenite_rx_instance *S, const selenite_rx_nr_state_view *src);

/* ---- audio output stage ------------------------------------------------------------------ */

/* Mirrors arm_fir_interpolate_init_f32 (FilteringFunctions/arm_fir_interpolate_init_f32.c:91-96) for every channel: ni_taps % interp != 0 is
 * a SELENITE_RX_LENGTH_ERROR, any other field out of range a SELENITE_RX_ARGUMENT_ERROR, and the instance is left as it was.  Clears the
 * stage's state and nothing else; out == NULL removes the stage.  selenite_rx_set_mode and selenite_rx_set_nr leave the stage alone,
 * selenite_rx_reset clears its state with the rest.  Every process entry point runs it (f32 and int16 slots, device and host pointers, the
 * timing calls, selenite_rx_global_process_f32_device behind phase 2); selenite_rx_global_phase1_device / _phase2_device exchange audio
 * at the decimated rate by contract: with a stage set they raise a sticky SELENITE_RX_ARGUMENT_ERROR and touch nothing. */
int      selenite_rx_set_out(selenite_rx_instance *S, const selenite_rx_out_config *out);
/* values per channel a process call of blockSize writes to pDstAudio (blockSize / decim without a stage) */
uint32_t selenite_rx_out_values(const selenite_rx_instance *S, uint32_t blockSize);
/* interp_state [channels][P - 1]: the last P - 1 audio samples, oldest first (arm_fir_interpolate_f32.c:433-475 copy-back order).
 * SELENITE_RX_ARGUMENT_ERROR while the stage is off, or with P <= 1 (nothing to keep). */
int      selenite_rx_get_out_state(selenite_rx_instance *S, float *interp_state);
int      selenite_rx_set_out_state(selenite_rx_instance *S, const float *interp_state);

/* ---- spectrum tap ------------------------------------------------------------------------ */

/* Sets the tap for every channel (selenite_rx_spec_config), or removes it (sp == NULL).  Clears the tap's state and nothing else.  A bad
 * field (fft_len: SELENITE_RX_LENGTH_ERROR, any other: SELENITE_RX_ARGUMENT_ERROR) leaves the instance as it was, a working tap included.
 * selenite_rx_set_mode, _set_nr and _set_out leave the tap alone; selenite_rx_reset clears rows, pending and position.  Every process
 * entry point that has input runs it once per call (f32 and int16 slots, device and host pointers, the timing calls, global phase 1 --
 * not phase 2).  With the tap off no launch, byte or output of any call changes. */
int selenite_rx_set_spectrum(selenite_rx_instance *S, const selenite_rx_spec_config *sp);
/* Host copy of the rows [channels][fft_len] (the state after the last transformed frame so far; +0.0f before the first) and the number
 * of frames transformed since set_spectrum / reset; either pointer may be NULL.  Drains the instance's stream.
 * SELENITE_RX_ARGUMENT_ERROR while the tap is off. */
int selenite_rx_get_spectrum(selenite_rx_instance *S, float *rows, uint64_t *frames);
/* The row buffer itself (device memory, [channels][fft_len]), for a consumer on the instance's stream; valid until the next
 * selenite_rx_set_spectrum / selenite_rx_free.  NULL while the tap is off. */
const float *selenite_rx_spectrum_device(const selenite_rx_instance *S);
int selenite_rx_get_spectrum_state(selenite_rx_instance *S, const selenite_rx_spec_state_view *dst);   /* SELENITE_RX_ARGUMENT_ERROR while off */
int selenite_rx_set_spectrum_state(selenite_rx_instance *S, const selenite_rx_spec_state_view *src);
/* Host only, no device: the table the kernel uses, tw[fft_len][2] = (cos, sin)(2 pi i / fft_len) -- twiddleCoef_64 / twiddleCoef_512
 * (CommonTables/arm_common_tables.c) entry for entry: each is the float of the nine-decimal rendering of the double value. */
int selenite_rx_spectrum_twiddles(float *tw, uint32_t fft_len);

/* ---- impulse noise blanker --------------------------------------------------------------- */

/* Sets the blanker for every channel (selenite_rx_nb_config), or removes it (nb == NULL).  Clears the blanker's state and nothing else.  A
 * bad field (frame: SELENITE_RX_LENGTH_ERROR, any other: SELENITE_RX_ARGUMENT_ERROR) leaves the instance as it was, a working blanker
 * included.  selenite_rx_set_mode, _set_nr, _set_out and _set_spectrum leave it alone; selenite_rx_reset returns level and both counters to
 * zero.  Every process entry point that has input runs it once per call (f32 and int16 slots, device and host pointers, the timing calls,
 * global phase 1, selenite_rx_global_process_f32_device -- not phase 2, not the roof timing calls).  The blanked copy lives in a buffer of
 * the instance, grown by the first call that needs it.  With the blanker off no launch, byte, allocation or output of any call changes. */
int selenite_rx_set_nb(selenite_rx_instance *S, const selenite_rx_nb_config *nb);
/* Host copies of the state.  Drains the instance's stream.  SELENITE_RX_ARGUMENT_ERROR while the blanker is off. */
int selenite_rx_get_nb_state(selenite_rx_instance *S, const selenite_rx_nb_state_view *dst);
int selenite_rx_set_nb_state(selenite_rx_instance *S, const selenite_rx_nb_state_view *src);

/* ---- I/Q correction ---------------------------------------------------------------------- */

/* Sets the I/Q correction for every channel (selenite_rx_iqc_config), or removes it (iqc == NULL).  Sets the stage's state to the config's
 * inits and touches nothing else.  A bad field (frame: SELENITE_RX_LENGTH_ERROR, any other: SELENITE_RX_ARGUMENT_ERROR) leaves the
 * instance as it was, a working stage included.  SELENITE_RX_DEVICE_ERROR is different: the old stage is released before the new state
 * rows are allocated, so a failed allocation leaves the instance with NO stage (as after iqc == NULL), its chain untouched.
 * selenite_rx_set_mode, _set_nr, _set_out, _set_spectrum and _set_nb leave it alone;
 * selenite_rx_reset returns the four floats to their inits and held to zero.  Every process entry point that has input runs it once per
 * call, in front of the noise blanker (f32 and int16 slots, device and host pointers, the timing calls, global phase 1,
 * selenite_rx_global_process_f32_device -- not phase 2, not the roof timing calls).  The corrected copy lives in a buffer of the instance,
 * grown by the first call that needs it.  With the stage off no launch, byte, allocation or output of any call changes. */
int selenite_rx_set_iqc(selenite_rx_instance *S, const selenite_rx_iqc_config *iqc);
/* Host copies of the state.  Drains the instance's stream.  SELENITE_RX_ARGUMENT_ERROR while the stage is off. */
int selenite_rx_get_iqc_state(selenite_rx_instance *S, const selenite_rx_iqc_state_view *dst);
int selenite_rx_set_iqc_state(selenite_rx_instance *S, const selenite_rx_iqc_state_view *src);

/* ---- signal-level meter and squelch ------------------------------------------------------- */

/* Sets the meter for every channel (selenite_rx_meter_config), or removes it (m == NULL).  Sets the stage's state to level_init, closed,
 * counters zero, and touches nothing else.  A bad field (SELENITE_RX_ARGUMENT_ERROR) leaves the instance as it was, a working stage
 * included.  SELENITE_RX_DEVICE_ERROR is different: the old stage is released before the new state rows are allocated, so a failed
 * allocation leaves the instance with NO stage (as after m == NULL), its chain untouched.  selenite_rx_set_mode, _set_nr, _set_out,
 * _set_spectrum, _set_nb and _set_iqc leave it alone; selenite_rx_reset returns it to its state after set_meter.  Every process entry
 * point runs it once per call (f32 and int16 slots, device and host pointers, the timing calls, selenite_rx_global_process_f32_device;
 * the split pair: the meter in global phase 1, the gate in phase 2, from the gate bytes phase 1 left in a buffer of the instance).  With
 * the stage on, the fused kernels run with their own AGC off and the generic AGC kernel finishes the call, as with NLMS.  With the stage
 * off no launch, byte, allocation or output of any call changes. */
int selenite_rx_set_meter(selenite_rx_instance *S, const selenite_rx_meter_config *m);
/* Host copies of the state.  Drains the instance's stream.  SELENITE_RX_ARGUMENT_ERROR while the stage is off. */
int selenite_rx_get_meter_state(selenite_rx_instance *S, const selenite_rx_meter_state_view *dst);
int selenite_rx_set_meter_state(selenite_rx_instance *S, const selenite_rx_meter_state_view *src);
/* The level and open rows themselves (device memory, [channels] each), for a consumer on the instance's stream; valid until the next
 * selenite_rx_set_meter / selenite_rx_free.  NULL while the stage is off. */
const float *selenite_rx_meter_level_device(const selenite_rx_instance *S);
const uint32_t *selenite_rx_meter_open_device(const selenite_rx_instance *S);

/* ---- audio biquad filter ------------------------------------------------------------------ */

/* Sets the filter for every channel (selenite_rx_afilt_config), or removes it and releases its buffers (f == NULL).  Clears the stage's
 * state to +0.0f and touches nothing else.  A bad field (SELENITE_RX_ARGUMENT_ERROR: n_stages out of range, per_channel not 0 / 1, NULL
 * or non-finite coeffs, a wrong struct_size, reserved != 0) leaves the instance as it was, a working stage included.
 * SELENITE_RX_DEVICE_ERROR is different: the old stage is released before the new rows are allocated, so a failed allocation leaves the
 * instance with NO stage (as after f == NULL), its chain untouched.  selenite_rx_set_mode, _set_nr, _set_meter, _set_out, _set_spectrum,
 * _set_nb and _set_iqc leave it alone; selenite_rx_reset clears the state and keeps the coefficients.  Every process entry point runs it
 * once per call (f32 and int16 slots, device and host pointers, the timing calls, global phase 1, selenite_rx_global_process_f32_device
 * -- not phase 2).  With the stage on, the fused kernels run with their own AGC off and the generic AGC kernel finishes the call, as with
 * NLMS.  With the stage off no launch, byte, allocation or output of any call changes. */
int selenite_rx_set_afilt(selenite_rx_instance *S, const selenite_rx_afilt_config *f);
/* Replaces the coefficient rows of channels first_channel .. first_channel + n_channels - 1 (coeffs [n_channels][n_stages][5], finite)
 * and leaves the state alone: a notch is retuned while the user listens, without the click of a cleared delay line.  Ordered on the
 * instance's stream: calls issued before it run with the old rows, calls issued after it with the new ones; the caller may free coeffs
 * on return.  per_channel == 0: the only valid range is (0, 1).  SELENITE_RX_ARGUMENT_ERROR (stage off, range out of bounds, NULL or
 * non-finite coeffs) leaves the stage as it was. */
int selenite_rx_set_afilt_coeffs(selenite_rx_instance *S, uint32_t first_channel, uint32_t n_channels, const float *coeffs);
/* Host copies of the state (and, get only, the coefficients).  Drains the instance's stream.  SELENITE_RX_ARGUMENT_ERROR while the stage
 * is off. */
int selenite_rx_get_afilt_state(selenite_rx_instance *S, const selenite_rx_afilt_state_view *dst);
int selenite_rx_set_afilt_state(selenite_rx_instance *S, const selenite_rx_afilt_state_view *src);

/* ---- tone-detector bank ----------------------------------------------------------------------- */

/* Sets the bank for every channel (selenite_rx_tones_config), or removes it and releases its buffers (f == NULL).  Puts the stage's state
 * at its start and touches nothing else.  A bad field (SELENITE_RX_ARGUMENT_ERROR: n_tones, frame_blocks, confirm or release out of range,
 * a frame of 2^31 samples or more, ratio outside [0, 1], min_power negative, either not finite, NULL or non-finite coeffs, a wrong
 * struct_size, reserved != 0) leaves the instance as it was, a working stage included.  SELENITE_RX_DEVICE_ERROR is different: the old
 * stage is released before the new rows are allocated, so a failed allocation leaves the instance with NO stage (as after f == NULL).
 * selenite_rx_set_mode and every other setter leave it alone; selenite_rx_reset returns it to its state after set_tones and keeps the
 * table.  Every process entry point runs it once per call (f32 and int16 slots, device and host pointers, the timing calls, global phase
 * 1, selenite_rx_global_process_f32_device -- not phase 2).  With the stage on, the fused kernels run with their own AGC off and the
 * generic AGC kernel finishes the call, as with NLMS.  With the stage off no launch, byte, allocation or output of any call changes. */
int selenite_rx_set_tones(selenite_rx_instance *S, const selenite_rx_tones_config *f);
/* Host copies of the state.  Drain the instance's stream.  SELENITE_RX_ARGUMENT_ERROR while the stage is off. */
int selenite_rx_get_tones_state(selenite_rx_instance *S, const selenite_rx_tones_state_view *dst);
int selenite_rx_set_tones_state(selenite_rx_instance *S, const selenite_rx_tones_state_view *src);
/* Host copies of what a reader wants: tone [channels], power [channels][n_tones] of the last whole frame, frames = position /
 * frame_blocks (whole frames since set_tones / reset).  NULL arguments are skipped.  Drains the instance's stream.
 * SELENITE_RX_ARGUMENT_ERROR while the stage is off. */
int selenite_rx_get_tones(selenite_rx_instance *S, uint32_t *tone, float *power, uint64_t *frames);
/* The rows on the device, readable on the instance's stream behind a call (a tone-squelch gate will read `tone`); NULL while the stage is
 * off; valid until the next selenite_rx_set_tones or selenite_rx_free. */
const uint32_t *selenite_rx_tones_tone_device(const selenite_rx_instance *S);
const float *selenite_rx_tones_power_device(const selenite_rx_instance *S);

/* Morse decoder (the law: selenite_rx_cwdec_config above).  f == NULL removes the stage and releases its buffers.  Puts the stage's state
 * at its start.  Drains the instance's stream first.  SELENITE_RX_ARGUMENT_ERROR (a field outside its range as the struct states them, a
 * wrong struct_size) leaves the instance as it was, a working stage included.  SELENITE_RX_DEVICE_ERROR is different: the old stage is
 * released before the new rows are allocated, so a failed allocation leaves the instance with NO stage (as after f == NULL).
 * selenite_rx_set_mode and every other setter leave it alone; selenite_rx_reset returns it to its state after set_cwdec and keeps the
 * parameters and the table.  Every process entry point runs it once per call (f32 and int16 slots, device and host pointers, the timing
 * calls, global phase 1, selenite_rx_global_process_f32_device -- not phase 2); the state rows of a channel chunk of a host-pointer call
 * move with its first channel.  With the stage on, the fused kernels run with their own AGC off and the generic AGC kernel finishes the
 * call, as with NLMS.  With the stage off no launch, byte, allocation or output of any call changes. */
int selenite_rx_set_cwdec(selenite_rx_instance *S, const selenite_rx_cwdec_config *f);
/* Host copies of the state.  Drain the instance's stream.  SELENITE_RX_ARGUMENT_ERROR while the stage is off. */
int selenite_rx_get_cwdec_state(selenite_rx_instance *S, const selenite_rx_cwdec_state_view *dst);
int selenite_rx_set_cwdec_state(selenite_rx_instance *S, const selenite_rx_cwdec_state_view *src);
/* Host copies of what a reader wants: text [channels][ring], count, unit, key [channels].  Character i of a channel (i < count, i >=
 * count - ring) is text[i % ring].  NULL arguments are skipped.  Drains the instance's stream.  SELENITE_RX_ARGUMENT_ERROR while the
 * stage is off. */
int selenite_rx_get_cwdec(selenite_rx_instance *S, uint8_t *text, uint64_t *count, uint32_t *unit, uint32_t *key);
/* The rows on the device, readable on the instance's stream behind a call; NULL while the stage is off; valid until the next
 * selenite_rx_set_cwdec or selenite_rx_free. */
const uint8_t *selenite_rx_cwdec_text_device(const selenite_rx_instance *S);
const uint64_t *selenite_rx_cwdec_count_device(const selenite_rx_instance *S);
const uint32_t *selenite_rx_cwdec_unit_device(const selenite_rx_instance *S);

/* FSK teleprinter decoder (the law: selenite_rx_fskdec_config above).  f == NULL removes the stage and releases its buffers.  Puts the
 * stage's state at its start.  Drains the instance's stream first.  SELENITE_RX_ARGUMENT_ERROR (a field outside its range as the struct
 * states them, a wrong struct_size) and SELENITE_RX_LENGTH_ERROR (tick does not divide cfg.block / cfg.decim) leave the instance as it
 * was, a working stage included.  SELENITE_RX_DEVICE_ERROR is different: the old stage is released before the new rows are allocated, so a
 * failed allocation leaves the instance with NO stage (as after f == NULL).  selenite_rx_set_mode and every other setter leave it alone;
 * selenite_rx_reset returns it to its state after set_fskdec and keeps the parameters and the table.  Every process entry point runs it
 * once per call (f32 and int16 slots, device and host pointers, the timing calls, global phase 1, selenite_rx_global_process_f32_device
 * -- not phase 2); the state rows of a channel chunk of a host-pointer call move with its first channel.  With the stage on, the fused
 * kernels run with their own AGC off and the generic AGC kernel finishes the call, as with NLMS.  With the stage off no launch, byte,
 * allocation or output of any call changes. */
int selenite_rx_set_fskdec(selenite_rx_instance *S, const selenite_rx_fskdec_config *f);
/* Host copies of the state.  Drain the instance's stream.  SELENITE_RX_ARGUMENT_ERROR while the stage is off. */
int selenite_rx_get_fskdec_state(selenite_rx_instance *S, const selenite_rx_fskdec_state_view *dst);
int selenite_rx_set_fskdec_state(selenite_rx_instance *S, const selenite_rx_fskdec_state_view *src);
/* Host copies of what a reader wants: text [channels][ring], count, ferr, lvl [channels].  Character i of a channel (i < count, i >=
 * count - ring) is text[i % ring].  NULL arguments are skipped.  Drains the instance's stream.  SELENITE_RX_ARGUMENT_ERROR while the
 * stage is off. */
int selenite_rx_get_fskdec(selenite_rx_instance *S, uint8_t *text, uint64_t *count, uint32_t *ferr, uint32_t *lvl);
/* The rows on the device, readable on the instance's stream behind a call; NULL while the stage is off; valid until the next
 * selenite_rx_set_fskdec or selenite_rx_free. */
const uint8_t *selenite_rx_fskdec_text_device(const selenite_rx_instance *S);
const uint64_t *selenite_rx_fskdec_count_device(const selenite_rx_instance *S);
const uint32_t *selenite_rx_fskdec_lvl_device(const selenite_rx_instance *S);

void *selenite_rx_device_alloc(size_t bytes);          /* hipMalloc; NULL on failure */
void  selenite_rx_device_free(void *dptr);
int   selenite_rx_memcpy_h2d(void *dptr, const void *hptr, size_t bytes);
int   selenite_rx_memcpy_d2h(void *hptr, const void *dptr, size_t bytes);
int   selenite_rx_device_count(void);                  /* number of HIP devices, 0 if none */
int   selenite_rx_set_device(int ordinal);             /* hipSetDevice for the calling thread */

/* ---- measurement support (bench.py) -------------------------------------- */

/* Synthetic I/Q of SURVEY.md 8d: per channel 3 complex tones + uniform noise, integer phase
 * accumulators and table-lerp sin/cos only, so host and device produce identical bits.
 * Fills iq[nch][nsamp][2] for channels first_channel .. first_channel+nch-1 and samples
 * first_sample .. first_sample+nsamp-1. */
void selenite_rx_synth_iq_host(float *iq, uint32_t first_channel, uint32_t nch,
                               uint64_t first_sample, uint32_t nsamp, uint64_t seed);
int  selenite_rx_synth_iq_device(selenite_rx_instance *S, float *dIQ, uint32_t first_channel,
                                 uint32_t nch, uint64_t first_sample, uint32_t nsamp,
                                 uint64_t seed);

/* Runs `iters` back-to-back process_f32_device calls bracketed by HIP events recorded on the
 * instance's stream; returns the mean milliseconds per call in *ms_per_call (state advances
 * as in normal streaming).  This is the live per-launch duration bench.py reports. */
int  selenite_rx_time_process_device(selenite_rx_instance *S, const float *dSrcIQ,
                                     float *dDstAudio, uint32_t blockSize, uint32_t iters,
                                     float *ms_per_call);
/* The same over the int16 slot format (selenite_rx_process_q15_device calls). */
int  selenite_rx_time_process_q15_device(selenite_rx_instance *S, const int16_t *dSrcIQ,
                                         int16_t *dDstAudio, uint32_t blockSize, uint32_t iters,
                                         float *ms_per_call);

/* The same with a HIP event between consecutive calls: ms_each[iters] receives the duration of every call (SURVEY.md 8d asks
 * for the median of >= 20 launches).  q15 != 0: the buffers are the int16 slot format.  The extra events cost a little
 * overlap between consecutive launches; bench.py reports both this median and the plain mean above. */
int  selenite_rx_time_process_each_device(selenite_rx_instance *S, const void *dSrcIQ, void *dDstAudio, uint32_t blockSize,
                                          uint32_t iters, float *ms_each, int q15);
/* The streaming roof of THIS instance's call, measured: `iters` launches of a kernel that moves exactly the algorithmic bytes of one
 * process call of blockSize samples (input in, audio out, per-channel state in and out -- a scratch copy, the instance's
 * state is not touched) with the access pattern of the fused kernels (persistent single-wave workgroups, 1 KB non-temporal wave loads,
 * next pass prefetched) and NO arithmetic; ms_each[iters] receives the per-launch durations.  dDstAudio is overwritten with junk.
 * bench.py reports the DSP kernels as a fraction of this floor beside the fraction of the nominal 8 TB/s. */
int  selenite_rx_time_streaming_roof_device(selenite_rx_instance *S, const void *dSrcIQ, void *dDstAudio, uint32_t blockSize,
                                            uint32_t iters, float *ms_each, int q15);
/* The same for the shapes of the systolic CW kernel (k_cw_fused: CW / CWR, no FIR stages, 2 / 4 / 8 biquad sections, DSP blocks of 128 / 256 /
 * 512), whose fetch pattern is its own: one wavefront streams 64 / n_biquad channel rows at once, 1 KB of a row per load.  The kernel timed here
 * issues exactly those bursts and stores (same descriptors, same number of bursts in flight, same residency) and `work` dependent vector
 * instructions per chunk where the biquad steps are -- 0: what the pattern alone costs.  Other configurations: SELENITE_RX_ARGUMENT_ERROR. */
int  selenite_rx_time_pattern_roof_device(selenite_rx_instance *S, const void *dSrcIQ, void *dDstAudio, uint32_t blockSize,
                                          uint32_t iters, float *ms_each, int q15, uint32_t work);

/* ---- kernel-selection overrides (tests, diagnosis) -------------------------------------
 * Process-wide words, NOT configuration: results never depend on them.  The test suite uses them to reach every product path (the generic
 * per-stage kernels, the NCO flavours, both grids of SELENITE_ARITH_AUTO's rerun pass).  Read by selenite_rx_init / selenite_tx_init when an
 * instance is planned (SELENITE_RX_OPT_RERUN_GRID: by every rerun launch).  The library reads no environment variable for any of this; its
 * only environment setting is SELENITE_RX_HOST_CHUNK_MB (chunk of the host-pointer pipeline, default 32). */
#define SELENITE_RX_OPT_FORCE_GENERIC     0   /* 1: RX instances created from now on use the generic per-stage kernels only */
#define SELENITE_RX_OPT_NO_SHARED_LO      1   /* 1: per-channel NCO in the kernel even when all channels share step and phase */
#define SELENITE_RX_OPT_NO_PERIODIC_LO    2   /* 1: a shared LO always as a per-call table, never a 256-sample period in registers (RX and TX) */
#define SELENITE_RX_OPT_RERUN_GRID        3   /* workgroups of SELENITE_ARITH_AUTO's rerun pass (1 .. 2^20); 0: sized from the last call's list */
#define SELENITE_RX_OPT_TX_FORCE_GENERIC  4   /* 1: TX instances created from now on use the generic kernels only */
#define SELENITE_RX_OPT_CW_GRID           5   /* workgroups of the systolic CW kernel (each takes the channel groups b, b + grid, ...; 1 .. 2^20);
                                               * 0: one per group, or a whole share of groups each where they divide evenly over the device */
#define SELENITE_RX_OPT_COUNT             6
int      selenite_rx_set_plan_option(int option, uint32_t value);   /* SELENITE_RX_ARGUMENT_ERROR: unknown option / value out of range */
uint32_t selenite_rx_get_plan_option(int option);
/* PCI bus id ("0000:05:00.0") of HIP device `ordinal` into buf; bench.py lists the devices of the ranks with it. */
int  selenite_rx_device_pci_bus_id(int ordinal, char *buf, size_t len);

/* Name of the kernel variant process_f32_device dispatches to for this instance
 * (e.g. "rx_ssb_fused<256,4,63>" or "generic"); for logs and profiles. */
const char *selenite_rx_kernel_name(const selenite_rx_instance *S);
/* How the NCO of the next call is served: "off", "per-channel arm_sin/cos_f32 in the kernel" (steps or phases differ
 * between channels: arm_sin_f32.c:72-119 per sample), "shared LO table per call" (one step, one phase: the table is
 * computed once per call with the same arm_sin/cos arithmetic), or "shared LO, period 256 samples, held in registers"
 * (same table; a step that is a multiple of 2^24 repeats it every 256 samples).  All three give identical results. */
const char *selenite_rx_nco_path(const selenite_rx_instance *S);

/* Algorithmic HBM bytes of one process call (SURVEY.md 8d formula):
 *   channels * (8*blockSize + 4*blockSize/decim + S_in + S_out).
 * read_bytes (optional) receives the read-only part 8*blockSize + S_in per channel. */
uint64_t selenite_rx_algorithmic_bytes(const selenite_rx_config *cfg, uint32_t blockSize,
                                       uint64_t *read_bytes);

/* ---- coefficient design helpers (host only, double precision -> float) ------------------ */
/* All write CMSIS coefficient order.  They are conveniences for callers and tests; the chain
 * itself only ever sees the arrays in selenite_rx_config. */

/* Hamming-windowed sinc low-pass, unity DC gain; cutoff as a fraction of the INPUT sample rate. */
int selenite_rx_design_lowpass(float *coeffs, uint32_t num_taps, double cutoff);
/* Hamming-windowed type-III Hilbert transformer (odd num_taps) and its matched delay
 * (unit impulse at (num_taps-1)/2). */
int selenite_rx_design_hilbert(float *hilb, float *delay, uint32_t num_taps);
/* n_stages identical RBJ constant-peak band-pass sections centred on f0 (fraction of the
 * sample rate) with quality factor q; coefficients in CMSIS sign convention (+a1, +a2). */
int selenite_rx_design_bandpass(float *coeffs, uint32_t n_stages, double f0, double q);

/* The interpolation low-pass of the output stage: selenite_rx_design_lowpass(ni_taps, cutoff) times `interp` (the pass-band level survives
 * the zero stuffing); cutoff as a fraction of the OUTPUT sample rate; interp 1, 2, 4 or 8 dividing ni_taps. */
int selenite_rx_design_interp(float *coeffs, uint32_t ni_taps, uint32_t interp, double cutoff);

/* A window for the spectrum tap, periodic form over n points (n >= 2): SELENITE_RX_WINDOW_HANN 0.5 - 0.5 cos(2 pi i / n), or
 * SELENITE_RX_WINDOW_BLACKMAN_HARRIS (four terms, -92 dB side lobes). */
int selenite_rx_design_window(float *w, uint32_t n, int kind);

/* One RBJ cookbook section for the audio filter stage, in CMSIS order and sign {b0, b1, b2, -a1, -a2} / a0: w = 2 pi f0 (0 < f0 < 0.5
 * cycles per sample), alpha = sin w / (2 q) (q > 0), A = 10^(gain_db / 40) (SELENITE_RX_BIQUAD_PEAKING only; finite).  Computed in double,
 * rounded once. */
#define SELENITE_RX_BIQUAD_NOTCH    0
#define SELENITE_RX_BIQUAD_PEAKING  1
#define SELENITE_RX_BIQUAD_LOWPASS  2
#define SELENITE_RX_BIQUAD_HIGHPASS 3
int selenite_rx_design_biquad(float coeffs[5], int kind, double f0, double q, double gain_db);
/* FM de-emphasis, one pole: p = exp(-1 / tau_samples) (tau_samples > 0: the time constant in samples of the audio rate, 75 us at 12 kHz
 * is 0.9), {1 - p, 0, 0, p, 0}: unity gain at DC. */
int selenite_rx_design_deemphasis(float coeffs[5], double tau_samples);

/* The tone table of the tone-detector bank: coeffs [n_tones][3] = {2 cos w, cos w, sin w}, w = 2 pi freq[k], 0 < freq[k] < 0.5 cycles per
 * sample of the audio rate.  Host only; computed in double, rounded once. */
int selenite_rx_design_tones(float *coeffs, const double *freq, uint32_t n_tones);
/* The 50 standard CTCSS frequencies in Hz, ascending, 67.0 .. 254.1; returns 50. */
uint32_t selenite_rx_ctcss_hz(double hz[50]);

/* The Morse decoder's table: index = the element pattern behind a leading 1, dit 0, dah 1, first element highest (`.-` is 0b101 = 5).
 * A-Z, 0-9, . (.-.-.-) , (--..--) ? (..--..) / (-..-.) = (-...-) + (.-.-.) - (-....-) @ (.--.-.); every other index, 0 (the overflow
 * character) included, is `unknown`.  Host only. */
int selenite_rx_design_morse(uint8_t table[256], uint8_t unknown);

/* The FSK decoder's tone filters: two constant-peak-gain band-pass sections, one at f_mark and one at f_space (cycles per audio sample, in
 * (0, 0.5)), each `bandwidth` wide (cycles per audio sample, > 0): w = 2 pi f0, alpha = sin w / (2 f0 / bandwidth),
 * {alpha, 0, -alpha, 2 cos w, -(1 - alpha)} / (1 + alpha) in CMSIS's sign convention ({b0, b1, b2, a1, a2}); double arithmetic, rounded
 * once.  SELENITE_RX_ARGUMENT_ERROR for a NULL pointer or an argument that is not finite or outside its range.  Host only. */
int selenite_rx_design_fsk(double f_mark, double f_space, double bandwidth, float mark[5], float space[5]);
/* The FSK decoder's built-in table, ITA2 with the US-TTY figures: table[code] the letter, table[32 + code] the figure of the 5-bit code
 * (bit 0 sent first); 0 where a code prints nothing (NUL, LTRS, FIGS); CR, LF, BEL (7) and the blank as themselves.  Host only. */
int selenite_rx_design_ita2(uint8_t table[64]);

int selenite_rx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SELENITE_RX_H */
