/* selenite_tx_cw.h -- the keyed CW transmit path of the TX chain (shaped keying, pitch offset, sidetone, break-in flag): part of the C-ABI
 * of selenite_tx.h, which includes this file (include that one).  Kept in a file of its own as selenite_tx_fm.h is; selenite_tx_config
 * does not change, and the audio entries keep serving SELENITE_MODE_CW / _CWR as the SSB modulator they are.
 */
#ifndef SELENITE_TX_CW_H
#define SELENITE_TX_CW_H

#include <stdint.h>

#include "selenite_tx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- keyed CW [build-defined] (DESIGN.md section 2 "TX CW keyed", section 5.17) ----
 * The reference has the key (KEY_DIT / KEY_DAH, the DTR line "works like external telegraph key", Core/Src/rxtx_if.c:332-350, 752-780),
 * the break-in timeout (KEY_TIMEOUT, rxtx_if.h:109) and the place of the sidetone (Core/Src/dsp_if.c:218) but no keyer DSP; what is
 * specified here is composed of CMSIS-DSP 1.5.3 primitives only, per channel, every float operation rounded to f32, no contraction:
 *
 *   key[n]  uint8 [channels][blockSize]; non-zero = key down
 *   e0[n] = key[n] ? 1.0f : +0.0f
 *   e[n]  = arm_fir_f32(shape_coeffs, ns_taps)(e0)          pState tail = the last ns_taps - 1 key values
 *   a[n]  = e[n] * amplitude                                 arm_scale_f32
 *   u[m]  = arm_fir_interpolate_f32(interp_coeffs, L)(a)     the instance's interpolator and the I rail of interp_state; L = 1: u = a
 *   x = (float)(nco_phase >> 8) * 0x1.921fb6p-22f;  out[m] = (arm_cos_f32(x) * u[m], arm_sin_f32(x) * u[m]);  nco_phase += step_eff
 *   step_eff = (nco_enable ? nco_step[c] : 0) + offset_step in SELENITE_MODE_CW, - offset_step in SELENITE_MODE_CWR (mod 2^32)
 *   int16 I/Q: arm_float_to_q15 under cfg.q15_rounding
 *
 * With offset_step = selenite_tx_tone_step(pitch, fs_out) the carrier lands where the audio entries in CW (upper sideband) put a tone of
 * that pitch, in CWR where the lower sideband puts it; nco_enable = 0 gives a zero-IF tone at +-pitch.  The products of the shaping FIR
 * are exact (e0 is 0 or 1): e[n] is the same in every arithmetic mode; the interpolator follows cfg.arith (SPLIT16 runs as FMA).
 *
 * Sidetone (the speaker mix of dsp_if.c:218), at the audio rate, phase side_phase[c] of its own:
 *   xs = (float)(side_phase >> 8) * 0x1.921fb6p-22f;  s = arm_sin_f32(xs);  g = e[n] * side_level;  y = s * g;  side_phase += side_step
 *   f32:   side_mix = 0: dst[n] = y;  side_mix = 1: dst[n] = dst[n] + y                                   (arm_add_f32)
 *   int16: q = arm_float_to_q15(y) (cfg.q15_rounding);  side_mix = 0: dst[n] = q;  side_mix = 1: dst[n] = arm_add_q15(dst[n], q)
 * A NULL sidetone destination writes nothing; side_phase advances all the same.
 *
 * Break-in flag (KEY_TIMEOUT semi break-in), per DSP block of cfg.block key samples; a readout for the T/R switch, it gates nothing:
 *   if (any key[n] != 0) { tx_on = 1; hold = hang_blocks; }  else if (tx_on) { if (hold == 0) tx_on = 0; else hold -= 1; }
 *
 * The path shares nco_phase and the I rail of interp_state with the audio entries; ALC and alc_gain, fir_state and the FM state are
 * untouched, the Q rail of interp_state takes blockSize samples of +0.0f as in FM.  After a keyed call every channel's phase is its own.
 * The process entries are valid while the mode is SELENITE_MODE_CW or _CWR and return the status code: ARGUMENT_ERROR before
 * selenite_tx_set_cw or in another mode, LENGTH_ERROR for a blockSize that is not a non-zero multiple of cfg.block or a layout over the
 * kernel's LDS budget.  A refused call writes nothing. */
typedef struct {
    uint32_t struct_size;        /* sizeof(selenite_tx_cw_config) */
    uint32_t ns_taps;            /* >= 1 */
    const float *shape_coeffs;   /* [ns_taps], CMSIS order, finite; copied */
    float    amplitude;          /* finite */
    uint32_t offset_step;        /* per OUTPUT sample */
    float    side_level;         /* finite */
    uint32_t side_step_all;      /* per AUDIO sample, used when side_step is NULL */
    const uint32_t *side_step;   /* [channels] or NULL; copied */
    uint32_t side_mix;           /* 0 store, 1 add */
    uint32_t hang_blocks;
    uint32_t reserved;           /* 0 */
} selenite_tx_cw_config;
typedef struct {
    uint8_t  *key_state;         /* [channels][ns_taps-1], 0/1, oldest first */
    uint32_t *side_phase, *tx_on, *hold;   /* [channels] each; NULL members are skipped */
} selenite_tx_cw_state_view;

/* NULL: keyed CW off again (allowed in any mode).  The first call (and the first after NULL) clears key_state, side_phase, tx_on and hold,
 * and so does selenite_tx_reset; a further call retunes and keeps them, except that a changed ns_taps clears key_state.  ARGUMENT_ERROR
 * (the previous setting stays) for a wrong struct_size, ns_taps = 0, a NULL or non-finite shape, non-finite amplitude or side_level,
 * side_mix > 1 or reserved != 0.  selenite_tx_set_mode keeps all state. */
int selenite_tx_set_cw(selenite_tx_instance *S, const selenite_tx_cw_config *cfg);
int selenite_tx_get_cw_state(selenite_tx_instance *S, const selenite_tx_cw_state_view *view);
int selenite_tx_set_cw_state(selenite_tx_instance *S, const selenite_tx_cw_state_view *view);   /* non-zero key_state bytes count as 1 */
/* device buffers (asynchronous on the instance's stream); dSide [channels][blockSize] or NULL */
int selenite_tx_process_key_f32_device(selenite_tx_instance *S, const uint8_t *dKey, float *dDstIQ, float *dSide, uint32_t blockSize);
int selenite_tx_process_key_q15_device(selenite_tx_instance *S, const uint8_t *dKey, int16_t *dDstIQ, int16_t *dSide, uint32_t blockSize);
/* host buffers (copied in and out, synchronous); with side_mix = 1 the sidetone buffer is copied in first */
int selenite_tx_process_key_f32(selenite_tx_instance *S, const uint8_t *pKey, float *pDstIQ, float *pSide, uint32_t blockSize);
int selenite_tx_process_key_q15(selenite_tx_instance *S, const uint8_t *pKey, int16_t *pDstIQ, int16_t *pSide, uint32_t blockSize);
const uint32_t *selenite_tx_cw_txon_device(selenite_tx_instance *S);   /* [channels] on the device; NULL before selenite_tx_set_cw */
/* mean milliseconds per process_key_f32_device call over `iters` calls (HIP events on the stream) */
int selenite_tx_time_process_key_device(selenite_tx_instance *S, const uint8_t *dKey, float *dDstIQ, float *dSide, uint32_t blockSize,
                                        uint32_t iters, float *ms_per_call);
/* Hann window w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (ns_taps + 1)) normalised to sum 1 in double, rounded once: the step response is a
 * raised-cosine edge of ns_taps samples; ns_taps = 1 gives {1.0f} (hard keying).  Host-only. */
int selenite_tx_design_keyshape(uint32_t ns_taps, float *coeffs);

#ifdef __cplusplus
}
#endif
#endif /* SELENITE_TX_CW_H */
