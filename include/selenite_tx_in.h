/* selenite_tx_in.h -- the audio input stage of the TX chain (slot-rate L/R frames in; pick, mic gain, decimator, VOX; then the chain): part of
 * the C-ABI of selenite_tx.h, which includes this file (include that one).  Kept in a file of its own as selenite_tx_fm.h and
 * selenite_tx_cw.h are; selenite_tx_config and selenite_tx_state_view do not change, and the audio and key entries stay as they are.
 */
#ifndef SELENITE_TX_IN_H
#define SELENITE_TX_IN_H

#include <stdint.h>

#include "selenite_tx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- TX input [build-defined] (DESIGN.md section 2 "TX input", section 5.18) ----
 * What produces transmit audio delivers interleaved left / right frames at the slot rate: the codec microphone path in TX
 * (DSP_In_Buff_Write, Core/Src/dsp_if.c:250-301, pbuf[k] = left, pbuf[k + 1] = right), the USB audio-out path (DSP_Out_Buff_Write,
 * dsp_if.c:116-180) and this library's own RX output stage (selenite_rx_set_out).  The reference has no TX decimator; what is specified
 * here is composed of CMSIS-DSP 1.5.3 primitives only, per channel, every float operation rounded to f32, no contraction in ANY arith mode
 * (the rule of the RX output stage), denormals kept:
 *
 *   frames  [channels][blockSize * M * (pick == MONO ? 1 : 2)]  f32 or int16; blockSize counts AUDIO samples, as everywhere in selenite_tx.h
 *   int16:  x = arm_q15_to_float(frame words)                    SupportFunctions/arm_q15_to_float.c:87, 113: (float)w / 32768.0f
 *   pick:   MONO s[i] = x[i];  LEFT s[i] = x[2i];  RIGHT s[i] = x[2i + 1]
 *           MIX  s[i] = (x[2i] + x[2i + 1]) * 0.5f               BasicMathFunctions/arm_add_f32.c:61-134, arm_scale_f32.c:77-153
 *   g[i]  = s[i] * gain                                          arm_scale_f32.c:148 (the mic gain; 1.0f leaves the bits alone)
 *   a[n]  = arm_fir_decimate_f32(M, nd_taps, coeffs)(g)          FilteringFunctions/arm_fir_decimate_f32.c:129-508: with
 *                                                                st = {the last nd_taps - 1 values of g before the call, oldest first} ++ g,
 *                                                                a[n] = sum over k = 0 .. nd_taps - 1, ascending, of st[n M + k] * coeffs[k],
 *                                                                one accumulator from +0.0f, the product rounded, then the sum rounded;
 *                                                                M == 1 && nd_taps == 0: a = g, no FIR
 *   VOX, per DSP block of cfg.block samples of a (f32, in front of the gate and of any int16 conversion):
 *           the law of selenite_rx_meter_config (include/selenite_rx.h) with sense ABOVE, word for word:
 *           pw = arm_power_f32(a, block)                         StatisticsFunctions/arm_power_f32.c:64-125: sum = +0.0f; sum = sum + in * in
 *           ms = pw / (float)block                               correctly rounded division
 *           ms <= FLT_MAX (false for NaN):  r = ms > level ? attack : decay;  d = ms - level;  level = level + r * d
 *           otherwise:                      level stays
 *           want_open = level > open_level;  want_close = level < close_level
 *           if (!open)           { if (want_open) { open = 1; hold = hang; opens += 1; } }
 *           else if (want_close) { if (hold == 0) open = 0; else hold -= 1; }
 *           else                   hold = hang;
 *           open_blocks += open
 *   gate == 1: a block whose `open` is 0 AFTER its update enters the chain as +0.0f; gate == 0: flag only
 *   f32 I/Q entries:   the rest of the call is selenite_tx_process_f32_device on a, bit for bit
 *   int16 I/Q entry:   q = arm_float_to_q15(a) under cfg.q15_rounding (SupportFunctions/arm_float_to_q15.c:117 / :90-101); the rest of the
 *                      call is selenite_tx_process_q15_device on q, bit for bit
 *
 * The stage is valid in every mode the audio entries serve: SSB, AM, DIG / PKT, CW / CWR as the SSB modulator they are, FM after
 * selenite_tx_set_fm.  An audio call or a keyed call between two frame calls touches none of the stage's state. */
#define SELENITE_TX_IN_MONO  0
#define SELENITE_TX_IN_LEFT  1
#define SELENITE_TX_IN_RIGHT 2
#define SELENITE_TX_IN_MIX   3
typedef struct {
    uint32_t struct_size;        /* sizeof(selenite_tx_in_config) */
    uint32_t M;                  /* 1, 2, 4 or 8 */
    uint32_t nd_taps;            /* 1 .. 256; 0 only with M = 1 (no FIR) */
    uint32_t pick;               /* SELENITE_TX_IN_* */
    const float *coeffs;         /* [nd_taps], CMSIS order (pCoeffs of arm_fir_decimate_f32), finite; copied */
    float    gain;               /* finite */
    uint32_t vox;                /* 0 off, 1 on */
    selenite_rx_meter_config meter;   /* read when vox = 1: the meter's own validity rules, sense = SELENITE_RX_SQ_ABOVE */
    uint32_t reserved;           /* 0 */
} selenite_tx_in_config;
typedef struct {
    float    *dec_state;         /* [channels][nd_taps-1], oldest first */
    float    *level;             /* [channels] each; NULL members are skipped */
    uint32_t *open, *hold;
    uint64_t *opens, *open_blocks;
} selenite_tx_in_state_view;

/* NULL: the stage off again.  The first call (and the first after NULL) clears dec_state and sets the VOX state to level_init, closed,
 * counters 0, and so does selenite_tx_reset; a further call retunes and keeps them, except that a changed nd_taps clears dec_state.
 * ARGUMENT_ERROR (the previous setting stays) for a wrong struct_size, M not 1 / 2 / 4 / 8, nd_taps > 256, nd_taps = 0 with M > 1, a NULL
 * or non-finite coeffs, pick > 3, a non-finite gain, vox > 1, with vox = 1 anything selenite_rx_set_meter refuses or a sense other than
 * ABOVE, or reserved != 0.  With vox = 0 the VOX words stay where they are and nothing is gated.  selenite_tx_set_mode keeps all state. */
int selenite_tx_set_in(selenite_tx_instance *S, const selenite_tx_in_config *cfg);
int selenite_tx_get_in_state(selenite_tx_instance *S, const selenite_tx_in_state_view *view);
int selenite_tx_set_in_state(selenite_tx_instance *S, const selenite_tx_in_state_view *view);
/* The process entries return the status code: ARGUMENT_ERROR before selenite_tx_set_in or for a NULL buffer, LENGTH_ERROR for a blockSize
 * that is not a non-zero multiple of cfg.block or a layout over a kernel's LDS budget.  A refused call writes nothing and moves no state.
 * device buffers (asynchronous on the instance's stream): */
int selenite_tx_process_frames_f32_device(selenite_tx_instance *S, const float *dFrames, float *dDstIQ, uint32_t blockSize);
int selenite_tx_process_frames_q15_device(selenite_tx_instance *S, const int16_t *dFrames, int16_t *dDstIQ, uint32_t blockSize);
/* int16 frames -> f32 I/Q: from a codec to selenite_comb, which takes f32 rows */
int selenite_tx_process_frames_q15_f32_device(selenite_tx_instance *S, const int16_t *dFrames, float *dDstIQ, uint32_t blockSize);
/* host buffers (copied in and out, synchronous) */
int selenite_tx_process_frames_f32(selenite_tx_instance *S, const float *pFrames, float *pDstIQ, uint32_t blockSize);
int selenite_tx_process_frames_q15(selenite_tx_instance *S, const int16_t *pFrames, int16_t *pDstIQ, uint32_t blockSize);
/* open[channels] on the device, for the T/R switch; NULL before selenite_tx_set_in */
const uint32_t *selenite_tx_in_vox_device(selenite_tx_instance *S);
/* the instance-owned device buffer [channels][blockSize] holding the stage's output of the last frame call -- a (f32) or q (int16), in the
 * entry's audio type, behind the gate: a monitor tap.  NULL before the first frame call; a later, longer call may move it. */
const void *selenite_tx_in_audio_device(selenite_tx_instance *S);
/* mean milliseconds of the stage kernel alone over `iters` launches (HIP events on the stream); kind selects the entry's types.  The
 * launches are real ones, and one more precedes the timed span: the stage's state moves as `iters + 1` frame calls would move it; the
 * chain behind the stage does not run. */
#define SELENITE_TX_IN_F32     0   /* f32 frames, f32 audio */
#define SELENITE_TX_IN_Q15     1   /* int16 frames, int16 audio */
#define SELENITE_TX_IN_Q15_F32 2   /* int16 frames, f32 audio */
int selenite_tx_time_in_stage_device(selenite_tx_instance *S, const void *dFrames, uint32_t kind, uint32_t blockSize, uint32_t iters,
                                     float *ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* SELENITE_TX_IN_H */
