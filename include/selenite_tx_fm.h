/* selenite_tx_fm.h -- the FM transmit mode of the TX chain, with a CTCSS tone encoder: part of the C-ABI of selenite_tx.h, which includes
 * this file (include that one).  Kept in a file of its own as the other stages added after ABI version 2 keep theirs apart
 * (selenite_chan.h, selenite_comb.h); selenite_tx_config does not change.
 */
#ifndef SELENITE_TX_FM_H
#define SELENITE_TX_FM_H

#include <stdint.h>

#include "selenite_tx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- FM transmit mode with a CTCSS tone encoder [build-defined] (DESIGN.md section 2 "TX FM") ----
 * FM is off until selenite_tx_set_fm has been called: until then selenite_tx_set_mode(S, SELENITE_MODE_FM) returns ARGUMENT_ERROR and keeps
 * the mode; selenite_tx_init with mode = FM stays ARGUMENT_ERROR.  In FM mode the instance's nco_phase[c] is the modulator's phase
 * accumulator -- it exists and advances with nco_enable = 0 too (zero-IF FM), is cleared by selenite_tx_reset and read / written by
 * selenite_tx_get_state / selenite_tx_set_state as in every mode.  v = (u[n] + tone) * deviation = 1 is a deviation of half the output
 * rate: the RX chain's FM demodulator (angle(z[n] conj z[n-1]) / pi) gives v back.  |v| >= 1 saturates in arm_float_to_q31; there is no
 * limiter in front of it.  A NaN sample gives d = 0.  The arithmetic of the FM tail is the same in every arith mode; the filters in front
 * of it follow cfg.arith (SPLIT16 runs as FMA).  All four process entries and selenite_tx_time_process_device serve FM. */
typedef struct {
    uint32_t struct_size;      /* sizeof(selenite_tx_fm_config) */
    float    deviation;        /* finite, > 0 */
    float    amplitude;        /* finite */
    uint32_t tone_enable;      /* 0 / 1 */
    float    tone_level;       /* finite */
    uint32_t tone_step_all;    /* per OUTPUT sample, used when tone_step is NULL */
    const uint32_t *tone_step; /* [channels] or NULL; copied */
    uint32_t reserved;         /* 0 */
} selenite_tx_fm_config;
typedef struct { uint32_t *tone_phase; /* [channels] */ } selenite_tx_fm_state_view;

/* ARGUMENT_ERROR (the previous setting stays in place) for a wrong struct_size, non-finite values, deviation <= 0, tone_enable > 1 or
 * reserved != 0.  The first call (and the first after FM was switched off) clears tone_phase, and so does selenite_tx_reset; a further call
 * retunes -- deviation, amplitude, tone -- and keeps tone_phase.  selenite_tx_set_mode between FM and the other modes keeps all state. */
int selenite_tx_set_fm(selenite_tx_instance *S, const selenite_tx_fm_config *cfg);   /* NULL: FM off again; ARGUMENT_ERROR (nothing changed) while the mode is FM */
int selenite_tx_get_fm_state(selenite_tx_instance *S, const selenite_tx_fm_state_view *view);
int selenite_tx_set_fm_state(selenite_tx_instance *S, const selenite_tx_fm_state_view *view);
uint32_t selenite_tx_tone_step(double hz, double fs_out);   /* round(hz / fs_out * 2^32), double, once; host-only, beside the selenite_rx_design_* helpers */

#ifdef __cplusplus
}
#endif
#endif /* SELENITE_TX_FM_H */
