// tx_internal.h -- kernel parameter blocks and launch interfaces of the TX kernels' files (tx_generic.hip, tx_fused.hip, tx_fm.hip,
// tx_cw.hip, tx_in.hip, tx_keyer.hip), as tx_api.hip and the stages' host sides call them.
// Not part of the C-ABI (include/selenite_tx.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/selenite_tx.h"
#include "rx_device.h"

namespace srx {

struct TxParams {
    uint32_t channels, block, L, ni, P, nh, mode, nco, alc, block_size;
    uint32_t q15_round;    // int16 output: 1 = the ARM_MATH_ROUNDING build of arm_float_to_q15 (selenite_tx_config::q15_rounding)
    uint32_t lo_period;    // shared LO: 256 when it repeats every 256 output samples (NCO step a multiple of 2^24), else 0
    const float *ic, *hc, *dc, *sintab;
    const uint32_t *step;
    uint32_t *phase;
    float *fir_state;      // [C][2][nh-1]
    float *int_state;      // [C][2][P-1]
    float *gain;
    AgcParams alcp;
};

// tx_generic.hip: k_tx_generic<ARITH, TIn, TOut>, any shape whose layout fits the LDS
size_t tx_lds_bytes(const TxParams &p);
hipError_t launch_tx_generic(const TxParams &p, int arith, const void *src, bool q15, void *dst, hipStream_t st);

// tx_fused.hip: the BASELINE-like shape (tx_select.h: tx_fused_ok).  `nco` = the flavour the decision names (TxDecision::nco);
// `lo` = shared LO of the call as produced by launch_lo_table (cos, -sin), read by flavours 2 and 3.
hipError_t launch_tx_fused(const TxParams &p, int arith, uint32_t nco, uint32_t delay_idx, const float2 *lo, const void *src, bool q15,
                           void *dst, hipStream_t st);

// SELENITE_ARITH_SPLIT16: the interpolator on the 16-bit matrix pipe (k_tx_split16), same shape as the fused kernel
hipError_t build_tx_split16_table(const float *interp_coeffs, void **d_table, int *tap_sc);
hipError_t launch_tx_split16(const TxParams &p, uint32_t nco, uint32_t delay_idx, const float2 *lo, const void *ttab16, int tap_sc,
                             const void *src, bool q15, void *dst, hipStream_t st);

// tx_fm.hip: SELENITE_MODE_FM (selenite_tx_set_fm).  k_tx_fm<ARITH, TIn, TOut>: any shape k_tx_generic serves, one single-wave
// workgroup per channel; p.phase is read and written whatever p.nco says (the phase accumulator is the modulator)
struct TxFmParams {
    float deviation, amplitude, tone_level;
    uint32_t tone_on;
    const uint32_t *tone_step;     // [C]
    uint32_t *tone_phase;          // [C]
};
size_t tx_fm_lds_bytes(const TxParams &p);
hipError_t launch_tx_fm(const TxParams &p, const TxFmParams &f, int arith, const void *src, bool q15, void *dst, hipStream_t st);

// tx_cw.hip: the keyed CW path (selenite_tx_set_cw, include/selenite_tx_cw.h).  k_tx_cw<ARITH, TOut, SIDE>: key bytes in, I/Q out, one
// single-wave workgroup per channel; of TxParams it reads the shape (channels, block, L, ni, P, block_size), nco, q15_round, ic, sintab,
// step, phase and int_state; p.phase is read and written whatever p.nco says
struct TxCwParams {
    uint32_t ns;                   // shape taps
    const float *shape;            // [ns] on the device
    float shape_sum;               // the taps summed in order from +0.0f: e[n] of a window that is all key-down
    float amplitude, side_level;
    uint32_t offset;               // + offset_step (CW) or - offset_step (CWR), modulo 2^32
    uint32_t side_mix, hang_blocks;
    const uint32_t *side_step;     // [C]
    uint32_t *side_phase, *tx_on, *hold;   // [C]
    uint8_t *key_state;            // [C][ns-1]
};
size_t tx_cw_lds_bytes(const TxParams &p, const TxCwParams &w);
hipError_t launch_tx_cw(const TxParams &p, const TxCwParams &w, int arith, const uint8_t *key, bool q15, void *dst, void *side, hipStream_t st);

// tx_in.hip: the audio input stage (selenite_tx_set_in, include/selenite_tx_in.h).  k_tx_in<M, PICK, TIn, TOut>: slot-rate frames in, the
// chain's audio out, one single-wave workgroup per channel row; no arith mode (nothing is contracted)
struct TxInParams {
    uint32_t channels, block, block_size;          // DSP block and call length in AUDIO samples (the stage's outputs)
    uint32_t M, nt, pick;
    uint32_t vox, gate, hang, q15_round;
    float gain, attack, decay, open_level, close_level;
    const float *coeffs;                           // [nt] on the device
    float *dec_state;                              // [C][nt-1]
    float *level;                                  // [C]
    uint32_t *open, *hold;                         // [C]
    uint64_t *opens, *open_blocks;                 // [C]
};
uint32_t tx_in_tile(const TxInParams &q);          // outputs of a tile: a whole number of DSP blocks
size_t tx_in_lds_bytes(const TxInParams &q);       // the sum in 64 bits
hipError_t launch_tx_in(const TxInParams &q, const void *frames, bool in_q15, void *audio, bool out_q15, hipStream_t st);

// tx_keyer.hip: the keyer stage (selenite_tx_set_keyer, include/selenite_tx_keyer.h).  k_tx_keyer: paddle bytes (or NULL) and the text
// memory in, key bytes out, one single-wave workgroup per channel; integers only, no arith mode
struct TxKeyerParams {
    uint32_t channels, block_size;                 // the call length in AUDIO samples
    uint32_t mode, ring;
    const uint32_t *unit;                          // [C]
    const uint8_t *codes;                          // [256]
    const uint8_t *text;                           // [C][ring]
    uint32_t *state;                               // [11][C]: phase, left, last, dit_mem, dah_mem, squeeze, code, tgap, tail, head, skipped
};
hipError_t launch_tx_keyer(const TxKeyerParams &q, const uint8_t *paddles, uint8_t *key, hipStream_t st);

}  // namespace srx
