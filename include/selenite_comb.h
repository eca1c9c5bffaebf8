/* selenite_comb.h -- C-ABI of the polyphase combiner (synthesis bank; DESIGN.md section 2 "behind the TX batch", section 5.15).
 *
 * The mirror image of the channeliser (selenite_chan.h): K = fft_len narrow-band TX channels per "band" go in, in the layout
 * selenite_tx_process_f32_device writes -- dSrc [bands * n_bins][nin][2] f32, nin = blockSize >= 1 samples per channel row -- and one
 * wideband I/Q stream per band comes out, interpolated by D = K / oversample: dDst [bands][nin * D][2], f32 or int16.  The reference
 * firmware has no combiner (it has one transmitter); the stage is build-defined, as a composition of the reference's CMSIS-DSP 1.5.3
 * primitives, matched bit for bit (citations relative to Drivers/CMSIS/DSP/Source):
 *
 *   transform          arm_cfft_f32       TransformFunctions/arm_cfft_f32.c:562-616         (&arm_cfft_sR_f32_lenK, v, 1, 1): inverse, natural order
 *                                         = imag negated (:571-580); arm_radix8_butterfly_f32 (arm_cfft_radix8_f32.c:45-285);
 *                                           arm_bitreversal_32; re = re * invL, im = (-im) * invL, invL = 1.0f / (float)K (:604-615)
 *   branch filters     arm_dot_prod_f32   BasicMathFunctions/arm_dot_prod_f32.c             acc = +0.0f; acc = acc + a * b, product rounded, then the sum
 *   int16 output       arm_float_to_q15   SupportFunctions/arm_float_to_q15.c:117           (q15_rounding 0: truncates) / :90-101 (1: ARM_MATH_ROUNDING);
 *                                                                                           both saturate
 *
 * A weighted-overlap-add synthesis bank.  P = taps_per_branch; Q = P * oversample frames overlap in one output sample.  Row i of band b feeds
 * bin bins[i] (bins == NULL: all K bins in natural order, n_bins = K); bins are distinct; a bin nobody feeds is +0.0f.  position counts the
 * wideband output samples per band since init / reset (one value for all bands), always f * D for the absolute frame index f.  Per input
 * frame f:
 *
 *   v[k] = (I, Q) of the row feeding bin k at frame f, else (+0.0f, +0.0f)
 *   arm_cfft_f32(&arm_cfft_sR_f32_lenK, v, 1, 1)
 *   u_f[0 .. K - 1] = v
 *
 *   for j = 0 .. D - 1:   n = f * D + j (absolute output index),  p = n mod K
 *       each rail (I, Q) on its own, arm_dot_prod_f32 over Q pairs:
 *       acc = +0.0f;  for t = 0 .. Q - 1 ascending:  acc = acc + g[(D - 1 - j) + t * D] * u_{f - Q + 1 + t}[p]
 *       out[n] = (accI, accQ)                          frames in front of the stream are +0.0f
 *
 * Every operation is rounded to f32, nothing is contracted, denormals are kept.  g is in CMSIS order, g[i] = h[K * P - 1 - i], as the
 * channeliser has it.  In float64 terms out[n] = (1 / K) sum_k e^(+2 pi i k n / K) sum_m c_k[m] h[n - m D]: every channel is interpolated by D
 * through h and mixed up to bin k by an LO tied to the absolute sample index, however the stream is cut into calls.  The 1 / K is
 * arm_cfft_f32's own: selenite_comb_design_prototype returns the channeliser's unity-DC-gain design scaled by K * D, so that a constant on
 * channel 0 leaves as that constant.  Non-finite input passes through as the arithmetic gives it; the object has no NANINF status.
 *
 * Supported: Q <= 16, i.e. P in {4, 8, 12, 16} with oversample 1 and P in {4, 8} with oversample 2 (the kernel keeps the Q newest frames of
 * its eight time-domain positions in registers).
 *
 * State: history [bands * n_bins][Q - 1][2] f32, the last Q - 1 INPUT samples of every row, oldest first, +0.0f after init and reset (their
 * transforms are recomputed: the transform is deterministic, so the bits are the same); position.
 *
 * Status codes are selenite_rx.h's: 0 success, -1 argument, -2 length, -7 device.  Device pointers only: selenite_rx_memcpy_* moves host data.
 */
#ifndef SELENITE_COMB_H_
#define SELENITE_COMB_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct selenite_comb selenite_comb;

/* The most bands one object takes: a band is a workgroup of 64 threads in the main kernel's grid x, and a launch holds fewer than 2^32
 * threads per dimension (as SELENITE_CHAN_MAX_BANDS). */
#define SELENITE_COMB_MAX_BANDS 0x3FFFFFFu

typedef struct {
    uint32_t struct_size;      /* sizeof(selenite_comb_config): the struct's own growth path */
    uint32_t bands;            /* wideband streams, 1 .. SELENITE_COMB_MAX_BANDS, and bands * n_bins < 2^32 */
    uint32_t fft_len;          /* K: 64 or 512 (the pure radix-8 lengths of arm_cfft_f32) */
    uint32_t oversample;       /* 1: critically sampled (D = K); 2: D = K / 2 */
    uint32_t taps_per_branch;  /* P: 4, 8, 12 or 16 with oversample 1; 4 or 8 with oversample 2 (P * oversample <= 16) */
    uint32_t n_bins;           /* input rows per band, 1 .. K; with bins == NULL it must be K */
    uint32_t q15_rounding;     /* int16 output: 0 truncates, 1 rounds (ARM_MATH_ROUNDING), as selenite_tx_config has it */
    uint32_t reserved;         /* 0 */
    const float *coeffs;       /* g[K * P], CMSIS order, finite; copied */
    const uint32_t *bins;      /* [n_bins], each < K, distinct, any order; or NULL; copied */
} selenite_comb_config;

/* Host-side view of the state (arrays owned by the caller); NULL members are skipped. */
typedef struct {
    float    *history;         /* [bands * n_bins][Q - 1][2] */
    uint64_t *position;        /* [1] */
} selenite_comb_state_view;

/* Validates first, then touches the device.  fft_len: LENGTH_ERROR; any other field, an unsupported (P, oversample), a non-finite tap, a bin
 * >= K or two equal bins: ARGUMENT_ERROR; no device: DEVICE_ERROR.  On failure *Cb = NULL. */
int  selenite_comb_init(selenite_comb **Cb, const selenite_comb_config *cfg);
void selenite_comb_free(selenite_comb *Cb);
int  selenite_comb_status(const selenite_comb *Cb);           /* sticky; 0 = ok */
const char *selenite_comb_error_string(const selenite_comb *Cb);
int  selenite_comb_set_stream(selenite_comb *Cb, void *hip_stream);   /* NULL: the object's own stream */
int  selenite_comb_sync(selenite_comb *Cb);
int  selenite_comb_reset(selenite_comb *Cb);                  /* history +0.0f, position 0; the sticky status is kept */
int  selenite_comb_get_state(selenite_comb *Cb, const selenite_comb_state_view *view);
int  selenite_comb_set_state(selenite_comb *Cb, const selenite_comb_state_view *view);   /* position must be a multiple of D */
uint32_t selenite_comb_in_channels(const selenite_comb *Cb);             /* bands * n_bins (0 for NULL) */
uint32_t selenite_comb_out_len(const selenite_comb *Cb, uint32_t blockSize);   /* blockSize * D, or 0 where the call would be refused */

/* dSrc [bands * n_bins][blockSize][2] f32, dDst [bands][blockSize * D][2] (f32, or int16 through arm_float_to_q15); asynchronous on the
 * object's stream.  blockSize that is zero or longer than a launch takes: sticky SELENITE_RX_LENGTH_ERROR, nothing launched, nothing written. */
void selenite_comb_process_f32_device(selenite_comb *Cb, const float *dSrc, float *dDst, uint32_t blockSize);
void selenite_comb_process_q15_device(selenite_comb *Cb, const float *dSrc, int16_t *dDst, uint32_t blockSize);

/* Host only: the channeliser's prototype of the same arguments (selenite_chan_design_prototype: pass band `width` channel spacings wide,
 * 0 < width <= 2, unity DC gain), each tap times K * D in double, then rounded.  The oversample it needs for D is the fifth argument. */
int  selenite_comb_design_prototype(float *coeffs, uint32_t fft_len, uint32_t taps_per_branch, double width, uint32_t oversample);

#ifdef __cplusplus
}
#endif
#endif /* SELENITE_COMB_H_ */
