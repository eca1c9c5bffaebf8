/* selenite_chan.h -- C-ABI of the polyphase channeliser (DESIGN.md section 2 "in front of the batch", section 5.14).
 *
 * One wideband I/Q stream per "band" goes in; K = fft_len channels per band come out, each 1/K of the band wide and decimated by
 * D = K / oversample, in the layout selenite_rx_process_f32_device reads: pSrcIQ [channels][blockSize][2] with channels = bands * n_bins.
 * The reference firmware has no channeliser (it has one receiver); the stage is build-defined, as a composition of the reference's
 * CMSIS-DSP 1.5.3 primitives, matched bit for bit (citations relative to Drivers/CMSIS/DSP/Source):
 *
 *   int16 input        arm_q15_to_float   SupportFunctions/arm_q15_to_float.c:87            (float)x / 32768.0f
 *   branch filters     arm_dot_prod_f32   BasicMathFunctions/arm_dot_prod_f32.c             acc = +0.0f; acc = acc + a * b, product rounded, then the sum
 *   transform          arm_cfft_f32       TransformFunctions/arm_cfft_f32.c:562-616         (&arm_cfft_sR_f32_lenK, v, 0, 1): forward, natural order
 *                                         = arm_radix8_butterfly_f32 (arm_cfft_radix8_f32.c:45-285) + arm_bitreversal_32
 *
 * A weighted-overlap-add analysis bank.  position counts the wideband samples per band since init / reset (one value for all bands, always
 * a multiple of D); samples in front of the stream are +0.0f.  A call brings blockSize samples per band, a non-zero multiple of D, and
 * produces nout = blockSize / D samples per channel.  Output m of the call works on the K * P newest samples that end at stream index
 * position + (m + 1) * D - 1, oldest first, s[0 .. K * P - 1] (P = taps_per_branch):
 *
 *   for r = 0 .. K - 1, each rail (I, Q) on its own:     arm_dot_prod_f32 over the P gathered pairs
 *       acc = +0.0f;  for t = 0 .. P - 1 ascending:  acc = acc + g[r + t * K] * s[r + t * K]
 *       v[(r + n0) mod K] = (accI, accQ),   n0 = (position + (m + 1) * D) mod K          (0, or K / 2 and 0 in turn with oversample 2)
 *   arm_cfft_f32(&arm_cfft_sR_f32_lenK, v, 0, 1)
 *   channel (band b, bin k), sample m = v[k]
 *
 * Every operation is rounded to f32, nothing is contracted, denormals are kept.  The rotation by n0 ties every channel's LO to the absolute
 * sample index: channel k is x[n] * e^(-2 pi i k n / K), filtered by h (g[j] = h[K * P - 1 - j]: CMSIS coefficient order) and decimated by
 * D, however the stream is cut into calls.  A tone exactly on bin k leaves channel k as a constant; bin k > K / 2 is the frequency k - K.
 *
 * Output is always f32: dst[(b * n_bins + i)][m][2], where bins[i] is the bin of output row i (bins == NULL: all K in natural order).
 * Non-finite input passes through as the arithmetic gives it; the object has no NANINF status.
 *
 * State: history [bands][K * P - D][2] f32, oldest first (int16 input is stored converted), +0.0f after init and reset; position.
 *
 * Status codes are selenite_rx.h's: 0 success, -1 argument, -2 length, -7 device.  Device pointers only: selenite_rx_memcpy_* moves host data.
 */
#ifndef SELENITE_CHAN_H_
#define SELENITE_CHAN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct selenite_chan selenite_chan;

/* The most bands one object takes: a band is a workgroup of 64 threads in the main kernel's grid x, and a launch holds fewer than 2^32
 * threads per dimension.  (Memory ends far sooner: the two history buffers of that many bands are 200 GB at K = 64, P = 4.) */
#define SELENITE_CHAN_MAX_BANDS 0x3FFFFFFu

typedef struct {
    uint32_t struct_size;      /* sizeof(selenite_chan_config): the struct's own growth path */
    uint32_t bands;            /* wideband streams, 1 .. SELENITE_CHAN_MAX_BANDS, and bands * n_bins < 2^32 */
    uint32_t fft_len;          /* K: 64 or 512 (the pure radix-8 lengths of arm_cfft_f32) */
    uint32_t oversample;       /* 1: critically sampled (D = K); 2: D = K / 2, adjacent channels overlap */
    uint32_t taps_per_branch;  /* P: 4, 8, 12 or 16 */
    uint32_t n_bins;           /* output rows per band; with bins == NULL it must be K */
    uint32_t reserved;         /* 0 */
    const float *coeffs;       /* g[K * P], CMSIS order, finite; copied */
    const uint32_t *bins;      /* [n_bins], each < K, any order, duplicates allowed; or NULL; copied */
} selenite_chan_config;

/* Host-side view of the state (arrays owned by the caller); NULL members are skipped. */
typedef struct {
    float    *history;         /* [bands][K * P - D][2] */
    uint64_t *position;        /* [1] */
} selenite_chan_state_view;

/* Validates first, then touches the device.  fft_len: LENGTH_ERROR; any other field, or a non-finite tap: ARGUMENT_ERROR; no device:
 * DEVICE_ERROR.  On failure *Ch = NULL. */
int  selenite_chan_init(selenite_chan **Ch, const selenite_chan_config *cfg);
void selenite_chan_free(selenite_chan *Ch);
int  selenite_chan_status(const selenite_chan *Ch);           /* sticky; 0 = ok */
const char *selenite_chan_error_string(const selenite_chan *Ch);
int  selenite_chan_set_stream(selenite_chan *Ch, void *hip_stream);   /* NULL: the object's own stream */
int  selenite_chan_sync(selenite_chan *Ch);
int  selenite_chan_reset(selenite_chan *Ch);                  /* history +0.0f, position 0; the sticky status is kept */
int  selenite_chan_get_state(selenite_chan *Ch, const selenite_chan_state_view *view);
int  selenite_chan_set_state(selenite_chan *Ch, const selenite_chan_state_view *view);   /* position must be a multiple of D */
uint32_t selenite_chan_out_channels(const selenite_chan *Ch);            /* bands * n_bins (0 for NULL) */
uint32_t selenite_chan_out_len(const selenite_chan *Ch, uint32_t blockSize);   /* blockSize / D, or 0 where the call would be refused */

/* dSrc [bands][blockSize][2] (f32, or int16 through arm_q15_to_float), dDst [bands * n_bins][blockSize / D][2] f32; asynchronous on the
 * object's stream.  blockSize that is zero or no multiple of D: sticky SELENITE_RX_LENGTH_ERROR, nothing written. */
void selenite_chan_process_f32_device(selenite_chan *Ch, const float *dSrc, float *dDst, uint32_t blockSize);
void selenite_chan_process_q15_device(selenite_chan *Ch, const int16_t *dSrc, float *dDst, uint32_t blockSize);

/* Host only: a prototype whose pass band is `width` channel spacings wide (0 < width <= 2):
 * selenite_rx_design_lowpass(coeffs, fft_len * taps_per_branch, 0.5 * width / fft_len). */
int  selenite_chan_design_prototype(float *coeffs, uint32_t fft_len, uint32_t taps_per_branch, double width);

#ifdef __cplusplus
}
#endif
#endif /* SELENITE_CHAN_H_ */
