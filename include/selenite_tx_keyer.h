/* selenite_tx_keyer.h -- the keyer stage in front of the keyed CW path (iambic paddles, straight key, a Morse text memory per channel):
 * part of the C-ABI of selenite_tx.h, which includes this file (include that one).  Kept in a file of its own as selenite_tx_cw.h and
 * selenite_tx_in.h are; the keyed path behind it (selenite_tx_cw.h) does not change: the stage writes the key bytes it reads.
 */
#ifndef SELENITE_TX_KEYER_H
#define SELENITE_TX_KEYER_H

#include <stdint.h>

#include "selenite_tx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the keyer [build-defined] (DESIGN.md section 2 "TX keyer", section 5.20) ----
 * The reference has the pins (KEY_DIT_Pin, KEY_DAH_Pin, Core/Src/rxtx_if.c:747-780; the DTR line "works like external telegraph key",
 * rxtx_if.c:330-350) and no keyer.  The law is integers only and the same in every arithmetic mode.  Per channel, u = the channel's unit
 * (audio samples per dit), the state words phase (0 IDLE, 1 MARK, 2 GAP), left (samples left in the phase), last (0 dit, 1 dah), dit_mem,
 * dah_mem, squeeze, code (the elements still to send behind a leading 1; 1 = none), tgap (gap units still owed), tail and head
 * (characters consumed and queued, modulo 2^32), skipped.  For every sample n, in this order:
 *
 *   p = paddles ? paddles[c][n] : 0;  s = (p >> 2) & 1
 *   STRAIGHT:  s |= (p & 3) != 0;  d = h = 0        else  d = p & 1;  h = (p >> 1) & 1
 *   if ((d | h | s) && (tail != head || code > 1 || tgap)) { tail = head; code = 1; tgap = 0; }    the operator takes over; a running
 *                                                                                                    mark keeps its length
 *   if (phase != IDLE) { if (last == 1) dit_mem |= d; else dah_mem |= h;  if (phase == MARK) squeeze |= d & h; }
 *   if (phase == MARK && left == 0) { phase = GAP; left = u; }
 *   else if (phase != MARK && left == 0) {                       IDLE, or a gap that has run out: decide
 *       if (mode == IAMBIC_A && squeeze && !(d | h)) dit_mem = dah_mem = 0       a squeeze let go: mode A sends nothing more
 *       wd = d | dit_mem;  wh = h | dah_mem
 *       if (wd && wh)  el = (phase == IDLE) ? 0 : 1 - last
 *       else if (wd) el = 0;  else if (wh) el = 1
 *       else if (mode == IAMBIC_B && squeeze) el = 1 - last
 *       else el = next_from_text()                               may instead start a GAP of tgap * u, or find nothing
 *       element el:  phase = MARK; left = (el ? 3 : 1) * u; last = el; squeeze = 0; (el ? dah_mem : dit_mem) = 0
 *       nothing:     phase = IDLE; left = 0; squeeze = 0
 *   }
 *   key[c][n] = (phase == MARK) | s;   if (phase != IDLE) left -= 1
 *
 * next_from_text() loops:  1. tgap != 0: phase = GAP, left = tgap * u, tgap = 0, done.   2. code > 1: pop the most significant element
 * behind the leading 1; if code is 1 now, tgap = 2; done.   3. tail == head: nothing, done.   4. k = codes[text[c][tail % ring]],
 * tail += 1;  k == 1: tgap += 4;  k >= 2: code = k;  k == 0: skipped += 1;  again.
 * Every mark is followed by a gap of one unit, a character end adds 2 (3 in all), a blank 4 more (7 in all): standard spacing.
 * STRAIGHT sends the text memory too.  A unit that changes takes effect with the next element or gap that starts. */
enum { SELENITE_KEYER_STRAIGHT = 0, SELENITE_KEYER_IAMBIC_A = 1, SELENITE_KEYER_IAMBIC_B = 2 };
enum { SELENITE_KEYER_DIT = 1, SELENITE_KEYER_DAH = 2, SELENITE_KEYER_KEY = 4 };   /* the paddle byte's bits; others are ignored */

typedef struct {
    uint32_t struct_size;        /* sizeof(selenite_tx_keyer_config) */
    uint32_t mode;               /* SELENITE_KEYER_* */
    uint32_t unit_all;           /* audio samples per dit, 1 ... 2^24; used when unit is NULL */
    const uint32_t *unit;        /* [channels] or NULL; copied */
    uint32_t ring;               /* text bytes per channel, 1 ... 65536 */
    const uint8_t *codes;        /* [256] character -> pattern (selenite_tx_design_morse_codes), copied; NULL: the built-in table */
    uint32_t reserved;           /* 0 */
} selenite_tx_keyer_config;
typedef struct {
    uint32_t *phase, *left, *last, *dit_mem, *dah_mem, *squeeze, *code, *tgap, *tail, *head, *skipped;   /* [channels] each */
    uint8_t  *text;              /* [channels][ring] */
} selenite_tx_keyer_state_view;  /* NULL members are skipped */

/* NULL: the stage off again.  Needs selenite_tx_set_cw (ARGUMENT_ERROR before it).  The first call (and the first after NULL) clears all
 * state (phase IDLE, code 1, everything else 0, the text zeroed), and so does selenite_tx_reset; a further call retunes mode, units and
 * codes and keeps the state, except that a changed ring clears the text queue (tail = head = 0, code = 1, tgap = 0).  ARGUMENT_ERROR (the
 * previous setting stays) for a wrong struct_size, a mode out of range, a unit of 0 or above 2^24, a ring out of range or reserved != 0. */
int selenite_tx_set_keyer(selenite_tx_instance *S, const selenite_tx_keyer_config *cfg);
/* Appends len bytes to the queue of every channel of [first_channel, first_channel + n_channels): per_channel = 0 the same `text[len]`,
 * per_channel = 1 `text[n_channels][len]`.  Synchronous.  LENGTH_ERROR, and nothing is written, when a channel of the range lacks room
 * (head - tail + len > ring); ARGUMENT_ERROR before selenite_tx_set_keyer, for a range outside the channels, NULL text with len != 0 or
 * per_channel > 1. */
int selenite_tx_keyer_send(selenite_tx_instance *S, uint32_t first_channel, uint32_t n_channels, const uint8_t *text, uint32_t len,
                           uint32_t per_channel);
int selenite_tx_keyer_pending(selenite_tx_instance *S, uint32_t *pending);   /* [channels]: head - tail, characters not yet begun */
/* dPaddles [channels][blockSize] bytes at the audio rate, or NULL (all zero: the text memory alone).  The stage writes the instance's key
 * buffer, then the call is selenite_tx_process_key_* on those bytes: the same validity rules and status codes, and ARGUMENT_ERROR before
 * selenite_tx_set_keyer.  A refused call writes nothing and moves no state. */
int selenite_tx_process_paddles_f32_device(selenite_tx_instance *S, const uint8_t *dPaddles, float *dDstIQ, float *dSide, uint32_t blockSize);
int selenite_tx_process_paddles_q15_device(selenite_tx_instance *S, const uint8_t *dPaddles, int16_t *dDstIQ, int16_t *dSide, uint32_t blockSize);
int selenite_tx_process_paddles_f32(selenite_tx_instance *S, const uint8_t *pPaddles, float *pDstIQ, float *pSide, uint32_t blockSize);
int selenite_tx_process_paddles_q15(selenite_tx_instance *S, const uint8_t *pPaddles, int16_t *pDstIQ, int16_t *pSide, uint32_t blockSize);
/* The stage alone, in any mode: key bytes [channels][blockSize] (0 / 1) into the caller's device buffer; only the keyer's state moves.
 * blockSize a non-zero multiple of cfg.block. */
int selenite_tx_keyer_run_device(selenite_tx_instance *S, const uint8_t *dPaddles, uint8_t *dKey, uint32_t blockSize);
/* the key bytes of the last paddle call, [channels][blockSize] on the device (grown on demand; NULL before the first such call) */
const uint8_t *selenite_tx_keyer_key_device(selenite_tx_instance *S);
int selenite_tx_get_keyer_state(selenite_tx_instance *S, const selenite_tx_keyer_state_view *view);
int selenite_tx_set_keyer_state(selenite_tx_instance *S, const selenite_tx_keyer_state_view *view);
/* mean milliseconds per launch of the stage's kernel alone (into the instance's key buffer) over `iters` launches behind one untimed
 * launch; the state moves */
int selenite_tx_time_keyer_stage_device(selenite_tx_instance *S, const uint8_t *dPaddles, uint32_t blockSize, uint32_t iters,
                                        float *ms_per_launch);
/* Host-only.  The inverse of selenite_rx_design_morse's table (NULL: the built-in one): codes[c] = the smallest pattern >= 2 whose
 * character is c, the filler table[0] excluded; a lower-case letter takes its upper-case letter's pattern; ' ' -> 1 (the word blank);
 * everything else 0 (skipped). */
int selenite_tx_design_morse_codes(uint8_t codes[256], const uint8_t table[256]);
/* Host-only.  round(1.2 * fs_audio / wpm) (PARIS timing), at least 1; 0 for arguments that are not finite and positive. */
uint32_t selenite_tx_keyer_unit(double wpm, double fs_audio);

#ifdef __cplusplus
}
#endif
#endif /* SELENITE_TX_KEYER_H */
