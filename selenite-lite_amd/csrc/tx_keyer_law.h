// tx_keyer_law.h -- the keyer's law (include/selenite_tx_keyer.h) as k_tx_keyer runs it: one sample, and a tile of up to 64 samples whose
// paddle bits are three 64-bit masks.  Plain integer C++ that compiles for the host as well as the device, so that the run-length form can
// be checked against the sample form on a CPU (tests/test_txkeyer_law_host.py); on the device every value here is wave-uniform.
// Not part of the C-ABI.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SRX_KEYER_HD __host__ __device__ __forceinline__
#else
#define SRX_KEYER_HD inline
#endif

namespace srx {

enum : uint32_t { kKeyIdle = 0, kKeyMark = 1, kKeyGap = 2 };
enum : uint32_t { kKeyerWords = 11 };             // state words of a channel, in the order of KeyerState and of the state view
struct KeyerState { uint32_t phase, left, last, dit_mem, dah_mem, squeeze, code, tgap, tail, head, skipped; };
struct KeyerText { const uint8_t *text; const uint8_t *codes; uint32_t ring; };      // the channel's ring, the 256 patterns

SRX_KEYER_HD bool keyer_queued(const KeyerState &k) { return k.tail != k.head || k.code > 1u || k.tgap != 0u; }

// One sample of the law.  Returns phase == MARK; the caller ORs the straight-key bit s into the key byte.
SRX_KEYER_HD uint32_t keyer_sample(KeyerState &k, uint32_t d, uint32_t h, uint32_t s, uint32_t u, uint32_t mode, const KeyerText &t)
{
    if ((d | h | s) && keyer_queued(k)) { k.tail = k.head; k.code = 1u; k.tgap = 0u; }
    if (k.phase != kKeyIdle) {
        if (k.last == 1u) k.dit_mem |= d; else k.dah_mem |= h;
        if (k.phase == kKeyMark) k.squeeze |= d & h;
    }
    if (k.phase == kKeyMark && k.left == 0u) {
        k.phase = kKeyGap; k.left = u;
    } else if (k.phase != kKeyMark && k.left == 0u) {
        if (mode == 1u && k.squeeze && !(d | h)) { k.dit_mem = 0u; k.dah_mem = 0u; }        // mode A: a squeeze let go takes its memories along
        const uint32_t wd = d | k.dit_mem, wh = h | k.dah_mem, other = k.last == 1u ? 0u : 1u;
        uint32_t el = 2u;                        // 0 dit, 1 dah, 2 nothing, 3 a text gap has begun
        if (wd && wh) el = k.phase == kKeyIdle ? 0u : other;
        else if (wd) el = 0u;
        else if (wh) el = 1u;
        else if (mode == 2u && k.squeeze) el = other;
        else {
            for (;;) {                           // next_from_text
                if (k.tgap) { k.phase = kKeyGap; k.left = k.tgap * u; k.tgap = 0u; el = 3u; break; }
                if (k.code > 1u) {
                    const uint32_t top = 30u - (uint32_t)__builtin_clz(k.code);      // the bit behind the leading 1
                    el = (k.code >> top) & 1u;
                    k.code = (1u << top) | (k.code & ((1u << top) - 1u));
                    if (k.code == 1u) k.tgap = 2u;
                    break;
                }
                if (k.tail == k.head) break;
                const uint32_t pat = t.codes[t.text[k.tail % t.ring]];
                k.tail += 1u;
                if (pat == 1u) k.tgap += 4u;
                else if (pat >= 2u) k.code = pat;
                else k.skipped += 1u;
            }
        }
        if (el < 2u) {
            k.phase = kKeyMark; k.left = (el ? 3u : 1u) * u; k.last = el; k.squeeze = 0u;
            if (el) k.dah_mem = 0u; else k.dit_mem = 0u;
        } else if (el == 2u) {
            k.phase = kKeyIdle; k.left = 0u; k.squeeze = 0u;
        }
    }
    const uint32_t mark = k.phase == kKeyMark ? 1u : 0u;
    if (k.phase != kKeyIdle) k.left -= 1u;
    return mark;
}

// Samples [0, nv) of a tile, nv <= 64: bit n of D, H, S is d, h, s of sample n (the STRAIGHT mapping already applied).  Returns the mask
// of the samples with phase == MARK.  The state changes only where a phase ends and where an idle keyer meets a paddle bit: everything
// between is one step, the latches and the take-over test being ORs over the run's bits.
SRX_KEYER_HD uint64_t keyer_tile(KeyerState &k, uint64_t D, uint64_t H, uint64_t S, uint32_t nv, uint32_t u, uint32_t mode, const KeyerText &t)
{
    const uint64_t valid = nv >= 64u ? ~0ull : (1ull << nv) - 1ull;
    D &= valid; H &= valid; S &= valid;
    const uint64_t any = D | H | S;
    uint64_t K = 0ull;
    uint32_t pos = 0u;
    while (pos < nv) {
        const uint64_t from = ~0ull << pos;
        const uint32_t rest = nv - pos;
        uint32_t r = 0u;
        if (k.left != 0u) {                      // a phase under way (IDLE with left != 0 can only be set from outside: nothing moves)
            r = (k.phase == kKeyIdle || k.left > rest) ? rest : k.left;
        } else if (k.phase == kKeyIdle && !keyer_queued(k) && !(k.dit_mem | k.dah_mem) && !(mode == 2u && k.squeeze)) {
            const uint64_t m = (D | H) & from;   // idle with nothing to send: up to the first dit or dah bit
            r = m ? (uint32_t)__builtin_ctzll(m) - pos : rest;
        }
        if (r) {
            const uint64_t R = from & (pos + r >= 64u ? ~0ull : (1ull << (pos + r)) - 1ull);
            if ((any & R) && keyer_queued(k)) { k.tail = k.head; k.code = 1u; k.tgap = 0u; }
            if (k.phase != kKeyIdle) {
                if (k.last == 1u) k.dit_mem |= (D & R) ? 1u : 0u; else k.dah_mem |= (H & R) ? 1u : 0u;
                if (k.phase == kKeyMark) { k.squeeze |= (D & H & R) ? 1u : 0u; K |= R; }
                k.left -= r;
            } else if (k.left == 0u) {
                k.squeeze = 0u;
            }
            pos += r;
        } else {
            if (keyer_sample(k, (uint32_t)(D >> pos) & 1u, (uint32_t)(H >> pos) & 1u, (uint32_t)(S >> pos) & 1u, u, mode, t)) K |= 1ull << pos;
            pos += 1u;
        }
    }
    return K;
}

}  // namespace srx
