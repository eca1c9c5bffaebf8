// rx_fskdec.hip -- FSK teleprinter decoder, an RTTY skimmer (step 4-r of DESIGN.md section 2, section 5.21).
// The stage is a tap, off by default, on the un-scaled audio behind the demodulator and the CW filter (step 4).  That is the tone bank's and
// the Morse decoder's position, in front of 4a / 4b / 4c / the AGC.  It works in every mode and every `arith` mode, and it changes none of
// the audio.  It neither raises nor clears SELENITE_RX_NANINF.
// One tick is T = tick consecutive audio samples, 4 <= T <= 256.  T must divide n = block / decim, otherwise the call returns
// SELENITE_RX_LENGTH_ERROR, as the noise blanker's frame does.  So ticks never straddle DSP blocks or calls, and nothing is left pending.
// Every float operation is rounded to f32, with no contraction and denormals kept.  These are the meter's rules.
// Per channel and tick, with x the tick's samples:
//   two arm_biquad_cascade_df1_f32 instances of ONE section each, coefficients {b0,b1,b2,a1,a2} = mark[5] / space[5] (one set for all channels),
//   state {x1,x2,y1,y2} each, running on across ticks, blocks and calls:
//       per sample:  acc = b0*x; acc = acc + b1*x1; acc = acc + b2*x2; acc = acc + a1*y1; acc = acc + a2*y2;  (each product rounded, then the sum)
//                    x2 = x1; x1 = x; y2 = y1; y1 = acc
//   pm = arm_power_f32(ym, T);  ps = arm_power_f32(ys, T);  pw = arm_power_f32(x, T)        (from +0.0f, ascending; no division)
//   if (reverse) swap(pm, ps)
//   if (pm <= FLT_MAX && ps <= FLT_MAX && pw <= FLT_MAX) {           (false for NaN: the followers stay)
//       d = pm - em; t = alpha*d; em = em + t;      es, ew likewise from ps, pw          (the AGC's form)
//   }
//   tot = em + es;  dd = em - es;  th = hyst*tot;  q = frac*ew
//   present = tot > q && tot > min_power && tot <= FLT_MAX
//   prev = lvl
//   if (!present) lvl = 1;  else if (dd > th) lvl = 1;  else if (-dd > th) lvl = 0;      (else lvl stays; 1 = mark = idle)
//   if (k == 0) { if (prev == 1 && lvl == 0) { k = 1; t_q8 = 0; shift = 0; } }            (start edge; nothing is sampled in this tick)
//   else {
//       t_q8 += 256
//       if (t_q8 >= (k-1)*bit + (bit >> 1)) {                                             (centre of bit k-1; bit: this channel's, Q8 ticks)
//           if (k == 1)      { k = lvl ? 0 : 2; }                                         (a start bit that did not last: false start)
//           else if (k <= 6) { shift |= lvl << (k-2); k += 1; }                           (five data bits, LSB first)
//           else { if (lvl) { c = shift;
//                             if (c == 31) figs = 0; else if (c == 27) figs = 1;
//                             else { b = table[figs*32 + c]; if (b) emit(b); if (usos && c == 4) figs = 0; } }
//                  else ferr += 1;                                                         (framing error: nothing is emitted)
//                  k = 0; }
//       }
//   }
//   emit(b):  text[count % ring] = b;  count += 1
// State per channel after set_fskdec / selenite_rx_reset: filt[2][4], em, es, ew: +0.0f; lvl: 1; k, t_q8, shift, figs, ferr: 0; bit: the
// config's bit_q8; count: 0 (u64); text[ring]: 0.  `bit` is a state row: through set_fskdec_state every channel can run at its own speed,
// the way `unit` does for the Morse decoder.  A non-finite sample poisons that channel's filters until reset or set_fskdec_state: the three
// followers stay where they stood.  The state moves with ChanRange.first.  set_mode and the other setters leave it alone.
// `table` is 64 bytes, copied: letters then figures, indexed by the 5-bit code; a 0 byte emits nothing.
//
// Every operation above is kept, in that order, and the unit is compiled with -ffp-contract=off and IEEE denormals, as rx_cwdec.hip is:
// bit-exact given its input in every arith mode, whatever the cut of the stream into calls.
//
// k_fskdec: single-wave workgroups, one lane per channel (the recurrence has no time parallelism at this rounding; the parallelism is
// channels, and within a channel the two filters):
//   load    the wave's 64 audio rows in tiles of 32 samples, coalesced (half a wave per row: 128 bytes), into registers; the NEXT tile's
//           loads are issued before the current tile's steps and land under them;
//   stage   the registers into LDS at row * 33 + i, read back transposed (lane = row), conflict-free both ways at the padded pitch;
//   step    mark and space are the two halves of float2 values: v_pk_mul_f32 / v_pk_add_f32 round each half on its own, so nothing
//           contracts and the bits are the reference's; the band power runs next to them in plain f32;
//   tick    its end is lane-uniform in time (T is one value), so the integer law runs once per T samples behind a scalar branch, with no
//           shuffle; a character is a plain byte store into the channel's ring.
// filt is two 16-byte loads and stores per lane and launch; the followers and the integers stay in registers from tick to tick.
#include "rx_host.h"

#include <cfloat>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace srx {

constexpr uint32_t kFsTile = 32;                 // samples of every row staged per tile (8448 bytes of LDS per wave)
constexpr uint32_t kFsRow = kFsTile + 1;         // words between the rows in LDS
typedef float f32x2 __attribute__((ext_vector_type(2)));    // .x: mark, .y: space

__global__ __launch_bounds__(64) void k_fskdec(FskdecParams q, const float *__restrict__ audio)
{
    __shared__ float rows[kWave * kFsRow];       // [row][33]

    const uint32_t lane = threadIdx.x;
    const uint32_t c0 = blockIdx.x * kWave, c = c0 + lane;
    const bool live = c < q.channels;
    const uint32_t total = q.nblk * q.n, T = q.tick;       // (launch_fskdec: total <= stride, T divides n)
    const uint32_t ring_mask = q.ring - 1u;
    const f32x2 b0 = { q.mark[0], q.space[0] }, b1 = { q.mark[1], q.space[1] }, b2 = { q.mark[2], q.space[2] };
    const f32x2 a1 = { q.mark[3], q.space[3] }, a2 = { q.mark[4], q.space[4] };

    f32x2 x1 = { 0.0f, 0.0f }, x2 = x1, y1 = x1, y2 = x1;
    float em = 0.0f, es = 0.0f, ew = 0.0f;
    uint32_t lvl = 1u, k = 0u, t_q8 = 0u, shift = 0u, figs = 0u, ferr = 0u, bit = 8u * 256u;
    uint64_t count = 0u;
    if (live) {
        const float4 fm = reinterpret_cast<const float4 *>(q.filt)[2u * (size_t)c], fs = reinterpret_cast<const float4 *>(q.filt)[2u * (size_t)c + 1u];
        x1 = f32x2{ fm.x, fs.x }; x2 = f32x2{ fm.y, fs.y }; y1 = f32x2{ fm.z, fs.z }; y2 = f32x2{ fm.w, fs.w };
        em = q.em[c]; es = q.es[c]; ew = q.ew[c];
        lvl = q.lvl[c]; k = q.k[c]; t_q8 = q.t_q8[c]; shift = q.shift[c]; figs = q.figs[c]; ferr = q.ferr[c]; bit = q.bit[c];
        count = q.count[c];
    }
    uint8_t *const text = q.text + (size_t)(live ? c : 0u) * q.ring;

    // a tile in registers: value j of a lane is sample lane % 32 of row 2 j + lane / 32.  A row past the launch's channels reads the last
    // channel's and a sample past the launch's end the last sample: every address is inside the audio, nothing is predicated, and what
    // such a load brings is never used (a lane past the channels writes nothing; the steps stop at the launch's end).  The offsets from
    // the wave's first row are 32-bit (launch_fskdec: 64 rows of at most 2^24 samples).
    const uint32_t li = lane & (kFsTile - 1u), lr = lane / kFsTile;
    const float *const wave_audio = audio + (size_t)c0 * q.stride;
    const uint32_t last_row = q.channels - 1u - c0;
    uint32_t row_at[kFsTile];
#pragma unroll
    for (uint32_t j = 0; j < kFsTile; ++j) row_at[j] = min(2u * j + lr, last_row) * q.stride;
    float stage[kFsTile];
    auto fetch = [&](uint32_t s0) {
        const uint32_t s = min(s0 + li, total - 1u);
#pragma unroll
        for (uint32_t j = 0; j < kFsTile; ++j) stage[j] = wave_audio[row_at[j] + s];
    };

    f32x2 pp = { 0.0f, 0.0f };                   // arm_power_f32 of ym, ys: from +0.0f
    float pw = 0.0f;                             // ... and of x
    uint32_t ph = 0u;                            // samples into the running tick (0 at both ends of a launch)
    fetch(0u);
    for (uint32_t s0 = 0; s0 < total; s0 += kFsTile) {
        const uint32_t tl = total - s0 < kFsTile ? total - s0 : kFsTile;
        __syncthreads();                         // (one wave: orders the LDS traffic across lanes for the compiler)
#pragma unroll
        for (uint32_t j = 0; j < kFsTile; ++j) rows[(2u * j + lr) * kFsRow + li] = stage[j];
        __syncthreads();
        if (s0 + kFsTile < total) fetch(s0 + kFsTile);      // in flight under this tile's steps
        const float *row = rows + lane * kFsRow;
        for (uint32_t i = 0; i < tl;) {
            const uint32_t left = T - ph, run = tl - i < left ? tl - i : left;
#pragma unroll 4
            for (uint32_t r = 0; r < run; ++r) {
                const float x = row[i + r];
                const f32x2 xx = { x, x };
                f32x2 acc = b0 * xx;
                f32x2 p = b1 * x1; acc = acc + p;
                p = b2 * x2; acc = acc + p;
                p = a1 * y1; acc = acc + p;
                p = a2 * y2; acc = acc + p;
                x2 = x1; x1 = xx; y2 = y1; y1 = acc;
                p = acc * acc; pp = pp + p;
                const float px = x * x; pw = pw + px;
            }
            i += run; ph += run;
            if (ph != T) continue;               // (wave-uniform)
            // ---- the tick's end ----
            float pm = q.reverse ? pp.y : pp.x, ps = q.reverse ? pp.x : pp.y;
            if (pm <= FLT_MAX && ps <= FLT_MAX && pw <= FLT_MAX) {       // (false for NaN: the followers stay)
                float d = pm - em, t = q.alpha * d; em = em + t;
                d = ps - es; t = q.alpha * d; es = es + t;
                d = pw - ew; t = q.alpha * d; ew = ew + t;
            }
            ph = 0u; pw = 0.0f; pp = f32x2{ 0.0f, 0.0f };
            const float tot = em + es, dd = em - es, th = q.hyst * tot, qq = q.frac * ew;
            const bool present = tot > qq && tot > q.min_power && tot <= FLT_MAX;
            const uint32_t prev = lvl;
            if (!present) lvl = 1u; else if (dd > th) lvl = 1u; else if (-dd > th) lvl = 0u;
            if (k == 0u) {
                if (prev == 1u && lvl == 0u) { k = 1u; t_q8 = 0u; shift = 0u; }     // start edge; nothing is sampled in this tick
            } else {
                t_q8 += 256u;
                if (t_q8 >= (k - 1u) * bit + (bit >> 1)) {                          // centre of bit k - 1
                    if (k == 1u) {
                        k = lvl ? 0u : 2u;                                          // a start bit that did not last: false start
                    } else if (k <= 6u) {
                        shift |= lvl << (k - 2u); k += 1u;                          // five data bits, LSB first
                    } else {
                        if (lvl) {
                            const uint32_t cc = shift;
                            if (cc == 31u) figs = 0u;
                            else if (cc == 27u) figs = 1u;
                            else {
                                const uint8_t b = q.table[(figs * 32u + cc) & 63u];    // (& 63: rows a caller set outside the law's range stay inside the table)
                                if (b) {
                                    if (live) text[(uint32_t)count & ring_mask] = b;
                                    count += 1u;
                                }
                                if (q.usos && cc == 4u) figs = 0u;
                            }
                        } else {
                            ferr += 1u;                                             // framing error: nothing is emitted
                        }
                        k = 0u;
                    }
                }
            }
        }
    }
    if (live) {
        reinterpret_cast<float4 *>(q.filt)[2u * (size_t)c] = float4{ x1.x, x2.x, y1.x, y2.x };
        reinterpret_cast<float4 *>(q.filt)[2u * (size_t)c + 1u] = float4{ x1.y, x2.y, y1.y, y2.y };
        q.em[c] = em; q.es[c] = es; q.ew[c] = ew;
        q.lvl[c] = lvl; q.k[c] = k; q.t_q8[c] = t_q8; q.shift[c] = shift; q.figs[c] = figs; q.ferr[c] = ferr;
        q.count[c] = count;                      // (`bit` is read, never written)
    }
}

hipError_t launch_fskdec(const FskdecParams &q, const float *audio, hipStream_t st)
{
    if (q.channels == 0 || q.nblk == 0) return hipSuccess;
    if (q.n == 0 || (uint64_t)q.nblk * q.n > q.stride || q.stride > (1u << 24) || q.tick == 0 || q.n % q.tick != 0 || q.ring == 0 || (q.ring & (q.ring - 1u)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fskdec, dim3((q.channels + kWave - 1) / kWave), dim3(kWave), 0, st, q, audio);
    return hipGetLastError();
}

// ---- host side of the stage ----
void FskdecStage::release()
{
    dev_free(d_table, d_text);
    dev_free(d_filt, d_em, d_es, d_ew);
    dev_free(d_lvl, d_k, d_t_q8, d_shift, d_figs, d_ferr, d_bit);
    dev_free(d_count);
    on = false;
    tick = bit_q8 = reverse = usos = ring = 0;
    alpha = hyst = frac = min_power = 0.0f;
    for (int i = 0; i < 5; ++i) mark[i] = space[i] = 0.0f;
}

// the stage's state as set_fskdec leaves it: +0.0f and 0, lvl 1 (mark, idle), bit at bit_q8, the ring zeros
int FskdecStage::init_state(selenite_rx_instance *S)
{
    if (!on) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels;
    HIPCHK(S, hipMemsetAsync(d_filt, 0, C * 8 * sizeof(float), S->stream));
    for (float *row : { d_em, d_es, d_ew }) HIPCHK(S, hipMemsetAsync(row, 0, C * sizeof(float), S->stream));
    for (uint32_t *row : { d_k, d_t_q8, d_shift, d_figs, d_ferr }) HIPCHK(S, hipMemsetAsync(row, 0, C * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_count, 0, C * sizeof(uint64_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_text, 0, C * ring, S->stream));
    const uint32_t one = 1u;
    if (int rc = fill_rows(S, d_lvl, C, &one)) return rc;
    return fill_rows(S, d_bit, C, &bit_q8);                 // (drains the stream)
}

// the stage's view of a launch: the channels and the audio geometry of `p`; the state rows and the rings move with the range
FskdecParams FskdecStage::params(ChanRange r, const RxParams &p) const
{
    const size_t c0 = r.first;
    FskdecParams q{};
    q.channels = p.channels; q.n = p.block / p.decim; q.nblk = p.block_size / p.block; q.stride = p.out_stride;
    q.tick = tick; q.reverse = reverse; q.usos = usos; q.ring = ring;
    for (int i = 0; i < 5; ++i) { q.mark[i] = mark[i]; q.space[i] = space[i]; }
    q.alpha = alpha; q.hyst = hyst; q.frac = frac; q.min_power = min_power;
    q.table = d_table;
    q.filt = d_filt + c0 * 8;
    q.em = d_em + c0; q.es = d_es + c0; q.ew = d_ew + c0;
    q.lvl = d_lvl + c0; q.k = d_k + c0; q.t_q8 = d_t_q8 + c0; q.shift = d_shift + c0; q.figs = d_figs + c0; q.ferr = d_ferr + c0;
    q.bit = d_bit + c0; q.count = d_count + c0;
    q.text = d_text + c0 * ring;
    return q;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_fskdec(selenite_rx_instance *S, const selenite_rx_fskdec_config *f)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_fskdec: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    if (f) {
        const char *bad = nullptr;
        int code = SELENITE_RX_ARGUMENT_ERROR;
        bool coeffs_ok = true;
        if (f->struct_size == sizeof(selenite_rx_fskdec_config))
            for (int i = 0; i < 5; ++i) coeffs_ok = coeffs_ok && std::isfinite(f->mark[i]) && std::isfinite(f->space[i]);
        if (f->struct_size != sizeof(selenite_rx_fskdec_config)) bad = "struct_size is not sizeof(selenite_rx_fskdec_config)";
        else if (f->tick < 4u || f->tick > 256u) bad = "tick is not 4 .. 256";
        else if ((S->cfg.block / S->cfg.decim) % f->tick != 0) { bad = "tick does not divide cfg.block / cfg.decim"; code = SELENITE_RX_LENGTH_ERROR; }
        else if (f->bit_q8 < 8u * 256u || f->bit_q8 > 1024u * 256u) bad = "bit_q8 is not 8 * 256 .. 1024 * 256";
        else if (f->reverse > 1u) bad = "reverse is not 0 or 1";
        else if (f->usos > 1u) bad = "usos is not 0 or 1";
        else if (f->ring < 16u || f->ring > 65536u || (f->ring & (f->ring - 1u))) bad = "ring is not a power of two, 16 .. 65536";
        else if (!coeffs_ok) bad = "mark / space is not finite";
        else if (!(std::isfinite(f->alpha) && f->alpha > 0.0f && f->alpha <= 1.0f)) bad = "alpha is not finite and in (0, 1]";
        else if (!(f->hyst >= 0.0f && f->hyst < 1.0f)) bad = "hyst is not in [0, 1)";
        else if (!(f->frac >= 0.0f && f->frac <= 1.0f)) bad = "frac is not in [0, 1]";
        else if (!(std::isfinite(f->min_power) && f->min_power >= 0.0f)) bad = "min_power is not finite and >= 0";
        if (bad) return refuse("selenite_rx_set_fskdec", bad, code);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    FskdecStage &st = S->fskdec;
    st.release();
    if (!f) return SELENITE_RX_SUCCESS;
    uint8_t table[64];
    if (f->table) std::memcpy(table, f->table, sizeof table);
    else (void)selenite_rx_design_ita2(table);
    const size_t C = S->cfg.channels;
    hipError_t e = dev_alloc(&st.d_table, sizeof table);
    if (e == hipSuccess) e = dev_alloc(&st.d_text, C * f->ring);
    if (e == hipSuccess) e = dev_alloc(&st.d_filt, C * 8);
    for (float **row : { &st.d_em, &st.d_es, &st.d_ew })
        if (e == hipSuccess) e = dev_alloc(row, C);
    for (uint32_t **row : { &st.d_lvl, &st.d_k, &st.d_t_q8, &st.d_shift, &st.d_figs, &st.d_ferr, &st.d_bit })
        if (e == hipSuccess) e = dev_alloc(row, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_count, C);
    if (e == hipSuccess) e = hipMemcpy(st.d_table, table, sizeof table, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_fskdec: ") + hipGetErrorString(e));
    }
    st.on = true;
    st.tick = f->tick; st.bit_q8 = f->bit_q8; st.reverse = f->reverse; st.usos = f->usos; st.ring = f->ring;
    for (int i = 0; i < 5; ++i) { st.mark[i] = f->mark[i]; st.space[i] = f->space[i]; }
    st.alpha = f->alpha; st.hyst = f->hyst; st.frac = f->frac; st.min_power = f->min_power;
    return st.init_state(S);
}

static int fskdec_state_copy(selenite_rx_instance *S, const selenite_rx_fskdec_state_view *v, bool to_host)
{
    if (!S || !v || !S->fskdec.on) return SELENITE_RX_ARGUMENT_ERROR;
    const FskdecStage &st = S->fskdec;
    const size_t C = S->cfg.channels, W = C * sizeof(uint32_t), F = C * sizeof(float);
    return copy_rows(S, to_host, { { st.d_filt, v->filt, 8 * F }, { st.d_em, v->em, F }, { st.d_es, v->es, F }, { st.d_ew, v->ew, F },
                                   { st.d_lvl, v->lvl, W }, { st.d_k, v->k, W }, { st.d_t_q8, v->t_q8, W }, { st.d_shift, v->shift, W },
                                   { st.d_figs, v->figs, W }, { st.d_ferr, v->ferr, W }, { st.d_bit, v->bit, W },
                                   { st.d_count, v->count, C * sizeof(uint64_t) }, { st.d_text, v->text, C * st.ring } });
}
extern "C" int selenite_rx_get_fskdec_state(selenite_rx_instance *S, const selenite_rx_fskdec_state_view *v) { return fskdec_state_copy(S, v, true); }
extern "C" int selenite_rx_set_fskdec_state(selenite_rx_instance *S, const selenite_rx_fskdec_state_view *v) { return fskdec_state_copy(S, v, false); }

extern "C" int selenite_rx_get_fskdec(selenite_rx_instance *S, uint8_t *text, uint64_t *count, uint32_t *ferr, uint32_t *lvl)
{
    if (!S || !S->fskdec.on) return SELENITE_RX_ARGUMENT_ERROR;
    const FskdecStage &st = S->fskdec;
    const size_t C = S->cfg.channels;
    return copy_rows(S, true, { { st.d_text, text, C * st.ring }, { st.d_count, count, C * sizeof(uint64_t) },
                                { st.d_ferr, ferr, C * sizeof(uint32_t) }, { st.d_lvl, lvl, C * sizeof(uint32_t) } });
}
extern "C" const uint8_t *selenite_rx_fskdec_text_device(const selenite_rx_instance *S) { return S && S->fskdec.on ? S->fskdec.d_text : nullptr; }
extern "C" const uint64_t *selenite_rx_fskdec_count_device(const selenite_rx_instance *S) { return S && S->fskdec.on ? S->fskdec.d_count : nullptr; }
extern "C" const uint32_t *selenite_rx_fskdec_lvl_device(const selenite_rx_instance *S) { return S && S->fskdec.on ? S->fskdec.d_lvl : nullptr; }
