// rx_cwdec.hip -- Morse decoder, a CW skimmer (step 4-d of DESIGN.md section 2, section 5.19).
// The stage is a tap, off by default, available in every mode and every `arith` mode.  It reads the un-scaled audio behind the
// demodulator and behind the CW filter (step 4).  That is the tone bank's position, in front of 4a / 4b / 4c / the AGC.  It changes none
// of the audio.  One tick is one DSP block of n = block / decim samples x.
// Every float operation is rounded to f32, with no contraction and denormals kept.  The division is correctly rounded.  These are the
// meter's rules.
// State per channel, with its value after set_cwdec / reset in brackets: peak, floor (f32; +0.0f); primed, key, flip, run (u32; 0);
// unit (u32, Q8 blocks; unit_init); code (u32; 1); word (u32; 0); count (u64; 0); text[ring] (u8; 0).
//   pw = arm_power_f32(x, n);  ms = pw / (float)n
//   raw = 0
//   if (ms <= FLT_MAX) {                                   (false for NaN: peak, floor stay, raw = 0)
//       if (!primed) { peak = ms; floor = ms; primed = 1; }
//       else {
//           r = ms > peak  ? peak_attack  : peak_decay;   d = ms - peak;   t = r * d;  peak  = peak  + t;
//           r = ms < floor ? floor_attack : floor_decay;  d = ms - floor;  t = r * d;  floor = floor + t;
//       }
//       span = peak - floor;  f = key ? off_frac : on_frac;  t = f * span;  thr = floor + t;
//       q = snr * floor;  active = peak > q && peak > min_power;
//       raw = active && ms > thr;
//   }
//   edge = 0
//   if (raw == key) { run = min(run + flip + 1, 65535); flip = 0; }
//   else { flip += 1;  if (flip >= debounce) { ended = run; key = raw; run = flip; flip = 0; edge = 1; } }
//   if (edge && key == 0) {                                (a mark of `ended` blocks is over)
//       m = ended << 8;  dah = m >= 2 * unit;              (unit as it stood before this update)
//       if (adapt) { g = dah ? m / 3 : m;
//                    if (g >= unit) unit += (g - unit) >> track; else unit -= (unit - g) >> track;
//                    unit = min(max(unit, unit_min), unit_max); }
//       code = (code == 0 || code >= 128) ? 0 : (code << 1) | dah;       (0: more than 7 elements)
//   }
//   if (key == 0) {
//       s = run << 8;
//       if (code != 1 && s >= 2 * unit) { emit(table[code]); code = 1; word = 1; }
//       if (word && s >= 5 * unit)      { emit(' ');         word = 0; }
//   }
//   emit(c):  text[count % ring] = c;  count += 1
// `table` is 256 bytes, copied, indexed by the element pattern behind a leading 1.  `.-` is 0b101.  Index 0 is the overflow character.
// The stage neither raises nor clears SELENITE_RX_NANINF.
//
// Every operation above is kept, in that order, and the unit is compiled with -ffp-contract=off, IEEE denormals and correctly rounded
// division, as rx_meter.hip is: bit-exact given its input in every arith mode, whatever the cut of the stream into calls.
//
// k_cwdec<B>: k_meter<B>'s plan (rx_meter.hip).  Single-wave workgroups; a tile is B consecutive DSP blocks of 64 / B consecutive channels
// (B = the power of two that holds the launch's blocks, at most 64), lane g * B + j owning block j of channel g:
//   load    the tile's audio rows, coalesced, into LDS at slot * 33 + i, at most 32 samples of every block per pass (a longer block takes
//           several passes, the lane's sum running on);
//   power   lane g * B + j sums its slot's samples in order from +0.0f, then the one correctly rounded division;
//   scan    the tile's blocks in order, the mean square of block j a ds_bpermute from lane g * B + j; every lane of a group runs its
//           channel's law, so no lane waits for another and nothing is broadcast back;
//   emit    a plain byte store into the channel's ring by lane j = 0 of the group.
// peak, floor and the nine integers run on from tile to tile in registers: the state rows are read and written once per launch.
#include "rx_host.h"

#include <cfloat>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace srx {

constexpr uint32_t kCdChunk = 32;                // samples of a DSP block staged per pass (8448 bytes of LDS per wave)
constexpr uint32_t kCdRow = kCdChunk + 1;        // words between the slots in LDS

template <int B>
__global__ __launch_bounds__(64) void k_cwdec(CwdecParams q, const float *__restrict__ audio)
{
    constexpr uint32_t G = kWave / B;            // channels of a wave
    __shared__ float rows[kWave * kCdRow];       // [slot = g * B + j][33]

    const uint32_t lane = threadIdx.x, g = lane / B, j = lane % B;
    const uint32_t c0 = blockIdx.x * G, c = c0 + g;
    const bool live = c < q.channels;
    const uint32_t n = q.n, nblk = q.nblk;
    const float fn = (float)n;
    const uint32_t ring_mask = q.ring - 1u;

    float peak = 0.0f, floor = 0.0f;
    uint32_t primed = 0u, key = 0u, flip = 0u, run = 0u, unit = q.unit_min, code = 1u, word = 0u;
    uint64_t count = 0u;
    if (live) {
        peak = q.peak[c]; floor = q.floor[c];
        primed = q.primed[c]; key = q.key[c]; flip = q.flip[c]; run = q.run[c]; unit = q.unit[c]; code = q.code[c]; word = q.word[c];
        count = q.count[c];
    }
    uint8_t *const text = q.text + (size_t)(live ? c : 0u) * q.ring;
    const bool writer = live && j == 0u;

    for (uint32_t b0 = 0; b0 < nblk; b0 += B) {
        const uint32_t nb = nblk - b0 < (uint32_t)B ? nblk - b0 : (uint32_t)B;       // blocks of this tile
        float sum = 0.0f;                        // arm_power_f32: from +0.0f
        for (uint32_t k0 = 0; k0 < n; k0 += kCdChunk) {
            const uint32_t kc = n - k0 < kCdChunk ? n - k0 : kCdChunk;
            // element e of the pass = sample e % kc of slot e / kc; e < 2048 and kc <= 32: (e * ceil(2^20 / kc)) >> 20 is e / kc exactly
            // (the error of the product is below e / 2^20 < 1 / 512 < 1 / kc), and e * magic < 2^32
            const uint32_t magic = ((1u << 20) + kc - 1u) / kc;
            __syncthreads();                     // (one wave: orders the LDS traffic across lanes for the compiler)
#pragma unroll 4
            for (uint32_t e = lane; e < kWave * kc; e += kWave) {
                const uint32_t slot = (e * magic) >> 20, i = e - slot * kc;
                const uint32_t ch = c0 + slot / B, sj = slot % B;
                if (ch < q.channels && sj < nb)
                    rows[slot * kCdRow + i] = audio[(size_t)ch * q.stride + (size_t)(b0 + sj) * n + k0 + i];
            }
            __syncthreads();
            if (live && j < nb) {
                const float *row = rows + lane * kCdRow;
#pragma unroll 8
                for (uint32_t i = 0; i < kc; ++i) {
                    const float v = row[i];
                    const float p = v * v;
                    sum = sum + p;
                }
            }
        }
        const float ms = __fdiv_rn(sum, fn);

        // the tile's blocks in order: every lane of group g runs channel g's law
#pragma unroll 1
        for (uint32_t jj = 0; jj < nb; ++jj) {   // (nb is wave-uniform: every lane takes part in the shuffle)
            const float m = __shfl(ms, (int)(g * B + jj));
            uint32_t raw = 0u;
            if (m <= FLT_MAX) {                  // (false for NaN: a NaN / Inf block leaves peak and floor, and reads as key-up)
                if (!primed) {
                    peak = m; floor = m; primed = 1u;
                } else {
                    const float rp = m > peak ? q.peak_attack : q.peak_decay;
                    const float dp = m - peak;
                    const float tp = rp * dp;
                    peak = peak + tp;
                    const float rf = m < floor ? q.floor_attack : q.floor_decay;
                    const float df = m - floor;
                    const float tf = rf * df;
                    floor = floor + tf;
                }
                const float span = peak - floor;
                const float f = key ? q.off_frac : q.on_frac;
                const float t = f * span;
                const float thr = floor + t;
                const float qq = q.snr * floor;
                const bool active = peak > qq && peak > q.min_power;
                raw = active && m > thr ? 1u : 0u;
            }
            bool edge = false;
            uint32_t ended = 0u;
            if (raw == key) {
                run = min(run + flip + 1u, 65535u);
                flip = 0u;
            } else {
                flip += 1u;
                if (flip >= q.debounce) { ended = run; key = raw; run = flip; flip = 0u; edge = true; }
            }
            if (edge && key == 0u) {             // a mark of `ended` blocks is over
                const uint32_t mk = ended << 8;
                const uint32_t dah = mk >= 2u * unit ? 1u : 0u;
                if (q.adapt) {
                    const uint32_t gl = dah ? mk / 3u : mk;
                    if (gl >= unit) unit += (gl - unit) >> q.track; else unit -= (unit - gl) >> q.track;
                    unit = min(max(unit, q.unit_min), q.unit_max);
                }
                code = (code == 0u || code >= 128u) ? 0u : ((code << 1) | dah);
            }
            if (key == 0u) {
                const uint32_t s = run << 8;
                if (code != 1u && s >= 2u * unit) {
                    if (writer) text[(uint32_t)count & ring_mask] = q.table[code & 255u];
                    count += 1u; code = 1u; word = 1u;
                }
                if (word && s >= 5u * unit) {
                    if (writer) text[(uint32_t)count & ring_mask] = (uint8_t)' ';
                    count += 1u; word = 0u;
                }
            }
        }
    }
    if (writer) {
        q.peak[c] = peak; q.floor[c] = floor;
        q.primed[c] = primed; q.key[c] = key; q.flip[c] = flip; q.run[c] = run; q.unit[c] = unit; q.code[c] = code; q.word[c] = word;
        q.count[c] = count;
    }
}

hipError_t launch_cwdec(const CwdecParams &q, const float *audio, hipStream_t st)
{
    if (q.channels == 0 || q.nblk == 0) return hipSuccess;
    if (q.n == 0 || (uint64_t)q.nblk * q.n > q.stride || q.ring == 0 || (q.ring & (q.ring - 1u))) return hipErrorInvalidValue;
    const dim3 blk(kWave);
#define SRX_CWDEC_LAUNCH(B) hipLaunchKernelGGL(k_cwdec<B>, dim3((q.channels + kWave / B - 1) / (kWave / B)), blk, 0, st, q, audio)
    if (q.nblk <= 1) SRX_CWDEC_LAUNCH(1);
    else if (q.nblk <= 2) SRX_CWDEC_LAUNCH(2);
    else if (q.nblk <= 4) SRX_CWDEC_LAUNCH(4);
    else if (q.nblk <= 8) SRX_CWDEC_LAUNCH(8);
    else if (q.nblk <= 16) SRX_CWDEC_LAUNCH(16);
    else if (q.nblk <= 32) SRX_CWDEC_LAUNCH(32);
    else SRX_CWDEC_LAUNCH(64);
#undef SRX_CWDEC_LAUNCH
    return hipGetLastError();
}

// ---- host side of the stage ----
void CwdecStage::release()
{
    dev_free(d_table, d_text);
    dev_free(d_peak, d_floor);
    dev_free(d_primed, d_key, d_flip, d_run, d_unit, d_code, d_word);
    dev_free(d_count);
    on = false;
    peak_attack = peak_decay = floor_attack = floor_decay = on_frac = off_frac = snr = min_power = 0.0f;
    debounce = adapt = track = unit_min = unit_init = unit_max = ring = 0;
}

// the stage's state as set_cwdec leaves it: +0.0f and 0, unit at unit_init, code 1 (the leading 1 alone), the ring zeros
int CwdecStage::init_state(selenite_rx_instance *S)
{
    if (!on) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels;
    HIPCHK(S, hipMemsetAsync(d_peak, 0, C * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(d_floor, 0, C * sizeof(float), S->stream));
    for (uint32_t *row : { d_primed, d_key, d_flip, d_run, d_word }) HIPCHK(S, hipMemsetAsync(row, 0, C * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_count, 0, C * sizeof(uint64_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_text, 0, C * ring, S->stream));
    const uint32_t one = 1u;
    if (int rc = fill_rows(S, d_code, C, &one)) return rc;
    return fill_rows(S, d_unit, C, &unit_init);             // (drains the stream)
}

// the stage's view of a launch: the channels and the audio geometry of `p`; the state rows and the rings move with the range
CwdecParams CwdecStage::params(ChanRange r, const RxParams &p) const
{
    const size_t c0 = r.first;
    CwdecParams q{};
    q.channels = p.channels; q.n = p.block / p.decim; q.nblk = p.block_size / p.block; q.stride = p.out_stride;
    q.peak_attack = peak_attack; q.peak_decay = peak_decay; q.floor_attack = floor_attack; q.floor_decay = floor_decay;
    q.on_frac = on_frac; q.off_frac = off_frac; q.snr = snr; q.min_power = min_power;
    q.debounce = debounce; q.adapt = adapt; q.track = track; q.unit_min = unit_min; q.unit_max = unit_max; q.ring = ring;
    q.table = d_table;
    q.peak = d_peak + c0; q.floor = d_floor + c0;
    q.primed = d_primed + c0; q.key = d_key + c0; q.flip = d_flip + c0; q.run = d_run + c0; q.unit = d_unit + c0; q.code = d_code + c0;
    q.word = d_word + c0; q.count = d_count + c0;
    q.text = d_text + c0 * ring;
    return q;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_cwdec(selenite_rx_instance *S, const selenite_rx_cwdec_config *f)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_cwdec: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    if (f) {
        auto rate = [](float v) { return std::isfinite(v) && v > 0.0f && v <= 1.0f; };
        const char *bad = nullptr;
        if (f->struct_size != sizeof(selenite_rx_cwdec_config)) bad = "struct_size is not sizeof(selenite_rx_cwdec_config)";
        else if (!rate(f->peak_attack)) bad = "peak_attack is not finite and in (0, 1]";
        else if (!rate(f->peak_decay)) bad = "peak_decay is not finite and in (0, 1]";
        else if (!rate(f->floor_attack)) bad = "floor_attack is not finite and in (0, 1]";
        else if (!rate(f->floor_decay)) bad = "floor_decay is not finite and in (0, 1]";
        else if (!(f->off_frac > 0.0f && f->off_frac <= f->on_frac && f->on_frac < 1.0f)) bad = "not 0 < off_frac <= on_frac < 1";
        else if (!(std::isfinite(f->snr) && f->snr >= 1.0f)) bad = "snr is not finite and >= 1";
        else if (!(std::isfinite(f->min_power) && f->min_power >= 0.0f)) bad = "min_power is not finite and >= 0";
        else if (f->debounce < 1u || f->debounce > 255u) bad = "debounce is not 1 .. 255";
        else if (f->adapt > 1u) bad = "adapt is not 0 or 1";
        else if (f->track > 8u) bad = "track is not 0 .. 8";
        else if (!(256u <= f->unit_min && f->unit_min <= f->unit_init && f->unit_init <= f->unit_max && f->unit_max <= 8192u * 256u))
            bad = "not 256 <= unit_min <= unit_init <= unit_max <= 8192 * 256";
        else if (f->ring < 16u || f->ring > 65536u || (f->ring & (f->ring - 1u))) bad = "ring is not a power of two, 16 .. 65536";
        if (bad) return refuse("selenite_rx_set_cwdec", bad);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    CwdecStage &st = S->cwdec;
    st.release();
    if (!f) return SELENITE_RX_SUCCESS;
    uint8_t table[256];
    if (f->table) std::memcpy(table, f->table, sizeof table);
    else (void)selenite_rx_design_morse(table, (uint8_t)'#');
    const size_t C = S->cfg.channels;
    hipError_t e = dev_alloc(&st.d_table, sizeof table);
    if (e == hipSuccess) e = dev_alloc(&st.d_text, C * f->ring);
    if (e == hipSuccess) e = dev_alloc(&st.d_peak, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_floor, C);
    for (uint32_t **row : { &st.d_primed, &st.d_key, &st.d_flip, &st.d_run, &st.d_unit, &st.d_code, &st.d_word })
        if (e == hipSuccess) e = dev_alloc(row, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_count, C);
    if (e == hipSuccess) e = hipMemcpy(st.d_table, table, sizeof table, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_cwdec: ") + hipGetErrorString(e));
    }
    st.on = true;
    st.peak_attack = f->peak_attack; st.peak_decay = f->peak_decay; st.floor_attack = f->floor_attack; st.floor_decay = f->floor_decay;
    st.on_frac = f->on_frac; st.off_frac = f->off_frac; st.snr = f->snr; st.min_power = f->min_power;
    st.debounce = f->debounce; st.adapt = f->adapt; st.track = f->track;
    st.unit_min = f->unit_min; st.unit_init = f->unit_init; st.unit_max = f->unit_max; st.ring = f->ring;
    return st.init_state(S);
}

static int cwdec_state_copy(selenite_rx_instance *S, const selenite_rx_cwdec_state_view *v, bool to_host)
{
    if (!S || !v || !S->cwdec.on) return SELENITE_RX_ARGUMENT_ERROR;
    const CwdecStage &st = S->cwdec;
    const size_t C = S->cfg.channels, W = C * sizeof(uint32_t);
    return copy_rows(S, to_host, { { st.d_peak, v->peak, C * sizeof(float) }, { st.d_floor, v->floor, C * sizeof(float) },
                                   { st.d_primed, v->primed, W }, { st.d_key, v->key, W }, { st.d_flip, v->flip, W }, { st.d_run, v->run, W },
                                   { st.d_unit, v->unit, W }, { st.d_code, v->code, W }, { st.d_word, v->word, W },
                                   { st.d_count, v->count, C * sizeof(uint64_t) }, { st.d_text, v->text, C * st.ring } });
}
extern "C" int selenite_rx_get_cwdec_state(selenite_rx_instance *S, const selenite_rx_cwdec_state_view *v) { return cwdec_state_copy(S, v, true); }
extern "C" int selenite_rx_set_cwdec_state(selenite_rx_instance *S, const selenite_rx_cwdec_state_view *v) { return cwdec_state_copy(S, v, false); }

extern "C" int selenite_rx_get_cwdec(selenite_rx_instance *S, uint8_t *text, uint64_t *count, uint32_t *unit, uint32_t *key)
{
    if (!S || !S->cwdec.on) return SELENITE_RX_ARGUMENT_ERROR;
    const CwdecStage &st = S->cwdec;
    const size_t C = S->cfg.channels;
    return copy_rows(S, true, { { st.d_text, text, C * st.ring }, { st.d_count, count, C * sizeof(uint64_t) },
                                { st.d_unit, unit, C * sizeof(uint32_t) }, { st.d_key, key, C * sizeof(uint32_t) } });
}
extern "C" const uint8_t *selenite_rx_cwdec_text_device(const selenite_rx_instance *S) { return S && S->cwdec.on ? S->cwdec.d_text : nullptr; }
extern "C" const uint64_t *selenite_rx_cwdec_count_device(const selenite_rx_instance *S) { return S && S->cwdec.on ? S->cwdec.d_count : nullptr; }
extern "C" const uint32_t *selenite_rx_cwdec_unit_device(const selenite_rx_instance *S) { return S && S->cwdec.on ? S->cwdec.d_unit : nullptr; }
