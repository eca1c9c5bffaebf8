// rx_meter.hip -- signal-level meter and squelch (step 4c of DESIGN.md section 2, section 5.11): per channel and per DSP block of
// n = block / decim UN-SCALED audio samples x -- the demodulator's output, behind the CW filter and behind NLMS when that is on, in front of
// the AGC:
//     pw = arm_power_f32(x, n)          StatisticsFunctions/arm_power_f32.c:64-125: sum = +0.0f; sum = sum + in * in, n ascending
//     ms = pw / (float)n                correctly rounded division (n is any block / decim: 24 is not a power of two)
//     ms <= FLT_MAX (false for NaN):    r = ms > level ? attack : decay; d = ms - level; level = level + r * d      (the AGC's form)
//     otherwise:                        level stays
//     want_open  = sense == ABOVE ? level > open_level  : level < open_level
//     want_close = sense == ABOVE ? level < close_level : level > close_level
//     if (!open)           { if (want_open) { open = 1; hold = hang; opens += 1; } }
//     else if (want_close) { if (hold == 0) open = 0; else hold -= 1; }
//     else                   hold = hang;
//     open_blocks += open
// and, with gate == 1, a block whose open is 0 after its update leaves the call as +0.0f (int16 slots: 0) -- BEHIND the AGC, which runs on
// the un-scaled audio of every block as it does without the stage (k_gate, the last launch of the dispatcher's run_part).
//
// Every operation above is kept, in that order, and the unit is compiled with -ffp-contract=off, IEEE denormals and correctly rounded
// division: bit-exact given its input in every arith mode.  The stage never touches the NaN / Inf flag word.
//
// k_meter<B>: single-wave workgroups; one wavefront owns the state of the channels it serves.  A block's sum is strictly sequential, so the
// parallelism is across blocks and channels: a tile is B consecutive DSP blocks of 64 / B consecutive channels (B = the power of two that
// holds the call's blocks, at most 64: cfg3's call of 16 blocks puts 4 channels in a wave, a call of 375 blocks runs one channel per wave
// in 6 tiles), lane g * B + j owning block j of channel g:
//   load    the tile's audio rows, coalesced (the B blocks of a channel are B * n consecutive floats), into LDS at slot * 33 + i, at most 32
//           samples of every block per pass (a longer block takes several passes, the lane's sum running on): one word of padding per slot;
//   power   lane g * B + j sums its slot's samples in order: the lanes read 33 words apart, conflict-free on the 32 banks;
//   scan    the tile's blocks in order, every lane of a channel's group computing that channel's level, open and hold (the mean square of
//           block j is a ds_bpermute from lane g * B + j); lane g * B + j keeps the gate bit behind block j and stores it; the counters
//           are integers;
// level, open, hold and the counters run on from tile to tile in registers.
// k_gate<TOut>: one wave per channel reads the call's gate bytes, 64 at a time, and writes zeros over the closed blocks of dst (a wave
// ballot, then one pass of whole-wave stores per closed block).  Open blocks are not touched, nothing else is read.
#include "rx_host.h"

#include <cfloat>
#include <cmath>
#include <vector>

namespace srx {

constexpr uint32_t kMtChunk = 32;                // samples of a DSP block staged per pass (8448 bytes of LDS per wave: 19 waves per CU)
constexpr uint32_t kMtRow = kMtChunk + 1;        // words between the slots in LDS

template <int B>
__global__ __launch_bounds__(64) void k_meter(MeterParams q, const float *__restrict__ audio)
{
    constexpr uint32_t G = kWave / B;            // channels of a wave
    __shared__ float rows[kWave * kMtRow];       // [slot = g * B + j][33]

    const uint32_t lane = threadIdx.x, g = lane / B, j = lane % B;
    const uint32_t c0 = blockIdx.x * G, c = c0 + g;
    const bool live = c < q.channels;
    const uint32_t n = q.n, nblk = q.nblk;
    const float fn = (float)n;
    const bool above = q.sense == SELENITE_RX_SQ_ABOVE;

    float level = 0.0f;
    uint32_t open = 0u, hold = 0u, opens = 0u, open_blocks = 0u;
    if (live) { level = q.level[c]; open = q.open[c]; hold = q.hold[c]; }

    for (uint32_t b0 = 0; b0 < nblk; b0 += B) {
        const uint32_t nb = nblk - b0 < (uint32_t)B ? nblk - b0 : (uint32_t)B;       // blocks of this tile
        float sum = 0.0f;                        // arm_power_f32: from +0.0f
        for (uint32_t k0 = 0; k0 < n; k0 += kMtChunk) {
            const uint32_t kc = n - k0 < kMtChunk ? n - k0 : kMtChunk;
            // element e of the pass = sample e % kc of slot e / kc; e < 2048 and kc <= 32: (e * ceil(2^20 / kc)) >> 20 is e / kc exactly
            // (the error of the product is below e / 2^20 < 1 / 512 < 1 / kc), and e * magic < 2^32
            const uint32_t magic = ((1u << 20) + kc - 1u) / kc;
            __syncthreads();                     // (one wave: orders the LDS traffic across lanes for the compiler)
#pragma unroll 4
            for (uint32_t e = lane; e < kWave * kc; e += kWave) {
                const uint32_t slot = (e * magic) >> 20, i = e - slot * kc;
                const uint32_t ch = c0 + slot / B, sj = slot % B;
                if (ch < q.channels && sj < nb)
                    rows[slot * kMtRow + i] = audio[(size_t)ch * q.stride + (size_t)(b0 + sj) * n + k0 + i];
            }
            __syncthreads();
            if (live && j < nb) {
                const float *row = rows + lane * kMtRow;
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
        uint32_t mine = 0u;
#pragma unroll 4
        for (uint32_t jj = 0; jj < (uint32_t)B; ++jj) {
            const float m = __shfl(ms, (int)(g * B + jj));
            if (jj < nb) {
                if (m <= FLT_MAX) {              // (false for NaN: a NaN / Inf block leaves the level)
                    const float r = m > level ? q.attack : q.decay;
                    const float d = m - level;
                    const float s = r * d;
                    level = level + s;
                }
                const bool want_open = above ? level > q.open_level : level < q.open_level;
                const bool want_close = above ? level < q.close_level : level > q.close_level;
                if (!open) {
                    if (want_open) { open = 1u; hold = q.hang; opens += 1u; }
                } else if (want_close) {
                    if (hold == 0u) open = 0u; else hold -= 1u;
                } else {
                    hold = q.hang;
                }
                open_blocks += open;
                if (j == jj) mine = open;
            }
        }
        if (live && j < nb) q.bits[(size_t)c * nblk + b0 + j] = (uint8_t)mine;
    }
    if (live && j == 0u) {
        q.level[c] = level; q.open[c] = open; q.hold[c] = hold;
        q.opens[c] += opens; q.open_blocks[c] += open_blocks;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void k_gate(MeterParams q, T *__restrict__ dst)
{
    const uint32_t lane = threadIdx.x, c = blockIdx.x, n = q.n, nblk = q.nblk;
    const uint8_t *bits = q.bits + (size_t)c * nblk;
    T *row = dst + (size_t)c * q.stride;
    for (uint32_t b0 = 0; b0 < nblk; b0 += kWave) {
        const uint32_t b = b0 + lane;
        uint64_t closed = __ballot(b < nblk && bits[b] == 0);
        while (closed) {                         // wave-uniform: the closed blocks of these 64, in order
            const uint32_t k = (uint32_t)__ffsll((unsigned long long)closed) - 1u;
            closed &= closed - 1u;
            T *x = row + (size_t)(b0 + k) * n;
            for (uint32_t i = lane; i < n; i += kWave) x[i] = T(0);
        }
    }
}

hipError_t launch_meter(const MeterParams &q, const float *audio, hipStream_t st)
{
    if (q.channels == 0 || q.nblk == 0) return hipSuccess;
    if (q.n == 0 || (uint64_t)q.nblk * q.n > q.stride) return hipErrorInvalidValue;
    const dim3 blk(kWave);
#define SRX_METER_LAUNCH(B) hipLaunchKernelGGL(k_meter<B>, dim3((q.channels + kWave / B - 1) / (kWave / B)), blk, 0, st, q, audio)
    if (q.nblk <= 1) SRX_METER_LAUNCH(1);
    else if (q.nblk <= 2) SRX_METER_LAUNCH(2);
    else if (q.nblk <= 4) SRX_METER_LAUNCH(4);
    else if (q.nblk <= 8) SRX_METER_LAUNCH(8);
    else if (q.nblk <= 16) SRX_METER_LAUNCH(16);
    else if (q.nblk <= 32) SRX_METER_LAUNCH(32);
    else SRX_METER_LAUNCH(64);
#undef SRX_METER_LAUNCH
    return hipGetLastError();
}

hipError_t launch_gate(const MeterParams &q, void *dst, bool dst_q15, hipStream_t st)
{
    if (q.channels == 0 || q.nblk == 0) return hipSuccess;
    if (q.n == 0 || (uint64_t)q.nblk * q.n > q.stride) return hipErrorInvalidValue;
    const dim3 grid(q.channels), blk(kWave);
    if (dst_q15) hipLaunchKernelGGL(k_gate<int16_t>, grid, blk, 0, st, q, static_cast<int16_t *>(dst));
    else hipLaunchKernelGGL(k_gate<float>, grid, blk, 0, st, q, static_cast<float *>(dst));
    return hipGetLastError();
}

// ---- host side of the stage ----
void MeterStage::release()
{
    dev_free(d_level, d_open, d_hold, d_opens, d_open_blocks, d_bits);
    bits_bytes = 0;
    on = false;
    sense = gate = hang = 0;
    attack = decay = open_level = close_level = level_init = 0.0f;
}

// the stage's state as set_meter leaves it: level at the config's init, the gate closed, the counters 0
int MeterStage::init_state(selenite_rx_instance *S)
{
    if (!on) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels;
    HIPCHK(S, hipMemsetAsync(d_open, 0, C * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_hold, 0, C * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_opens, 0, C * sizeof(uint64_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_open_blocks, 0, C * sizeof(uint64_t), S->stream));
    return fill_rows(S, d_level, C, &level_init);           // (drains the stream)
}

// the stage's view of a launch: the channels and the audio geometry of `p`; the state rows and the gate bytes move with the range
MeterParams MeterStage::params(ChanRange r, const RxParams &p) const
{
    const size_t c0 = r.first;
    MeterParams q{};
    q.channels = p.channels; q.n = p.block / p.decim; q.nblk = p.block_size / p.block; q.stride = p.out_stride;
    q.sense = sense; q.hang = hang;
    q.attack = attack; q.decay = decay; q.open_level = open_level; q.close_level = close_level;
    q.level = d_level + c0; q.open = d_open + c0; q.hold = d_hold + c0; q.opens = d_opens + c0; q.open_blocks = d_open_blocks + c0;
    q.bits = d_bits + c0 * q.nblk;
    return q;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_meter(selenite_rx_instance *S, const selenite_rx_meter_config *m)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_meter: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    if (m) {
        const char *bad = nullptr;
        if (m->struct_size != sizeof(selenite_rx_meter_config)) bad = "struct_size is not sizeof(selenite_rx_meter_config)";
        else if (m->sense != SELENITE_RX_SQ_ABOVE && m->sense != SELENITE_RX_SQ_BELOW) bad = "sense is not a SELENITE_RX_SQ_* value";
        else if (m->gate > 1u) bad = "gate is not 0 or 1";
        else if (m->hang > 65535u) bad = "hang is not 0 .. 65535";
        else if (!(m->attack > 0.0f && m->attack <= 1.0f)) bad = "attack is not in (0, 1]";
        else if (!(m->decay > 0.0f && m->decay <= 1.0f)) bad = "decay is not in (0, 1]";
        else if (!(std::isfinite(m->open_level) && m->open_level >= 0.0f)) bad = "open_level is not finite and >= 0";
        else if (!(std::isfinite(m->close_level) && m->close_level >= 0.0f)) bad = "close_level is not finite and >= 0";
        else if (m->sense == SELENITE_RX_SQ_ABOVE && !(m->close_level <= m->open_level)) bad = "SELENITE_RX_SQ_ABOVE: close_level is above open_level";
        else if (m->sense == SELENITE_RX_SQ_BELOW && !(m->close_level >= m->open_level)) bad = "SELENITE_RX_SQ_BELOW: close_level is below open_level";
        else if (!(std::isfinite(m->level_init) && m->level_init >= 0.0f)) bad = "level_init is not finite and >= 0";
        if (bad) return refuse("selenite_rx_set_meter", bad);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    MeterStage &st = S->meter;
    st.release();
    if (!m) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels;
    hipError_t e = dev_alloc(&st.d_level, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_open, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_hold, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_opens, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_open_blocks, C);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_meter: hipMalloc: ") + hipGetErrorString(e));
    }
    st.on = true;
    st.sense = m->sense; st.gate = m->gate; st.hang = m->hang;
    st.attack = m->attack; st.decay = m->decay; st.open_level = m->open_level; st.close_level = m->close_level; st.level_init = m->level_init;
    return st.init_state(S);
}

static int meter_state_copy(selenite_rx_instance *S, const selenite_rx_meter_state_view *v, bool to_host)
{
    if (!S || !v || !S->meter.on) return SELENITE_RX_ARGUMENT_ERROR;
    const MeterStage &st = S->meter;
    const size_t C = S->cfg.channels;
    return copy_rows(S, to_host, { { st.d_level, v->level, C * sizeof(float) }, { st.d_open, v->open, C * sizeof(uint32_t) },
                                   { st.d_hold, v->hold, C * sizeof(uint32_t) }, { st.d_opens, v->opens, C * sizeof(uint64_t) },
                                   { st.d_open_blocks, v->open_blocks, C * sizeof(uint64_t) } });
}
extern "C" int selenite_rx_get_meter_state(selenite_rx_instance *S, const selenite_rx_meter_state_view *v) { return meter_state_copy(S, v, true); }
extern "C" int selenite_rx_set_meter_state(selenite_rx_instance *S, const selenite_rx_meter_state_view *v) { return meter_state_copy(S, v, false); }
extern "C" const float *selenite_rx_meter_level_device(const selenite_rx_instance *S) { return S && S->meter.on ? S->meter.d_level : nullptr; }
extern "C" const uint32_t *selenite_rx_meter_open_device(const selenite_rx_instance *S) { return S && S->meter.on ? S->meter.d_open : nullptr; }
