// rx_tones.hip -- tone-detector bank (step 4-t of DESIGN.md section 2, section 5.13): the power at K known frequencies per channel -- CTCSS,
// DTMF, selective calling, a 1750 Hz burst, a CW pitch indicator.  A TAP on the UN-SCALED audio behind the demodulator and the CW filter, in
// front of the audio filter, NLMS, the level meter and the AGC: it reads the audio and changes none of it.  The audio of a channel is one
// stream; a frame is frame_blocks consecutive DSP blocks of n = block / decim samples, N = frame_blocks * n, counted from set_tones / reset.
// Per sample x and tone k, state s1, s2 (+0.0f at a frame's start), the Goertzel recurrence in three rounded operations:
//     t = c * s1;  s0 = x + t;  s0 = s0 - s2;  s2 = s1;  s1 = s0                       c = 2 cos w
// (arm_biquad_cascade_df1_f32 with the one section {1, 0, 0, c, -1} less its two dead products 0 * x1, 0 * x2: the same bits on finite input
// that holds no -0.0f), and once per channel the frame energy of arm_power_f32, from +0.0f at a frame's start:
//     e = x * x;  E = E + e
// At the frame's last sample, per tone (the form of arm_cmplx_mag_squared_f32):
//     u = cw * s2;  re = s1 - u;  im = sw * s2;  a = re * re;  b = im * im;  p[k] = a + b
// then per channel
//     (p_best, best) = arm_max_f32(p, K)          the first index of the maximum; a NaN wins only at index 0
//     t = ratio * E;  t = t * (float)N;  hit = p_best > t && p_best > min_power && p_best <= FLT_MAX;  w = hit ? best : NONE
//     if (w == cand) run = min(run + 1, 65535); else { cand = w; run = 1; }
//     if (cand != tone && run >= (cand == NONE ? release : confirm)) { tone = cand; changes += 1; }
//     power[k] = p[k];  frame_energy = E;  last_best = best;  s1 = s2 = E = +0.0f
// Every operation is rounded to f32 in that order; the unit is compiled with -ffp-contract=off and IEEE denormals: bit-exact given its
// input in every arith mode, whatever the cut of the stream into calls.  The stage never touches the NaN / Inf flag word.
//
// k_tones<KL>: the recurrence has no time parallelism at this rounding, so the parallelism is channels x tones.  Single-wave workgroups;
// KL = 8, 16, 32 or 64 tone lanes per channel (the power of two that holds K), lane = KL * g + k: 64 / KL channels per wave.  A lane keeps
// c, cw, sw, s1, s2 in registers for the whole launch.  The rows of the wave's channels stream through LDS in tiles of kTnTile = 64 samples
// (one wave load per row piece: 256 bytes, coalesced; rows need no alignment) as pairs { x, x * x }, rows 65 pairs apart: the square of a
// sample is computed once, by the lane that stages it.  A step reads the pair of the lane's channel as an LDS broadcast and is three vector
// instructions: the product c * s1, ONE packed add { x + t, e + E } that carries the tone's sum and the energy's (every lane of a channel
// carries E: no lane is set apart, no select in the loop), and the difference.
// The loads of tile t + 1 are in flight under the steps of tile t.  The frame position is the same for every channel (one `position`), so
// a frame end inside a tile is wave-uniform: the tile's steps run in segments that end where a frame ends, and behind such a segment the
// KL lanes of a channel reduce (p, index) by a butterfly that keeps arm_max_f32's order -- the larger value, on a tie the lower index, a
// NaN never taken except at index 0 -- and lane 0 of the channel takes the integer decision.  Lanes k >= K load no coefficient and no
// state, store nothing and never enter the reduction.
#include "rx_host.h"

#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace srx {

constexpr int kTnTile = 64;                      // samples of a channel row per tile: one wave load
constexpr int kTnRow = kTnTile + 1;              // {x, x * x} pairs between the rows in LDS
typedef float tn_v2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void tn_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int KL>
__global__ __launch_bounds__(64) void k_tones(TonesParams q, const float *__restrict__ audio)
{
    constexpr int G = 64 / KL;
    __shared__ tn_v2 tile[G * kTnRow];           // [G] rows of { x, x * x }

    const int lane = threadIdx.x;
    const uint32_t g = (uint32_t)lane / KL, k = (uint32_t)lane % KL;
    const uint32_t K = q.n_tones, nout = q.nout;
    const uint32_t c0 = blockIdx.x * G, c = c0 + g;
    const uint32_t nrow = min((uint32_t)G, q.channels - c0);                  // channel rows of this wave
    const bool chan = c < q.channels, live = chan && k < K;

    float kc = 0.0f, kcw = 0.0f, ksw = 0.0f, s1 = 0.0f, s2 = 0.0f, E = 0.0f;
    float *const s_row = q.s + ((size_t)c * K + k) * 2;
    if (live) {
        kc = q.coeffs[k * 3]; kcw = q.coeffs[k * 3 + 1]; ksw = q.coeffs[k * 3 + 2];
        const float2 st = *reinterpret_cast<const float2 *>(s_row);
        s1 = st.x; s2 = st.y;
    }
    if (chan) E = q.energy[c];

    // the wave's piece of tile t: row r = 64 consecutive floats of channel c0 + r
    float pre[G];
    auto load_tile = [&](uint32_t t) {
        const uint32_t i = t * kTnTile + (uint32_t)lane;
#pragma unroll
        for (int r = 0; r < G; ++r)
            pre[r] = ((uint32_t)r < nrow && i < nout) ? audio[(size_t)(c0 + r) * q.stride + i] : 0.0f;
    };
    auto put_tile = [&]() {
#pragma unroll
        for (int r = 0; r < G; ++r) {
            const float x = pre[r];
            tile[r * kTnRow + lane] = tn_v2{ x, x * x };
        }
    };
    const uint32_t ntile = (nout + kTnTile - 1) / kTnTile;
    load_tile(0);
    put_tile();
    if (ntile > 1) load_tile(1);
    tn_lds_sync();

    const tn_v2 *const row = tile + g * kTnRow;
    const uint32_t frame_n = q.frame_blocks * q.n;                            // N
    uint32_t left = frame_n - q.fb0 * q.n;                                    // samples to the end of the running frame

    for (uint32_t t = 0; t < ntile; ++t) {
        const uint32_t tn = min((uint32_t)kTnTile, nout - t * kTnTile);       // samples of this tile
        uint32_t i = 0;
        while (i < tn) {
            const uint32_t seg = min(tn - i, left);                           // wave-uniform
            const uint32_t end = i + seg;
#pragma unroll 4
            for (; i < end; ++i) {                                            // mul, one packed add { x + t, e + E }, sub
                tn_v2 te = { kc * s1, E };
                te = row[i] + te;
                const float s0 = te.x - s2;
                s2 = s1;
                s1 = s0;
                E = te.y;
            }
            left -= seg;
            if (left == 0) {                                                  // a frame ends behind sample i - 1
                const float u = kcw * s2;
                const float re = s1 - u;
                const float im = ksw * s2;
                const float a = re * re;
                const float b = im * im;
                const float p = a + b;
                // arm_max_f32 over the K lanes of the channel: value, index, `ok` = in the running
                float v = p;
                uint32_t bi = k;
                bool ok = k < K && !(p != p);
#pragma unroll
                for (int m = 1; m < KL; m <<= 1) {
                    const float ov = __shfl_xor(v, m);
                    const uint32_t oi = (uint32_t)__shfl_xor((int)bi, m);
                    const bool ook = __shfl_xor((int)ok, m) != 0;
                    const bool take = ook && (!ok || ov > v || (ov == v && oi < bi));
                    if (take) { v = ov; bi = oi; ok = true; }
                }
                const float p0 = __shfl(p, (int)(g * KL));
                if (p0 != p0) { v = p0; bi = 0u; }                            // a NaN at index 0 stays
                if (live) q.power[(size_t)c * K + k] = p;
                if (chan && k == 0u) {
                    float th = q.ratio * E;
                    th = th * (float)frame_n;
                    const bool hit = v > th && v > q.min_power && v <= FLT_MAX;
                    const uint32_t w = hit ? bi : SELENITE_RX_TONE_NONE;
                    uint32_t tone = q.tone[c], cand = q.cand[c], run = q.run[c];
                    if (w == cand) run = min(run + 1u, 65535u); else { cand = w; run = 1u; }
                    if (cand != tone && run >= (cand == SELENITE_RX_TONE_NONE ? q.release : q.confirm)) {
                        tone = cand;
                        q.changes[c] += 1u;
                    }
                    q.tone[c] = tone; q.cand[c] = cand; q.run[c] = run;
                    q.frame_energy[c] = E; q.last_best[c] = bi;
                }
                s1 = 0.0f; s2 = 0.0f; E = 0.0f;
                left = frame_n;
            }
        }
        tn_lds_sync();
        if (t + 1 < ntile) {
            put_tile();
            if (t + 2 < ntile) load_tile(t + 2);
            tn_lds_sync();
        }
    }
    if (live) *reinterpret_cast<float2 *>(s_row) = make_float2(s1, s2);
    if (chan && k == 0u) q.energy[c] = E;
}

hipError_t launch_tones(const TonesParams &q, const float *audio, hipStream_t st)
{
    if (q.channels == 0) return hipSuccess;
    if (q.nout == 0 || q.nout > q.stride || q.n == 0 || q.nout % q.n != 0 || q.n_tones == 0 || q.n_tones > SELENITE_RX_TONES_MAX ||
        q.frame_blocks == 0 || q.fb0 >= q.frame_blocks)
        return hipErrorInvalidValue;
#define SRX_TONES_LAUNCH(KL) hipLaunchKernelGGL(k_tones<KL>, dim3((q.channels + 64 / KL - 1) / (64 / KL)), dim3(kWave), 0, st, q, audio)
    if (q.n_tones <= 8) SRX_TONES_LAUNCH(8);
    else if (q.n_tones <= 16) SRX_TONES_LAUNCH(16);
    else if (q.n_tones <= 32) SRX_TONES_LAUNCH(32);
    else SRX_TONES_LAUNCH(64);
#undef SRX_TONES_LAUNCH
    return hipGetLastError();
}

// ---- host side of the stage ----
void TonesStage::release()
{
    dev_free(d_coeffs, d_s, d_energy, d_power, d_frame_energy);
    dev_free(d_last_best, d_tone, d_cand, d_run);
    dev_free(d_changes);
    on = false;
    n_tones = frame_blocks = confirm = rel = 0;
    ratio = min_power = 0.0f;
    pos = 0;
}

// the stage's state as set_tones leaves it: +0.0f, the counters 0, tone and cand NONE, the stream at its start
int TonesStage::init_state(selenite_rx_instance *S)
{
    if (!on) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels, K = n_tones;
    HIPCHK(S, hipMemsetAsync(d_s, 0, C * K * 2 * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(d_energy, 0, C * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(d_power, 0, C * K * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(d_frame_energy, 0, C * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(d_last_best, 0, C * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_tone, 0xFF, C * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_cand, 0xFF, C * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_run, 0, C * sizeof(uint32_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_changes, 0, C * sizeof(uint64_t), S->stream));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    pos = 0;
    return SELENITE_RX_SUCCESS;
}

// the stage's view of a launch: the channels and the audio geometry of `p`; the state rows move with the range.  blocks_before: the DSP
// blocks of this call that earlier launches of it have run (the second part of a cut call)
TonesParams TonesStage::params(ChanRange r, const RxParams &p, uint32_t blocks_before) const
{
    const size_t c0 = r.first;
    TonesParams q{};
    q.channels = p.channels; q.nout = p.nout; q.stride = p.out_stride; q.n = p.block / p.decim;
    q.n_tones = n_tones; q.frame_blocks = frame_blocks; q.fb0 = (uint32_t)((pos + blocks_before) % frame_blocks);
    q.confirm = confirm; q.release = rel; q.ratio = ratio; q.min_power = min_power;
    q.coeffs = d_coeffs;
    q.s = d_s + c0 * n_tones * 2; q.energy = d_energy + c0; q.power = d_power + c0 * n_tones; q.frame_energy = d_frame_energy + c0;
    q.last_best = d_last_best + c0; q.tone = d_tone + c0; q.cand = d_cand + c0; q.run = d_run + c0; q.changes = d_changes + c0;
    return q;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_tones(selenite_rx_instance *S, const selenite_rx_tones_config *f)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_tones: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    if (f) {
        const char *bad = nullptr;
        if (f->struct_size != sizeof(selenite_rx_tones_config)) bad = "struct_size is not sizeof(selenite_rx_tones_config)";
        else if (f->n_tones < 1u || f->n_tones > SELENITE_RX_TONES_MAX) bad = "n_tones is not 1 .. 64";
        else if (f->frame_blocks < 1u || f->frame_blocks > 65535u) bad = "frame_blocks is not 1 .. 65535";
        else if ((uint64_t)f->frame_blocks * (S->cfg.block / S->cfg.decim) >= (1ull << 31)) bad = "a frame of frame_blocks DSP blocks is 2^31 samples or more";
        else if (f->confirm < 1u || f->confirm > 65535u) bad = "confirm is not 1 .. 65535";
        else if (f->release < 1u || f->release > 65535u) bad = "release is not 1 .. 65535";
        else if (f->reserved != 0u) bad = "reserved is not 0";
        else if (!(std::isfinite(f->ratio) && f->ratio >= 0.0f && f->ratio <= 1.0f)) bad = "ratio is not finite and in [0, 1]";
        else if (!(std::isfinite(f->min_power) && f->min_power >= 0.0f)) bad = "min_power is not finite and >= 0";
        else if (!f->coeffs) bad = "coeffs is NULL";
        else
            for (size_t i = 0; i < (size_t)f->n_tones * 3; ++i)
                if (!std::isfinite(f->coeffs[i])) bad = "a coefficient is not finite";
        if (bad) return refuse("selenite_rx_set_tones", bad);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    TonesStage &st = S->tones;
    st.release();
    if (!f) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels, K = f->n_tones;
    hipError_t e = dev_alloc(&st.d_coeffs, K * 3);
    if (e == hipSuccess) e = dev_alloc(&st.d_s, C * K * 2);
    if (e == hipSuccess) e = dev_alloc(&st.d_energy, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_power, C * K);
    if (e == hipSuccess) e = dev_alloc(&st.d_frame_energy, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_last_best, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_tone, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_cand, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_run, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_changes, C);
    if (e == hipSuccess) e = hipMemcpy(st.d_coeffs, f->coeffs, K * 3 * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_tones: ") + hipGetErrorString(e));
    }
    st.on = true;
    st.n_tones = f->n_tones; st.frame_blocks = f->frame_blocks; st.confirm = f->confirm; st.rel = f->release;
    st.ratio = f->ratio; st.min_power = f->min_power;
    return st.init_state(S);
}

static int tones_state_copy(selenite_rx_instance *S, const selenite_rx_tones_state_view *v, bool to_host)
{
    if (!S || !v || !S->tones.on) return SELENITE_RX_ARGUMENT_ERROR;
    TonesStage &st = S->tones;
    const size_t C = S->cfg.channels, K = st.n_tones;
    if (int rc = copy_rows(S, to_host, { { st.d_s, v->s, C * K * 2 * sizeof(float) }, { st.d_energy, v->energy, C * sizeof(float) },
                                         { st.d_power, v->power, C * K * sizeof(float) }, { st.d_frame_energy, v->frame_energy, C * sizeof(float) },
                                         { st.d_last_best, v->last_best, C * sizeof(uint32_t) }, { st.d_tone, v->tone, C * sizeof(uint32_t) },
                                         { st.d_cand, v->cand, C * sizeof(uint32_t) }, { st.d_run, v->run, C * sizeof(uint32_t) },
                                         { st.d_changes, v->changes, C * sizeof(uint64_t) } })) return rc;
    if (v->position) {
        if (to_host) *v->position = st.pos;
        else st.pos = *v->position;
    }
    return SELENITE_RX_SUCCESS;
}
extern "C" int selenite_rx_get_tones_state(selenite_rx_instance *S, const selenite_rx_tones_state_view *v) { return tones_state_copy(S, v, true); }
extern "C" int selenite_rx_set_tones_state(selenite_rx_instance *S, const selenite_rx_tones_state_view *v) { return tones_state_copy(S, v, false); }

extern "C" int selenite_rx_get_tones(selenite_rx_instance *S, uint32_t *tone, float *power, uint64_t *frames)
{
    if (!S || !S->tones.on) return SELENITE_RX_ARGUMENT_ERROR;
    const TonesStage &st = S->tones;
    const size_t C = S->cfg.channels;
    if (int rc = copy_rows(S, true, { { st.d_tone, tone, C * sizeof(uint32_t) }, { st.d_power, power, C * st.n_tones * sizeof(float) } })) return rc;
    if (frames) *frames = st.pos / st.frame_blocks;
    return SELENITE_RX_SUCCESS;
}
extern "C" const uint32_t *selenite_rx_tones_tone_device(const selenite_rx_instance *S) { return S && S->tones.on ? S->tones.d_tone : nullptr; }
extern "C" const float *selenite_rx_tones_power_device(const selenite_rx_instance *S) { return S && S->tones.on ? S->tones.d_power : nullptr; }
