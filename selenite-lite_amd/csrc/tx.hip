// tx.hip -- batched TX chain (include/selenite_tx.h): ALC -> Hilbert pair -> sideband select ->
// arm_fir_interpolate_f32 by L -> NCO up-mix, one wavefront per channel, ALC block by ALC block.
// Arithmetic contract as in rx_device.h: every step keeps the CMSIS-DSP 1.5.3 operation order
// (oracle/tx_oracle.c restates it, oracle/ref_tx.c composes the real functions); SELENITE_ARITH_FMA
// fuses the FIR tap loops only.  This is the "any configuration" kernel of the TX direction (the
// counterpart of rx_generic.hip): plain LDS arrays, runtime tap loops, coalesced 8-byte I/Q stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/selenite_tx.h"
#include "rx_device.h"
#include "rx_internal.h"
#include "tx_internal.h"

struct selenite_tx_instance {
    selenite_tx_config cfg;
    int device = 0;
    float *d_ic = nullptr, *d_hc = nullptr, *d_dc = nullptr, *d_sintab = nullptr;
    uint32_t *d_step = nullptr, *d_phase = nullptr;
    float *d_fir_state = nullptr, *d_int_state = nullptr, *d_gain = nullptr;
    void *d_io_in = nullptr, *d_io_out = nullptr;
    size_t io_in_bytes = 0, io_out_bytes = 0;
    std::vector<uint32_t> h_step;
    // fused-kernel planning (tx_fused.hip) and the shared LO of a call
    bool delay_is_impulse = false, hilb_odd_only = false, phase_uniform = true, steps_same = true, force_generic = false, no_periodic_lo = false;
    uint32_t delay_index = 0, phase_host = 0;
    float2 *d_lo = nullptr;
    bool lo_valid = false; uint32_t lo_phase = 0, lo_step = 0, lo_n = 0;   // what d_lo holds
    size_t lo_bytes = 0;
    void *d_ttab16 = nullptr;     // k_tx_split16: Toeplitz fragments of the interpolator phases
    int tpost = 0;                // tap scale exponent of that table
    // SELENITE_MODE_FM (selenite_tx_set_fm, tx_fm.hip)
    bool fm_set = false;
    srx::TxFmParams fm{};         // d_tone_step / d_tone_phase live as long as the instance once allocated
    uint32_t *d_tone_step = nullptr, *d_tone_phase = nullptr;
    // keyed CW (selenite_tx_set_cw, tx_cw.hip); cw.offset holds + offset_step, the mode's sign is applied per call
    bool cw_set = false;
    srx::TxCwParams cw{};
    float *d_shape = nullptr;
    uint32_t *d_side_step = nullptr, *d_side_phase = nullptr, *d_tx_on = nullptr, *d_hold = nullptr;
    uint8_t *d_key_state = nullptr;
    void *d_io_side = nullptr;
    size_t io_side_bytes = 0;
    // the audio input stage (selenite_tx_set_in, tx_in.hip); in.coeffs, in.dec_state and the VOX rows are the d_in_* below
    bool in_set = false;
    srx::TxInParams in{};
    float in_level_init = 0.0f;
    float *d_in_coeffs = nullptr, *d_in_dec = nullptr, *d_in_level = nullptr;
    uint32_t *d_in_open = nullptr, *d_in_hold = nullptr;
    uint64_t *d_in_opens = nullptr, *d_in_open_blocks = nullptr;
    void *d_in_audio = nullptr;   // the stage's output of the last frame call: what run() then reads
    size_t in_audio_bytes = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;
    int status = 0;
    std::string err;
};

namespace {

using namespace srx;

__device__ __forceinline__ float load_audio(const float *p, size_t i) { return p[i]; }
__device__ __forceinline__ float load_audio(const int16_t *p, size_t i) { return q15_to_float(p[i]); }
__device__ __forceinline__ void store_iq(float *p, size_t i, float re, float im, uint32_t = 0u)
{
    reinterpret_cast<float2 *>(p)[i] = make_float2(re, im);
}
__device__ __forceinline__ void store_iq(int16_t *p, size_t i, float re, float im, uint32_t round = 0u)
{
    short2 v;
    v.x = float_to_q15(re, round);
    v.y = float_to_q15(im, round);
    reinterpret_cast<short2 *>(p)[i] = v;
}

typedef float v2f __attribute__((ext_vector_type(2)));

static __host__ __device__ inline uint32_t up4(uint32_t v) { return (v + 3u) & ~3u; }

// LDS of k_tx_generic, in floats: sine table | interpolator taps | (delay, Hilbert) tap pairs |
// (delay-instance, Hilbert-instance) state pairs | (I, Q) interpolator state pairs.  Pairs: one
// ds_read_b64 and one packed MAC serve both members.
struct TxLds { uint32_t tab, ci, chd, H, Z, total; };
static __host__ __device__ inline TxLds tx_layout(uint32_t ni, uint32_t nh, uint32_t P, uint32_t nb)
{
    TxLds L;
    const uint32_t nh1 = nh ? nh - 1 : 0;
    uint32_t o = 0;
    L.tab = o; o += 516;
    L.ci = o;  o += up4(ni);
    L.chd = o; o += up4(2 * nh);
    L.H = o;   o += up4(2 * (nh1 + nb));
    L.Z = o;   o += up4(2 * ((P - 1) + nb));
    L.total = o;
    return L;
}

size_t tx_lds_bytes(const TxParams &p)
{
    return sizeof(float) * tx_layout(p.ni, p.nh, p.P, p.block).total;
}

template <int ARITH>
__device__ __forceinline__ v2f tx_mac2(v2f acc, v2f w, v2f c2)
{
    if constexpr (ARITH == 1) return __builtin_elementwise_fma(w, c2, acc);
    else { const v2f pr = w * c2; return acc + pr; }
}

template <int ARITH, typename TIn, typename TOut>
__global__ __launch_bounds__(64) void k_tx_generic(TxParams p, const TIn *__restrict__ src, TOut *__restrict__ dst)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    const uint32_t nb = p.block, L = p.L, P = p.P, nh = p.nh, nh1 = nh ? nh - 1 : 0, p1 = P - 1;
    const TxLds Y = tx_layout(p.ni, nh, P, nb);
    float *tab = lds + Y.tab, *ci = lds + Y.ci;
    v2f *chd = reinterpret_cast<v2f *>(lds + Y.chd);             // (delay tap, Hilbert tap)
    v2f *H = reinterpret_cast<v2f *>(lds + Y.H);                 // arm_fir_f32 pState of the (delay, Hilbert) instances
    v2f *Z = reinterpret_cast<v2f *>(lds + Y.Z);                 // arm_fir_interpolate_f32 pState of the (I, Q) rails
    if (p.nco)
        for (int i = lane; i < 513; i += kWave) tab[i] = p.sintab[i];
    for (uint32_t i = lane; i < p.ni; i += kWave) ci[i] = p.ic[i];
    for (uint32_t i = lane; i < nh; i += kWave) chd[i] = v2f{ p.dc[i], p.hc[i] };
    for (uint32_t i = lane; i < nh1; i += kWave)
        H[i] = v2f{ p.fir_state[(size_t)c * 2 * nh1 + i], p.fir_state[(size_t)c * 2 * nh1 + nh1 + i] };
    for (uint32_t i = lane; i < p1; i += kWave)
        Z[i] = v2f{ p.int_state[(size_t)c * 2 * p1 + i], p.int_state[(size_t)c * 2 * p1 + p1 + i] };
    float gain = p.alc ? p.gain[c] : 1.0f;
    const uint32_t ph0 = p.nco ? p.phase[c] : 0u, step = p.nco ? p.step[c] : 0u;
    const bool am = p.mode == SELENITE_MODE_AM, up = mode_is_upper(p.mode);
    const uint32_t nblk = p.block_size / nb;
    __syncthreads();

    for (uint32_t b = 0; b < nblk; ++b) {
        // 1. ALC: arm_abs_f32 + arm_max_f32 -> gain law -> arm_scale_f32
        const size_t ib = (size_t)c * p.block_size + (size_t)b * nb;
        float m = 0.0f;
        for (uint32_t i = lane; i < nb; i += kWave) m = fmaxf(m, fabsf(load_audio(src, ib + i)));
        if (p.alc) {
            m = wave_max(m);
            gain = agc_update<0>(p.alcp, gain, m);
        }
        for (uint32_t i = lane; i < nb; i += kWave) {
            float a = load_audio(src, ib + i);
            if (p.alc) a = a * gain;
            if (nh) H[nh1 + i] = v2f{ a, a };
            else Z[p1 + i] = v2f{ a, 0.0f };
        }
        __syncthreads();
        // 2.-3. Hilbert pair (arm_fir_f32 x2 as one packed tap loop) and sideband select
        if (nh) {
            for (uint32_t i = lane; i < nb; i += kWave) {
                v2f r = { 0.0f, 0.0f };
#pragma unroll 4
                for (uint32_t k = 0; k < nh; ++k) r = tx_mac2<ARITH>(r, H[i + k], chd[k]);
                Z[p1 + i] = r;
            }
            __syncthreads();
            for (uint32_t i0 = 0; i0 < nh1; i0 += kWave) {     // history tails, 64-wide slices
                const uint32_t i = i0 + lane;
                const v2f t = (i < nh1) ? H[nb + i] : v2f{ 0.0f, 0.0f };
                __syncthreads();
                if (i < nh1) H[i] = t;
                __syncthreads();
            }
        }
        for (uint32_t i = lane; i < nb; i += kWave) {
            v2f z = Z[p1 + i];
            if (am) {                                          // arm_scale_f32(0.5) then arm_offset_f32(0.5); Q = 0
                const float t = z.x * 0.5f;
                z = v2f{ t + 0.5f, 0.0f };
            } else if (!up) {
                z.y = -z.y;                                    // arm_negate_f32
            }
            Z[p1 + i] = z;
        }
        __syncthreads();
        // 4.-5. interpolator on both rails (one packed MAC per tap), NCO up-mix, store
        const size_t ob = ((size_t)c * p.block_size + (size_t)b * nb) * L;
        for (uint32_t o = lane; o < nb * L; o += kWave) {
            const uint32_t n = o / L, phs = o % L;
            v2f u;
            if (p.ni) {
                u = v2f{ 0.0f, 0.0f };
                const float *cf = ci + (L - 1 - phs);
#pragma unroll 4
                for (uint32_t t = 0; t < P; ++t) {
                    const float cc = cf[t * L];
                    u = tx_mac2<ARITH>(u, Z[n + t], v2f{ cc, cc });
                }
            } else {
                u = Z[n];
            }
            float re = u.x, im = u.y;
            if (p.nco) {
                const uint32_t phase = ph0 + (uint32_t)(b * nb * L + o) * step;
                const float x = (float)(phase >> 8) * kNcoK;
                const float lc = cos_f32<0>(tab, x), ls = sin_f32<0>(tab, x);
                const float2 r = cmul<0>(make_float2(u.x, u.y), make_float2(lc, ls));
                re = r.x; im = r.y;
            }
            store_iq(dst, ob + o, re, im, p.q15_round);
        }
        __syncthreads();
        if (p.ni) {
            for (uint32_t i0 = 0; i0 < p1; i0 += kWave) {
                const uint32_t i = i0 + lane;
                const v2f t = (i < p1) ? Z[nb + i] : v2f{ 0.0f, 0.0f };
                __syncthreads();
                if (i < p1) Z[i] = t;
                __syncthreads();
            }
        }
    }
    for (uint32_t i = lane; i < nh1; i += kWave) {
        p.fir_state[(size_t)c * 2 * nh1 + i] = H[i].x;
        p.fir_state[(size_t)c * 2 * nh1 + nh1 + i] = H[i].y;
    }
    for (uint32_t i = lane; i < p1; i += kWave) {
        p.int_state[(size_t)c * 2 * p1 + i] = Z[i].x;
        p.int_state[(size_t)c * 2 * p1 + p1 + i] = Z[i].y;
    }
    if (lane == 0) {
        if (p.alc) p.gain[c] = gain;
        if (p.nco) p.phase[c] = ph0 + p.block_size * L * step;
    }
}

int fail(selenite_tx_instance *S, int code, const std::string &msg)
{
    if (S && S->status == 0) { S->status = code; S->err = msg; }
    return code;
}

#define TCHK(S, call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((S), SELENITE_RX_DEVICE_ERROR, std::string(#call ": ") + hipGetErrorString(e_)); \
    } while (0)

bool tx_mode_ok(uint8_t m)
{
    return m == SELENITE_MODE_LSB || m == SELENITE_MODE_USB || m == SELENITE_MODE_CW || m == SELENITE_MODE_CWR ||
           m == SELENITE_MODE_AM || m == SELENITE_MODE_DIG || m == SELENITE_MODE_PKT;
}

TxParams make_params(const selenite_tx_instance *S, uint32_t block_size)
{
    const selenite_tx_config &g = S->cfg;
    TxParams p{};
    p.channels = g.channels; p.block = g.block; p.L = g.interp; p.ni = g.ni_taps;
    p.P = g.ni_taps ? g.ni_taps / g.interp : 1; p.nh = g.nh_taps; p.mode = g.mode;
    p.nco = g.nco_enable ? 1 : 0; p.alc = g.alc_enable ? 1 : 0; p.block_size = block_size; p.q15_round = g.q15_rounding ? 1u : 0u;
    p.ic = S->d_ic; p.hc = S->d_hc; p.dc = S->d_dc; p.sintab = S->d_sintab;
    p.step = S->d_step; p.phase = S->d_phase;
    p.fir_state = S->d_fir_state; p.int_state = S->d_int_state; p.gain = S->d_gain;
    p.alcp = AgcParams{ g.alc_target, g.alc_attack, g.alc_decay, g.alc_gain_min, g.alc_gain_max, g.alc_env_floor };
    return p;
}

template <int ARITH, typename TIn, typename TOut>
hipError_t launch(const TxParams &p, const void *src, void *dst, hipStream_t st)
{
    const size_t lds = tx_lds_bytes(p);
    auto k = k_tx_generic<ARITH, TIn, TOut>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k, dim3(p.channels), dim3(64), lds, st, p, static_cast<const TIn *>(src), static_cast<TOut *>(dst));
    return hipGetLastError();
}

bool block_size_ok(selenite_tx_instance *S, uint32_t bs, const char *who)
{
    if (!S) return false;
    if (bs == 0 || bs % S->cfg.block != 0) {
        fail(S, SELENITE_RX_LENGTH_ERROR, std::string(who) + ": blockSize is not a non-zero multiple of cfg.block");
        return false;
    }
    return true;
}

int ensure(selenite_tx_instance *S, void **buf, size_t *cap, size_t need);

int run(selenite_tx_instance *S, const void *src, void *dst, bool q15, uint32_t bs)
{
    TCHK(S, hipSetDevice(S->device));
    const selenite_tx_config &g = S->cfg;
    const TxParams p = make_params(S, bs);
    if (g.mode == SELENITE_MODE_FM) {
        // the phase accumulator carries the modulation: every channel's phase is its own from here on (no shared LO until
        // reset or set_state say otherwise)
        S->phase_uniform = false;
        if (tx_fm_lds_bytes(p) > 64 * 1024) return fail(S, SELENITE_RX_LENGTH_ERROR, "filter lengths exceed the LDS budget of the TX kernel");
        TCHK(S, launch_tx_fm(p, S->fm, (int)g.arith, src, q15, dst, S->stream));
        return 0;
    }
    const uint32_t phase_now = S->phase_host;
    if (g.nco_enable) S->phase_host += bs * g.interp * S->h_step[0];
    if (!S->force_generic && tx_fused_ok(g, S->delay_is_impulse, S->hilb_odd_only, bs)) {
        const float2 *lo = nullptr;
        if (g.nco_enable && S->phase_uniform) {
            // every channel shares step and phase: one LO per call, read from L2 by every wavefront
            // the table is a pure function of (start phase, step, length): reused when the call starts where it starts
            // (every call for an LO on the fs / 256 grid: the phase advance of a call is then a multiple of 2^32)
            const uint32_t nlo = bs * g.interp;
            if (!(S->lo_valid && S->lo_phase == phase_now && S->lo_step == S->h_step[0] && S->lo_n >= nlo)) {
                S->lo_valid = false;
                if (ensure(S, (void **)&S->d_lo, &S->lo_bytes, (size_t)nlo * sizeof(float2))) return S->status;
                TCHK(S, launch_lo_table(S->d_lo, S->d_sintab, phase_now, S->h_step[0], nlo, S->stream));
                S->lo_valid = true; S->lo_phase = phase_now; S->lo_step = S->h_step[0]; S->lo_n = nlo;
            }
            lo = S->d_lo;
        }
        if (g.arith == SELENITE_ARITH_SPLIT16 && S->d_ttab16) {
            TxParams ps = p;
            ps.lo_period = (lo && (S->h_step[0] & 0x00FFFFFFu) == 0 && !S->no_periodic_lo) ? 256u : 0u;   // k_tx_split16 keeps it in registers
            TCHK(S, launch_tx_split16(ps, S->delay_index, lo, S->d_ttab16, S->tpost, src, q15, dst, S->stream));
        }
        else
            TCHK(S, launch_tx_fused(p, (int)g.arith, S->delay_index, lo, src, q15, dst, S->stream));
        return 0;
    }
    if (tx_lds_bytes(p) > 64 * 1024) return fail(S, SELENITE_RX_LENGTH_ERROR, "filter lengths exceed the LDS budget of the TX kernel");
    const bool fma = g.arith != SELENITE_ARITH_CMSIS;
    hipError_t e;
    if (q15) e = fma ? launch<1, int16_t, int16_t>(p, src, dst, S->stream) : launch<0, int16_t, int16_t>(p, src, dst, S->stream);
    else e = fma ? launch<1, float, float>(p, src, dst, S->stream) : launch<0, float, float>(p, src, dst, S->stream);
    TCHK(S, e);
    return 0;
}

template <typename T>
int upload(selenite_tx_instance *S, T **dp, const T *h, size_t n)
{
    *dp = nullptr;
    if (!n) return 0;
    TCHK(S, hipMalloc((void **)dp, n * sizeof(T)));
    if (h) TCHK(S, hipMemcpy(*dp, h, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// the input stage's state as the first selenite_tx_set_in leaves it: the decimator tail +0.0f and, with `vox`, level_init, closed, counters 0
int in_clear_state(selenite_tx_instance *S, bool vox, const std::vector<float> &level_init)
{
    const size_t C = S->cfg.channels, h1 = S->in.nt ? S->in.nt - 1 : 0;
    if (h1) TCHK(S, hipMemsetAsync(S->d_in_dec, 0, C * h1 * sizeof(float), S->stream));
    if (!vox) return 0;
    TCHK(S, hipMemcpyAsync(S->d_in_level, level_init.data(), C * sizeof(float), hipMemcpyHostToDevice, S->stream));
    TCHK(S, hipMemsetAsync(S->d_in_open, 0, C * sizeof(uint32_t), S->stream));
    TCHK(S, hipMemsetAsync(S->d_in_hold, 0, C * sizeof(uint32_t), S->stream));
    TCHK(S, hipMemsetAsync(S->d_in_opens, 0, C * sizeof(uint64_t), S->stream));
    TCHK(S, hipMemsetAsync(S->d_in_open_blocks, 0, C * sizeof(uint64_t), S->stream));
    return 0;
}

int reset_state(selenite_tx_instance *S)
{
    const selenite_tx_config &g = S->cfg;
    const size_t C = g.channels, nh1 = g.nh_taps ? g.nh_taps - 1 : 0, p1 = g.ni_taps ? g.ni_taps / g.interp - 1 : 0;
    if (nh1) TCHK(S, hipMemsetAsync(S->d_fir_state, 0, C * 2 * nh1 * sizeof(float), S->stream));
    if (p1) TCHK(S, hipMemsetAsync(S->d_int_state, 0, C * 2 * p1 * sizeof(float), S->stream));
    TCHK(S, hipMemsetAsync(S->d_phase, 0, C * sizeof(uint32_t), S->stream));
    if (S->d_tone_phase) TCHK(S, hipMemsetAsync(S->d_tone_phase, 0, C * sizeof(uint32_t), S->stream));
    if (S->cw_set) {
        if (S->cw.ns > 1) TCHK(S, hipMemsetAsync(S->d_key_state, 0, C * (S->cw.ns - 1), S->stream));
        TCHK(S, hipMemsetAsync(S->d_side_phase, 0, C * sizeof(uint32_t), S->stream));
        TCHK(S, hipMemsetAsync(S->d_tx_on, 0, C * sizeof(uint32_t), S->stream));
        TCHK(S, hipMemsetAsync(S->d_hold, 0, C * sizeof(uint32_t), S->stream));
    }
    std::vector<float> gi(C, g.alc_gain_init), li(C, S->in_level_init);   // (alive until the stream is drained)
    if (S->in_set && in_clear_state(S, true, li)) return S->status;
    TCHK(S, hipMemcpyAsync(S->d_gain, gi.data(), C * sizeof(float), hipMemcpyHostToDevice, S->stream));
    TCHK(S, hipStreamSynchronize(S->stream));
    S->phase_host = 0;
    S->phase_uniform = S->steps_same;
    return 0;
}

int ensure(selenite_tx_instance *S, void **buf, size_t *cap, size_t need)
{
    if (*cap >= need) return 0;
    TCHK(S, hipStreamSynchronize(S->stream));
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *cap = 0;
    TCHK(S, hipMalloc(buf, need));
    *cap = need;
    return 0;
}

void process_host(selenite_tx_instance *S, const void *src, void *dst, uint32_t bs, bool q15, const char *who)
{
    if (!block_size_ok(S, bs, who)) return;
    const selenite_tx_config &g = S->cfg;
    const size_t esz = q15 ? sizeof(int16_t) : sizeof(float);
    const size_t nin = (size_t)g.channels * bs * esz, nout = (size_t)g.channels * bs * g.interp * 2 * esz;
    if (hipSetDevice(S->device) != hipSuccess) { fail(S, SELENITE_RX_DEVICE_ERROR, "hipSetDevice"); return; }
    if (ensure(S, &S->d_io_in, &S->io_in_bytes, nin) || ensure(S, &S->d_io_out, &S->io_out_bytes, nout)) return;
    if (hipMemcpyAsync(S->d_io_in, src, nin, hipMemcpyHostToDevice, S->stream) != hipSuccess) { fail(S, SELENITE_RX_DEVICE_ERROR, "H2D copy failed"); return; }
    if (run(S, S->d_io_in, S->d_io_out, q15, bs)) return;
    if (hipMemcpyAsync(dst, S->d_io_out, nout, hipMemcpyDeviceToHost, S->stream) != hipSuccess ||
        hipStreamSynchronize(S->stream) != hipSuccess)
        fail(S, SELENITE_RX_DEVICE_ERROR, "D2H copy failed");
}

// keyed CW: every refusal comes before anything is written
int key_call_ok(selenite_tx_instance *S, const void *key, const void *dst, uint32_t bs, const char *who)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    if (!S->cw_set) return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": keyed CW is not configured (selenite_tx_set_cw)");
    if (S->cfg.mode != SELENITE_MODE_CW && S->cfg.mode != SELENITE_MODE_CWR)
        return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": the mode is neither CW nor CWR");
    if (!key || !dst) return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": NULL buffer");
    if (!block_size_ok(S, bs, who)) return SELENITE_RX_LENGTH_ERROR;
    if (tx_cw_lds_bytes(make_params(S, bs), S->cw) > 64 * 1024)
        return fail(S, SELENITE_RX_LENGTH_ERROR, "filter lengths exceed the LDS budget of the TX kernel");
    return 0;
}

int run_key(selenite_tx_instance *S, const uint8_t *key, void *dst, void *side, bool q15, uint32_t bs)
{
    TCHK(S, hipSetDevice(S->device));
    const TxParams p = make_params(S, bs);
    TxCwParams w = S->cw;
    if (S->cfg.mode == SELENITE_MODE_CWR) w.offset = 0u - w.offset;
    // the carrier offset went into the phase accumulator: every channel's phase is its own from here on, as after FM
    S->phase_uniform = false;
    TCHK(S, launch_tx_cw(p, w, (int)S->cfg.arith, key, q15, dst, side, S->stream));
    return 0;
}

int process_key_host(selenite_tx_instance *S, const uint8_t *key, void *dst, void *side, uint32_t bs, bool q15, const char *who)
{
    if (int r = key_call_ok(S, key, dst, bs, who)) return r;
    const selenite_tx_config &g = S->cfg;
    const size_t esz = q15 ? sizeof(int16_t) : sizeof(float);
    const size_t nin = (size_t)g.channels * bs, nout = nin * g.interp * 2 * esz, nside = nin * esz;
    TCHK(S, hipSetDevice(S->device));
    if (ensure(S, &S->d_io_in, &S->io_in_bytes, nin) || ensure(S, &S->d_io_out, &S->io_out_bytes, nout) ||
        (side && ensure(S, &S->d_io_side, &S->io_side_bytes, nside)))
        return S->status;
    TCHK(S, hipMemcpyAsync(S->d_io_in, key, nin, hipMemcpyHostToDevice, S->stream));
    if (side && S->cw.side_mix) TCHK(S, hipMemcpyAsync(S->d_io_side, side, nside, hipMemcpyHostToDevice, S->stream));
    if (int r = run_key(S, static_cast<const uint8_t *>(S->d_io_in), S->d_io_out, side ? S->d_io_side : nullptr, q15, bs)) return r;
    TCHK(S, hipMemcpyAsync(dst, S->d_io_out, nout, hipMemcpyDeviceToHost, S->stream));
    if (side) TCHK(S, hipMemcpyAsync(side, S->d_io_side, nside, hipMemcpyDeviceToHost, S->stream));
    TCHK(S, hipStreamSynchronize(S->stream));
    return 0;
}

}  // namespace

extern "C" int selenite_tx_init(selenite_tx_instance **out, const selenite_tx_config *caller_cfg)
{
    if (!out) return SELENITE_RX_ARGUMENT_ERROR;
    *out = nullptr;
    if (!caller_cfg) return SELENITE_RX_ARGUMENT_ERROR;
    // struct_size says which header the caller was built against (include/selenite_rx.h: ABI versions); version 1 ends with alc_gain_init
    static_assert(offsetof(selenite_tx_config, q15_rounding) == 92 && sizeof(selenite_tx_config) == 104, "selenite_tx_config layout (LP64)");
    selenite_tx_config own{};
    if (caller_cfg->struct_size == SELENITE_TX_CONFIG_SIZE_V1) {
        std::memcpy(&own, caller_cfg, offsetof(selenite_tx_config, q15_rounding));
        own.abi_version = 1;
    } else if (caller_cfg->struct_size == sizeof(selenite_tx_config)) {
        own = *caller_cfg;
        if (own.abi_version != SELENITE_RX_ABI_VERSION || own.reserved != 0) return SELENITE_RX_ARGUMENT_ERROR;
    } else {
        return SELENITE_RX_ARGUMENT_ERROR;
    }
    own.struct_size = (uint32_t)sizeof(selenite_tx_config);
    const selenite_tx_config *g = &own;
    if (g->q15_rounding > 1u || !g->channels || !g->block || !g->interp || !tx_mode_ok(g->mode) ||
        g->arith > SELENITE_ARITH_SPLIT16)
        return SELENITE_RX_ARGUMENT_ERROR;
    if ((g->interp > 1) != (g->ni_taps > 0)) return SELENITE_RX_ARGUMENT_ERROR;
    if (g->ni_taps && !g->interp_coeffs) return SELENITE_RX_ARGUMENT_ERROR;
    if (g->nh_taps && (!g->hilb_coeffs || !g->delay_coeffs)) return SELENITE_RX_ARGUMENT_ERROR;
    if (g->ni_taps % g->interp) return SELENITE_RX_LENGTH_ERROR;        // arm_fir_interpolate_init_f32.c:91-96
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return SELENITE_RX_DEVICE_ERROR;   // no CPU fallback
    selenite_tx_instance *S = new selenite_tx_instance;
    S->cfg = *g;
    S->cfg.interp_coeffs = S->cfg.hilb_coeffs = S->cfg.delay_coeffs = nullptr;
    S->cfg.nco_step = nullptr;
    auto bail = [&](int code) { selenite_tx_free(S); return code; };
    if (hipGetDevice(&S->device) != hipSuccess) return bail(SELENITE_RX_DEVICE_ERROR);
    if (hipStreamCreateWithFlags(&S->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(SELENITE_RX_DEVICE_ERROR);
    S->stream = S->own_stream;
    const size_t C = g->channels, nh1 = g->nh_taps ? g->nh_taps - 1 : 0, p1 = g->ni_taps ? g->ni_taps / g->interp - 1 : 0;
    S->h_step.resize(C);
    for (size_t c = 0; c < C; ++c) S->h_step[c] = g->nco_step ? g->nco_step[c] : g->nco_step_all;
    S->steps_same = true;
    for (size_t c = 1; c < C; ++c) S->steps_same = S->steps_same && S->h_step[c] == S->h_step[0];
    {   // what tx_fused.hip relies on: a unit-impulse delay FIR and a type-III Hilbert (taps at even
        // distance from the centre exactly +0.0f) -- same classification as the RX side (rx_api.hip: classify_coeffs)
        const uint32_t nh = g->nh_taps;
        int ones = 0, idx = -1;
        bool rest_zero = true;
        for (uint32_t k = 0; k < nh; ++k) {
            const float v = g->delay_coeffs[k];
            if (v == 1.0f) { ++ones; idx = (int)k; }
            else if (!(v == 0.0f && !std::signbit(v))) rest_zero = false;
        }
        if (nh && ones == 1 && rest_zero) { S->delay_is_impulse = true; S->delay_index = (uint32_t)idx; }
        if (nh % 2 == 1) {
            const int cc = (int)(nh - 1) / 2;
            bool ok = true;
            for (uint32_t k = 0; k < nh && ok; ++k)
                if ((((int)k - cc) & 1) == 0) {
                    const float v = g->hilb_coeffs[k];
                    if (!(v == 0.0f && !std::signbit(v))) ok = false;
                }
            S->hilb_odd_only = ok;
        }
        // kernel-selection overrides of the tests (selenite_rx_set_plan_option)
        S->force_generic = srx::plan_option(SELENITE_RX_OPT_TX_FORCE_GENERIC) != 0;
        S->no_periodic_lo = srx::plan_option(SELENITE_RX_OPT_NO_PERIODIC_LO) != 0;
    }
    if (g->arith == SELENITE_ARITH_SPLIT16 && tx_fused_ok(*g, S->delay_is_impulse, S->hilb_odd_only, 256) &&
        build_tx_split16_table(g->interp_coeffs, &S->d_ttab16, &S->tpost) != hipSuccess)
        return bail(SELENITE_RX_DEVICE_ERROR);
    if (upload(S, &S->d_ic, g->interp_coeffs, (size_t)g->ni_taps) || upload(S, &S->d_hc, g->hilb_coeffs, (size_t)g->nh_taps) ||
        upload(S, &S->d_dc, g->delay_coeffs, (size_t)g->nh_taps) || upload(S, &S->d_sintab, srx::host_sin_table(), (size_t)513) ||
        upload(S, &S->d_step, S->h_step.data(), C) || upload<uint32_t>(S, &S->d_phase, nullptr, C) ||
        upload<float>(S, &S->d_fir_state, nullptr, C * 2 * nh1) || upload<float>(S, &S->d_int_state, nullptr, C * 2 * p1) ||
        upload<float>(S, &S->d_gain, nullptr, C))
        return bail(SELENITE_RX_DEVICE_ERROR);
    if (reset_state(S)) return bail(SELENITE_RX_DEVICE_ERROR);
    *out = S;
    return SELENITE_RX_SUCCESS;
}

extern "C" void selenite_tx_free(selenite_tx_instance *S)
{
    if (!S) return;
    void *ptrs[] = { S->d_ic, S->d_hc, S->d_dc, S->d_sintab, S->d_step, S->d_phase, S->d_fir_state, S->d_int_state,
                     S->d_gain, S->d_io_in, S->d_io_out, S->d_lo, S->d_ttab16, S->d_tone_step, S->d_tone_phase,
                     S->d_shape, S->d_side_step, S->d_side_phase, S->d_tx_on, S->d_hold, S->d_key_state, S->d_io_side,
                     S->d_in_coeffs, S->d_in_dec, S->d_in_level, S->d_in_open, S->d_in_hold, S->d_in_opens, S->d_in_open_blocks, S->d_in_audio };
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (S->own_stream) (void)hipStreamDestroy(S->own_stream);
    delete S;
}

extern "C" int selenite_tx_set_mode(selenite_tx_instance *S, uint8_t mode)
{
    // instance stays usable in its old mode; FM exists once selenite_tx_set_fm has configured it
    if (!S || !(tx_mode_ok(mode) || (mode == SELENITE_MODE_FM && S->fm_set))) return SELENITE_RX_ARGUMENT_ERROR;
    S->cfg.mode = mode;
    return SELENITE_RX_SUCCESS;
}

extern "C" const char *selenite_tx_kernel_name(const selenite_tx_instance *S)
{
    if (!S) return "";
    if (S->cfg.mode == SELENITE_MODE_FM) return "k_tx_fm";
    if (S->force_generic || !tx_fused_ok(S->cfg, S->delay_is_impulse, S->hilb_odd_only, 256)) return "k_tx_generic";
    return (S->cfg.arith == SELENITE_ARITH_SPLIT16 && S->d_ttab16) ? "k_tx_split16<4,256,63>" : "k_tx_fused<4,256,63>";
}

extern "C" int selenite_tx_status(const selenite_tx_instance *S) { return S ? S->status : SELENITE_RX_ARGUMENT_ERROR; }
extern "C" const char *selenite_tx_error_string(const selenite_tx_instance *S) { return S ? S->err.c_str() : "null instance"; }

extern "C" void selenite_tx_process_f32(selenite_tx_instance *S, const float *src, float *dst, uint32_t bs)
{
    process_host(S, src, dst, bs, false, "selenite_tx_process_f32");
}
extern "C" void selenite_tx_process_q15(selenite_tx_instance *S, const int16_t *src, int16_t *dst, uint32_t bs)
{
    process_host(S, src, dst, bs, true, "selenite_tx_process_q15");
}
extern "C" void selenite_tx_process_f32_device(selenite_tx_instance *S, const float *src, float *dst, uint32_t bs)
{
    if (block_size_ok(S, bs, "selenite_tx_process_f32_device")) run(S, src, dst, false, bs);
}
extern "C" void selenite_tx_process_q15_device(selenite_tx_instance *S, const int16_t *src, int16_t *dst, uint32_t bs)
{
    if (block_size_ok(S, bs, "selenite_tx_process_q15_device")) run(S, src, dst, true, bs);
}

extern "C" int selenite_tx_set_stream(selenite_tx_instance *S, void *hip_stream)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : S->own_stream;
    if (next != S->stream) {                                // the streaming state is shared: drain the old stream first
        TCHK(S, hipStreamSynchronize(S->stream));
        S->stream = next;
    }
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_tx_sync(selenite_tx_instance *S)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    TCHK(S, hipStreamSynchronize(S->stream));
    return S->status;
}

extern "C" int selenite_tx_get_state(selenite_tx_instance *S, const selenite_tx_state_view *v)
{
    if (!S || !v) return SELENITE_RX_ARGUMENT_ERROR;
    const selenite_tx_config &g = S->cfg;
    const size_t C = g.channels, nh1 = g.nh_taps ? g.nh_taps - 1 : 0, p1 = g.ni_taps ? g.ni_taps / g.interp - 1 : 0;
    TCHK(S, hipStreamSynchronize(S->stream));
    if (v->fir_state && nh1) TCHK(S, hipMemcpy(v->fir_state, S->d_fir_state, C * 2 * nh1 * sizeof(float), hipMemcpyDeviceToHost));
    if (v->interp_state && p1) TCHK(S, hipMemcpy(v->interp_state, S->d_int_state, C * 2 * p1 * sizeof(float), hipMemcpyDeviceToHost));
    if (v->alc_gain) TCHK(S, hipMemcpy(v->alc_gain, S->d_gain, C * sizeof(float), hipMemcpyDeviceToHost));
    if (v->nco_phase) TCHK(S, hipMemcpy(v->nco_phase, S->d_phase, C * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int selenite_tx_set_state(selenite_tx_instance *S, const selenite_tx_state_view *v)
{
    if (!S || !v) return SELENITE_RX_ARGUMENT_ERROR;
    const selenite_tx_config &g = S->cfg;
    const size_t C = g.channels, nh1 = g.nh_taps ? g.nh_taps - 1 : 0, p1 = g.ni_taps ? g.ni_taps / g.interp - 1 : 0;
    TCHK(S, hipStreamSynchronize(S->stream));
    if (v->fir_state && nh1) TCHK(S, hipMemcpy(S->d_fir_state, v->fir_state, C * 2 * nh1 * sizeof(float), hipMemcpyHostToDevice));
    if (v->interp_state && p1) TCHK(S, hipMemcpy(S->d_int_state, v->interp_state, C * 2 * p1 * sizeof(float), hipMemcpyHostToDevice));
    if (v->alc_gain) TCHK(S, hipMemcpy(S->d_gain, v->alc_gain, C * sizeof(float), hipMemcpyHostToDevice));
    if (v->nco_phase) {
        TCHK(S, hipMemcpy(S->d_phase, v->nco_phase, C * sizeof(uint32_t), hipMemcpyHostToDevice));
        bool same = S->steps_same;
        for (size_t c = 1; c < C; ++c) same = same && v->nco_phase[c] == v->nco_phase[0];
        S->phase_uniform = same;
        S->phase_host = v->nco_phase[0];
    }
    return 0;
}

extern "C" int selenite_tx_set_fm(selenite_tx_instance *S, const selenite_tx_fm_config *f)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    static_assert(sizeof(selenite_tx_fm_config) == 40 && offsetof(selenite_tx_fm_config, tone_step) == 24, "selenite_tx_fm_config layout (LP64)");
    if (!f) {                                               // FM off again: not from under a running FM mode
        if (S->cfg.mode == SELENITE_MODE_FM) return SELENITE_RX_ARGUMENT_ERROR;
        S->fm_set = false;
        return SELENITE_RX_SUCCESS;
    }
    if (f->struct_size != sizeof(selenite_tx_fm_config) || f->reserved != 0 || f->tone_enable > 1u ||
        !std::isfinite(f->deviation) || !(f->deviation > 0.0f) || !std::isfinite(f->amplitude) || !std::isfinite(f->tone_level))
        return SELENITE_RX_ARGUMENT_ERROR;                  // the previous setting stays
    const size_t C = S->cfg.channels;
    TCHK(S, hipSetDevice(S->device));
    TCHK(S, hipStreamSynchronize(S->stream));
    if (!S->d_tone_step) TCHK(S, hipMalloc((void **)&S->d_tone_step, C * sizeof(uint32_t)));
    if (!S->d_tone_phase) TCHK(S, hipMalloc((void **)&S->d_tone_phase, C * sizeof(uint32_t)));
    std::vector<uint32_t> ts(C);
    for (size_t c = 0; c < C; ++c) ts[c] = f->tone_step ? f->tone_step[c] : f->tone_step_all;
    TCHK(S, hipMemcpy(S->d_tone_step, ts.data(), C * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!S->fm_set) TCHK(S, hipMemset(S->d_tone_phase, 0, C * sizeof(uint32_t)));     // a retune keeps the tone's phase
    S->fm = srx::TxFmParams{ f->deviation, f->amplitude, f->tone_level, f->tone_enable, S->d_tone_step, S->d_tone_phase };
    S->fm_set = true;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_tx_get_fm_state(selenite_tx_instance *S, const selenite_tx_fm_state_view *v)
{
    if (!S || !v || !S->fm_set) return SELENITE_RX_ARGUMENT_ERROR;
    TCHK(S, hipStreamSynchronize(S->stream));
    if (v->tone_phase) TCHK(S, hipMemcpy(v->tone_phase, S->d_tone_phase, S->cfg.channels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int selenite_tx_set_fm_state(selenite_tx_instance *S, const selenite_tx_fm_state_view *v)
{
    if (!S || !v || !S->fm_set) return SELENITE_RX_ARGUMENT_ERROR;
    TCHK(S, hipStreamSynchronize(S->stream));
    if (v->tone_phase) TCHK(S, hipMemcpy(S->d_tone_phase, v->tone_phase, S->cfg.channels * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int selenite_tx_reset(selenite_tx_instance *S)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    return reset_state(S);
}

extern "C" int selenite_tx_time_process_device(selenite_tx_instance *S, const float *src, float *dst, uint32_t bs,
                                               uint32_t iters, float *ms_per_call)
{
    if (!S || !ms_per_call || iters == 0) return SELENITE_RX_ARGUMENT_ERROR;
    if (!block_size_ok(S, bs, "selenite_tx_time_process_device")) return S->status;
    struct EventPair {                                      // destroyed on every exit path
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    TCHK(S, hipEventCreate(&ev.e0));
    TCHK(S, hipEventCreate(&ev.e1));
    TCHK(S, hipEventRecord(ev.e0, S->stream));
    for (uint32_t i = 0; i < iters; ++i)
        if (run(S, src, dst, false, bs)) return S->status;
    TCHK(S, hipEventRecord(ev.e1, S->stream));
    TCHK(S, hipEventSynchronize(ev.e1));
    float ms = 0.0f;
    TCHK(S, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *ms_per_call = ms / (float)iters;
    return 0;
}

// ---- keyed CW (include/selenite_tx_cw.h) ----

extern "C" int selenite_tx_set_cw(selenite_tx_instance *S, const selenite_tx_cw_config *f)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    static_assert(sizeof(selenite_tx_cw_config) == 56 && offsetof(selenite_tx_cw_config, side_step) == 32, "selenite_tx_cw_config layout (LP64)");
    if (!f) {                                               // keyed CW off again, in any mode: the audio entries never needed it
        S->cw_set = false;
        return SELENITE_RX_SUCCESS;
    }
    if (f->struct_size != sizeof(selenite_tx_cw_config) || f->reserved != 0 || f->side_mix > 1u || f->ns_taps == 0 || !f->shape_coeffs ||
        !std::isfinite(f->amplitude) || !std::isfinite(f->side_level))
        return SELENITE_RX_ARGUMENT_ERROR;                  // the previous setting stays
    float sum = 0.0f;                                       // e[n] of a window that is all key-down: the taps in the FIR's own order
    for (uint32_t k = 0; k < f->ns_taps; ++k) {
        if (!std::isfinite(f->shape_coeffs[k])) return SELENITE_RX_ARGUMENT_ERROR;
        sum = sum + f->shape_coeffs[k];
    }
    const size_t C = S->cfg.channels, ns1 = f->ns_taps - 1;
    const bool first = !S->cw_set, new_len = first || f->ns_taps != S->cw.ns;
    TCHK(S, hipSetDevice(S->device));
    TCHK(S, hipStreamSynchronize(S->stream));
    if (!S->d_side_step) TCHK(S, hipMalloc((void **)&S->d_side_step, C * sizeof(uint32_t)));
    if (!S->d_side_phase) TCHK(S, hipMalloc((void **)&S->d_side_phase, C * sizeof(uint32_t)));
    if (!S->d_tx_on) TCHK(S, hipMalloc((void **)&S->d_tx_on, C * sizeof(uint32_t)));
    if (!S->d_hold) TCHK(S, hipMalloc((void **)&S->d_hold, C * sizeof(uint32_t)));
    // what depends on ns_taps is allocated before anything of the previous setting is given up
    float *shape = S->d_shape;
    uint8_t *ks = S->d_key_state;
    if (new_len || !shape) {
        TCHK(S, hipMalloc((void **)&shape, f->ns_taps * sizeof(float)));
        ks = nullptr;
        if (ns1 && hipMalloc((void **)&ks, C * ns1) != hipSuccess) {
            (void)hipFree(shape);
            return fail(S, SELENITE_RX_DEVICE_ERROR, "hipMalloc(key_state)");
        }
    }
    if (shape != S->d_shape) {
        if (S->d_shape) (void)hipFree(S->d_shape);
        if (S->d_key_state) (void)hipFree(S->d_key_state);
        S->d_shape = shape; S->d_key_state = ks;
    }
    std::vector<uint32_t> ss(C);
    for (size_t c = 0; c < C; ++c) ss[c] = f->side_step ? f->side_step[c] : f->side_step_all;
    TCHK(S, hipMemcpy(S->d_shape, f->shape_coeffs, f->ns_taps * sizeof(float), hipMemcpyHostToDevice));
    TCHK(S, hipMemcpy(S->d_side_step, ss.data(), C * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (new_len && ns1) TCHK(S, hipMemset(S->d_key_state, 0, C * ns1));
    if (first) {                                            // a retune keeps the sidetone's phase and the break-in state
        TCHK(S, hipMemset(S->d_side_phase, 0, C * sizeof(uint32_t)));
        TCHK(S, hipMemset(S->d_tx_on, 0, C * sizeof(uint32_t)));
        TCHK(S, hipMemset(S->d_hold, 0, C * sizeof(uint32_t)));
    }
    S->cw = srx::TxCwParams{ f->ns_taps, S->d_shape, sum, f->amplitude, f->side_level, f->offset_step, f->side_mix, f->hang_blocks,
                             S->d_side_step, S->d_side_phase, S->d_tx_on, S->d_hold, S->d_key_state };
    S->cw_set = true;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_tx_get_cw_state(selenite_tx_instance *S, const selenite_tx_cw_state_view *v)
{
    if (!S || !v || !S->cw_set) return SELENITE_RX_ARGUMENT_ERROR;
    const size_t C = S->cfg.channels, ns1 = S->cw.ns - 1;
    TCHK(S, hipStreamSynchronize(S->stream));
    if (v->key_state && ns1) TCHK(S, hipMemcpy(v->key_state, S->d_key_state, C * ns1, hipMemcpyDeviceToHost));
    if (v->side_phase) TCHK(S, hipMemcpy(v->side_phase, S->d_side_phase, C * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (v->tx_on) TCHK(S, hipMemcpy(v->tx_on, S->d_tx_on, C * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (v->hold) TCHK(S, hipMemcpy(v->hold, S->d_hold, C * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int selenite_tx_set_cw_state(selenite_tx_instance *S, const selenite_tx_cw_state_view *v)
{
    if (!S || !v || !S->cw_set) return SELENITE_RX_ARGUMENT_ERROR;
    const size_t C = S->cfg.channels, ns1 = S->cw.ns - 1;
    TCHK(S, hipStreamSynchronize(S->stream));
    if (v->key_state && ns1) {
        std::vector<uint8_t> ks(C * ns1);
        for (size_t i = 0; i < ks.size(); ++i) ks[i] = v->key_state[i] ? 1 : 0;
        TCHK(S, hipMemcpy(S->d_key_state, ks.data(), C * ns1, hipMemcpyHostToDevice));
    }
    if (v->side_phase) TCHK(S, hipMemcpy(S->d_side_phase, v->side_phase, C * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (v->tx_on) TCHK(S, hipMemcpy(S->d_tx_on, v->tx_on, C * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (v->hold) TCHK(S, hipMemcpy(S->d_hold, v->hold, C * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int selenite_tx_process_key_f32_device(selenite_tx_instance *S, const uint8_t *key, float *dst, float *side, uint32_t bs)
{
    if (int r = key_call_ok(S, key, dst, bs, "selenite_tx_process_key_f32_device")) return r;
    return run_key(S, key, dst, side, false, bs);
}
extern "C" int selenite_tx_process_key_q15_device(selenite_tx_instance *S, const uint8_t *key, int16_t *dst, int16_t *side, uint32_t bs)
{
    if (int r = key_call_ok(S, key, dst, bs, "selenite_tx_process_key_q15_device")) return r;
    return run_key(S, key, dst, side, true, bs);
}
extern "C" int selenite_tx_process_key_f32(selenite_tx_instance *S, const uint8_t *key, float *dst, float *side, uint32_t bs)
{
    return process_key_host(S, key, dst, side, bs, false, "selenite_tx_process_key_f32");
}
extern "C" int selenite_tx_process_key_q15(selenite_tx_instance *S, const uint8_t *key, int16_t *dst, int16_t *side, uint32_t bs)
{
    return process_key_host(S, key, dst, side, bs, true, "selenite_tx_process_key_q15");
}

extern "C" const uint32_t *selenite_tx_cw_txon_device(selenite_tx_instance *S)
{
    return (S && S->cw_set) ? S->d_tx_on : nullptr;
}

extern "C" int selenite_tx_time_process_key_device(selenite_tx_instance *S, const uint8_t *key, float *dst, float *side, uint32_t bs,
                                                   uint32_t iters, float *ms_per_call)
{
    if (!S || !ms_per_call || iters == 0) return SELENITE_RX_ARGUMENT_ERROR;
    if (int r = key_call_ok(S, key, dst, bs, "selenite_tx_time_process_key_device")) return r;
    struct EventPair {                                      // destroyed on every exit path
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    TCHK(S, hipEventCreate(&ev.e0));
    TCHK(S, hipEventCreate(&ev.e1));
    TCHK(S, hipEventRecord(ev.e0, S->stream));
    for (uint32_t i = 0; i < iters; ++i)
        if (int r = run_key(S, key, dst, side, false, bs)) return r;
    TCHK(S, hipEventRecord(ev.e1, S->stream));
    TCHK(S, hipEventSynchronize(ev.e1));
    float ms = 0.0f;
    TCHK(S, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *ms_per_call = ms / (float)iters;
    return 0;
}

// ---- the audio input stage (include/selenite_tx_in.h) ----

namespace {

TxInParams in_params(const selenite_tx_instance *S, uint32_t bs)
{
    TxInParams q = S->in;
    q.channels = S->cfg.channels; q.block = S->cfg.block; q.block_size = bs; q.q15_round = S->cfg.q15_rounding ? 1u : 0u;
    return q;
}

// what run() would refuse behind the stage: asked first, so that a refused call moves no state
bool chain_budget_ok(const selenite_tx_instance *S, uint32_t bs)
{
    const TxParams p = make_params(S, bs);
    if (S->cfg.mode == SELENITE_MODE_FM) return tx_fm_lds_bytes(p) <= 64 * 1024;
    if (!S->force_generic && tx_fused_ok(S->cfg, S->delay_is_impulse, S->hilb_odd_only, bs)) return true;
    return tx_lds_bytes(p) <= 64 * 1024;
}

// frame calls: every refusal comes before anything is written
int frames_call_ok(selenite_tx_instance *S, const void *frames, const void *dst, uint32_t bs, const char *who)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    if (!S->in_set) return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": the input stage is not configured (selenite_tx_set_in)");
    if (!frames || !dst) return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": NULL buffer");
    if (!block_size_ok(S, bs, who)) return SELENITE_RX_LENGTH_ERROR;
    if (tx_in_lds_bytes(in_params(S, bs)) > 64 * 1024 || !chain_budget_ok(S, bs))
        return fail(S, SELENITE_RX_LENGTH_ERROR, std::string(who) + ": the layout exceeds the LDS budget of a TX kernel");
    return 0;
}

int run_in_stage(selenite_tx_instance *S, const void *frames, bool in_q15, bool out_q15, uint32_t bs)
{
    TCHK(S, hipSetDevice(S->device));
    const size_t need = (size_t)S->cfg.channels * bs * (out_q15 ? sizeof(int16_t) : sizeof(float));
    if (ensure(S, &S->d_in_audio, &S->in_audio_bytes, need)) return S->status;
    TCHK(S, launch_tx_in(in_params(S, bs), frames, in_q15, S->d_in_audio, out_q15, S->stream));
    return 0;
}

int run_frames(selenite_tx_instance *S, const void *frames, bool in_q15, void *dst, bool out_q15, uint32_t bs)
{
    if (int r = run_in_stage(S, frames, in_q15, out_q15, bs)) return r;
    return run(S, S->d_in_audio, dst, out_q15, bs);              // the existing chain on the stage's audio, unchanged
}

int process_frames_host(selenite_tx_instance *S, const void *frames, void *dst, uint32_t bs, bool q15, const char *who)
{
    if (int r = frames_call_ok(S, frames, dst, bs, who)) return r;
    const selenite_tx_config &g = S->cfg;
    const size_t esz = q15 ? sizeof(int16_t) : sizeof(float);
    const size_t fw = S->in.pick == SELENITE_TX_IN_MONO ? 1 : 2;
    const size_t nin = (size_t)g.channels * bs * S->in.M * fw * esz, nout = (size_t)g.channels * bs * g.interp * 2 * esz;
    TCHK(S, hipSetDevice(S->device));
    if (ensure(S, &S->d_io_in, &S->io_in_bytes, nin) || ensure(S, &S->d_io_out, &S->io_out_bytes, nout)) return S->status;
    TCHK(S, hipMemcpyAsync(S->d_io_in, frames, nin, hipMemcpyHostToDevice, S->stream));
    if (int r = run_frames(S, S->d_io_in, q15, S->d_io_out, q15, bs)) return r;
    TCHK(S, hipMemcpyAsync(dst, S->d_io_out, nout, hipMemcpyDeviceToHost, S->stream));
    TCHK(S, hipStreamSynchronize(S->stream));
    return 0;
}

}  // namespace

extern "C" int selenite_tx_set_in(selenite_tx_instance *S, const selenite_tx_in_config *f)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    static_assert(sizeof(selenite_tx_in_config) == 72 && offsetof(selenite_tx_in_config, coeffs) == 16 && offsetof(selenite_tx_in_config, meter) == 32 &&
                  sizeof(selenite_tx_in_state_view) == 48, "selenite_tx_in_config layout (LP64)");
    if (!f) {                                               // the stage off again, in any mode: the audio and key entries never needed it
        S->in_set = false;
        return SELENITE_RX_SUCCESS;
    }
    if (f->struct_size != sizeof(selenite_tx_in_config) || f->reserved != 0 || !(f->M == 1 || f->M == 2 || f->M == 4 || f->M == 8) ||
        f->nd_taps > 256 || (f->nd_taps == 0 && f->M != 1) || (f->nd_taps && !f->coeffs) || f->pick > SELENITE_TX_IN_MIX ||
        !std::isfinite(f->gain) || f->vox > 1u)
        return SELENITE_RX_ARGUMENT_ERROR;                  // the previous setting stays
    for (uint32_t k = 0; k < f->nd_taps; ++k)
        if (!std::isfinite(f->coeffs[k])) return SELENITE_RX_ARGUMENT_ERROR;
    const selenite_rx_meter_config &m = f->meter;
    if (f->vox) {                                           // selenite_rx_set_meter's own rules, sense ABOVE
        if (m.struct_size != sizeof(selenite_rx_meter_config) || m.sense != SELENITE_RX_SQ_ABOVE || m.gate > 1u || m.hang > 65535u ||
            !(m.attack > 0.0f && m.attack <= 1.0f) || !(m.decay > 0.0f && m.decay <= 1.0f) ||
            !(std::isfinite(m.open_level) && m.open_level >= 0.0f) || !(std::isfinite(m.close_level) && m.close_level >= 0.0f) ||
            !(m.close_level <= m.open_level) || !(std::isfinite(m.level_init) && m.level_init >= 0.0f))
            return SELENITE_RX_ARGUMENT_ERROR;
    }
    const size_t C = S->cfg.channels, h1 = f->nd_taps ? f->nd_taps - 1 : 0;
    const bool first = !S->in_set, new_len = first || f->nd_taps != S->in.nt;
    TCHK(S, hipSetDevice(S->device));
    TCHK(S, hipStreamSynchronize(S->stream));
    if (!S->d_in_level) TCHK(S, hipMalloc((void **)&S->d_in_level, C * sizeof(float)));
    if (!S->d_in_open) TCHK(S, hipMalloc((void **)&S->d_in_open, C * sizeof(uint32_t)));
    if (!S->d_in_hold) TCHK(S, hipMalloc((void **)&S->d_in_hold, C * sizeof(uint32_t)));
    if (!S->d_in_opens) TCHK(S, hipMalloc((void **)&S->d_in_opens, C * sizeof(uint64_t)));
    if (!S->d_in_open_blocks) TCHK(S, hipMalloc((void **)&S->d_in_open_blocks, C * sizeof(uint64_t)));
    // what depends on nd_taps is allocated before anything of the previous setting is given up
    float *coeffs = S->d_in_coeffs, *dec = S->d_in_dec;
    if (new_len) {
        coeffs = dec = nullptr;
        if (f->nd_taps) TCHK(S, hipMalloc((void **)&coeffs, f->nd_taps * sizeof(float)));
        if (h1 && hipMalloc((void **)&dec, C * h1 * sizeof(float)) != hipSuccess) {
            (void)hipFree(coeffs);
            return fail(S, SELENITE_RX_DEVICE_ERROR, "hipMalloc(dec_state)");
        }
        if (S->d_in_coeffs) (void)hipFree(S->d_in_coeffs);
        if (S->d_in_dec) (void)hipFree(S->d_in_dec);
        S->d_in_coeffs = coeffs; S->d_in_dec = dec;
    }
    if (f->nd_taps) TCHK(S, hipMemcpy(S->d_in_coeffs, f->coeffs, f->nd_taps * sizeof(float), hipMemcpyHostToDevice));
    TxInParams q{};
    q.M = f->M; q.nt = f->nd_taps; q.pick = f->pick; q.gain = f->gain; q.vox = f->vox;
    if (f->vox) {
        q.gate = m.gate; q.hang = m.hang; q.attack = m.attack; q.decay = m.decay; q.open_level = m.open_level; q.close_level = m.close_level;
        S->in_level_init = m.level_init;
    }
    q.coeffs = S->d_in_coeffs; q.dec_state = S->d_in_dec; q.level = S->d_in_level; q.open = S->d_in_open; q.hold = S->d_in_hold;
    q.opens = S->d_in_opens; q.open_blocks = S->d_in_open_blocks;
    S->in = q;
    if (first || new_len) {                                 // a retune keeps the decimator tail (same nd_taps) and the VOX state
        if (first && !f->vox) S->in_level_init = 0.0f;
        const std::vector<float> li(C, S->in_level_init);
        if (in_clear_state(S, first, li)) return S->status;
        TCHK(S, hipStreamSynchronize(S->stream));
    }
    S->in_set = true;
    return SELENITE_RX_SUCCESS;
}

static int in_state_copy(selenite_tx_instance *S, const selenite_tx_in_state_view *v, bool to_host)
{
    if (!S || !v || !S->in_set) return SELENITE_RX_ARGUMENT_ERROR;
    const size_t C = S->cfg.channels, h1 = S->in.nt ? S->in.nt - 1 : 0;
    TCHK(S, hipStreamSynchronize(S->stream));
    struct Row { void *dev; void *host; size_t bytes; };
    const Row rows[] = { { S->d_in_dec, v->dec_state, C * h1 * sizeof(float) }, { S->d_in_level, v->level, C * sizeof(float) },
                         { S->d_in_open, v->open, C * sizeof(uint32_t) }, { S->d_in_hold, v->hold, C * sizeof(uint32_t) },
                         { S->d_in_opens, v->opens, C * sizeof(uint64_t) }, { S->d_in_open_blocks, v->open_blocks, C * sizeof(uint64_t) } };
    for (const Row &r : rows) {
        if (!r.host || !r.bytes) continue;                  // NULL members are skipped
        if (to_host) TCHK(S, hipMemcpy(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost));
        else TCHK(S, hipMemcpy(r.dev, r.host, r.bytes, hipMemcpyHostToDevice));
    }
    return 0;
}
extern "C" int selenite_tx_get_in_state(selenite_tx_instance *S, const selenite_tx_in_state_view *v) { return in_state_copy(S, v, true); }
extern "C" int selenite_tx_set_in_state(selenite_tx_instance *S, const selenite_tx_in_state_view *v) { return in_state_copy(S, v, false); }

extern "C" int selenite_tx_process_frames_f32_device(selenite_tx_instance *S, const float *frames, float *dst, uint32_t bs)
{
    if (int r = frames_call_ok(S, frames, dst, bs, "selenite_tx_process_frames_f32_device")) return r;
    return run_frames(S, frames, false, dst, false, bs);
}
extern "C" int selenite_tx_process_frames_q15_device(selenite_tx_instance *S, const int16_t *frames, int16_t *dst, uint32_t bs)
{
    if (int r = frames_call_ok(S, frames, dst, bs, "selenite_tx_process_frames_q15_device")) return r;
    return run_frames(S, frames, true, dst, true, bs);
}
extern "C" int selenite_tx_process_frames_q15_f32_device(selenite_tx_instance *S, const int16_t *frames, float *dst, uint32_t bs)
{
    if (int r = frames_call_ok(S, frames, dst, bs, "selenite_tx_process_frames_q15_f32_device")) return r;
    return run_frames(S, frames, true, dst, false, bs);
}
extern "C" int selenite_tx_process_frames_f32(selenite_tx_instance *S, const float *frames, float *dst, uint32_t bs)
{
    return process_frames_host(S, frames, dst, bs, false, "selenite_tx_process_frames_f32");
}
extern "C" int selenite_tx_process_frames_q15(selenite_tx_instance *S, const int16_t *frames, int16_t *dst, uint32_t bs)
{
    return process_frames_host(S, frames, dst, bs, true, "selenite_tx_process_frames_q15");
}

extern "C" const uint32_t *selenite_tx_in_vox_device(selenite_tx_instance *S) { return (S && S->in_set) ? S->d_in_open : nullptr; }
extern "C" const void *selenite_tx_in_audio_device(selenite_tx_instance *S) { return (S && S->in_set) ? S->d_in_audio : nullptr; }

extern "C" int selenite_tx_time_in_stage_device(selenite_tx_instance *S, const void *frames, uint32_t kind, uint32_t bs, uint32_t iters,
                                                float *ms_per_launch)
{
    if (!S || !ms_per_launch || iters == 0 || kind > SELENITE_TX_IN_Q15_F32) return SELENITE_RX_ARGUMENT_ERROR;
    if (int r = frames_call_ok(S, frames, ms_per_launch, bs, "selenite_tx_time_in_stage_device")) return r;
    const bool in_q15 = kind != SELENITE_TX_IN_F32, out_q15 = kind == SELENITE_TX_IN_Q15;
    struct EventPair {                                      // destroyed on every exit path
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    TCHK(S, hipEventCreate(&ev.e0));
    TCHK(S, hipEventCreate(&ev.e1));
    if (int r = run_in_stage(S, frames, in_q15, out_q15, bs)) return r;      // (grows the audio buffer outside the timed span)
    TCHK(S, hipEventRecord(ev.e0, S->stream));
    for (uint32_t i = 0; i < iters; ++i)
        if (int r = run_in_stage(S, frames, in_q15, out_q15, bs)) return r;
    TCHK(S, hipEventRecord(ev.e1, S->stream));
    TCHK(S, hipEventSynchronize(ev.e1));
    float ms = 0.0f;
    TCHK(S, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *ms_per_launch = ms / (float)iters;
    return 0;
}
