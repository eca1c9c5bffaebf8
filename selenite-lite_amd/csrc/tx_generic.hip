// tx_generic.hip -- batched TX chain (include/selenite_tx.h): ALC -> Hilbert pair -> sideband select ->
// arm_fir_interpolate_f32 by L -> NCO up-mix, one wavefront per channel, ALC block by ALC block.
// Arithmetic contract as in rx_device.h: every step keeps the CMSIS-DSP 1.5.3 operation order
// (oracle/tx_oracle.c restates it, oracle/ref_tx.c composes the real functions); SELENITE_ARITH_FMA
// fuses the FIR tap loops only.  This is the "any configuration" kernel of the TX direction (the
// counterpart of rx_generic.hip): plain LDS arrays, runtime tap loops, coalesced 8-byte I/Q stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rx_device.h"
#include "rx_internal.h"
#include "tx_internal.h"

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

}  // namespace

namespace srx {

size_t tx_lds_bytes(const TxParams &p)
{
    return sizeof(float) * tx_layout(p.ni, p.nh, p.P, p.block).total;
}

hipError_t launch_tx_generic(const TxParams &p, int arith, const void *src, bool q15, void *dst, hipStream_t st)
{
    const bool fma = arith != SELENITE_ARITH_CMSIS;              // SPLIT16 runs as FMA
    if (q15) return fma ? launch<1, int16_t, int16_t>(p, src, dst, st) : launch<0, int16_t, int16_t>(p, src, dst, st);
    return fma ? launch<1, float, float>(p, src, dst, st) : launch<0, float, float>(p, src, dst, st);
}

}  // namespace srx
