// tx_fm.hip -- the FM transmit mode of the batched TX chain (include/selenite_tx.h: selenite_tx_set_fm; DESIGN.md section 2 "TX FM",
// section 5.16).  ALC -> arm_fir_f32 (delay taps) -> arm_fir_interpolate_f32 by L on ONE rail -> optional CTCSS tone -> deviation ->
// arm_float_to_q31 -> the NCO's 32-bit phase as the running sum -> (cos, sin) * amplitude.
//
// The only TX mode whose output sample n depends on every sample before it.  The dependence is an integer sum modulo 2^32, so a
// wave-wide prefix scan of (uint32)d[n] + step gives the bits of the sequential loop; everything in front of it is k_tx_generic's
// chain on one rail (same per-output accumulation order: one accumulator from +0.0f, taps ascending), two outputs per packed MAC.
// One single-wave workgroup per channel, ALC block by ALC block, 64 outputs per scan slice.
// Kernel, launcher and the host side of the mode: selenite_tx_set_fm and the tone's state accessors.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "rx_device.h"
#include "tx_host.h"

namespace srx {

namespace {

__device__ __forceinline__ float fm_load_audio(const float *p, size_t i) { return p[i]; }
__device__ __forceinline__ float fm_load_audio(const int16_t *p, size_t i) { return q15_to_float(p[i]); }
__device__ __forceinline__ void fm_store_iq(float *p, size_t i, float re, float im, uint32_t)
{
    reinterpret_cast<float2 *>(p)[i] = make_float2(re, im);
}
__device__ __forceinline__ void fm_store_iq(int16_t *p, size_t i, float re, float im, uint32_t round)
{
    short2 v;
    v.x = float_to_q15(re, round);
    v.y = float_to_q15(im, round);
    reinterpret_cast<short2 *>(p)[i] = v;
}

typedef float fm_v2f __attribute__((ext_vector_type(2)));

__host__ __device__ inline uint32_t fm_up4(uint32_t v) { return (v + 3u) & ~3u; }

// LDS of k_tx_fm, in floats: sine table | interpolator taps | delay taps | arm_fir_f32 pState (one rail: both instances see the
// same samples) | arm_fir_interpolate_f32 pState of the I rail
struct FmLds { uint32_t tab, ci, cd, H, Z, total; };
__host__ __device__ inline FmLds fm_layout(uint32_t ni, uint32_t nh, uint32_t P, uint32_t nb)
{
    FmLds L;
    const uint32_t nh1 = nh ? nh - 1 : 0;
    uint32_t o = 0;
    L.tab = o; o += 516;
    L.ci = o;  o += fm_up4(ni);
    L.cd = o;  o += fm_up4(nh);
    L.H = o;   o += fm_up4(nh1 + nb);
    L.Z = o;   o += fm_up4((P - 1) + nb);
    L.total = o;
    return L;
}

// SupportFunctions/arm_float_to_q31.c:129 (ARM_MATH_ROUNDING off): clip_q63_to_q31((q63_t)(in * 2147483648.0f)) -- truncation toward
// zero, saturation at both ends; NaN -> 0 (C leaves it undefined)
__device__ __forceinline__ uint32_t fm_float_to_q31(float v)
{
    const float s = v * 2147483648.0f;
    int q = (s > -2147483648.0f && s < 2147483648.0f) ? (int)s : 0;     // in range (NaN compares false: 0)
    q = (s >= 2147483648.0f) ? 0x7FFFFFFF : q;
    q = (s <= -2147483648.0f) ? (int)0x80000000u : q;
    return (uint32_t)q;
}

// DPP: lane l receives lane l - N of its row of 16, lanes without a source (and rows outside row_mask) receive 0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t fm_dpp0(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// inclusive prefix sum over the 64 lanes, modulo 2^32 (integer addition is associative: the bits of the sequential sum):
// row_shr 1, 2, 4, 8 inside each row of 16, then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3.
// All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v)
{
    v += fm_dpp0<0x111, 0xf>(v);
    v += fm_dpp0<0x112, 0xf>(v);
    v += fm_dpp0<0x114, 0xf>(v);
    v += fm_dpp0<0x118, 0xf>(v);
    v += fm_dpp0<0x142, 0xa>(v);
    v += fm_dpp0<0x143, 0xc>(v);
    return v;
}

template <int ARITH>
__device__ __forceinline__ fm_v2f fm_mac2(fm_v2f acc, fm_v2f w, fm_v2f c2)
{
    if constexpr (ARITH == 1) return __builtin_elementwise_fma(w, c2, acc);
    else { const fm_v2f pr = w * c2; return acc + pr; }
}

template <int ARITH, typename TIn, typename TOut>
__global__ __launch_bounds__(64) void k_tx_fm(TxParams p, TxFmParams f, const TIn *__restrict__ src, TOut *__restrict__ dst)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    const uint32_t nb = p.block, L = p.L, P = p.P, nh = p.nh, nh1 = nh ? nh - 1 : 0, p1 = P - 1;
    const FmLds Y = fm_layout(p.ni, nh, P, nb);
    float *tab = lds + Y.tab, *ci = lds + Y.ci, *cd = lds + Y.cd;
    float *H = lds + Y.H;                                        // arm_fir_f32 pState (the delay and the Hilbert instance hold the same)
    float *Z = lds + Y.Z;                                        // arm_fir_interpolate_f32 pState of the I rail
    for (uint32_t i = lane; i < 513; i += kWave) tab[i] = p.sintab[i];
    for (uint32_t i = lane; i < p.ni; i += kWave) ci[i] = p.ic[i];
    for (uint32_t i = lane; i < nh; i += kWave) cd[i] = p.dc[i];
    for (uint32_t i = lane; i < nh1; i += kWave) H[i] = p.fir_state[(size_t)c * 2 * nh1 + i];
    for (uint32_t i = lane; i < p1; i += kWave) Z[i] = p.int_state[(size_t)c * 2 * p1 + i];
    float gain = p.alc ? p.gain[c] : 1.0f;
    const uint32_t step = p.nco ? p.step[c] : 0u;
    const uint32_t tph0 = f.tone_on ? f.tone_phase[c] : 0u, tstep = f.tone_on ? f.tone_step[c] : 0u;
    uint32_t carry = p.phase[c];                                 // wave-uniform: the phase behind the last output written
    const uint32_t nblk = p.block_size / nb, no = nb * L;
    __syncthreads();

    for (uint32_t b = 0; b < nblk; ++b) {
        // 1. ALC: arm_abs_f32 + arm_max_f32 -> gain law -> arm_scale_f32
        const size_t ib = (size_t)c * p.block_size + (size_t)b * nb;
        float m = 0.0f;
        for (uint32_t i = lane; i < nb; i += kWave) m = fmaxf(m, fabsf(fm_load_audio(src, ib + i)));
        if (p.alc) {
            m = wave_max(m);
            gain = agc_update<0>(p.alcp, gain, m);
        }
        for (uint32_t i = lane; i < nb; i += kWave) {
            float a = fm_load_audio(src, ib + i);
            if (p.alc) a = a * gain;
            if (nh) H[nh1 + i] = a;
            else Z[p1 + i] = a;
        }
        __syncthreads();
        // 2. arm_fir_f32 with the delay taps: the modulating signal I' (outputs i and i + 64 in one packed MAC)
        if (nh) {
            for (uint32_t i0 = 0; i0 < nb; i0 += 2 * kWave) {
                const uint32_t ia = i0 + lane, ib2 = ia + kWave;
                const uint32_t ra = ia < nb ? ia : 0u, rb = ib2 < nb ? ib2 : ra;     // lanes past the block read in bounds, store nothing
                fm_v2f r = { 0.0f, 0.0f };
#pragma unroll 4
                for (uint32_t k = 0; k < nh; ++k) {
                    const float cc = cd[k];
                    r = fm_mac2<ARITH>(r, fm_v2f{ H[ra + k], H[rb + k] }, fm_v2f{ cc, cc });
                }
                if (ia < nb) Z[p1 + ia] = r.x;
                if (ib2 < nb) Z[p1 + ib2] = r.y;
            }
            __syncthreads();
            for (uint32_t i0 = 0; i0 < nh1; i0 += kWave) {     // history tail, 64-wide slices
                const uint32_t i = i0 + lane;
                const float t = (i < nh1) ? H[nb + i] : 0.0f;
                __syncthreads();
                if (i < nh1) H[i] = t;
                __syncthreads();
            }
        }
        // 3.-5. interpolator on the I rail (two slices of 64 outputs per packed MAC), then the FM tail slice by slice
        const size_t ob = ((size_t)c * p.block_size + (size_t)b * nb) * L;
        for (uint32_t o0 = 0; o0 < no; o0 += 2 * kWave) {
            const uint32_t oa = o0 + lane, ob2 = oa + kWave;
            const uint32_t qa = oa < no ? oa : 0u, qb = ob2 < no ? ob2 : qa;         // in-bounds stand-ins for the lanes past the block
            fm_v2f u;
            if (p.ni) {
                const uint32_t na = qa / L, nb2 = qb / L;
                const float *ca = ci + (L - 1 - qa % L), *cb = ci + (L - 1 - qb % L);
                u = fm_v2f{ 0.0f, 0.0f };
#pragma unroll 4
                for (uint32_t t = 0; t < P; ++t)
                    u = fm_mac2<ARITH>(u, fm_v2f{ Z[na + t], Z[nb2 + t] }, fm_v2f{ ca[t * L], cb[t * L] });
            } else {
                u = fm_v2f{ Z[qa], Z[qb] };
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t o = h ? ob2 : oa;
                if (o0 + h * kWave >= no) break;                 // wave-uniform: no second slice
                const bool live = o < no;
                float w = h ? u.y : u.x;
                if (f.tone_on) {                                 // arm_sin_f32 -> arm_scale_f32 -> arm_add_f32
                    const uint32_t tp = tph0 + (b * no + o) * tstep;
                    const float xt = (float)(tp >> 8) * kNcoK;
                    const float t = sin_f32<0>(tab, xt) * f.tone_level;
                    w = w + t;
                }
                const float v = w * f.deviation;                 // arm_scale_f32
                const uint32_t d = fm_float_to_q31(v);
                const uint32_t inc = live ? d + step : 0u;
                const uint32_t incl = wave_scan_add(inc);        // all 64 lanes active here
                const uint32_t phase = carry + incl - step;      // phase += d; use; phase += step
                carry += __builtin_amdgcn_readlane(incl, 63);
                if (live) {
                    const float x = (float)(phase >> 8) * kNcoK;
                    const float re = cos_f32<0>(tab, x) * f.amplitude, im = sin_f32<0>(tab, x) * f.amplitude;
                    fm_store_iq(dst, ob + o, re, im, p.q15_round);
                }
            }
        }
        __syncthreads();
        if (p.ni) {
            for (uint32_t i0 = 0; i0 < p1; i0 += kWave) {
                const uint32_t i = i0 + lane;
                const float t = (i < p1) ? Z[nb + i] : 0.0f;
                __syncthreads();
                if (i < p1) Z[i] = t;
                __syncthreads();
            }
        }
    }
    for (uint32_t i = lane; i < nh1; i += kWave) {
        const float t = H[i];
        p.fir_state[(size_t)c * 2 * nh1 + i] = t;
        p.fir_state[(size_t)c * 2 * nh1 + nh1 + i] = t;
    }
    for (uint32_t i = lane; i < p1; i += kWave) p.int_state[(size_t)c * 2 * p1 + i] = Z[i];
    // the Q rail took block_size samples of +0.0f: what is older than that moves down
    float *qs = p.int_state + (size_t)c * 2 * p1 + p1;
    for (uint32_t i0 = 0; i0 < p1; i0 += kWave) {
        const uint32_t i = i0 + lane;
        const uint64_t from = (uint64_t)i + p.block_size;
        const float t = (i < p1 && from < p1) ? qs[from] : 0.0f;
        __syncthreads();
        if (i < p1) qs[i] = t;
        __syncthreads();
    }
    if (lane == 0) {
        if (p.alc) p.gain[c] = gain;
        p.phase[c] = carry;
        if (f.tone_on) f.tone_phase[c] = tph0 + p.block_size * L * tstep;
    }
}

template <int ARITH, typename TIn, typename TOut>
hipError_t launch_fm(const TxParams &p, const TxFmParams &f, const void *src, void *dst, hipStream_t st)
{
    const size_t lds = tx_fm_lds_bytes(p);
    auto k = k_tx_fm<ARITH, TIn, TOut>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k, dim3(p.channels), dim3(64), lds, st, p, f, static_cast<const TIn *>(src), static_cast<TOut *>(dst));
    return hipGetLastError();
}

}  // namespace

size_t tx_fm_lds_bytes(const TxParams &p)
{
    return sizeof(float) * fm_layout(p.ni, p.nh, p.P, p.block).total;
}

hipError_t launch_tx_fm(const TxParams &p, const TxFmParams &f, int arith, const void *src, bool q15, void *dst, hipStream_t st)
{
    const bool fma = arith != SELENITE_ARITH_CMSIS;              // SPLIT16 runs as FMA
    if (q15) return fma ? launch_fm<1, int16_t, int16_t>(p, f, src, dst, st) : launch_fm<0, int16_t, int16_t>(p, f, src, dst, st);
    return fma ? launch_fm<1, float, float>(p, f, src, dst, st) : launch_fm<0, float, float>(p, f, src, dst, st);
}

// ---- the host side (tx_host.h) ----

void tx_fm_free(selenite_tx_instance *S) { dev_free(S->fm.d_tone_step, S->fm.d_tone_phase); }

int tx_fm_reset(selenite_tx_instance *S)
{
    if (S->fm.d_tone_phase) HIPCHK(S, hipMemsetAsync(S->fm.d_tone_phase, 0, S->cfg.channels * sizeof(uint32_t), S->stream));
    return 0;
}

static int fm_state_copy(selenite_tx_instance *S, const selenite_tx_fm_state_view *v, bool to_host)
{
    if (!S || !v || !S->fm.set) return SELENITE_RX_ARGUMENT_ERROR;
    return copy_rows(S, to_host, { { S->fm.d_tone_phase, v->tone_phase, S->cfg.channels * sizeof(uint32_t) } });
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_tx_set_fm(selenite_tx_instance *S, const selenite_tx_fm_config *f)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    static_assert(sizeof(selenite_tx_fm_config) == 40 && offsetof(selenite_tx_fm_config, tone_step) == 24, "selenite_tx_fm_config layout (LP64)");
    selenite_tx_instance::Fm &F = S->fm;
    if (!f) {                                               // FM off again: not from under a running FM mode
        if (S->cfg.mode == SELENITE_MODE_FM) return SELENITE_RX_ARGUMENT_ERROR;
        F.set = false;
        return SELENITE_RX_SUCCESS;
    }
    if (f->struct_size != sizeof(selenite_tx_fm_config) || f->reserved != 0 || f->tone_enable > 1u ||
        !std::isfinite(f->deviation) || !(f->deviation > 0.0f) || !std::isfinite(f->amplitude) || !std::isfinite(f->tone_level))
        return SELENITE_RX_ARGUMENT_ERROR;                  // the previous setting stays
    const size_t C = S->cfg.channels;
    if (int rc = drain(S)) return rc;
    if (!F.d_tone_step) HIPCHK(S, dev_alloc(&F.d_tone_step, C));
    if (!F.d_tone_phase) HIPCHK(S, dev_alloc(&F.d_tone_phase, C));
    std::vector<uint32_t> ts(C);
    for (size_t c = 0; c < C; ++c) ts[c] = f->tone_step ? f->tone_step[c] : f->tone_step_all;
    HIPCHK(S, hipMemcpy(F.d_tone_step, ts.data(), C * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!F.set) HIPCHK(S, hipMemset(F.d_tone_phase, 0, C * sizeof(uint32_t)));       // a retune keeps the tone's phase
    F.p = TxFmParams{ f->deviation, f->amplitude, f->tone_level, f->tone_enable, F.d_tone_step, F.d_tone_phase };
    F.set = true;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_tx_get_fm_state(selenite_tx_instance *S, const selenite_tx_fm_state_view *v) { return fm_state_copy(S, v, true); }
extern "C" int selenite_tx_set_fm_state(selenite_tx_instance *S, const selenite_tx_fm_state_view *v) { return fm_state_copy(S, v, false); }
