// tx_cw.hip -- the keyed CW path of the batched TX chain (include/selenite_tx_cw.h: selenite_tx_set_cw; DESIGN.md section 2 "TX CW keyed",
// section 5.17).  key bytes -> e0 in {+0.0f, 1.0f} -> arm_fir_f32 (shape taps) -> amplitude -> arm_fir_interpolate_f32 by L on ONE rail ->
// (cos, sin) of the integer phase times the envelope; beside it the sidetone at the audio rate and the break-in flag per DSP block.
//
// No audio is read: one key byte in, 8 L bytes of I/Q out.  k_tx_fm's unit of work (one single-wave workgroup per channel, DSP block by
// DSP block) without the ALC pass and without the scan: the phase of output m is phase0 + m * step_eff.  A lane owns two ADJACENT
// outputs: for an even L they share their input samples (one LDS read of the state feeds both halves of the packed MAC, the two taps
// come as one aligned 8-byte read) and leave as one 16-byte (int16: 8-byte) store.
// A DSP block whose key window (history and block) is all up or all down skips the shaping FIR: with every e0 = 1.0f the accumulator
// takes the taps themselves in order (1.0f * c is c), which is TxCwParams::shape_sum, summed in that order on the host; with every
// e0 = +0.0f each product is +-0.0f and the accumulator, started at +0.0f, stays +0.0f under round-to-nearest (finite taps).
// Kernel, launcher and the host side of the path: selenite_tx_set_cw, its state accessors and the key entries.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "rx_device.h"
#include "tx_host.h"

namespace srx {

namespace {

typedef float cw_v2f __attribute__((ext_vector_type(2)));

__host__ __device__ inline uint32_t cw_up4(uint32_t v) { return (v + 3u) & ~3u; }

// LDS of k_tx_cw, in floats: sine table | interpolator taps | shape taps | key window (as e0: ns - 1 of history, then the block) |
// arm_fir_interpolate_f32 pState of the I rail
struct CwLds { uint32_t tab, ci, cs, K, Z, total; };
__host__ __device__ inline CwLds cw_layout(uint32_t ni, uint32_t ns, uint32_t P, uint32_t nb)
{
    CwLds L;
    uint32_t o = 0;
    L.tab = o; o += 516;
    L.ci = o;  o += cw_up4(ni);
    L.cs = o;  o += cw_up4(ns);
    L.K = o;   o += cw_up4((ns - 1) + nb);
    L.Z = o;   o += cw_up4((P - 1) + nb);
    L.total = o;
    return L;
}

template <int ARITH>
__device__ __forceinline__ cw_v2f cw_mac2(cw_v2f acc, cw_v2f w, cw_v2f c2)
{
    if constexpr (ARITH == 1) return __builtin_elementwise_fma(w, c2, acc);
    else { const cw_v2f pr = w * c2; return acc + pr; }
}

__device__ __forceinline__ void cw_store_iq(float *p, size_t i, float re, float im, uint32_t)
{
    reinterpret_cast<float2 *>(p)[i] = make_float2(re, im);
}
__device__ __forceinline__ void cw_store_iq(int16_t *p, size_t i, float re, float im, uint32_t round)
{
    short2 v;
    v.x = float_to_q15(re, round);
    v.y = float_to_q15(im, round);
    reinterpret_cast<short2 *>(p)[i] = v;
}
// outputs i and i + 1 (i even, the destination 16-byte / 8-byte aligned) as one store
__device__ __forceinline__ void cw_store_iq2(float *p, size_t i, float re0, float im0, float re1, float im1, uint32_t)
{
    reinterpret_cast<float4 *>(p)[i >> 1] = make_float4(re0, im0, re1, im1);
}
__device__ __forceinline__ void cw_store_iq2(int16_t *p, size_t i, float re0, float im0, float re1, float im1, uint32_t round)
{
    short4 v;
    v.x = float_to_q15(re0, round);
    v.y = float_to_q15(im0, round);
    v.z = float_to_q15(re1, round);
    v.w = float_to_q15(im1, round);
    reinterpret_cast<short4 *>(p)[i >> 1] = v;
}

// the speaker mix: arm_add_f32 / arm_add_q15 (BasicMathFunctions/arm_add_q15.c: __SSAT(a + b, 16))
__device__ __forceinline__ void cw_side(float *p, size_t i, float y, uint32_t mix, uint32_t)
{
    p[i] = mix ? p[i] + y : y;
}
__device__ __forceinline__ void cw_side(int16_t *p, size_t i, float y, uint32_t mix, uint32_t round)
{
    const int16_t q = float_to_q15(y, round);
    if (mix) {
        int s = (int)p[i] + (int)q;
        s = s > 32767 ? 32767 : (s < -32768 ? -32768 : s);
        p[i] = (int16_t)s;
    } else {
        p[i] = q;
    }
}

template <int ARITH, typename TOut, bool SIDE>
__global__ __launch_bounds__(64) void k_tx_cw(TxParams p, TxCwParams w, const uint8_t *__restrict__ key, TOut *__restrict__ dst, TOut *side,
                                              uint32_t wide)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    const uint32_t nb = p.block, L = p.L, P = p.P, p1 = P - 1, ns = w.ns, ns1 = ns - 1;
    const CwLds Y = cw_layout(p.ni, ns, P, nb);
    float *tab = lds + Y.tab, *ci = lds + Y.ci, *cs = lds + Y.cs;
    float *K = lds + Y.K;                                        // arm_fir_f32 pState of the shaping FIR: e0 of the key window
    float *Z = lds + Y.Z;                                        // arm_fir_interpolate_f32 pState of the I rail
    for (uint32_t i = lane; i < 513; i += kWave) tab[i] = p.sintab[i];
    for (uint32_t i = lane; i < p.ni; i += kWave) ci[i] = p.ic[i];
    for (uint32_t i = lane; i < ns; i += kWave) cs[i] = w.shape[i];
    for (uint32_t i = lane; i < ns1; i += kWave) K[i] = w.key_state[(size_t)c * ns1 + i] ? 1.0f : 0.0f;
    for (uint32_t i = lane; i < p1; i += kWave) Z[i] = p.int_state[(size_t)c * 2 * p1 + i];
    const uint32_t ph0 = p.phase[c], step = (p.nco ? p.step[c] : 0u) + w.offset;
    const uint32_t sph0 = w.side_phase[c], sstep = w.side_step[c];
    uint32_t tx_on = w.tx_on[c], hold = w.hold[c];
    const uint32_t nblk = p.block_size / nb, no = nb * L;
    const bool words = (nb & 3u) == 0 && (reinterpret_cast<uintptr_t>(key) & 3u) == 0;     // block_size is a multiple of nb
    const bool pairs = (L & 1u) == 0;                            // a lane's two outputs share their input samples
    __syncthreads();

    for (uint32_t b = 0; b < nblk; ++b) {
        // 1. the key bytes of the block, as words where the layout allows it; the break-in flag of the block
        const size_t kb = (size_t)c * p.block_size + (size_t)b * nb;
        bool down = false;
        if (words) {
            const uint32_t *kw = reinterpret_cast<const uint32_t *>(key + kb);
            for (uint32_t i = lane; i < nb / 4; i += kWave) {
                const uint32_t v = kw[i];
                float *k4 = K + ns1 + 4 * i;
                k4[0] = (v & 0x000000FFu) ? 1.0f : 0.0f;
                k4[1] = (v & 0x0000FF00u) ? 1.0f : 0.0f;
                k4[2] = (v & 0x00FF0000u) ? 1.0f : 0.0f;
                k4[3] = (v & 0xFF000000u) ? 1.0f : 0.0f;
                down = down || v != 0u;
            }
        } else {
            for (uint32_t i = lane; i < nb; i += kWave) {
                const bool v = key[kb + i] != 0;
                K[ns1 + i] = v ? 1.0f : 0.0f;
                down = down || v;
            }
        }
        if (__ballot(down) != 0ull) { tx_on = 1u; hold = w.hang_blocks; }
        else if (tx_on) { if (hold == 0u) tx_on = 0u; else hold -= 1u; }
        __syncthreads();
        // 2. arm_fir_f32 with the shape taps -> e, arm_scale_f32 -> a (the interpolator's input), the sidetone from e
        bool someup = false, somedown = false;
        for (uint32_t i = lane; i < ns1 + nb; i += kWave) {
            const bool v = K[i] != 0.0f;
            someup = someup || v;
            somedown = somedown || !v;
        }
        const bool allup = __ballot(somedown) == 0ull, alldown = __ballot(someup) == 0ull;       // wave-uniform
        auto finish = [&](uint32_t i, float e) {
            Z[p1 + i] = e * w.amplitude;
            if constexpr (SIDE) {
                const uint32_t sp = sph0 + (b * nb + i) * sstep;
                const float xs = (float)(sp >> 8) * kNcoK;
                const float s = sin_f32<0>(tab, xs);
                const float g = e * w.side_level;
                cw_side(side, kb + i, s * g, w.side_mix, p.q15_round);
            }
        };
        if (allup || alldown) {
            const float e = allup ? w.shape_sum : 0.0f;
            for (uint32_t i = lane; i < nb; i += kWave) finish(i, e);
        } else {
            for (uint32_t i0 = 0; i0 < nb; i0 += 2 * kWave) {    // outputs i and i + 64 in one packed MAC; the products are exact
                const uint32_t ia = i0 + lane, ib = ia + kWave;
                const uint32_t ra = ia < nb ? ia : 0u, rb = ib < nb ? ib : ra;       // lanes past the block read in bounds, store nothing
                cw_v2f r = { 0.0f, 0.0f };
#pragma unroll 4
                for (uint32_t k = 0; k < ns; ++k) {
                    const float cc = cs[k];
                    r = cw_mac2<0>(r, cw_v2f{ K[ra + k], K[rb + k] }, cw_v2f{ cc, cc });
                }
                if (ia < nb) finish(ia, r.x);
                if (ib < nb) finish(ib, r.y);
            }
        }
        __syncthreads();
        for (uint32_t i0 = 0; i0 < ns1; i0 += kWave) {           // key history, 64-wide slices
            const uint32_t i = i0 + lane;
            const float t = (i < ns1) ? K[nb + i] : 0.0f;
            __syncthreads();
            if (i < ns1) K[i] = t;
            __syncthreads();
        }
        // 3. interpolator on the I rail, two adjacent outputs per lane and packed MAC; carrier at phase0 + m * step; store
        const size_t ob = ((size_t)c * p.block_size + (size_t)b * nb) * L;
        for (uint32_t o0 = 0; o0 < no; o0 += 2 * kWave) {
            const uint32_t oa = o0 + 2 * lane, ob2 = oa + 1;
            const uint32_t qa = oa < no ? oa : 0u, qb = ob2 < no ? ob2 : qa;         // in-bounds stand-ins for the lanes past the block
            cw_v2f u;
            if (p.ni) {
                u = cw_v2f{ 0.0f, 0.0f };
                if (pairs) {
                    const uint32_t n = qa / L, phs = qa % L;     // phs even: the taps of outputs qa + 1 and qa are an aligned pair
                    const cw_v2f *cp = reinterpret_cast<const cw_v2f *>(ci + (L - 2 - phs));
                    const uint32_t l2 = L >> 1;
#pragma unroll 4
                    for (uint32_t t = 0; t < P; ++t) {
                        const float z = Z[n + t];
                        const cw_v2f cc = cp[t * l2];
                        u = cw_mac2<ARITH>(u, cw_v2f{ z, z }, cw_v2f{ cc.y, cc.x });
                    }
                } else {
                    const uint32_t na = qa / L, nb2 = qb / L;
                    const float *ca = ci + (L - 1 - qa % L), *cb = ci + (L - 1 - qb % L);
#pragma unroll 4
                    for (uint32_t t = 0; t < P; ++t)
                        u = cw_mac2<ARITH>(u, cw_v2f{ Z[na + t], Z[nb2 + t] }, cw_v2f{ ca[t * L], cb[t * L] });
                }
            } else {
                u = cw_v2f{ Z[qa], Z[qb] };
            }
            const uint32_t pha = ph0 + (b * no + oa) * step, phb = pha + step;
            const float xa = (float)(pha >> 8) * kNcoK, xb = (float)(phb >> 8) * kNcoK;
            const float rea = cos_f32<0>(tab, xa) * u.x, ima = sin_f32<0>(tab, xa) * u.x;      // arm_scale_f32
            const float reb = cos_f32<0>(tab, xb) * u.y, imb = sin_f32<0>(tab, xb) * u.y;
            if (wide) {                                          // L even: ob + oa is even and ob2 < no whenever oa < no
                if (oa < no) cw_store_iq2(dst, ob + oa, rea, ima, reb, imb, p.q15_round);
            } else {
                if (oa < no) cw_store_iq(dst, ob + oa, rea, ima, p.q15_round);
                if (ob2 < no) cw_store_iq(dst, ob + ob2, reb, imb, p.q15_round);
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
    for (uint32_t i = lane; i < ns1; i += kWave) w.key_state[(size_t)c * ns1 + i] = K[i] != 0.0f ? 1 : 0;
    for (uint32_t i = lane; i < p1; i += kWave) p.int_state[(size_t)c * 2 * p1 + i] = Z[i];
    // the Q rail took block_size samples of +0.0f: what is older than that moves down (as in k_tx_fm)
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
        p.phase[c] = ph0 + p.block_size * L * step;
        w.side_phase[c] = sph0 + p.block_size * sstep;
        w.tx_on[c] = tx_on;
        w.hold[c] = hold;
    }
}

template <int ARITH, typename TOut>
hipError_t launch_cw(const TxParams &p, const TxCwParams &w, const uint8_t *key, void *dst, void *side, hipStream_t st)
{
    const size_t lds = tx_cw_lds_bytes(p, w);
    auto k = side ? k_tx_cw<ARITH, TOut, true> : k_tx_cw<ARITH, TOut, false>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // one store for a lane's two outputs: L even (every block of a channel then starts at an even output) and the destination aligned to it
    const uint32_t wide = (p.L & 1u) == 0 && (reinterpret_cast<uintptr_t>(dst) % (4 * sizeof(TOut))) == 0 ? 1u : 0u;
    hipLaunchKernelGGL(k, dim3(p.channels), dim3(64), lds, st, p, w, key, static_cast<TOut *>(dst), static_cast<TOut *>(side), wide);
    return hipGetLastError();
}

}  // namespace

size_t tx_cw_lds_bytes(const TxParams &p, const TxCwParams &w)
{
    // cw_layout's sum in 64 bits: ns_taps is the caller's and may be anything
    const uint64_t words = 516ull + cw_up4(p.ni) + (((uint64_t)w.ns + 3u) & ~3ull) + (((uint64_t)w.ns - 1u + p.block + 3u) & ~3ull) +
                           (((uint64_t)p.P - 1u + p.block + 3u) & ~3ull);
    return (size_t)(sizeof(float) * words);
}

hipError_t launch_tx_cw(const TxParams &p, const TxCwParams &w, int arith, const uint8_t *key, bool q15, void *dst, void *side, hipStream_t st)
{
    const bool fma = arith != SELENITE_ARITH_CMSIS;              // SPLIT16 runs as FMA
    if (q15) return fma ? launch_cw<1, int16_t>(p, w, key, dst, side, st) : launch_cw<0, int16_t>(p, w, key, dst, side, st);
    return fma ? launch_cw<1, float>(p, w, key, dst, side, st) : launch_cw<0, float>(p, w, key, dst, side, st);
}

// ---- the host side (tx_host.h) ----

void tx_cw_free(selenite_tx_instance *S)
{
    selenite_tx_instance::Cw &W = S->cw;
    dev_free(W.d_shape, W.d_side_step, W.d_side_phase, W.d_tx_on, W.d_hold, W.d_key_state, W.d_io_side);
}

int tx_cw_reset(selenite_tx_instance *S)
{
    const selenite_tx_instance::Cw &W = S->cw;
    const size_t C = S->cfg.channels;
    if (!W.set) return 0;
    if (W.p.ns > 1) HIPCHK(S, hipMemsetAsync(W.d_key_state, 0, C * (W.p.ns - 1), S->stream));
    for (uint32_t *row : { W.d_side_phase, W.d_tx_on, W.d_hold }) HIPCHK(S, hipMemsetAsync(row, 0, C * sizeof(uint32_t), S->stream));
    return 0;
}

// keyed CW: every refusal comes before anything is written
static int key_call_ok(selenite_tx_instance *S, const void *key, const void *dst, uint32_t bs, const char *who)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    if (!S->cw.set) return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": keyed CW is not configured (selenite_tx_set_cw)");
    if (S->cfg.mode != SELENITE_MODE_CW && S->cfg.mode != SELENITE_MODE_CWR)
        return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": the mode is neither CW nor CWR");
    if (!key || !dst) return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": NULL buffer");
    if (!block_size_ok(S, bs, who)) return SELENITE_RX_LENGTH_ERROR;
    if (decide(S, make_params(S, bs), true).refused)
        return fail(S, SELENITE_RX_LENGTH_ERROR, "filter lengths exceed the LDS budget of the TX kernel");
    return 0;
}

static int run_key(selenite_tx_instance *S, const uint8_t *key, void *dst, void *side, bool q15, uint32_t bs)
{
    HIPCHK(S, hipSetDevice(S->device));
    const TxParams p = make_params(S, bs);
    TxCwParams w = S->cw.p;
    if (S->cfg.mode == SELENITE_MODE_CWR) w.offset = 0u - w.offset;
    if (decide(S, p, true).clears_uniform) S->phase_uniform = false;   // the carrier offset went into the phase accumulator, as after FM
    HIPCHK(S, launch_tx_cw(p, w, (int)S->cfg.arith, key, q15, dst, side, S->stream));
    return 0;
}

static int process_key_device(selenite_tx_instance *S, const uint8_t *key, void *dst, void *side, uint32_t bs, bool q15, const char *who)
{
    if (int r = key_call_ok(S, key, dst, bs, who)) return r;
    return run_key(S, key, dst, side, q15, bs);
}

static int process_key_host(selenite_tx_instance *S, const uint8_t *key, void *dst, void *side, uint32_t bs, bool q15, const char *who)
{
    if (int r = key_call_ok(S, key, dst, bs, who)) return r;
    selenite_tx_instance::Cw &W = S->cw;
    const size_t nin = (size_t)S->cfg.channels * bs, nside = nin * sample_bytes(q15), nout = nside * S->cfg.interp * 2;
    return staged_call(S, { { key, nin, kToDevice, &S->d_io_in, &S->io_in_bytes }, { dst, nout, kToHost, &S->d_io_out, &S->io_out_bytes },
                            { side, nside, W.p.side_mix ? kToDevice | kToHost : kToHost, &W.d_io_side, &W.io_side_bytes } },
                       [&] { return run_key(S, static_cast<const uint8_t *>(S->d_io_in), S->d_io_out, side ? W.d_io_side : nullptr, q15, bs); });
}

// the two halves of a key call, for the keyer stage (tx_keyer.hip), which runs them on the bytes it generates
int tx_key_call_ok(selenite_tx_instance *S, const void *key, const void *dst, uint32_t bs, const char *who) { return key_call_ok(S, key, dst, bs, who); }
int tx_run_key(selenite_tx_instance *S, const uint8_t *key, void *dst, void *side, bool q15, uint32_t bs) { return run_key(S, key, dst, side, q15, bs); }

static int cw_state_copy(selenite_tx_instance *S, const selenite_tx_cw_state_view *v, bool to_host)
{
    if (!S || !v || !S->cw.set) return SELENITE_RX_ARGUMENT_ERROR;
    const selenite_tx_instance::Cw &W = S->cw;
    const size_t C = S->cfg.channels, nk = C * (W.p.ns - 1);
    std::vector<uint8_t> ks;                                // into the device: any non-zero byte is key-down
    if (!to_host && v->key_state) ks.assign(v->key_state, v->key_state + nk);
    for (uint8_t &k : ks) k = k ? 1 : 0;
    return copy_rows(S, to_host, { { W.d_key_state, ks.empty() ? v->key_state : ks.data(), nk }, { W.d_side_phase, v->side_phase, C * sizeof(uint32_t) },
                                   { W.d_tx_on, v->tx_on, C * sizeof(uint32_t) }, { W.d_hold, v->hold, C * sizeof(uint32_t) } });
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_tx_set_cw(selenite_tx_instance *S, const selenite_tx_cw_config *f)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    static_assert(sizeof(selenite_tx_cw_config) == 56 && offsetof(selenite_tx_cw_config, side_step) == 32, "selenite_tx_cw_config layout (LP64)");
    selenite_tx_instance::Cw &W = S->cw;
    if (!f) {                                               // keyed CW off again, in any mode: the audio entries never needed it
        W.set = false;
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
    const bool first = !W.set, new_len = first || f->ns_taps != W.p.ns;
    if (int rc = drain(S)) return rc;
    for (uint32_t **row : { &W.d_side_step, &W.d_side_phase, &W.d_tx_on, &W.d_hold })
        if (!*row) HIPCHK(S, dev_alloc(row, C));
    // what depends on ns_taps is allocated before anything of the previous setting is given up
    float *shape = W.d_shape;
    uint8_t *ks = W.d_key_state;
    if (new_len || !shape) {
        HIPCHK(S, dev_alloc(&shape, (size_t)f->ns_taps));
        if (dev_alloc(&ks, C * ns1) != hipSuccess) {
            (void)hipFree(shape);
            return fail(S, SELENITE_RX_DEVICE_ERROR, "hipMalloc(key_state)");
        }
    }
    if (shape != W.d_shape) {
        dev_free(W.d_shape, W.d_key_state);
        W.d_shape = shape; W.d_key_state = ks;
    }
    std::vector<uint32_t> ss(C);
    for (size_t c = 0; c < C; ++c) ss[c] = f->side_step ? f->side_step[c] : f->side_step_all;
    HIPCHK(S, hipMemcpy(W.d_shape, f->shape_coeffs, f->ns_taps * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(S, hipMemcpy(W.d_side_step, ss.data(), C * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (new_len && ns1) HIPCHK(S, hipMemset(W.d_key_state, 0, C * ns1));
    if (first)                                              // a retune keeps the sidetone's phase and the break-in state
        for (uint32_t *row : { W.d_side_phase, W.d_tx_on, W.d_hold }) HIPCHK(S, hipMemset(row, 0, C * sizeof(uint32_t)));
    W.p = TxCwParams{ f->ns_taps, W.d_shape, sum, f->amplitude, f->side_level, f->offset_step, f->side_mix, f->hang_blocks,
                      W.d_side_step, W.d_side_phase, W.d_tx_on, W.d_hold, W.d_key_state };
    W.set = true;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_tx_get_cw_state(selenite_tx_instance *S, const selenite_tx_cw_state_view *v) { return cw_state_copy(S, v, true); }
extern "C" int selenite_tx_set_cw_state(selenite_tx_instance *S, const selenite_tx_cw_state_view *v) { return cw_state_copy(S, v, false); }

extern "C" int selenite_tx_process_key_f32_device(selenite_tx_instance *S, const uint8_t *key, float *dst, float *side, uint32_t bs) { return process_key_device(S, key, dst, side, bs, false, "selenite_tx_process_key_f32_device"); }
extern "C" int selenite_tx_process_key_q15_device(selenite_tx_instance *S, const uint8_t *key, int16_t *dst, int16_t *side, uint32_t bs) { return process_key_device(S, key, dst, side, bs, true, "selenite_tx_process_key_q15_device"); }
extern "C" int selenite_tx_process_key_f32(selenite_tx_instance *S, const uint8_t *key, float *dst, float *side, uint32_t bs) { return process_key_host(S, key, dst, side, bs, false, "selenite_tx_process_key_f32"); }
extern "C" int selenite_tx_process_key_q15(selenite_tx_instance *S, const uint8_t *key, int16_t *dst, int16_t *side, uint32_t bs) { return process_key_host(S, key, dst, side, bs, true, "selenite_tx_process_key_q15"); }

extern "C" const uint32_t *selenite_tx_cw_txon_device(selenite_tx_instance *S) { return (S && S->cw.set) ? S->cw.d_tx_on : nullptr; }

extern "C" int selenite_tx_time_process_key_device(selenite_tx_instance *S, const uint8_t *key, float *dst, float *side, uint32_t bs,
                                                   uint32_t iters, float *ms_per_call)
{
    if (!S || !ms_per_call || iters == 0) return SELENITE_RX_ARGUMENT_ERROR;
    if (int r = key_call_ok(S, key, dst, bs, "selenite_tx_time_process_key_device")) return r;
    return timed_loop(S, iters, ms_per_call, [&] { return run_key(S, key, dst, side, false, bs); });
}
