// rx_out.hip -- audio output stage (step 7 of DESIGN.md section 2): arm_fir_interpolate_f32 of CMSIS-DSP 1.5.3
// (FilteringFunctions/arm_fir_interpolate_f32.c:136-563) per channel on the scaled audio behind the AGC, arm_float_to_q15 for the int16
// slots, and the mono / stereo frame format DSP_Out_Buff_Read writes (Core/Src/dsp_if.c:204-219: pbuf[k] = i, pbuf[k + 1] = q).
//
// Every output is independent: phase ph (0 .. L - 1) of input sample n is
//     y[n * L + ph] = sum_{t = 0}^{P - 1} x[n - (P - 1) + t] * pCoeffs[(L - 1 - ph) + t * L]
// one accumulator from +0.0f, t ascending, product rounded, then sum rounded (:389-440; the four-sample block :166-330 has the same order per
// output) -- no recurrence, so the bits do not depend on how the stream is cut into calls, and the unit is compiled with -ffp-contract=off:
// bit-exact against the reference in every arith mode.
//
// The kernel is bound by its stores (at L = 4, 4 bytes read and 8 .. 32 written per audio sample).  One single-wave workgroup per channel row:
// the row streams through LDS in tiles of kOutTile samples behind its P - 1 samples of history (first tile: the channel's state; the last
// P - 1 samples of history + tile are the next tile's history and, after the last tile, the new state -- a call shorter than P - 1 shifts
// the state, it does not overwrite it).  The taps sit in LDS phase-reversed (cs[t * L + ph]), so a lane's phases are consecutive words.
// A lane owns 16 consecutive bytes of the output row: 4 f32 / 2 f32 pairs / 8 int16 / 4 int16 pairs, packed to four dwords and stored as one
// non-temporal global_store_dwordx4 -- a wave store covers 1 KiB of the row; the audio, written a moment ago by the chain, is read with
// default (cached) loads.  Rows that are not 16-byte multiples (or a dst that is not 16-byte aligned) take element stores (OutParams::vec).
#include "rx_host.h"

#include <cmath>

namespace srx {

constexpr uint32_t kOutTile = 256;      // audio samples per LDS tile
constexpr uint32_t kOutMaxP = 64;       // phase length (arm_fir_interpolate_instance_f32.phaseLength) the LDS images are sized for
constexpr uint32_t kOutMaxL = 8;

typedef uint32_t u4v __attribute__((ext_vector_type(4)));

enum { kOutF32Mono = 0, kOutF32Stereo = 1, kOutQ15Mono = 2, kOutQ15Stereo = 3 };

template <int L, int FMT>
__global__ __launch_bounds__(64) void k_out(OutParams q, const float *__restrict__ audio, void *__restrict__ dst)
{
    constexpr uint32_t B = FMT == kOutF32Mono ? 4u : FMT == kOutF32Stereo ? 8u : FMT == kOutQ15Mono ? 2u : 4u;   // bytes per interpolated sample
    constexpr uint32_t K = 16u / B;                          // interpolated samples in a lane's 16 bytes
    constexpr uint32_t NPH = K < (uint32_t)L ? K : (uint32_t)L;   // ... as NPH consecutive phases of NI consecutive audio samples
    constexpr uint32_t NI = K / NPH;
    // (+ NI: a lane of a row's last, partial group reads up to NI - 1 samples behind the tile -- for outputs it then does not store)
    __shared__ float xs[kOutMaxP - 1 + kOutTile + 8];
    __shared__ float cs[kOutMaxP * kOutMaxL];

    const uint32_t lane = threadIdx.x, c = blockIdx.x;
    const uint32_t P = q.phase_len, H = P ? P - 1u : 0u, nout = q.nout;
    for (uint32_t i = lane; i < P * (uint32_t)L; i += kWave) cs[i] = q.coeffs[(i / L) * L + ((uint32_t)L - 1u - i % L)];
    float h = lane < H ? q.state[(size_t)c * H + lane] : 0.0f;
    const float *row = audio + (size_t)c * q.stride;
    bool nonfinite = false;

    for (uint32_t t0 = 0; t0 < nout; t0 += kOutTile) {
        const uint32_t nt = nout - t0 < kOutTile ? nout - t0 : kOutTile;
        __syncthreads();                                     // (one wave: orders the LDS traffic across lanes for the compiler)
        if (lane < H) xs[lane] = h;
        for (uint32_t i = lane; i < nt; i += kWave) xs[H + i] = row[t0 + i];
        __syncthreads();
        if (lane < H) h = xs[nt + lane];                     // the last P - 1 samples of history + tile

        const uint32_t ntl = nt * (uint32_t)L;               // interpolated samples of this tile
        for (uint32_t o0 = lane * K; o0 < ntl; o0 += kWave * K) {
            const uint32_t n0 = o0 / (uint32_t)L, phb = o0 % (uint32_t)L;
            float v[K];
            if (P == 0) {                                    // frames only (L == 1)
#pragma unroll
                for (uint32_t k = 0; k < K; ++k) v[k] = xs[n0 + k];
            } else {
                float acc[NI][NPH];
#pragma unroll
                for (uint32_t i = 0; i < NI; ++i)
#pragma unroll
                    for (uint32_t j = 0; j < NPH; ++j) acc[i][j] = 0.0f;
                const float *xp = xs + n0, *cp = cs + phb;
#pragma unroll 1
                for (uint32_t t = 0; t < P; ++t) {
                    float xv[NI], cv[NPH];
#pragma unroll
                    for (uint32_t i = 0; i < NI; ++i) xv[i] = xp[t + i];
#pragma unroll
                    for (uint32_t j = 0; j < NPH; ++j) cv[j] = cp[t * (uint32_t)L + j];
#pragma unroll
                    for (uint32_t i = 0; i < NI; ++i)
#pragma unroll
                        for (uint32_t j = 0; j < NPH; ++j) {
                            const float p = xv[i] * cv[j];
                            acc[i][j] = acc[i][j] + p;
                        }
                }
#pragma unroll
                for (uint32_t i = 0; i < NI; ++i)
#pragma unroll
                    for (uint32_t j = 0; j < NPH; ++j) v[i * NPH + j] = acc[i][j];
            }
            const uint32_t nval = ntl - o0 < K ? ntl - o0 : K;      // (K unless the row's bytes are no multiple of 16)
#pragma unroll
            for (uint32_t k = 0; k < K; ++k) nonfinite = nonfinite || (k < nval && !__builtin_isfinite(v[k]));

            const size_t o = ((size_t)c * nout + t0) * (uint32_t)L + o0;      // interpolated-sample index in dst
            char *at = static_cast<char *>(dst) + o * B;
            if (q.vec) {
                u4v w;
                if constexpr (FMT == kOutF32Mono) {
                    w = u4v{ __float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]) };
                } else if constexpr (FMT == kOutF32Stereo) {
                    w = u4v{ __float_as_uint(v[0]), __float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[1]) };
                } else if constexpr (FMT == kOutQ15Mono) {
                    uint32_t w0, w1, w2, w3;
                    float4_to_q15(v[0], v[1], v[2], v[3], q.q15_round, w0, w1);
                    float4_to_q15(v[4], v[5], v[6], v[7], q.q15_round, w2, w3);
                    w = u4v{ w0, w1, w2, w3 };
                } else {
                    uint32_t w0, w1, w2, w3;
                    float4_to_q15(v[0], v[0], v[1], v[1], q.q15_round, w0, w1);
                    float4_to_q15(v[2], v[2], v[3], v[3], q.q15_round, w2, w3);
                    w = u4v{ w0, w1, w2, w3 };
                }
                // (the non-temporal store as the instruction itself, as the fused kernels' audio store: written once, never read back;
                // s_nop: the wait states a VALU write of the data registers needs behind a store wider than 64 bits)
                asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" :: "v"(at), "v"(w) : "memory");
            } else {
#pragma unroll
                for (uint32_t k = 0; k < K; ++k) {
                    if (k >= nval) break;
                    if constexpr (FMT == kOutF32Mono) {
                        reinterpret_cast<float *>(at)[k] = v[k];
                    } else if constexpr (FMT == kOutF32Stereo) {
                        reinterpret_cast<float *>(at)[2 * k] = v[k];
                        reinterpret_cast<float *>(at)[2 * k + 1] = v[k];
                    } else if constexpr (FMT == kOutQ15Mono) {
                        reinterpret_cast<int16_t *>(at)[k] = float_to_q15(v[k], q.q15_round);
                    } else {
                        const int16_t s = float_to_q15(v[k], q.q15_round);
                        reinterpret_cast<int16_t *>(at)[2 * k] = s;
                        reinterpret_cast<int16_t *>(at)[2 * k + 1] = s;
                    }
                }
            }
        }
    }
    if (lane < H) q.state[(size_t)c * H + lane] = h;
    if (nonfinite) q.flags[kFlagNanInf] = 1u;        // ARM_MATH_NANINF, read by selenite_rx_sync / the host-pointer calls
}

template <int L>
static void launch_out_l(const OutParams &q, int fmt, const float *audio, void *dst, hipStream_t st)
{
    const dim3 grid(q.channels), blk(kWave);
    switch (fmt) {
    case kOutF32Mono: hipLaunchKernelGGL((k_out<L, kOutF32Mono>), grid, blk, 0, st, q, audio, dst); break;
    case kOutF32Stereo: hipLaunchKernelGGL((k_out<L, kOutF32Stereo>), grid, blk, 0, st, q, audio, dst); break;
    case kOutQ15Mono: hipLaunchKernelGGL((k_out<L, kOutQ15Mono>), grid, blk, 0, st, q, audio, dst); break;
    default: hipLaunchKernelGGL((k_out<L, kOutQ15Stereo>), grid, blk, 0, st, q, audio, dst); break;
    }
}

hipError_t launch_out(const OutParams &q, uint32_t interp, bool stereo, bool dst_q15, const float *audio, void *dst, hipStream_t st)
{
    if (q.channels == 0 || q.nout == 0) return hipSuccess;
    if (q.phase_len > kOutMaxP || (q.phase_len == 0 && interp != 1)) return hipErrorInvalidValue;
    const int fmt = dst_q15 ? (stereo ? kOutQ15Stereo : kOutQ15Mono) : (stereo ? kOutF32Stereo : kOutF32Mono);
    switch (interp) {
    case 1: launch_out_l<1>(q, fmt, audio, dst, st); break;
    case 2: launch_out_l<2>(q, fmt, audio, dst, st); break;
    case 4: launch_out_l<4>(q, fmt, audio, dst, st); break;
    case 8: launch_out_l<8>(q, fmt, audio, dst, st); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- host side of the stage ----
void OutStage::release()
{
    dev_free(d_coeffs, d_state, d_audio);
    audio_bytes = 0;
    on = false;
    interp = 1; taps = 0; frames = SELENITE_RX_OUT_MONO;
}

// the output stage's state as arm_fir_interpolate_init_f32 leaves it (arm_fir_interpolate_init_f32.c:101-104): cleared
int OutStage::init_state(selenite_rx_instance *S)
{
    if (!on || taps / interp < 2) return SELENITE_RX_SUCCESS;
    const size_t n = (size_t)S->cfg.channels * (taps / interp - 1);
    HIPCHK(S, hipMemsetAsync(d_state, 0, n * sizeof(float), S->stream));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    return SELENITE_RX_SUCCESS;
}

OutParams OutStage::params(const selenite_rx_instance *S, ChanRange r, const void *dst, bool dst_q15, uint32_t block_size) const
{
    OutParams q{};
    q.channels = r.count;
    q.nout = block_size / S->cfg.decim; q.stride = q.nout;
    q.phase_len = taps / interp;
    q.q15_round = S->cfg.q15_rounding ? 1u : 0u;
    const size_t row_bytes = (size_t)q.nout * interp * out_sample_bytes(frames == SELENITE_RX_OUT_STEREO, dst_q15);
    q.vec = (reinterpret_cast<uintptr_t>(dst) % 16 == 0 && row_bytes % 16 == 0) ? 1u : 0u;
    q.coeffs = d_coeffs;
    q.state = d_state ? d_state + (size_t)r.first * (q.phase_len - 1) : nullptr;
    q.flags = S->d_flags;
    return q;
}

// grown, never allocated per call
int OutStage::audio_buffer(selenite_rx_instance *S, ChanRange r, uint32_t block_size, float **audio)
{
    int rc = ensure(S, (void **)&d_audio, &audio_bytes, (size_t)r.count * (block_size / S->cfg.decim) * sizeof(float));
    *audio = d_audio;
    return rc;
}

int OutStage::run(selenite_rx_instance *S, ChanRange r, const float *audio, void *dst, bool dst_q15, uint32_t block_size) const
{
    HIPCHK(S, launch_out(params(S, r, dst, dst_q15, block_size), interp, frames == SELENITE_RX_OUT_STEREO, dst_q15, audio, dst, S->stream));
    return SELENITE_RX_SUCCESS;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_out(selenite_rx_instance *S, const selenite_rx_out_config *out)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_out: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    if (out) {
        const uint32_t L = out->interp;
        const char *bad = nullptr;
        int code = SELENITE_RX_ARGUMENT_ERROR;
        if (out->struct_size != sizeof(selenite_rx_out_config)) bad = "struct_size is not sizeof(selenite_rx_out_config)";
        else if (L != 1 && L != 2 && L != 4 && L != 8) bad = "interp is not 1, 2, 4 or 8";
        else if (out->ni_taps % L != 0) { bad = "ni_taps is not a multiple of interp"; code = SELENITE_RX_LENGTH_ERROR; }   // arm_fir_interpolate_init_f32.c:91-96
        else if (out->ni_taps / L > 64 || (out->ni_taps == 0 && L != 1)) bad = "ni_taps / interp is not 1 .. 64 (0 taps: interp 1 only)";
        else if (out->frames != SELENITE_RX_OUT_MONO && out->frames != SELENITE_RX_OUT_STEREO) bad = "frames is not a SELENITE_RX_OUT_* value";
        else if (out->ni_taps && !out->coeffs) bad = "coeffs is NULL";
        else
            for (uint32_t k = 0; k < out->ni_taps && !bad; ++k)
                if (!std::isfinite(out->coeffs[k])) bad = "coeffs holds a non-finite tap";
        if (bad) return refuse("selenite_rx_set_out", bad, code);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    OutStage &st = S->out;
    st.release();
    if (!out) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels, P = out->ni_taps / out->interp;
    hipError_t e = dev_upload(&st.d_coeffs, out->coeffs, (size_t)out->ni_taps);
    if (e == hipSuccess) e = dev_alloc(&st.d_state, P > 1 ? C * (P - 1) : 0);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_out: hipMalloc: ") + hipGetErrorString(e));
    }
    st.on = true; st.interp = out->interp; st.taps = out->ni_taps; st.frames = out->frames;
    return st.init_state(S);
}

extern "C" uint32_t selenite_rx_out_values(const selenite_rx_instance *S, uint32_t blockSize)
{
    if (!S) return 0;
    const uint32_t n = blockSize / S->cfg.decim;
    return S->out.on ? n * S->out.interp * (S->out.frames == SELENITE_RX_OUT_STEREO ? 2u : 1u) : n;
}

static int out_state_copy(selenite_rx_instance *S, float *host, bool to_host)
{
    if (!S || !host || !S->out.on || S->out.taps / S->out.interp < 2) return SELENITE_RX_ARGUMENT_ERROR;
    return copy_rows(S, to_host, { { S->out.d_state, host, (size_t)S->cfg.channels * (S->out.taps / S->out.interp - 1) * sizeof(float) } });
}
extern "C" int selenite_rx_get_out_state(selenite_rx_instance *S, float *interp_state) { return out_state_copy(S, interp_state, true); }
extern "C" int selenite_rx_set_out_state(selenite_rx_instance *S, const float *interp_state)
{
    return out_state_copy(S, const_cast<float *>(interp_state), false);
}
