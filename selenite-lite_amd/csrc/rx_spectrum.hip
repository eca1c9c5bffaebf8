// rx_spectrum.hip -- spectrum tap (step 0b of DESIGN.md section 2, section 5.8): per channel, on the raw input I/Q of the call in front of the
// NCO, the power spectrum a panadapter draws.  The stream is cut into frames of N = 64 or 512 complex samples; every stride-th frame is
//     arm_cmplx_mult_real_f32(frame, window)          ComplexMathFunctions/arm_cmplx_mult_real_f32.c (absent without a window)
//     arm_cfft_f32(&arm_cfft_sR_f32_lenN, frame, 0, 1) TransformFunctions/arm_cfft_f32.c:562-616 = arm_radix8_butterfly_f32
//                                                     (arm_cfft_radix8_f32.c:45-285) + the base-8 digit reversal of arm_bitreversal_32
//     arm_cmplx_mag_squared_f32                        re * re, im * im, then the sum, each rounded
// and the row is either that power or row + alpha * (p - row), stored display-ordered (bin k at (k + N / 2) mod N).
//
// Every operation of the reference is kept, in its order, and the unit is compiled with -ffp-contract=off and IEEE denormals: bit-exact in
// every arith mode.  The transform, its lane layout and its LDS exchanges are fft8_passes (rx_fft8.h).
//
// One single-wave workgroup per channel; no two wavefronts touch one channel's state.  N = 512: lane j loads elements j + 64 m with eight
// 512-byte wave loads (256 bytes for int16 slots) straight into registers, where the window multiply runs.  N = 64: eight frames per wave
// (lane 8 f + j owns elements j + 8 m of frame slot f; the slots are consecutive TRANSFORMED frames, so a stride leaves no lane idle); their
// powers go through LDS to lane k = display index, which averages them in order.
// The row lives in registers across the frames of a call: read once (averaging only) and written once per call.  The pending frame is read
// only by a call that starts inside a transformed frame and written only by one that ends inside one; skipped frames are never read.
#include "rx_host.h"
#include "rx_fft8.h"       // spec_twiddles, fft8_twiddles, fft8_passes

#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace srx {

template <int N, typename TIn>
__global__ __launch_bounds__(64) void k_spectrum(SpecParams q, const TIn *__restrict__ src)
{
    constexpr uint32_t NF = N == 512 ? 1u : 8u;              // frames per trip of the wave
    __shared__ float2 fs[576];                               // 512 elements + the padding of either exchange (N = 64: 8 rows of 72 powers)

    const uint32_t lane = threadIdx.x, c = blockIdx.x, j2 = lane & 7u, g = lane >> 3;
    const TIn *x = src + (size_t)c * q.in_stride * 2;
    float *pend = q.pending + (size_t)c * N * 2;
    float *row = q.rows + (size_t)c * N;
    // the call's samples are v = 0 .. L - 1; the samples of its first frame that came with earlier calls are v = -off .. -1, in pending[0 .. off)
    const int64_t off = q.off, L = q.block_size;
    const uint32_t nfr = (uint32_t)((off + L) / N);          // frames this call completes: i = 0 .. nfr - 1, frame i starts at v = i * N - off
    // the transformed ones are i = first + t * stride, t < ne
    const uint32_t ne = nfr > q.first ? (nfr - 1u - q.first) / q.stride + 1u : 0u;
    auto elem = [&](int64_t v) -> float2 {
        if (v < 0) return reinterpret_cast<const float2 *>(pend)[v + off];
        return load_iq(x, v);
    };

    if (ne) {
        // lane's elements in the load layout, its window values and twiddles
        const uint32_t e0 = N == 512 ? lane : j2, es = N == 512 ? 64u : 8u;
        float w[8];
        float2 tw1[7], tw2[7];
#pragma unroll
        for (int m = 0; m < 8; ++m) w[m] = q.window ? q.window[e0 + es * m] : 1.0f;
        fft8_twiddles<N>(q.tw, lane, tw1, tw2);
        // display index of power m of this lane: N = 512: position 8 * lane + m = digits (g, j2, m) holds bin 64 m + 8 j2 + g;
        // N = 64: position 8 * j2 + m of the lane's frame holds bin 8 m + j2 (arm_bitreversal_32 with armBitRevIndexTableN: base-8 digit reversal)
        const uint32_t dlo = N == 512 ? 8u * j2 + g : j2, dst = N == 512 ? 64u : 8u;
        float r[8];
        float r64 = 0.0f;
        if (q.average) {
            if (N == 512) {
#pragma unroll
                for (int m = 0; m < 8; ++m) r[m] = row[dst * ((m + 4) & 7) + dlo];
            } else {
                r64 = row[lane];
            }
        }

        for (uint32_t t0 = q.average ? 0u : ne - 1u; t0 < ne; t0 += NF) {      // (no averaging: the row is the last transformed frame's power)
            const uint32_t t = t0 + (N == 512 ? 0u : g);
            const bool have = t < ne;
            const int64_t v0 = (int64_t)(q.first + (uint64_t)t * q.stride) * N - off;
            float2 a[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) a[m] = have ? elem(v0 + e0 + es * m) : make_float2(0.0f, 0.0f);
            if (q.window) {
#pragma unroll
                for (int m = 0; m < 8; ++m) a[m] = make_float2(a[m].x * w[m], a[m].y * w[m]);
            }
            fft8_passes<N>(a, tw1, tw2, fs, lane);

            float p[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const float re2 = a[m].x * a[m].x, im2 = a[m].y * a[m].y;
                p[m] = re2 + im2;
            }
            if (N == 512) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    if (q.average) {
                        const float d = p[m] - r[m], s = q.alpha * d;
                        r[m] = r[m] + s;
                    } else {
                        r[m] = p[m];
                    }
                }
            } else {
                float *ps = reinterpret_cast<float *>(fs);
                __syncthreads();
#pragma unroll
                for (int m = 0; m < 8; ++m) ps[72u * g + 8u * ((m + 4) & 7) + j2] = p[m];
                __syncthreads();
                for (uint32_t f = 0; f < 8u && t0 + f < ne; ++f) {
                    const float pk = ps[72u * f + lane];
                    if (q.average) {
                        const float d = pk - r64, s = q.alpha * d;
                        r64 = r64 + s;
                    } else {
                        r64 = pk;
                    }
                }
            }
        }
        if (N == 512) {
#pragma unroll
            for (int m = 0; m < 8; ++m) row[dst * ((m + 4) & 7) + dlo] = r[m];
        } else {
            row[lane] = r64;
        }
    }

    // the frame the call ends in, when it will be transformed: its samples so far wait in pending (those of earlier calls stay where they are)
    const int64_t vt = (int64_t)nfr * N - off;
    if (vt < L && nfr >= q.first && (nfr - q.first) % q.stride == 0u)
        for (int64_t v = (vt > 0 ? vt : 0) + lane; v < L; v += kWave) reinterpret_cast<float2 *>(pend)[v - vt] = load_iq(x, v);
}

hipError_t launch_spectrum(const SpecParams &q, uint32_t fft_len, const void *src, bool src_q15, hipStream_t st)
{
    if (q.channels == 0 || q.block_size == 0) return hipSuccess;
    if (q.stride == 0 || q.off >= fft_len) return hipErrorInvalidValue;
    const dim3 grid(q.channels), blk(kWave);
    if (fft_len == 512 && !src_q15) hipLaunchKernelGGL((k_spectrum<512, float>), grid, blk, 0, st, q, static_cast<const float *>(src));
    else if (fft_len == 512) hipLaunchKernelGGL((k_spectrum<512, int16_t>), grid, blk, 0, st, q, static_cast<const int16_t *>(src));
    else if (fft_len == 64 && !src_q15) hipLaunchKernelGGL((k_spectrum<64, float>), grid, blk, 0, st, q, static_cast<const float *>(src));
    else if (fft_len == 64) hipLaunchKernelGGL((k_spectrum<64, int16_t>), grid, blk, 0, st, q, static_cast<const int16_t *>(src));
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- host side of the stage ----
void SpecStage::release()
{
    dev_free(d_tw, d_window, d_rows, d_pending);
    len = 0; stride = 1; average = 0; alpha = 1.0f; pos = 0;
}

// the spectrum tap's state as set_spectrum leaves it: rows +0.0f, no pending samples, position 0
int SpecStage::init_state(selenite_rx_instance *S)
{
    if (!len) return SELENITE_RX_SUCCESS;
    const size_t n = (size_t)S->cfg.channels * len;
    HIPCHK(S, hipMemsetAsync(d_rows, 0, n * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(d_pending, 0, 2 * n * sizeof(float), S->stream));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    pos = 0;
    return SELENITE_RX_SUCCESS;
}

bool SpecStage::params(ChanRange r, uint64_t at, uint32_t block_size, SpecParams &q) const
{
    const uint32_t N = len;
    const uint64_t f0 = at / N;
    q = SpecParams{};
    q.off = (uint32_t)(at % N);
    q.first = (uint32_t)((stride - f0 % stride) % stride);
    if (((uint64_t)q.off + block_size - 1) / N < q.first) return false;      // the frames the call touches are all skipped ones
    q.channels = r.count;
    q.block_size = block_size; q.in_stride = block_size;
    q.stride = stride; q.average = average; q.alpha = alpha;
    q.tw = d_tw; q.window = d_window;
    q.rows = d_rows + (size_t)r.first * N; q.pending = d_pending + (size_t)r.first * N * 2;
    return true;
}

// Step 0b: in front of everything else.  A call that touches no transformed frame launches nothing.
int SpecStage::run(selenite_rx_instance *S, ChanRange r, uint64_t at, const void *src, bool src_q15, uint32_t block_size) const
{
    SpecParams q;
    if (!params(r, at, block_size, q)) return SELENITE_RX_SUCCESS;
    HIPCHK(S, hipSetDevice(S->device));
    HIPCHK(S, launch_spectrum(q, len, src, src_q15, S->stream));
    return SELENITE_RX_SUCCESS;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_spectrum(selenite_rx_instance *S, const selenite_rx_spec_config *sp)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_spectrum: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    if (sp) {
        const char *bad = nullptr;
        int code = SELENITE_RX_ARGUMENT_ERROR;
        if (sp->struct_size != sizeof(selenite_rx_spec_config)) bad = "struct_size is not sizeof(selenite_rx_spec_config)";
        else if (sp->fft_len != 64 && sp->fft_len != 512) { bad = "fft_len is not 64 or 512 (the pure radix-8 lengths of arm_cfft_f32)"; code = SELENITE_RX_LENGTH_ERROR; }
        else if (sp->stride < 1 || sp->stride > 65535) bad = "stride is not 1 .. 65535";
        else if (sp->average > 1) bad = "average is not 0 or 1";
        else if (!(sp->alpha > 0.0f && sp->alpha <= 1.0f)) bad = "alpha is not finite in (0, 1]";
        else if (sp->window)
            for (uint32_t k = 0; k < sp->fft_len && !bad; ++k)
                if (!std::isfinite(sp->window[k])) bad = "window holds a non-finite value";
        if (bad) return refuse("selenite_rx_set_spectrum", bad, code);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    SpecStage &st = S->spec;
    st.release();
    if (!sp) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels, N = sp->fft_len;
    std::vector<float> tw(2 * N);
    spec_twiddles(tw.data(), (uint32_t)N);
    hipError_t e = dev_upload(&st.d_tw, tw.data(), 2 * N);
    if (e == hipSuccess && sp->window) e = dev_upload(&st.d_window, sp->window, N);
    if (e == hipSuccess) e = dev_alloc(&st.d_rows, C * N);
    if (e == hipSuccess) e = dev_alloc(&st.d_pending, C * N * 2);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_spectrum: hipMalloc: ") + hipGetErrorString(e));
    }
    st.len = (uint32_t)N; st.stride = sp->stride; st.average = sp->average; st.alpha = sp->alpha;
    return st.init_state(S);
}

extern "C" int selenite_rx_get_spectrum(selenite_rx_instance *S, float *rows, uint64_t *frames)
{
    if (!S || !S->spec.len) return SELENITE_RX_ARGUMENT_ERROR;
    const SpecStage &st = S->spec;
    if (int rc = copy_rows(S, true, { { st.d_rows, rows, (size_t)S->cfg.channels * st.len * sizeof(float) } })) return rc;
    // frames transformed since set_spectrum / reset: the complete frames f < pos / N with f % stride == 0
    if (frames) *frames = (st.pos / st.len + st.stride - 1) / st.stride;
    return SELENITE_RX_SUCCESS;
}

extern "C" const float *selenite_rx_spectrum_device(const selenite_rx_instance *S) { return S ? S->spec.d_rows : nullptr; }

static int spec_state_copy(selenite_rx_instance *S, const selenite_rx_spec_state_view *v, bool to_host)
{
    if (!S || !v || !S->spec.len) return SELENITE_RX_ARGUMENT_ERROR;
    SpecStage &st = S->spec;
    const size_t n = (size_t)S->cfg.channels * st.len * sizeof(float);
    if (int rc = copy_rows(S, to_host, { { st.d_rows, v->rows, n }, { st.d_pending, v->pending, 2 * n } })) return rc;
    if (v->position) {
        if (to_host) *v->position = st.pos;
        else st.pos = *v->position;
    }
    return SELENITE_RX_SUCCESS;
}
extern "C" int selenite_rx_get_spectrum_state(selenite_rx_instance *S, const selenite_rx_spec_state_view *v) { return spec_state_copy(S, v, true); }
extern "C" int selenite_rx_set_spectrum_state(selenite_rx_instance *S, const selenite_rx_spec_state_view *v) { return spec_state_copy(S, v, false); }

extern "C" int selenite_rx_spectrum_twiddles(float *tw, uint32_t fft_len)
{
    if (!tw) return SELENITE_RX_ARGUMENT_ERROR;
    if (fft_len != 64 && fft_len != 512) return SELENITE_RX_LENGTH_ERROR;
    srx::spec_twiddles(tw, fft_len);
    return SELENITE_RX_SUCCESS;
}
