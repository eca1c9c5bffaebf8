// chan.hip -- polyphase channeliser (include/selenite_chan.h): per wideband stream ("band") a weighted-overlap-add
// analysis bank of K = 64 or 512 channels, decimated by D = K / oversample.  Output m of a call:
//     arm_dot_prod_f32 (BasicMathFunctions/arm_dot_prod_f32.c) per FFT position and rail over the P samples K apart: acc = +0.0f,
//                      acc = acc + g[r + t K] * s[r + t K], product rounded, then the sum;
//     arm_cfft_f32(&arm_cfft_sR_f32_lenK, v, 0, 1)  (TransformFunctions/arm_cfft_f32.c:562-616): fft8_passes (rx_fft8.h), one transform of
//                      512 or eight of 64 per wave.
// Compiled with -ffp-contract=off and IEEE denormals: bit-exact against the composition of the reference's functions.
//
// The sum over r lands at v[(r + n0) mod K], n0 = (position + (m + 1) D) mod K: FFT position p always holds the samples whose ABSOLUTE index
// is = p (mod K).  So a lane that owns positions p owns, for the whole run, the samples = p (mod K): P of them per position, a shift
// register in VGPRs that takes one new sample when the window moves over it.
//   oversample 1  every position takes one sample per output; the tap of position p is g[p + t K];
//   oversample 2  the window moves by K / 2: the positions below K / 2 take a sample on the outputs that end on an odd multiple of K / 2,
//                 the others on those that end on a multiple of K, and the tap row alternates between p and p ^ (K / 2).  The lane owns
//                 p = e0 + es * m, so "below K / 2" is m < 4 and p ^ (K / 2) is m ^ 4: both steps are straight-line code over fixed registers.
// Each wideband sample is fetched from HBM once per run, plus the K P - D overlap at the run's start, by the loads pass 1 of the transform
// wants (K = 512: eight 512-byte wave loads per output).
//
// Unit of work: one single-wave workgroup = one band (K = 512) or eight bands (K = 64: lane 8 f + j owns positions j + 8 m of band slot f, the
// load layout of fft8_passes<64>; slots past the last band idle) x a run of kPfbRun = 64 consecutive outputs, in tiles of kPfbT = 16 (pfb.h): the
// longer the run, the less the overlap at its start weighs (P 16, oversample 1: 15 K samples in front of 64 K).  A tile's K x 16 results are
// transposed through LDS (row stride 17 float2: conflict-free writes) and every store instruction covers four channel rows x 128 contiguous
// bytes; rows of bins nobody selected are never stored.  The taps sit in LDS, loaded once per workgroup.  The loads of a step are
// unconditional (they are always the call's own samples) and in flight together; those of the run's start choose between the history and
// the call sample by sample.
//
// State: the main kernel only READS the history (of the calls before); a small launch behind it forms the new history from the old tail
// and the call's samples into the OTHER of two buffers, which are swapped per call -- no workgroup reads what another one of the same
// launch writes, whatever the call length.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/selenite_chan.h"
#include "../../include/selenite_rx.h"
#include "pfb.h"
#include "rx_device.h"

struct selenite_chan : srx::PfbObject {};      // history [bands][K P - D][2]

namespace srx {
namespace {

struct ChanParams {
    uint32_t bands, n_bins, nout, block_size;
    uint32_t poff;                  // position mod K: 0, or K / 2 (oversample 2 behind an odd number of outputs)
    const float *taps;              // g[K P]
    const float *tw;                // [K][2] (rx_fft8.h: spec_twiddles)
    const float *hist;              // [bands][K P - D][2]: read only
    const uint32_t *bins;           // [n_bins] or NULL
    float *dst;                     // [bands n_bins][nout][2]
};

template <int K, int P, int OVS, typename TIn>
__global__ __launch_bounds__(64) void k_chan(ChanParams q, const TIn *__restrict__ src)
{
    constexpr int D = K / OVS, H = K * P - D;
    constexpr int NS = K == 512 ? 1 : 8;                     // band slots of the wave
    constexpr uint32_t HALF = OVS == 2 ? 4u : 0u;            // m ^ 4 = position ^ (K / 2)
    __shared__ float2 tile[NS * K * kPfbRow];
    __shared__ float2 fs[576];                               // the exchanges of fft8_passes
    __shared__ float gs[K * P];

    const uint32_t lane = threadIdx.x, j2 = lane & 7u, g = lane >> 3;
    const uint32_t b = K == 512 ? blockIdx.x : blockIdx.x * 8u + g;
    const bool have = b < q.bands;
    const uint32_t o0 = blockIdx.y * (uint32_t)kPfbRun;
    const uint32_t nR = q.nout - o0 < (uint32_t)kPfbRun ? q.nout - o0 : (uint32_t)kPfbRun;
    const uint32_t e0 = K == 512 ? lane : j2, es = K == 512 ? 64u : 8u;     // the lane owns positions e0 + es * m

    for (uint32_t i = lane; i < (uint32_t)(K * P); i += kWave) gs[i] = q.taps[i];
    float2 tw1[7], tw2[7];
#pragma unroll
    for (int k = 1; k < 8; ++k) {      // fft8_twiddles<K> (rx_fft8.h), kept inline: the call costs K = 512 an instruction (profiles/pfb_shared/README.md)
        if (K == 512) tw1[k - 1] = reinterpret_cast<const float2 *>(q.tw)[k * lane];
        tw2[k - 1] = reinterpret_cast<const float2 *>(q.tw)[(K / 64) * k * j2];
    }

    // the band's samples in the call's own index v: v >= 0 from the call, -H <= v < 0 from the history; what lies further back has left
    // every window of this run and is never multiplied
    const uint32_t bb = have ? b : 0u;                       // (an idle slot loads band 0's samples and drops them)
    const TIn *x = src + (int64_t)bb * q.block_size * 2;
    const float *hb = q.hist + (int64_t)bb * H * 2;
    const float2 zero = make_float2(0.0f, 0.0f);
    const int64_t last = (int64_t)q.block_size - 1;
    auto elem = [&](int64_t v) -> float2 {                   // anywhere at or behind the run's start
        if (!have || v < -(int64_t)H || v > last) return zero;
        if (v < 0) return reinterpret_cast<const float2 *>(hb)[v + H];
        return load_iq(x, v);
    };
    auto fresh = [&](int64_t v) -> float2 {                  // a sample the window moves over inside the run: always one of the call's own
        const float2 fx = load_iq(x, v);
        return have ? fx : zero;
    };

    // w = v + poff is the absolute index mod K.  In front of the run's first output the registers hold, per position, the P newest samples
    // below E0 = o0 D + poff, oldest first: w = E0 - K P + r0 + t K with r0 = (p - E0) mod K
    const int64_t E0 = (int64_t)o0 * D + q.poff;
    float2 h[8][P];
    {
        const uint32_t z0 = (OVS == 2 && (E0 % K) != 0) ? HALF : 0u;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int64_t v0 = E0 - (int64_t)K * P + (e0 + es * ((uint32_t)m ^ z0)) - q.poff;
#pragma unroll
            for (int t = 0; t < P; ++t) h[m][t] = elem(v0 + (int64_t)t * K);
        }
    }
    __syncthreads();                                         // (one wave: orders the LDS traffic across lanes for the compiler)

    // The D samples [E - D, E) an output takes in are loaded one output ahead: a single wave has nothing else to hide their latency behind
    // than its own arithmetic.  nx[j] is the sample at E - D + e0 + es j (in w).
    constexpr int NX = 8 / OVS;
    float2 nx[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) nx[j] = fresh(E0 + (e0 + es * (uint32_t)j) - q.poff);

    // one output that ends at E (exclusive, in w): PAR = 1 when E is an odd multiple of K / 2; `more`: another output of the run follows
    auto step = [&](auto par_c, uint32_t oi, int64_t E, bool more) __attribute__((always_inline)) {
        constexpr uint32_t PAR = decltype(par_c)::value;
        // the new samples go to the positions they are congruent to
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            if (OVS == 2 && ((m < 4) != (PAR == 1u))) continue;
#pragma unroll
            for (int t = 0; t + 1 < P; ++t) h[m][t] = h[m][t + 1];
            h[m][P - 1] = nx[OVS == 2 ? (m & 3) : m];
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < NX; ++j) nx[j] = fresh(E + (e0 + es * (uint32_t)j) - q.poff);
        }
        float2 a[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) a[m] = pfb_dot<K>(gs, e0 + es * ((uint32_t)m ^ (PAR ? HALF : 0u)), h[m]);
        fft8_passes<K>(a, tw1, tw2, fs, lane);
        // K = 512: position 8 * lane + m = digits (g, j2, m) holds bin 64 m + 8 j2 + g; K = 64: position 8 * j2 + m of slot g holds bin 8 m + j2
        // (arm_bitreversal_32: base-8 digit reversal)
        const uint32_t row0 = K == 512 ? 8u * j2 + g : 64u * g + j2, rs = K == 512 ? 64u : 8u;
#pragma unroll
        for (int m = 0; m < 8; ++m) tile[(row0 + rs * m) * kPfbRow + oi] = a[m];
    };

    const uint32_t c = lane & 15u;
#pragma unroll 1
    for (uint32_t t0 = 0; t0 < nR; t0 += (uint32_t)kPfbT) {
        const uint32_t nT = nR - t0 < (uint32_t)kPfbT ? nR - t0 : (uint32_t)kPfbT;
#pragma unroll 1
        for (uint32_t oi = 0; oi < nT; ++oi) {
            const int64_t E = E0 + (int64_t)(t0 + oi + 1u) * D;
            const bool more = t0 + oi + 1u < nR;
            if (OVS == 2 && (E % K) != 0) step(std::integral_constant<uint32_t, 1u>{}, oi, E, more);
            else step(std::integral_constant<uint32_t, 0u>{}, oi, E, more);
        }
        __syncthreads();
        // the tile's selected rows: lane 16 i + c stores output c of row i -- four rows x 128 contiguous bytes per instruction
        for (uint32_t s = 0; s < (uint32_t)NS; ++s) {
            const uint32_t bs = K == 512 ? blockIdx.x : blockIdx.x * 8u + s;
            if (bs >= q.bands) break;
            for (uint32_t i = lane >> 4; i < q.n_bins; i += 4u) {
                if (c >= nT) continue;
                const uint32_t bin = q.bins ? q.bins[i] : i;
                const int64_t at = ((int64_t)bs * q.n_bins + i) * q.nout + o0 + t0 + c;
                reinterpret_cast<float2 *>(q.dst)[at] = tile[(s * (uint32_t)K + bin) * kPfbRow + c];
            }
        }
        __syncthreads();
    }
}

// the history behind the call: the newest H samples of (old history, call), into the other buffer; blockIdx.y counts the bands from b0
template <typename TIn>
__global__ __launch_bounds__(256) void k_chan_hist(const TIn *__restrict__ src, const float *__restrict__ old, float *__restrict__ neu,
                                                   uint32_t H, uint32_t block_size, uint32_t b0)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, b = b0 + blockIdx.y;
    if (i >= H) return;
    const int64_t j = (int64_t)i + block_size;
    const float2 v = j < (int64_t)H ? reinterpret_cast<const float2 *>(old)[(int64_t)b * H + j]
                                    : load_iq(src + (int64_t)b * block_size * 2, j - H);
    reinterpret_cast<float2 *>(neu)[(int64_t)b * H + i] = v;
}

template <int K, int P, typename TIn>
void launch_kp(uint32_t ovs, dim3 grid, hipStream_t st, const ChanParams &q, const TIn *src)
{
    if (ovs == 1) hipLaunchKernelGGL((k_chan<K, P, 1, TIn>), grid, dim3(kWave), 0, st, q, src);
    else hipLaunchKernelGGL((k_chan<K, P, 2, TIn>), grid, dim3(kWave), 0, st, q, src);
}
template <int K, typename TIn>
void launch_k(uint32_t P, uint32_t ovs, dim3 grid, hipStream_t st, const ChanParams &q, const TIn *src)
{
    switch (P) {
    case 4: launch_kp<K, 4, TIn>(ovs, grid, st, q, src); break;
    case 8: launch_kp<K, 8, TIn>(ovs, grid, st, q, src); break;
    case 12: launch_kp<K, 12, TIn>(ovs, grid, st, q, src); break;
    default: launch_kp<K, 16, TIn>(ovs, grid, st, q, src); break;
    }
}

// 0 where the call would be refused
uint32_t out_len(const selenite_chan *Ch, uint32_t block_size)
{
    if (!Ch || block_size == 0 || block_size % Ch->D() != 0) return 0;
    const uint32_t nout = block_size / Ch->D();
    return (nout + kPfbRun - 1) / kPfbRun > 65535u ? 0 : nout;          // (the runs are the grid's y)
}

template <typename TIn>
int process(selenite_chan *Ch, const TIn *src, float *dst, uint32_t block_size, const char *who)
{
    if (!Ch) return SELENITE_RX_ARGUMENT_ERROR;
    if (!src || !dst) return fail(Ch, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": NULL buffer");
    const uint32_t nout = out_len(Ch, block_size);
    if (!nout)
        return fail(Ch, SELENITE_RX_LENGTH_ERROR, std::string(who) + ": blockSize is not a non-zero multiple of fft_len / oversample (or longer than 64 x 65535 outputs)");
    PFB_CHK(Ch, hipSetDevice(Ch->device));
    ChanParams q{};
    q.bands = Ch->bands; q.n_bins = Ch->n_bins; q.nout = nout; q.block_size = block_size;
    q.poff = (uint32_t)(Ch->position % Ch->K);
    q.taps = Ch->d_taps; q.tw = Ch->d_tw; q.hist = Ch->d_hist[Ch->cur]; q.bins = Ch->all_bins ? nullptr : Ch->d_bins; q.dst = dst;
    const uint32_t runs = (nout + kPfbRun - 1) / kPfbRun;
    if (Ch->K == 512) launch_k<512, TIn>(Ch->P, Ch->ovs, dim3(Ch->bands, runs), Ch->stream, q, src);
    else launch_k<64, TIn>(Ch->P, Ch->ovs, dim3((Ch->bands + 7u) / 8u, runs), Ch->stream, q, src);
    PFB_CHK(Ch, hipGetLastError());
    const uint32_t H = Ch->K * Ch->P - Ch->D();
    // gridDim.y is limited to 65535: loop over band slabs (as launch_synth does over channels)
    for (uint32_t b0 = 0; b0 < Ch->bands; b0 += 32768u) {
        const uint32_t n = Ch->bands - b0 < 32768u ? Ch->bands - b0 : 32768u;
        hipLaunchKernelGGL((k_chan_hist<TIn>), dim3((H + 255u) / 256u, n), dim3(256), 0, Ch->stream, src, Ch->d_hist[Ch->cur],
                           Ch->d_hist[1 - Ch->cur], H, block_size, b0);
    }
    PFB_CHK(Ch, hipGetLastError());
    Ch->cur = 1 - Ch->cur;
    Ch->position += block_size;
    return SELENITE_RX_SUCCESS;
}

}  // namespace
}  // namespace srx

using namespace srx;

extern "C" int selenite_chan_init(selenite_chan **out, const selenite_chan_config *cfg)
{
    if (!out) return SELENITE_RX_ARGUMENT_ERROR;
    *out = nullptr;
    // everything is validated before the device is touched
    if (!cfg || cfg->struct_size != sizeof(selenite_chan_config)) return SELENITE_RX_ARGUMENT_ERROR;
    if (int rc = pfb_validate(cfg, SELENITE_CHAN_MAX_BANDS, true)) return rc;
    const size_t H = (size_t)cfg->fft_len * cfg->taps_per_branch - cfg->fft_len / cfg->oversample;
    selenite_chan *Ch = new selenite_chan;
    if (int rc = pfb_create(Ch, cfg, (size_t)cfg->bands * H * 2 * sizeof(float))) {
        pfb_free(Ch);
        return rc;
    }
    *out = Ch;
    return SELENITE_RX_SUCCESS;
}

extern "C" void selenite_chan_free(selenite_chan *Ch) { pfb_free(Ch); }
extern "C" int selenite_chan_status(const selenite_chan *Ch) { return Ch ? Ch->status : SELENITE_RX_ARGUMENT_ERROR; }
extern "C" const char *selenite_chan_error_string(const selenite_chan *Ch) { return Ch ? Ch->err.c_str() : "null channeliser"; }
extern "C" int selenite_chan_set_stream(selenite_chan *Ch, void *hip_stream) { return pfb_set_stream(Ch, hip_stream); }
extern "C" int selenite_chan_sync(selenite_chan *Ch) { return pfb_sync(Ch); }
extern "C" int selenite_chan_reset(selenite_chan *Ch) { return Ch ? pfb_reset(Ch) : SELENITE_RX_ARGUMENT_ERROR; }
extern "C" int selenite_chan_get_state(selenite_chan *Ch, const selenite_chan_state_view *v)
{
    return pfb_state_copy(Ch, v, true, "selenite_chan_get_state");
}
extern "C" int selenite_chan_set_state(selenite_chan *Ch, const selenite_chan_state_view *v)
{
    return pfb_state_copy(Ch, v, false, "selenite_chan_set_state");
}

extern "C" uint32_t selenite_chan_out_channels(const selenite_chan *Ch) { return Ch ? Ch->bands * Ch->n_bins : 0; }
extern "C" uint32_t selenite_chan_out_len(const selenite_chan *Ch, uint32_t blockSize) { return out_len(Ch, blockSize); }

extern "C" void selenite_chan_process_f32_device(selenite_chan *Ch, const float *dSrc, float *dDst, uint32_t blockSize)
{
    process(Ch, dSrc, dDst, blockSize, "selenite_chan_process_f32_device");
}
extern "C" void selenite_chan_process_q15_device(selenite_chan *Ch, const int16_t *dSrc, float *dDst, uint32_t blockSize)
{
    process(Ch, dSrc, dDst, blockSize, "selenite_chan_process_q15_device");
}

extern "C" int selenite_chan_design_prototype(float *coeffs, uint32_t fft_len, uint32_t taps_per_branch, double width)
{
    if (!coeffs || !(width > 0.0 && width <= 2.0)) return SELENITE_RX_ARGUMENT_ERROR;
    if (fft_len != 64 && fft_len != 512) return SELENITE_RX_LENGTH_ERROR;
    if (taps_per_branch != 4 && taps_per_branch != 8 && taps_per_branch != 12 && taps_per_branch != 16) return SELENITE_RX_ARGUMENT_ERROR;
    return selenite_rx_design_lowpass(coeffs, fft_len * taps_per_branch, 0.5 * width / (double)fft_len);
}
