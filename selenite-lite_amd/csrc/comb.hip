// comb.hip -- polyphase combiner (include/selenite_comb.h): per wideband stream ("band") a weighted-overlap-add
// synthesis bank of K = 64 or 512 channels, interpolated by D = K / oversample: the channeliser (chan.hip) run backwards.  Per input frame f:
//     arm_cfft_f32(&arm_cfft_sR_f32_lenK, v, 1, 1)  (TransformFunctions/arm_cfft_f32.c:562-616): imag negated, the passes of fft8_passes
//                      (rx_fft8.h, which explains the layout; this kernel holds them inline), re * invL and (-im) * invL -> u_f[0 .. K - 1];
//     arm_dot_prod_f32 (BasicMathFunctions/arm_dot_prod_f32.c) per output sample and rail over the Q = P * oversample frames that overlap in
//                      it: out[f D + j] = sum_t g[(D - 1 - j) + t D] * u_{f - Q + 1 + t}[p], p = (f D + j) mod K, acc = +0.0f, product rounded,
//                      then the sum, t ascending.
// Compiled with -ffp-contract=off and IEEE denormals: bit-exact against the composition of the reference's functions.
//
// Behind the passes a lane holds eight time-domain positions p = pb + es * m (the digit-reversed layout fft8_passes returns: es = 64 or
// 8).  It keeps, per owned position, the Q newest u[p] as a shift register in VGPRs (8 Q float2: 256 VGPRs at Q = 16, which is why Q <= 16);
// every register shifts on every frame.
//   oversample 1  a frame emits all K positions, j = p;
//   oversample 2  a frame emits the lower (m < 4) or the upper (m >= 4) half of the positions in turn -- the parity is that of
//                 position / D + frame -- with j = p mod D = pb + es * (m & 3): two straight-line forms chosen by a uniform branch.
//
// Unit of work: one single-wave workgroup = one band (K = 512) or eight bands (K = 64: lane 8 s + j2 works for band slot s; slots past the last
// band idle) x a run of kPfbRun = 64 consecutive frames (the grid's y), in tiles of kPfbT = 16 (pfb.h).  The rows of one frame lie nin * 8 bytes
// apart, so a tile is loaded row-wise -- 16 frames = 128 contiguous bytes per row, four rows per wave instruction, kCombLoads = 8 such loads
// in flight before the first is written (a single wave has nothing else to hide their latency behind) -- into an LDS
// tile [K][17] float2; the rows of bins nobody feeds are zeroed once and never written.  The Q - 1 frames in
// front of a run are loaded and transformed the same way, from the history (the call's first run) or from the call (every other run: a run
// is longer than Q - 1), and emit nothing: (Q - 1) / 64 extra transforms.  A frame's D results go through LDS and leave as contiguous
// stores (K = 512: 512 bytes per wave instruction; K = 64: 256 bytes per band slot, 128 as int16); the int16 instantiation converts in
// registers (arm_float_to_q15).  The taps sit in LDS, loaded once per workgroup.
//
// State: the main kernel only READS the history (of the calls before); a small launch behind it forms the new history -- the last Q - 1
// input samples of every row -- from the old one and the call into the OTHER of two buffers, which are swapped per call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/selenite_chan.h"
#include "../../include/selenite_comb.h"
#include "../../include/selenite_rx.h"
#include "pfb.h"
#include "rx_device.h"

struct selenite_comb : srx::PfbObject {          // history [bands n_bins][Q - 1][2]
    uint32_t round = 0;
    uint32_t Q() const { return P * ovs; }
    size_t rows() const { return (size_t)bands * n_bins; }
};

namespace srx {
namespace {

constexpr int kCombLoads = 8;       // wave loads of the input tile in flight together

struct CombParams {
    uint32_t bands, n_bins, nin;
    uint32_t par0;                  // (position / D) & 1: the half the call's first frame emits with oversample 2
    uint32_t round;                 // int16 output: arm_float_to_q15's ARM_MATH_ROUNDING build
    const float *taps;              // g[K P]
    const float *tw;                // [K][2] (rx_fft8.h: spec_twiddles)
    const float *hist;              // [bands n_bins][Q - 1][2]: read only
    const uint32_t *bins;           // [n_bins] or NULL
    const float *src;               // [bands n_bins][nin][2]
};

template <typename TOut> struct CombOut;
template <> struct CombOut<float> {
    typedef float2 pair;
    static __device__ __forceinline__ pair make(float i, float q, uint32_t) { return make_float2(i, q); }
};
template <> struct CombOut<int16_t> {
    typedef short2 pair;
    static __device__ __forceinline__ pair make(float i, float q, uint32_t round)
    {
        return make_short2(float_to_q15(i, round), float_to_q15(q, round));     // arm_float_to_q15
    }
};

template <int K, int Q, int OVS, typename TOut>
__global__ __launch_bounds__(64) void k_comb(CombParams q, TOut *__restrict__ dst)
{
    constexpr int D = K / OVS;
    constexpr int NS = K == 512 ? 1 : 8;                     // band slots of the wave
    constexpr int SD = D + 8;                                // a slot's stride in the output exchange
    constexpr float invL = 1.0f / (float)K;                  // arm_cfft_f32.c:606
    typedef typename CombOut<TOut>::pair Pair;
    __shared__ float2 tile[NS * K * kPfbRow];
    __shared__ float2 fs[576];                               // the exchanges of fft8_passes
    __shared__ float gs[D * Q];                              // K P taps
    __shared__ Pair os[NS * SD];                             // a frame's results, in output order
    __shared__ uint32_t binl[K];                             // the bin of input row i

    const uint32_t lane = threadIdx.x, j2 = lane & 7u, g = lane >> 3;
    const uint32_t o0 = blockIdx.y * (uint32_t)kPfbRun;
    const uint32_t nR = q.nin - o0 < (uint32_t)kPfbRun ? q.nin - o0 : (uint32_t)kPfbRun;
    const uint32_t es = K == 512 ? 64u : 8u;
    const uint32_t e0 = K == 512 ? lane : 64u * g + j2;      // pass 1 reads the tile rows e0 + es * m (K = 64: bins j2 + 8 m of slot g)
    // behind the passes a[m] is time-domain position pb + es * m (arm_bitreversal_32: base-8 digit reversal; K = 512: position 8 * lane + m =
    // digits (g, j2, m) holds index 64 m + 8 j2 + g; K = 64: position 8 * j2 + m of slot g holds index 8 m + j2)
    const uint32_t pb = K == 512 ? 8u * j2 + g : j2;
    const uint32_t slot = K == 512 ? 0u : g;

    const float2 zero = make_float2(0.0f, 0.0f);
    for (uint32_t i = lane; i < (uint32_t)(D * Q); i += kWave) gs[i] = q.taps[i];
    for (uint32_t i = lane; i < q.n_bins; i += kWave) binl[i] = q.bins ? q.bins[i] : i;
    for (uint32_t i = lane; i < (uint32_t)(NS * K * kPfbRow); i += kWave) tile[i] = zero;      // rows of unfed bins and idle slots stay +0.0f
    float2 tw1[7], tw2[7];
    // The twiddle gather, the passes and the tap sum below are fft8_twiddles / fft8_passes (rx_fft8.h) and pfb_dot (pfb.h) kept inline: with the
    // calls this kernel's register allocation and schedule move and some instantiations get slower (profiles/pfb_shared/README.md)
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        if (K == 512) tw1[k - 1] = reinterpret_cast<const float2 *>(q.tw)[k * lane];
        tw2[k - 1] = reinterpret_cast<const float2 *>(q.tw)[(K / 64) * k * j2];
    }

    // h[m][t]: u_{f - Q + 1 + t}[pb + es * m] behind frame f.  Frames in front of the stream are the transforms of the history's +0.0f rows:
    // zeros of either sign, whose products with the finite taps are zeros, and acc = +0.0f plus a zero of either sign is +0.0f
    float2 h[8][Q];
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int t = 0; t < Q; ++t) h[m][t] = zero;
    __syncthreads();                                         // (one wave: orders the LDS traffic across lanes for the compiler)

    // one frame, column ci of the tile: the inverse transform, then every shift register takes its position's new value
    auto xform = [&](uint32_t ci) __attribute__((always_inline)) {
        float2 a[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const float2 v = tile[(e0 + es * (uint32_t)m) * kPfbRow + ci];
            a[m] = make_float2(v.x, -v.y);                   // arm_cfft_f32.c:571-580
        }
        if (K == 512) {                                      // fft8_passes<K>, inline (see above)
            bfly8(a);
            if (lane != 0u) twiddle7(a, tw1);
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 8; ++m) fs[lane + 72u * m] = a[m];
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 8; ++m) a[m] = fs[72u * g + j2 + 8u * m];
        }
        bfly8(a);
        if (j2 != 0u) twiddle7(a, tw2);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 8; ++m) fs[72u * g + j2 + 9u * m] = a[m];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 8; ++m) a[m] = fs[9u * lane + m];
        bfly8(a);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
#pragma unroll
            for (int t = 0; t + 1 < Q; ++t) h[m][t] = h[m][t + 1];
            const float ni = -a[m].y;
            h[m][Q - 1] = make_float2(a[m].x * invL, ni * invL);      // arm_cfft_f32.c:610-611
        }
    };

    // the D output samples of call frame fr: PAR = 1 emits the upper half of the positions (oversample 2)
    auto emit = [&](auto par_c, uint32_t fr) __attribute__((always_inline)) {
        constexpr uint32_t PAR = decltype(par_c)::value;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            if (OVS == 2 && ((m >= 4) != (PAR == 1u))) continue;
            const uint32_t jj = pb + es * (uint32_t)(OVS == 2 ? (m & 3) : m);      // j = p mod D
            const uint32_t r = (uint32_t)(D - 1) - jj;
            float ai = 0.0f, aq = 0.0f;                      // pfb_dot<D>, inline (see above)
#pragma unroll
            for (int t = 0; t < Q; ++t) {
                const float c = gs[r + (uint32_t)(t * D)];
                const float pi = c * h[m][t].x, pq = c * h[m][t].y;
                ai = ai + pi;
                aq = aq + pq;
            }
            os[slot * (uint32_t)SD + jj] = CombOut<TOut>::make(ai, aq, q.round);
        }
        __syncthreads();
        for (uint32_t idx = lane; idx < (uint32_t)(NS * D); idx += kWave) {
            const uint32_t s = idx / (uint32_t)D, j = idx % (uint32_t)D;
            const uint32_t bs = K == 512 ? blockIdx.x : blockIdx.x * 8u + s;
            if (bs < q.bands) reinterpret_cast<Pair *>(dst)[((int64_t)bs * q.nin + fr) * D + j] = os[s * (uint32_t)SD + j];
        }
        __syncthreads();
    };

    const uint32_t c = lane & 15u;
    // tile -1 is the run's start: the Q - 1 frames in front of it, which emit nothing
#pragma unroll 1
    for (int32_t t0 = -kPfbT; t0 < (int32_t)nR; t0 += kPfbT) {
        const bool pro = t0 < 0;
        const uint32_t nT = pro ? (uint32_t)(Q - 1) : (nR - (uint32_t)t0 < (uint32_t)kPfbT ? nR - (uint32_t)t0 : (uint32_t)kPfbT);
        const bool from_hist = pro && o0 == 0u;
        const float2 *base = reinterpret_cast<const float2 *>(from_hist ? q.hist : q.src);
        const int64_t stride = from_hist ? (int64_t)(Q - 1) : (int64_t)q.nin;
        const int64_t off = from_hist ? 0 : (pro ? (int64_t)o0 - (Q - 1) : (int64_t)o0 + t0);      // (o0 >= 64 > Q - 1 behind the first run)
        // lane 16 i + c loads frame c of row i: four rows x 128 contiguous bytes per instruction
        for (uint32_t s = 0; s < (uint32_t)NS; ++s) {
            const uint32_t bs = K == 512 ? blockIdx.x : blockIdx.x * 8u + s;
            if (bs >= q.bands) break;
            // kCombLoads wave loads in flight before the first of them is waited for and written to the tile
            for (uint32_t i0 = lane >> 4; i0 < q.n_bins; i0 += 4u * (uint32_t)kCombLoads) {
                float2 v[kCombLoads];
#pragma unroll
                for (int u = 0; u < kCombLoads; ++u) {
                    const uint32_t i = i0 + 4u * (uint32_t)u;
                    if (i < q.n_bins && c < nT) v[u] = base[((int64_t)bs * q.n_bins + i) * stride + off + c];
                }
#pragma unroll
                for (int u = 0; u < kCombLoads; ++u) {
                    const uint32_t i = i0 + 4u * (uint32_t)u;
                    if (i < q.n_bins && c < nT) tile[(s * (uint32_t)K + binl[i]) * kPfbRow + c] = v[u];
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t ci = 0; ci < nT; ++ci) {
            xform(ci);
            if (pro) continue;
            const uint32_t fr = o0 + (uint32_t)t0 + ci;
            if (OVS == 2 && ((q.par0 + fr) & 1u)) emit(std::integral_constant<uint32_t, 1u>{}, fr);
            else emit(std::integral_constant<uint32_t, 0u>{}, fr);
        }
        __syncthreads();
    }
}

// the history behind the call: per row the newest Q - 1 samples of (old history, call), into the other buffer.  A grid-stride loop over the
// bands n_bins (Q - 1) samples: the grid is at most kCombHistBlocks workgroups, whatever the number of rows
constexpr uint32_t kCombHistBlocks = 2048;
__global__ __launch_bounds__(256) void k_comb_hist(const float *__restrict__ src, const float *__restrict__ old, float *__restrict__ neu,
                                                   uint32_t Q1, uint32_t nin, uint64_t total)
{
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < total; e += step) {
        const uint64_t row = e / Q1, j = e % Q1 + nin;
        const float2 v = j < Q1 ? reinterpret_cast<const float2 *>(old)[row * Q1 + j]
                                : reinterpret_cast<const float2 *>(src)[row * nin + (j - Q1)];
        reinterpret_cast<float2 *>(neu)[e] = v;
    }
}

template <int K, typename TOut>
void launch_k(uint32_t Q, uint32_t ovs, dim3 grid, hipStream_t st, const CombParams &q, TOut *dst)
{
    if (ovs == 1) {
        switch (Q) {
        case 4: hipLaunchKernelGGL((k_comb<K, 4, 1, TOut>), grid, dim3(kWave), 0, st, q, dst); break;
        case 8: hipLaunchKernelGGL((k_comb<K, 8, 1, TOut>), grid, dim3(kWave), 0, st, q, dst); break;
        case 12: hipLaunchKernelGGL((k_comb<K, 12, 1, TOut>), grid, dim3(kWave), 0, st, q, dst); break;
        default: hipLaunchKernelGGL((k_comb<K, 16, 1, TOut>), grid, dim3(kWave), 0, st, q, dst); break;
        }
    } else if (Q == 8) {
        hipLaunchKernelGGL((k_comb<K, 8, 2, TOut>), grid, dim3(kWave), 0, st, q, dst);
    } else {
        hipLaunchKernelGGL((k_comb<K, 16, 2, TOut>), grid, dim3(kWave), 0, st, q, dst);
    }
}

// 0 where the call would be refused
uint32_t out_len(const selenite_comb *Cb, uint32_t block_size)
{
    if (!Cb || block_size == 0) return 0;
    if (block_size > (uint32_t)kPfbRun * 65535u) return 0;                               // (the runs are the grid's y)
    const uint64_t n = (uint64_t)block_size * Cb->D();
    return n > 0xFFFFFFFFull ? 0 : (uint32_t)n;
}

template <typename TOut>
int process(selenite_comb *Cb, const float *src, TOut *dst, uint32_t block_size, const char *who)
{
    if (!Cb) return SELENITE_RX_ARGUMENT_ERROR;
    if (!src || !dst) return fail(Cb, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": NULL buffer");
    if (!out_len(Cb, block_size))
        return fail(Cb, SELENITE_RX_LENGTH_ERROR, std::string(who) + ": blockSize is zero or longer than 64 x 65535 frames");
    PFB_CHK(Cb, hipSetDevice(Cb->device));
    CombParams q{};
    q.bands = Cb->bands; q.n_bins = Cb->n_bins; q.nin = block_size;
    q.par0 = (uint32_t)((Cb->position / Cb->D()) & 1u); q.round = Cb->round;
    q.taps = Cb->d_taps; q.tw = Cb->d_tw; q.hist = Cb->d_hist[Cb->cur]; q.bins = Cb->all_bins ? nullptr : Cb->d_bins; q.src = src;
    const uint32_t runs = (block_size + kPfbRun - 1) / kPfbRun;
    if (Cb->K == 512) launch_k<512, TOut>(Cb->Q(), Cb->ovs, dim3(Cb->bands, runs), Cb->stream, q, dst);
    else launch_k<64, TOut>(Cb->Q(), Cb->ovs, dim3((Cb->bands + 7u) / 8u, runs), Cb->stream, q, dst);
    PFB_CHK(Cb, hipGetLastError());
    // (bands n_bins < 2^32 rows of Q - 1 <= 15 samples: the count needs 64 bits, and one thread each would not be a legal grid)
    const uint32_t Q1 = Cb->Q() - 1;
    const uint64_t total = (uint64_t)Cb->rows() * Q1;
    const uint64_t blocks = (total + 255u) / 256u;
    hipLaunchKernelGGL(k_comb_hist, dim3(blocks < kCombHistBlocks ? (uint32_t)blocks : kCombHistBlocks), dim3(256), 0, Cb->stream, src,
                       Cb->d_hist[Cb->cur], Cb->d_hist[1 - Cb->cur], Q1, block_size, total);
    PFB_CHK(Cb, hipGetLastError());
    Cb->cur = 1 - Cb->cur;
    Cb->position += (uint64_t)block_size * Cb->D();
    return SELENITE_RX_SUCCESS;
}

bool shape_ok(uint32_t P, uint32_t ovs)
{
    return (ovs == 1 || ovs == 2) && (P == 4 || P == 8 || P == 12 || P == 16) && P * ovs <= 16;      // Q <= 16: the shift registers are VGPRs
}

}  // namespace
}  // namespace srx

using namespace srx;

extern "C" int selenite_comb_init(selenite_comb **out, const selenite_comb_config *cfg)
{
    if (!out) return SELENITE_RX_ARGUMENT_ERROR;
    *out = nullptr;
    // everything is validated before the device is touched
    if (!cfg || cfg->struct_size != sizeof(selenite_comb_config)) return SELENITE_RX_ARGUMENT_ERROR;
    const bool own_ok = shape_ok(cfg->taps_per_branch, cfg->oversample) && cfg->n_bins <= cfg->fft_len && cfg->q15_rounding <= 1u;
    if (int rc = pfb_validate(cfg, SELENITE_COMB_MAX_BANDS, own_ok)) return rc;
    if (cfg->bins) {
        std::vector<bool> fed(cfg->fft_len, false);
        for (uint32_t i = 0; i < cfg->n_bins; ++i) {
            if (fed[cfg->bins[i]]) return SELENITE_RX_ARGUMENT_ERROR;      // two rows on one bin have no defined sum
            fed[cfg->bins[i]] = true;
        }
    }
    const size_t Q1 = cfg->taps_per_branch * cfg->oversample - 1;
    selenite_comb *Cb = new selenite_comb;
    Cb->round = cfg->q15_rounding;
    if (int rc = pfb_create(Cb, cfg, (size_t)cfg->bands * cfg->n_bins * Q1 * 2 * sizeof(float))) {
        pfb_free(Cb);
        return rc;
    }
    *out = Cb;
    return SELENITE_RX_SUCCESS;
}

extern "C" void selenite_comb_free(selenite_comb *Cb) { pfb_free(Cb); }
extern "C" int selenite_comb_status(const selenite_comb *Cb) { return Cb ? Cb->status : SELENITE_RX_ARGUMENT_ERROR; }
extern "C" const char *selenite_comb_error_string(const selenite_comb *Cb) { return Cb ? Cb->err.c_str() : "null combiner"; }
extern "C" int selenite_comb_set_stream(selenite_comb *Cb, void *hip_stream) { return pfb_set_stream(Cb, hip_stream); }
extern "C" int selenite_comb_sync(selenite_comb *Cb) { return pfb_sync(Cb); }
extern "C" int selenite_comb_reset(selenite_comb *Cb) { return Cb ? pfb_reset(Cb) : SELENITE_RX_ARGUMENT_ERROR; }
extern "C" int selenite_comb_get_state(selenite_comb *Cb, const selenite_comb_state_view *v)
{
    return pfb_state_copy(Cb, v, true, "selenite_comb_get_state");
}
extern "C" int selenite_comb_set_state(selenite_comb *Cb, const selenite_comb_state_view *v)
{
    return pfb_state_copy(Cb, v, false, "selenite_comb_set_state");
}

extern "C" uint32_t selenite_comb_in_channels(const selenite_comb *Cb) { return Cb ? Cb->bands * Cb->n_bins : 0; }
extern "C" uint32_t selenite_comb_out_len(const selenite_comb *Cb, uint32_t blockSize) { return out_len(Cb, blockSize); }

extern "C" void selenite_comb_process_f32_device(selenite_comb *Cb, const float *dSrc, float *dDst, uint32_t blockSize)
{
    process(Cb, dSrc, dDst, blockSize, "selenite_comb_process_f32_device");
}
extern "C" void selenite_comb_process_q15_device(selenite_comb *Cb, const float *dSrc, int16_t *dDst, uint32_t blockSize)
{
    process(Cb, dSrc, dDst, blockSize, "selenite_comb_process_q15_device");
}

extern "C" int selenite_comb_design_prototype(float *coeffs, uint32_t fft_len, uint32_t taps_per_branch, double width, uint32_t oversample)
{
    if (!coeffs || !(width > 0.0 && width <= 2.0)) return SELENITE_RX_ARGUMENT_ERROR;
    if (fft_len != 64 && fft_len != 512) return SELENITE_RX_LENGTH_ERROR;
    if (!shape_ok(taps_per_branch, oversample)) return SELENITE_RX_ARGUMENT_ERROR;
    const int rc = selenite_chan_design_prototype(coeffs, fft_len, taps_per_branch, width);
    if (rc) return rc;
    // arm_cfft_f32's inverse divides by K and each output sample sums one tap in D: K * D restores unity gain from a channel to the stream
    const double scale = (double)fft_len * (double)(fft_len / oversample);
    for (uint32_t i = 0; i < fft_len * taps_per_branch; ++i) coeffs[i] = (float)((double)coeffs[i] * scale);
    return SELENITE_RX_SUCCESS;
}
