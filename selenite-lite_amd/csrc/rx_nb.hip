// rx_nb.hip -- impulse noise blanker (step 0c of DESIGN.md section 2, section 5.9): per channel, on the raw input I/Q of the call, behind the
// spectrum tap and in front of the NCO.  The call is cut into frames of F = 32, 64 or 128 complex samples (F divides the DSP block, so a
// frame never straddles two calls); per frame
//     p[n] = arm_cmplx_mag_squared_f32          ComplexMathFunctions/arm_cmplx_mag_squared_f32.c: re * re, im * im, then the sum, each rounded
//     m    = arm_mean_f32(p, F)                 StatisticsFunctions/arm_mean_f32.c:67-120: s = 0; s += p[n], n ascending; m = s / F
//     level > 0:  hit[n] = p[n] > threshold * level; 1 <= hits <= max_hits: the hits and `guard` samples either side of each (clipped at the
//                 frame's edges) become (+0, +0); hits > max_hits: a signal that came up, nothing blanked, bursts += 1;
//                 level += alpha * (min(m, clamp * level) - level)
//     otherwise:  nothing blanked, level = m
// and every sample that is not blanked is copied as the word(s) it is.  The level never depends on what was blanked, which is what makes the
// stage parallel in time: the frame means of a tile in parallel, a scan over them for the level in front of every frame, then the blanking
// in parallel.
//
// Every operation above is kept, in that order, and the unit is compiled with -ffp-contract=off and IEEE denormals: bit-exact in every
// arith mode.  (s / F is s * (1 / F) here: F is a power of two, so both are the one correctly rounded value of the same real number,
// denormal results included.)
//
// One single-wave workgroup per channel; no two wavefronts touch one channel's state.  A tile is 1024 samples = 16 wave loads of one sample
// per lane (512 bytes each; 256 for int16 slots), kept in registers until they are stored again:
//   load    sample i * 64 + lane; its power goes to LDS at frame * (F + 1) + n -- one word of padding per frame;
//   means   lane f sums the F powers of frame f in order: the lanes read F + 1 words apart, conflict-free on the 32 banks;
//   scan    the tile's frames in order, every lane computing the same level (the mean of frame f is a v_readlane); lane f keeps the level in
//           front of frame f;
//   blank   the threshold of a sample's frame comes from that lane; the hits of 64 samples are one wave ballot, a frame's mask is half of
//           one, one, or two of them; the count is a population count and the guard ORs of the mask shifted by 1 .. guard -- scalar work;
//   store   the word(s) of the sample, or zero: whole-wave stores.
// Calls longer than a tile loop over tiles; the level runs on from tile to tile in a register.
#include "rx_host.h"

#include <cmath>

namespace srx {

constexpr int kNbTile = 1024;                    // samples of a tile
constexpr int kNbIter = kNbTile / kWave;         // wave loads of a tile

// the words of one complex sample, moved as they are: f32 (re, im) | int16 (I in the low half)
template <typename T> struct NbWord;
template <> struct NbWord<float> { typedef uint2 type; };
template <> struct NbWord<int16_t> { typedef uint32_t type; };

// arm_cmplx_mag_squared_f32 (int16 slots: of the arm_q15_to_float values)
__device__ __forceinline__ float nb_power(uint2 w)
{
    const float re = __uint_as_float(w.x), im = __uint_as_float(w.y);
    const float re2 = re * re, im2 = im * im;
    return re2 + im2;
}
__device__ __forceinline__ float nb_power(uint32_t w)
{
    const float re = q15_to_float((int16_t)(w & 0xFFFFu)), im = q15_to_float((int16_t)(w >> 16));
    const float re2 = re * re, im2 = im * im;
    return re2 + im2;
}

// the level behind a frame of mean m: the AGC's form, every operation rounded
__device__ __forceinline__ float nb_level_step(float level, float m, float alpha, float clamp)
{
    if (!(level > 0.0f)) return m;               // not primed (zero, negative, NaN)
    const float c = clamp * level;
    const float mc = (m < c) ? m : c;
    const float d = mc - level;
    const float s = alpha * d;
    return level + s;
}

// One frame's decision on its hit mask (bit n = sample n; F = 32: bits 0 .. 31 of lo, F = 64: lo, F = 128: lo and hi): the mask of the blanked
// samples comes back in its place.  Wave-uniform: scalar registers.
template <int F>
__device__ __forceinline__ void nb_frame(uint64_t &lo, uint64_t &hi, uint32_t guard, uint32_t max_hits, uint64_t &blanked, uint64_t &bursts)
{
    const uint32_t k = (uint32_t)__popcll(lo) + (F == 128 ? (uint32_t)__popcll(hi) : 0u);
    if (k == 0u) return;
    if (k > max_hits) {                          // not impulse noise
        bursts += 1u;
        lo = 0u; hi = 0u;
        return;
    }
    uint64_t bl = lo, bh = hi;
    for (uint32_t d = 1; d <= guard; ++d) {      // (a shift drops what leaves the frame: the guard is clipped at its edges)
        bl |= (lo << d) | (lo >> d);
        if (F == 128) {
            bl |= hi << (64u - d);
            bh |= (hi << d) | (hi >> d) | (lo >> (64u - d));
        }
    }
    if (F == 32) bl &= 0xFFFFFFFFull;
    lo = bl; hi = bh;
    blanked += (uint32_t)__popcll(bl) + (F == 128 ? (uint32_t)__popcll(bh) : 0u);
}

template <int F, typename T>
__global__ __launch_bounds__(64) void k_nb(NbParams q, const T *__restrict__ src, T *__restrict__ dst)
{
    typedef typename NbWord<T>::type W;
    constexpr int NT = kNbTile / F;              // frames of a tile (<= 64: one per lane)
    constexpr int PS = F + 1;                    // words between the frames in LDS
    constexpr int U = F == 128 ? 2 : 1;          // wave loads of a blanking step: whole frames
    __shared__ float ps[NT * PS];

    const uint32_t lane = threadIdx.x, c = blockIdx.x, L = q.block_size;
    const W *x = reinterpret_cast<const W *>(src) + (size_t)c * L;
    W *y = reinterpret_cast<W *>(dst) + (size_t)c * L;
    float level = q.level[c];
    uint64_t blanked = 0u, bursts = 0u;

    for (uint32_t t0 = 0; t0 < L; t0 += kNbTile) {
        const uint32_t rem = L - t0 < (uint32_t)kNbTile ? L - t0 : (uint32_t)kNbTile;      // samples of this tile: whole frames
        const uint32_t nf = rem / F;
        W raw[kNbIter];
        __syncthreads();                         // (one wave: orders the LDS traffic across lanes for the compiler)
#pragma unroll
        for (int i = 0; i < kNbIter; ++i) {
            raw[i] = W{};
            const uint32_t s = i * kWave + lane;
            if ((uint32_t)(i * kWave) < rem && s < rem) {
                raw[i] = x[t0 + s];
                ps[(s / F) * PS + (s % F)] = nb_power(raw[i]);
            }
        }
        __syncthreads();

        // arm_mean_f32 of frame `lane`
        float m = 0.0f;
        if (lane < nf) {
            float s = 0.0f;
#pragma unroll 8
            for (int n = 0; n < F; ++n) s = s + ps[lane * PS + n];
            m = s * (1.0f / (float)F);
        }

        // the level in front of every frame of the tile
        float before = 0.0f;
#pragma unroll
        for (int f = 0; f < NT; ++f) {
            if ((uint32_t)f < nf) {
                const float mf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), f));
                if (lane == (uint32_t)f) before = level;
                level = nb_level_step(level, mf, q.alpha, q.clamp);
            }
        }
        // lane f: the threshold of frame f; a frame the level is not primed for has no hits
        const float thr_frame = before > 0.0f ? q.threshold * before : INFINITY;

#pragma unroll
        for (int u = 0; u < kNbIter / U; ++u) {
            if ((uint32_t)(u * U * kWave) < rem) {
                uint64_t hit[2] = { 0u, 0u };
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const int i = u * U + j;
                    const uint32_t s = i * kWave + lane;
                    const float thr = __shfl(thr_frame, (int)(s / F));
                    hit[j] = __ballot(s < rem && nb_power(raw[i]) > thr);
                }
                if constexpr (F == 32) {
                    uint64_t a = hit[0] & 0xFFFFFFFFull, b = hit[0] >> 32, none = 0u;
                    nb_frame<32>(a, none, q.guard, q.max_hits, blanked, bursts);
                    nb_frame<32>(b, none, q.guard, q.max_hits, blanked, bursts);
                    hit[0] = a | (b << 32);
                } else {
                    nb_frame<F>(hit[0], hit[1], q.guard, q.max_hits, blanked, bursts);
                }
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const int i = u * U + j;
                    const uint32_t s = i * kWave + lane;
                    if (s < rem) y[t0 + s] = ((hit[j] >> lane) & 1u) ? W{} : raw[i];
                }
            }
        }
    }
    if (lane == 0u) {
        q.level[c] = level;
        q.blanked[c] += blanked;
        q.bursts[c] += bursts;
    }
}

hipError_t launch_nb(const NbParams &q, uint32_t frame, const void *src, bool src_q15, void *dst, hipStream_t st)
{
    if (q.channels == 0 || q.block_size == 0) return hipSuccess;
    if (q.block_size % frame != 0) return hipErrorInvalidValue;
    const dim3 grid(q.channels), blk(kWave);
#define SRX_NB_LAUNCH(F)                                                                                                             \
    do {                                                                                                                             \
        if (src_q15) hipLaunchKernelGGL((k_nb<F, int16_t>), grid, blk, 0, st, q, static_cast<const int16_t *>(src), static_cast<int16_t *>(dst)); \
        else hipLaunchKernelGGL((k_nb<F, float>), grid, blk, 0, st, q, static_cast<const float *>(src), static_cast<float *>(dst));  \
    } while (0)
    if (frame == 32) SRX_NB_LAUNCH(32);
    else if (frame == 64) SRX_NB_LAUNCH(64);
    else if (frame == 128) SRX_NB_LAUNCH(128);
    else return hipErrorInvalidValue;
#undef SRX_NB_LAUNCH
    return hipGetLastError();
}

// ---- host side of the stage ----
void NbStage::release()
{
    dev_free(d_level, d_blanked, d_bursts, d_buf);
    buf_bytes = 0;
    frame = 0; guard = 0; max_hits = 0; threshold = 0.0f; alpha = 0.0f; clamp = 0.0f;
}

// the blanker's state as set_nb leaves it: level +0.0f (not primed), both counters 0
int NbStage::init_state(selenite_rx_instance *S)
{
    if (!frame) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels;
    const float unprimed = 0.0f;
    HIPCHK(S, hipMemsetAsync(d_blanked, 0, C * sizeof(uint64_t), S->stream));
    HIPCHK(S, hipMemsetAsync(d_bursts, 0, C * sizeof(uint64_t), S->stream));
    return fill_rows(S, d_level, C, &unprimed);             // (drains the stream)
}

// Step 0c: one launch on the instance's stream writes the blanked copy of the call's input, in the caller's format and with the caller's
// stride (block_size samples per channel), to the instance's buffer -- grown by the first call that needs it -- and the chain reads that.
// (The chunks of a host-pointer call run their kernels on this one stream, one behind the other: one buffer serves them all.)
int NbStage::run(selenite_rx_instance *S, ChanRange r, const void *src, bool src_q15, uint32_t block_size, const void **blanked_src)
{
    HIPCHK(S, hipSetDevice(S->device));
    const size_t need = (size_t)r.count * block_size * 2 * (src_q15 ? sizeof(int16_t) : sizeof(float));
    if (int rc = ensure(S, &d_buf, &buf_bytes, need)) return rc;
    NbParams q{};
    q.channels = r.count; q.block_size = block_size;
    q.guard = guard; q.max_hits = max_hits;
    q.threshold = threshold; q.alpha = alpha; q.clamp = clamp;
    q.level = d_level + r.first; q.blanked = d_blanked + r.first; q.bursts = d_bursts + r.first;
    HIPCHK(S, launch_nb(q, frame, src, src_q15, d_buf, S->stream));
    *blanked_src = d_buf;
    return SELENITE_RX_SUCCESS;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_nb(selenite_rx_instance *S, const selenite_rx_nb_config *nb)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_nb: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    if (nb) {
        const char *bad = nullptr;
        int code = SELENITE_RX_ARGUMENT_ERROR;
        if (nb->struct_size != sizeof(selenite_rx_nb_config)) bad = "struct_size is not sizeof(selenite_rx_nb_config)";
        else if (nb->frame != 32 && nb->frame != 64 && nb->frame != 128) { bad = "frame is not 32, 64 or 128"; code = SELENITE_RX_LENGTH_ERROR; }
        else if (S->cfg.block % nb->frame != 0) { bad = "frame does not divide cfg.block"; code = SELENITE_RX_LENGTH_ERROR; }
        else if (nb->guard > 8) bad = "guard is not 0 .. 8";
        else if (nb->max_hits < 1 || nb->max_hits > nb->frame / 4) bad = "max_hits is not 1 .. frame / 4";
        else if (!(std::isfinite(nb->threshold) && nb->threshold >= 1.0f)) bad = "threshold is not finite and >= 1";
        else if (!(nb->alpha > 0.0f && nb->alpha <= 1.0f)) bad = "alpha is not in (0, 1]";
        else if (!(std::isfinite(nb->clamp) && nb->clamp >= 1.0f)) bad = "clamp is not finite and >= 1";
        if (bad) return refuse("selenite_rx_set_nb", bad, code);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    NbStage &st = S->nb;
    st.release();
    if (!nb) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels;
    hipError_t e = dev_alloc(&st.d_level, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_blanked, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_bursts, C);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_nb: hipMalloc: ") + hipGetErrorString(e));
    }
    st.frame = nb->frame; st.guard = nb->guard; st.max_hits = nb->max_hits;
    st.threshold = nb->threshold; st.alpha = nb->alpha; st.clamp = nb->clamp;
    return st.init_state(S);
}

static int nb_state_copy(selenite_rx_instance *S, const selenite_rx_nb_state_view *v, bool to_host)
{
    if (!S || !v || !S->nb.frame) return SELENITE_RX_ARGUMENT_ERROR;
    const NbStage &st = S->nb;
    const size_t C = S->cfg.channels;
    return copy_rows(S, to_host, { { st.d_level, v->level, C * sizeof(float) }, { st.d_blanked, v->blanked, C * sizeof(uint64_t) },
                                   { st.d_bursts, v->bursts, C * sizeof(uint64_t) } });
}
extern "C" int selenite_rx_get_nb_state(selenite_rx_instance *S, const selenite_rx_nb_state_view *v) { return nb_state_copy(S, v, true); }
extern "C" int selenite_rx_set_nb_state(selenite_rx_instance *S, const selenite_rx_nb_state_view *v) { return nb_state_copy(S, v, false); }
