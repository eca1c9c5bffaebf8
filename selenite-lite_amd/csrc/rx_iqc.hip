// rx_iqc.hip -- I/Q correction (step 0b2 of DESIGN.md section 2, section 5.10): per channel, on the raw input I/Q of the call, behind the
// spectrum tap and in front of the noise blanker.  The call is cut into frames of F = 32, 64 or 128 complex samples (F divides the DSP
// block, so a frame never straddles two calls), I[n] = x[2n], Q[n] = x[2n + 1]; per frame, with the coefficients in front of it,
//     i[n] = I[n] - dc_i, q[n] = Q[n] - dc_q        arm_offset_f32 with the negated offset (BasicMathFunctions/arm_offset_f32.c:145)
//     Iout[n] = i[n], Qout[n] = (q[n] - i[n] * p) * g      arm_scale_f32, arm_sub_f32, arm_scale_f32: three roundings
// and behind it
//     dc_alpha > 0:  m = arm_mean_f32(rail, F) (StatisticsFunctions/arm_mean_f32.c:67-120); finite: dc += dc_alpha * (m - dc), per rail
//     alpha > 0:     pii = arm_power_f32(i), pqq = arm_power_f32(q), piq = arm_dot_prod_f32(i, q): sum = sum + a * b, n ascending
//                    a = piq / pii; r = pqq - a * piq; b = sqrtf(pii / r)
//                    valid (pii, r in (min_power, FLT_MAX]):  p += alpha * (clamp(a, +-p_max) - p); g += alpha * (clamp(b, g_min, g_max) - g)
//                    otherwise p and g stay and held += 1
// The estimates read the raw input and the dc in front of the frame, never the corrected output, which is what makes the stage parallel in
// time: the frame means of a tile in parallel, a scan over them for the dc in front of every frame, the three power sums of the DC-removed
// rails in parallel, a, r, b and the validity test in parallel, a scan for p and g, then the correction in parallel.
//
// Every operation above is kept, in that order, and the unit is compiled with -ffp-contract=off, IEEE denormals and correctly rounded
// division and square root: bit-exact in every arith mode.  (s / F is s * (1 / F) here: F is a power of two, so both are the one correctly
// rounded value of the same real number, denormal results included.)
//
// One single-wave workgroup per channel; no two wavefronts touch one channel's state.  A tile is 1024 samples = 16 wave loads of one sample
// per lane (512 bytes each; 256 for int16 slots), kept in registers as the two floats they are until they are corrected and stored; the
// next tile's loads are issued as soon as this tile's rails are in LDS and fly under its sums and scans:
//   load     sample i * 64 + lane; its rails go to LDS at frame * (F + 1) + n -- one word of padding per frame;
//   means    lane r * NT + f sums the F values of rail r of frame f in order (NT frames in a tile): one instruction stream for both rails; the
//            lanes read F + 1 words apart, conflict-free on the 32 banks;
//   dc scan  the tile's frames in order, every lane computing the same dc (the means of frame f are two v_readlane); lane f keeps the dc in
//            front of frame f;
//   powers   F = 64, 128: lane g * NT + f runs one accumulator over frame f -- g = 0: i * i, 1: q * q, 2: i * q, the rails picked by address --
//            so the three sums are one instruction stream, and lane f collects them; F = 32 (96 lanes would be needed): lane f runs the three
//            itself.  Then a, r, b and the validity test in lane f;
//   pg scan  as the dc scan; lane f keeps p and g in front of frame f;
//   correct  a sample's four coefficients come from its frame's lane (v_readlane: the frame of a wave load is known at compile time, two
//            of them at F = 32); whole-wave stores of 512 bytes.
// Calls longer than a tile loop over tiles; dc, p and g run on from tile to tile in registers.
#include "rx_host.h"

#include <cfloat>
#include <cmath>
#include <vector>

namespace srx {

constexpr int kIqcTile = 1024;                   // samples of a tile
constexpr int kIqcIter = kIqcTile / kWave;       // wave loads of a tile

// the word(s) of one complex sample as loaded: f32 (re, im) | int16 (I in the low half)
template <typename T> struct IqcWord;
template <> struct IqcWord<float> { typedef float2 type; };
template <> struct IqcWord<int16_t> { typedef uint32_t type; };

__device__ __forceinline__ void iqc_rails(float2 w, float &i, float &q) { i = w.x; q = w.y; }
__device__ __forceinline__ void iqc_rails(uint32_t w, float &i, float &q)
{
    i = q15_to_float((int16_t)(w & 0xFFFFu));
    q = q15_to_float((int16_t)(w >> 16));
}

// x + alpha * (target - x): the AGC's form, every operation rounded
__device__ __forceinline__ float iqc_follow(float x, float target, float alpha)
{
    const float d = target - x;
    const float s = alpha * d;
    return x + s;
}

__device__ __forceinline__ float iqc_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// the value lane `frame of sample i * 64 + lane` holds: the frame of a wave load is a constant, or two
template <int F>
__device__ __forceinline__ float iqc_of_frame(float v, int i, uint32_t lane)
{
    if constexpr (F == 32) {
        const float lo = iqc_lane(v, 2 * i), hi = iqc_lane(v, 2 * i + 1);
        return lane < 32u ? lo : hi;
    } else {
        return iqc_lane(v, i * kWave / F);
    }
}

// the tile at t0 (< L): sample i * 64 + lane of it as two floats, zeros past the end of the call
template <typename W>
__device__ __forceinline__ void iqc_load_tile(const W *x, uint32_t t0, uint32_t L, uint32_t lane, float2 (&w)[kIqcIter])
{
    const uint32_t rem = L - t0 < (uint32_t)kIqcTile ? L - t0 : (uint32_t)kIqcTile;
#pragma unroll
    for (int i = 0; i < kIqcIter; ++i) {
        w[i] = make_float2(0.0f, 0.0f);
        const uint32_t s = i * kWave + lane;
        if ((uint32_t)(i * kWave) < rem && s < rem) iqc_rails(x[t0 + s], w[i].x, w[i].y);
    }
}

template <int F, typename T>
__global__ __launch_bounds__(64) void k_iqc(IqcParams q, const T *__restrict__ src, float *__restrict__ dst)
{
    typedef typename IqcWord<T>::type W;
    constexpr int NT = kIqcTile / F;             // frames of a tile (<= 64: one per lane)
    constexpr int PS = F + 1;                    // words between the frames in LDS
    constexpr bool kSplit = 3 * NT <= kWave;     // F = 64, 128: the three power sums of a frame run in three lanes
    __shared__ float rails[2 * NT * PS];         // [rail][frame][F + 1]
    float *const ri = rails, *const rq = rails + NT * PS;

    const uint32_t lane = threadIdx.x, c = blockIdx.x, L = q.block_size;
    const W *x = reinterpret_cast<const W *>(src) + (size_t)c * L;
    float2 *y = reinterpret_cast<float2 *>(dst) + (size_t)c * L;
    const bool est_dc = q.dc_alpha > 0.0f, est = q.alpha > 0.0f;
    float dci = q.dc_i[c], dcq = q.dc_q[c], p = q.p[c], g = q.g[c];
    uint32_t held = 0u;

    float2 next[kIqcIter];
    iqc_load_tile(x, 0u, L, lane, next);
    for (uint32_t t0 = 0; t0 < L; t0 += kIqcTile) {
        const uint32_t rem = L - t0 < (uint32_t)kIqcTile ? L - t0 : (uint32_t)kIqcTile;    // samples of this tile: whole frames
        const uint32_t nf = rem / F;
        float vi[kIqcIter], vq[kIqcIter];
        __syncthreads();                         // (one wave: orders the LDS traffic across lanes for the compiler)
#pragma unroll
        for (int i = 0; i < kIqcIter; ++i) {
            const uint32_t s = i * kWave + lane;
            iqc_rails(next[i], vi[i], vq[i]);
            if ((uint32_t)(i * kWave) < rem && s < rem) {
                ri[(s / F) * PS + (s % F)] = vi[i];
                rq[(s / F) * PS + (s % F)] = vq[i];
            }
        }
        __syncthreads();
        // the next tile's loads fly under this tile's sums and scans
        if (t0 + (uint32_t)kIqcTile < L) iqc_load_tile(x, t0 + (uint32_t)kIqcTile, L, lane, next);

        // arm_mean_f32: lane r * NT + f sums rail r of frame f (one instruction stream for both rails)
        const uint32_t lf = lane % NT, lg = lane / NT;
        float m = 0.0f;
        if (est_dc && lg < 2u && lf < nf) {
            const float *row = rails + (lg * NT + lf) * PS;
            float s = 0.0f;
#pragma unroll 8
            for (int n = 0; n < F; ++n) s = s + row[n];
            m = s * (1.0f / (float)F);
        }

        // the dc in front of every frame of the tile
        float bi = dci, bq = dcq;
#pragma unroll
        for (int f = 0; f < NT; ++f) {
            if ((uint32_t)f < nf) {
                if (lane == (uint32_t)f) { bi = dci; bq = dcq; }
                if (est_dc) {
                    const float mfi = iqc_lane(m, f), mfq = iqc_lane(m, NT + f);
                    if (fabsf(mfi) <= FLT_MAX) dci = iqc_follow(dci, mfi, q.dc_alpha);      // (a NaN or Inf mean: the rail keeps its dc)
                    if (fabsf(mfq) <= FLT_MAX) dcq = iqc_follow(dcq, mfq, q.dc_alpha);
                }
            }
        }

        // lane f: arm_power_f32 / arm_dot_prod_f32 of frame f's DC-removed rails, the estimate and whether it is valid
        float ea = 0.0f, eb = 0.0f;
        int valid = 0;
        float pii = 0.0f, pqq = 0.0f, piq = 0.0f;
        if constexpr (kSplit) {
            // lane g * NT + f: g = 0: sum i * i, 1: sum q * q, 2: sum i * q of frame f -- one instruction stream, the rails picked by address
            const float di = __shfl(bi, (int)lf), dq = __shfl(bq, (int)lf);
            float acc = 0.0f;
            if (est && lg < 3u && lf < nf) {
                const float *ra = rails + ((lg == 1u ? NT : 0) + lf) * PS, *rb = rails + ((lg == 0u ? 0 : NT) + lf) * PS;
                const float da = lg == 1u ? dq : di, db = lg == 0u ? di : dq;
#pragma unroll 8
                for (int n = 0; n < F; ++n) {
                    const float va = ra[n] - da, vb = rb[n] - db;
                    const float pr = va * vb;
                    acc = acc + pr;
                }
            }
            pii = __shfl(acc, (int)lf); pqq = __shfl(acc, (int)(NT + lf)); piq = __shfl(acc, (int)(2 * NT + lf));
        } else if (est && lane < nf) {
#pragma unroll 8
            for (int n = 0; n < F; ++n) {
                const float i = ri[lane * PS + n] - bi, qv = rq[lane * PS + n] - bq;
                const float ii = i * i, qq = qv * qv, iq = i * qv;
                pii = pii + ii;
                pqq = pqq + qq;
                piq = piq + iq;
            }
        }
        if (est && lane < nf) {
            const float a = piq / pii;
            const float ap = a * piq;
            const float r = pqq - ap;
            const float b = sqrtf(pii / r);
            valid = (pii > q.min_power && pii <= FLT_MAX && r > q.min_power && r <= FLT_MAX) ? 1 : 0;
            ea = a < -q.p_max ? -q.p_max : (a > q.p_max ? q.p_max : a);
            eb = b < q.g_min ? q.g_min : (b > q.g_max ? q.g_max : b);
        }

        // p and g in front of every frame of the tile
        float bp = p, bg = g;
#pragma unroll
        for (int f = 0; f < NT; ++f) {
            if ((uint32_t)f < nf) {
                if (lane == (uint32_t)f) { bp = p; bg = g; }
                if (est) {
                    if (__builtin_amdgcn_readlane(valid, f)) {
                        p = iqc_follow(p, iqc_lane(ea, f), q.alpha);
                        g = iqc_follow(g, iqc_lane(eb, f), q.alpha);
                    } else {
                        held += 1u;
                    }
                }
            }
        }

        // the correction, with the coefficients in front of the sample's frame
#pragma unroll
        for (int i = 0; i < kIqcIter; ++i) {
            if ((uint32_t)(i * kWave) < rem) {
                const uint32_t s = i * kWave + lane;
                const float ci = iqc_of_frame<F>(bi, i, lane), cq = iqc_of_frame<F>(bq, i, lane);
                const float cp = iqc_of_frame<F>(bp, i, lane), cg = iqc_of_frame<F>(bg, i, lane);
                const float iv = vi[i] - ci, qv = vq[i] - cq;
                const float t = iv * cp;
                const float u = qv - t;
                if (s < rem) y[t0 + s] = make_float2(iv, u * cg);
            }
        }
    }
    if (lane == 0u) {
        q.dc_i[c] = dci; q.dc_q[c] = dcq;
        q.p[c] = p; q.g[c] = g;
        q.held[c] += held;
    }
}

hipError_t launch_iqc(const IqcParams &q, uint32_t frame, const void *src, bool src_q15, float *dst, hipStream_t st)
{
    if (q.channels == 0 || q.block_size == 0) return hipSuccess;
    if (q.block_size % frame != 0) return hipErrorInvalidValue;
    const dim3 grid(q.channels), blk(kWave);
#define SRX_IQC_LAUNCH(F)                                                                                                            \
    do {                                                                                                                             \
        if (src_q15) hipLaunchKernelGGL((k_iqc<F, int16_t>), grid, blk, 0, st, q, static_cast<const int16_t *>(src), dst);           \
        else hipLaunchKernelGGL((k_iqc<F, float>), grid, blk, 0, st, q, static_cast<const float *>(src), dst);                       \
    } while (0)
    if (frame == 32) SRX_IQC_LAUNCH(32);
    else if (frame == 64) SRX_IQC_LAUNCH(64);
    else if (frame == 128) SRX_IQC_LAUNCH(128);
    else return hipErrorInvalidValue;
#undef SRX_IQC_LAUNCH
    return hipGetLastError();
}

// ---- host side of the stage ----
void IqcStage::release()
{
    dev_free(d_dc_i, d_dc_q, d_p, d_g, d_held, d_buf);
    buf_bytes = 0;
    frame = 0;
    alpha = dc_alpha = p_max = g_min = g_max = min_power = 0.0f;
    p_init = g_init = dc_i_init = dc_q_init = 0.0f;
}

// the stage's state as set_iqc leaves it: the four floats at the config's inits, held 0
int IqcStage::init_state(selenite_rx_instance *S)
{
    if (!frame) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels;
    HIPCHK(S, hipMemsetAsync(d_held, 0, C * sizeof(uint64_t), S->stream));
    if (int rc = fill_rows(S, d_dc_i, C, &dc_i_init)) return rc;
    if (int rc = fill_rows(S, d_dc_q, C, &dc_q_init)) return rc;
    if (int rc = fill_rows(S, d_p, C, &p_init)) return rc;
    return fill_rows(S, d_g, C, &g_init);                   // (each of them drains the stream)
}

// Step 0b2: one launch on the instance's stream writes the corrected copy of the call's input, always f32 and with the caller's stride
// (block_size samples per channel), to the instance's buffer -- grown by the first call that needs it -- and the rest of the call reads
// that.  (The chunks of a host-pointer call run their kernels on this one stream, one behind the other: one buffer serves them all.)
int IqcStage::run(selenite_rx_instance *S, ChanRange r, const void *src, bool src_q15, uint32_t block_size, const void **corrected_src)
{
    HIPCHK(S, hipSetDevice(S->device));
    const size_t need = (size_t)r.count * block_size * 2 * sizeof(float);
    if (int rc = ensure(S, (void **)&d_buf, &buf_bytes, need)) return rc;
    IqcParams q{};
    q.channels = r.count; q.block_size = block_size;
    q.alpha = alpha; q.dc_alpha = dc_alpha;
    q.p_max = p_max; q.g_min = g_min; q.g_max = g_max; q.min_power = min_power;
    q.dc_i = d_dc_i + r.first; q.dc_q = d_dc_q + r.first; q.p = d_p + r.first; q.g = d_g + r.first; q.held = d_held + r.first;
    HIPCHK(S, launch_iqc(q, frame, src, src_q15, d_buf, S->stream));
    *corrected_src = d_buf;
    return SELENITE_RX_SUCCESS;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_iqc(selenite_rx_instance *S, const selenite_rx_iqc_config *iqc)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_iqc: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    float g_min = 0.0f;
    if (iqc) {
        const char *bad = nullptr;
        int code = SELENITE_RX_ARGUMENT_ERROR;
        const bool g_ok = iqc->struct_size == sizeof(selenite_rx_iqc_config) && std::isfinite(iqc->g_max) && iqc->g_max >= 1.0f;
        if (g_ok) g_min = 1.0f / iqc->g_max;
        if (iqc->struct_size != sizeof(selenite_rx_iqc_config)) bad = "struct_size is not sizeof(selenite_rx_iqc_config)";
        else if (iqc->frame != 32 && iqc->frame != 64 && iqc->frame != 128) { bad = "frame is not 32, 64 or 128"; code = SELENITE_RX_LENGTH_ERROR; }
        else if (S->cfg.block % iqc->frame != 0) { bad = "frame does not divide cfg.block"; code = SELENITE_RX_LENGTH_ERROR; }
        else if (!(iqc->alpha >= 0.0f && iqc->alpha <= 1.0f)) bad = "alpha is not in [0, 1]";
        else if (!(iqc->dc_alpha >= 0.0f && iqc->dc_alpha <= 1.0f)) bad = "dc_alpha is not in [0, 1]";
        else if (!(iqc->p_max > 0.0f && iqc->p_max <= 1.0f)) bad = "p_max is not in (0, 1]";
        else if (!g_ok) bad = "g_max is not finite and >= 1";
        else if (!(std::isfinite(iqc->min_power) && iqc->min_power >= 0.0f)) bad = "min_power is not finite and >= 0";
        else if (!(iqc->p_init >= -iqc->p_max && iqc->p_init <= iqc->p_max)) bad = "p_init is not within +-p_max";
        else if (!(iqc->g_init >= g_min && iqc->g_init <= iqc->g_max)) bad = "g_init is not within [1 / g_max, g_max]";
        else if (!std::isfinite(iqc->dc_i_init) || !std::isfinite(iqc->dc_q_init)) bad = "dc_i_init / dc_q_init is not finite";
        if (bad) return refuse("selenite_rx_set_iqc", bad, code);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    IqcStage &st = S->iqc;
    st.release();
    if (!iqc) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels;
    hipError_t e = dev_alloc(&st.d_dc_i, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_dc_q, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_p, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_g, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_held, C);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_iqc: hipMalloc: ") + hipGetErrorString(e));
    }
    st.frame = iqc->frame;
    st.alpha = iqc->alpha; st.dc_alpha = iqc->dc_alpha;
    st.p_max = iqc->p_max; st.g_max = iqc->g_max; st.g_min = g_min; st.min_power = iqc->min_power;
    st.p_init = iqc->p_init; st.g_init = iqc->g_init; st.dc_i_init = iqc->dc_i_init; st.dc_q_init = iqc->dc_q_init;
    return st.init_state(S);
}

static int iqc_state_copy(selenite_rx_instance *S, const selenite_rx_iqc_state_view *v, bool to_host)
{
    if (!S || !v || !S->iqc.frame) return SELENITE_RX_ARGUMENT_ERROR;
    const IqcStage &st = S->iqc;
    const size_t C = S->cfg.channels;
    return copy_rows(S, to_host, { { st.d_dc_i, v->dc_i, C * sizeof(float) }, { st.d_dc_q, v->dc_q, C * sizeof(float) }, { st.d_p, v->p, C * sizeof(float) },
                                   { st.d_g, v->g, C * sizeof(float) }, { st.d_held, v->held, C * sizeof(uint64_t) } });
}
extern "C" int selenite_rx_get_iqc_state(selenite_rx_instance *S, const selenite_rx_iqc_state_view *v) { return iqc_state_copy(S, v, true); }
extern "C" int selenite_rx_set_iqc_state(selenite_rx_instance *S, const selenite_rx_iqc_state_view *v) { return iqc_state_copy(S, v, false); }
