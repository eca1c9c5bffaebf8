// rx_fused_kernels.h -- k_ssb_fused (the fused SSB kernel on the vector ALU, both exact arithmetic contracts) and its launcher,
// shared by the two translation units that instantiate it: rx_fused.hip (fma arithmetic; planning and dispatch; k_ssb_mfma) and
// rx_fused_exact.hip (CMSIS arithmetic: the bit-exact kernels, also the rerun pass of SELENITE_ARITH_AUTO).  Two units so the
// ~1000 instantiations compile in parallel (the single unit took 6 minutes).
#pragma once
#include "rx_fused_common.h"
#include "rx_hist_exact.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

#pragma clang fp contract(off)

namespace srx {

// arm_fir_decimate_f32 on BOTH rails for the 4 adjacent outputs j = 4*lane + r.
// Output j needs s[(j - HQ4 + q)*M + p] * cq[q*M + p], q = 0..HQ4 ascending, p ascending: the
// loops below visit (q, p) in exactly that order for every r, so each accumulator sees the
// reference's tap order.  Coefficients live lane-distributed in creg and reach the SGPR file by
// v_readlane (no scalar-memory latency, one fetch serves both rails and up to 4 outputs).
template <int ARITH, int ND, int M, int NH>
__device__ __forceinline__ void decim_quad(const float *S, int lane, const float (&creg)[Geo<ND, M, NH>::NCR],
                                           v2f (&acc)[4])
{
    using G = Geo<ND, M, NH>;
    const float *base = S + 12 * lane;
#pragma unroll
    for (int o = 0; o < (G::HQ4 + 4) / 2; ++o) {
        float4 W[M];
#pragma unroll
        for (int p = 0; p < M; ++p)
            W[p] = lds_ld4f(base + p * G::PSF + 4 * (3 * (o >> 1) + (o & 1)));
#pragma unroll
        for (int e = 0; e < 2; ++e) {
#pragma unroll
            for (int p = 0; p < M; ++p) {
                const v2f w = e ? v2f{ W[p].z, W[p].w } : v2f{ W[p].x, W[p].y };
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = 2 * o + e - r;
                    const int kk = q * M + p;
                    if (q < 0 || q > G::HQ4 || (q == G::HQ4 && p > 0) || kk < G::F) continue;
                    const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(creg[kk >> 6]), kk & 63));
                    acc[r] = mac2<ARITH>(acc[r], w, c);
                }
            }
        }
    }
}

// The same FIR for a SHORT pass (round 4: calls of up to 64 audio samples -- the firmware's one- and two-slot callbacks, the 256-sample
// call: most of what SELENITE_ARITH_AUTO sends here because it is too short for the matrix kernel): output j = lane, ONE output
// per lane instead of four adjacent ones, so that every lane works on an output that exists -- a quarter of the tile's multiply-adds.  Per accumulator the same visit order (q ascending, p ascending), the same products: the same bits.  Element j + q of
// phase p sits at elem(j + q) = 12 ((j + q) >> 2) + 2 ((j + q) & 3); with q = 4 a + b that is a per-lane base for each b plus the
// compile-time offset 12 a: four address registers, immediate offsets, one ds_read_b64 per tap.  The 4 M reads of step a + 1 are issued
// before step a's products are formed (left to the compiler, every read was followed by its own s_waitcnt: 257 LDS round trips per
// pass, as long as the four-output form).
// The same FIR for a SHORT pass (round 4: calls of up to 64 audio samples -- the firmware's one- and two-slot callbacks, the 256-sample
// call: most of what SELENITE_ARITH_AUTO sends to this kernel because it is too short for the matrix kernel): output j = lane (+ 64 k),
// ONE output per lane instead of four adjacent ones, so that every lane works on an output that exists -- a quarter of the tile's
// multiply-adds.  Per accumulator the same visit order (q ascending, p ascending), the same products: the same bits.  Element j + q of
// phase p sits at elem(j + q) = 12 ((j + q) >> 2) + 2 ((j + q) & 3); with q = 4 a + b that is a per-lane base for each b plus the
// compile-time offset 12 (a + 16 k): four address registers, immediate offsets, one ds_read_b64 per tap.  The 4 M reads of step a + 1
// are issued before step a's products are formed -- left to the compiler every read was followed by its own s_waitcnt, 257 LDS round
// trips per pass: as long as the four-output form.  (Only K = 1 is used: a second round for outputs 64 .. 127 -- a second copy of the
// walk, a loop around it, or K = 2 -- and even this function returning its sum by value cost the kernel 1.6 KB of scratch.)
template <int ARITH, int ND, int M, int NH, int K>
__device__ __forceinline__ void decim_spread(const float *S, int lane, const float (&creg)[Geo<ND, M, NH>::NCR], v2f (&acc)[K])
{
    using G = Geo<ND, M, NH>;
    const float *bs[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) bs[b] = S + G::elem(lane + b);
    // software pipeline over a: the 4 M K reads of step a + 1 are in flight while step a's products are formed
    v2f w[2][4][M][K];
    auto load = [&](int a, int slot) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int p = 0; p < M; ++p)
#pragma unroll
                for (int k = 0; k < K; ++k)
                    w[slot][b][p][k] = *reinterpret_cast<const v2f *>(bs[b] + 12 * (a + 16 * k) + p * G::PSF);
    };
    load(0, 0);
#pragma unroll
    for (int a = 0; a <= G::HQ4 / 4; ++a) {
        if (a < G::HQ4 / 4) load(a + 1, (a + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int q = 4 * a + b;
            if (q > G::HQ4) continue;
#pragma unroll
            for (int p = 0; p < M; ++p) {
                const int kk = q * M + p;
                if ((q == G::HQ4 && p > 0) || kk < G::F) continue;
                const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(creg[kk >> 6]), kk & 63));
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] = mac2<ARITH>(acc[k], w[a & 1][b][p][k], c);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Steps 3-5 of a pass, shared by the VALU and the MFMA kernels: Hilbert FIR on Q (structural zeros
// skipped) and unit-impulse delay on I from the decimated rails in LDS, sideband combine, AGC per
// DSP block (group lanes), one 4-sample store per lane.
// GROUP = lanes per DSP block as a compile-time constant (16: 64-sample blocks, 64: 256-sample blocks;
// 0 = runtime `group`): constant lane indices turn the block-envelope broadcasts into v_readlane and
// the lane reductions into DPP instead of ds_bpermute round trips.
// The exact kernel as the rerun pass of SELENITE_ARITH_AUTO evaluates the parity guard itself (round 4, hysteresis): a channel it
// recomputes stays with it (kFlagHold: the matrix kernel skips the channel in the next calls) until TWO calls in a row show no DSP
// block under 1.25 x the guard ratio (2 dB), so a level hovering at the ratio does not bounce between the kernels -- a bounce costs
// the matrix pass AND the exact pass of a call; a wide margin would keep quiet-but-clean channels (the survey of
// profiles/r3/guard_ratio_survey.txt has a third of its in-band blocks between 0.25 and 0.5) on the slow kernel for good.
struct GuardEx {
    float thr, thr2;    // guard ratio x / 1.25 x guard ratio x the largest |component| of the mixed samples the pass and the pass before it hold
    uint32_t n, n2;     // DSP blocks of the call under thr / thr2
};

// The FIR pair with ARBITRARY taps (round 4, VERDICT r3 missing 4): arm_fir_f32 (FilteringFunctions/arm_fir_f32.c:553-979) on both rails for
// the 4 adjacent outputs n = 4 lane + r -- I' = delay_coeffs * I, Q' = hilb_coeffs * Q, every tap of both, no structure assumed (a dense
// Hilbert design, a fractional-delay FIR on the I rail, an even tap count), nh <= NH taps zero-padded in FRONT (older samples times
// +0.0f).  The taps come from LDS by broadcast reads: table index u = k + FH + 3 holds padded tap k, so step t (window elements
// 4 t .. 4 t + 3 of the rail) needs exactly the quads u = 4 t .. 4 t + 7; steps whose taps are all padding are skipped (t0).  Per output
// the reference's order: one accumulator from 0, taps ascending, product rounded, then sum rounded (mac<ARITH>).
template <int NH> struct DenseTab { static constexpr int LEN = ((NH - 1 + 3) & ~3) + 12; };      // floats per FIR: padded taps + offset + the last step's reach
// BOTH: the delay FIR on the I rail is dense too (DENSE == 1); else only the Hilbert FIR is (DENSE == 2: the common case of a dense
// Hilbert design beside a unit-impulse delay, whose I rail stays one LDS read per output as in the type-III kernels).
// (A version with two outputs per packed instruction -- tap pairs from a second, shifted copy of the table, the broadcast in op_sel:
// half the vector instructions of this loop -- was bit-exact and no faster: the kernel sits at the package power cap, where time
// follows the floating-point work, not the instruction count; profiles/r4/README.md.)
template <int ARITH, int ND, int M, int NH, bool BOTH>
__device__ __forceinline__ void dense_pair_quad(const float *di, const float *dq, const float *ptab, int lane, int t0, float (&ai)[4], float (&aq)[4])
{
    const float *td = ptab, *th = ptab + DenseTab<NH>::LEN;
    for (int t = t0; t < HilbertSteps<ND, M, NH>::N; ++t) {
        const v4f wq = lds_ld4(dq + 4 * lane + 4 * t);
        const v4f h0 = lds_ld4(th + 4 * t), h1 = lds_ld4(th + 4 * t + 4);
        const float hh[8] = { h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w };
        v4f wi = { 0.0f, 0.0f, 0.0f, 0.0f };
        float dd[8] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        if constexpr (BOTH) {
            wi = lds_ld4(di + 4 * lane + 4 * t);
            const v4f d0 = lds_ld4(td + 4 * t), d1 = lds_ld4(td + 4 * t + 4);
            dd[0] = d0.x; dd[1] = d0.y; dd[2] = d0.z; dd[3] = d0.w; dd[4] = d1.x; dd[5] = d1.y; dd[6] = d1.z; dd[7] = d1.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int r = 0; r < 4; ++r) {                             // tap k = 4 t + e - r - FH  <->  table index 4 t + (e - r + 3)
                if constexpr (BOTH) ai[r] = mac<ARITH>(ai[r], wi[e], dd[e - r + 3]);
                aq[r] = mac<ARITH>(aq[r], wq[e], hh[e - r + 3]);
            }
    }
}

// AM: 0 = SSB combine, 1 = AM / FM (fa.am says which), 2 = decided at run time by fa.am (k_ssb_fused, round 4: one kernel per shape
// and slot format instead of one per NCO flavour and demodulator -- the binary was 35 MB)
// DENSE: the FIR pair with arbitrary taps (dense_pair_quad; fa.ptab: their LDS table) instead of the type-III Hilbert / unit-delay pair
template <int ARITH, int GROUP, int ND, int M, int NH, typename TOut, int AM = 0, int DENSE = 0>
__device__ __forceinline__ void demod_agc_store(const RxParams &p, const FusedArgs &fa, const float *dI,
                                                const float *dQ, int lane, int group,
                                                const float (&hreg)[(NH + 63) / 64 ? (NH + 63) / 64 : 1], float &gain,
                                                TOut *__restrict__ dst, size_t out_index, bool &nonfinite,
                                                int nvb = 64,        // DSP blocks of this pass that exist (whole passes: all of them)
                                                float *env_row = nullptr,   // global gain, phase 1, as the rerun pass of SELENITE_ARITH_AUTO:
                                                                            // max |audio| of the pass's DSP blocks goes here (what the split16 kernel left
                                                                            // for this channel came from the arithmetic being replaced)
                                                GuardEx *gx = nullptr)      // rerun pass of SELENITE_ARITH_AUTO: count the blocks under the guard thresholds
{
    using G = Geo<ND, M, NH>;
    float au[4];
    const bool am_on = AM == 2 ? fa.am != 0u : AM != 0;               // (wave-uniform; a compile-time constant for AM = 0 / 1)
    if (NH > 0 && am_on) {
        // AM: envelope of the decimated rails; new sample n of a pass sits at HH4 + n
        const float4 vi = lds_ld4f(dI + G::HH4 + 4 * lane);
        const float4 vq = lds_ld4f(dQ + G::HH4 + 4 * lane);
        if (fa.am == 2u) {
            // FM (a run-time flavour of the AM instantiations): z[n] * conj(z[n-1]); the sample in front of the pass is the
            // newest entry of the Hilbert-pair history, which this mode keeps running (and writes back)
            const float pi0 = dI[G::HH4 + 4 * lane - 1], pq0 = dQ[G::HH4 + 4 * lane - 1];
            au[0] = fm_disc(vi.x, vq.x, pi0, pq0);  au[1] = fm_disc(vi.y, vq.y, vi.x, vq.x);
            au[2] = fm_disc(vi.z, vq.z, vi.y, vq.y); au[3] = fm_disc(vi.w, vq.w, vi.z, vq.z);
            if (gx) {                                             // the matrix kernel's FM guard (rx_split16_kernels.h): thresholds over min|z| of the pass
                float zz = fminf(fminf(vi.x * vi.x + vq.x * vq.x, vi.y * vi.y + vq.y * vq.y), fminf(vi.z * vi.z + vq.z * vq.z, vi.w * vi.w + vq.w * vq.w));
                zz = fminf(zz, pi0 * pi0 + pq0 * pq0);
                const float zmin = __builtin_sqrtf(__uint_as_float(~wave_umax_bits(__uint_as_float(~__float_as_uint(zz)))));
                gx->thr = gx->thr / zmin;
                gx->thr2 = gx->thr2 / zmin;
            }
        } else {
            au[0] = cmag<0>(vi.x, vq.x); au[1] = cmag<0>(vi.y, vq.y);
            au[2] = cmag<0>(vi.z, vq.z); au[3] = cmag<0>(vi.w, vq.w);
        }
    } else if (NH > 0 && DENSE != 0) {
        float i2[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, q2[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        dense_pair_quad<ARITH, ND, M, NH, DENSE == 1>(dI, dQ, fa.ptab_lds, lane, (int)fa.dense_t0, i2, q2);
        if constexpr (DENSE == 2) {                                   // unit-impulse delay FIR: 0.0f + 1.0f * x of the dense loop (fa.delay_idx: in the PADDED taps)
            const float *di = dI + G::FH + fa.delay_idx + 4 * lane;
#pragma unroll
            for (int r = 0; r < 4; ++r) i2[r] = di[r] + 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) au[r] = fa.upper ? (i2[r] - q2[r]) : (i2[r] + q2[r]);       // arm_sub_f32 / arm_add_f32
    } else if (NH > 0) {
        float q2[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        hilbert_quad<ARITH, ND, M, NH>(dQ, lane, hreg, q2);
        const float *di = dI + G::FH + fa.delay_idx + 4 * lane;   // unit-impulse delay FIR
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float i2 = di[r] + 0.0f;                        // 0.0f + 1.0f*x of the dense loop
            au[r] = fa.upper ? (i2 - q2[r]) : (i2 + q2[r]);       // arm_sub_f32 / arm_add_f32
        }
    } else {
        const float4 v = lds_ld4f(dI + 4 * lane);
        au[0] = v.x; au[1] = v.y; au[2] = v.z; au[3] = v.w;
    }
    // arm_abs + arm_max per DSP block (group lanes): the block maximum in every lane of the block -- for the AGC, for the block maxima a
    // global-gain call wants (env_row) and for the guard evaluation of the rerun pass (gx); computed once, and unconditionally: a
    // wave-uniform branch around it cost the rerun pass a fifth of its time (it split the pass into small basic blocks)
    float m = fmaxf(fmaxf(fabsf(au[0]), fabsf(au[1])), fmaxf(fabsf(au[2]), fabsf(au[3])));
    const int gl = GROUP ? GROUP : group;
    if constexpr (GROUP > 0) {
#pragma unroll
        for (int off = 1; off < GROUP; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    } else if ((group & (group - 1)) == 0) {                  // power of two: butterfly
#pragma unroll
        for (int off = 1; off < 64; off <<= 1)
            if (off < group) m = fmaxf(m, __shfl_xor(m, off, 64));
    } else {                                                  // e.g. 6 lanes: the firmware's 96-frame blocks by 4 (dsp_if.h:69-73)
        float mm = 0.0f;
        for (int j = 0; j < group; ++j) mm = fmaxf(mm, __shfl(m, ((lane / group) * group + j) & 63, 64));
        m = mm;
    }
    {
        const bool first = lane % gl == 0 && lane / gl < nvb;     // the first lane of every DSP block that exists
        if (env_row && first) env_row[lane / gl] = m;
        if (gx) {
            gx->n += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(first && m < gx->thr));
            gx->n2 += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(first && m < gx->thr2));
        }
    }
    // AGC: gain law on the block maxima, arm_scale
    if (p.agc) {
        float g = gain, mine = gain;
        if constexpr (GROUP > 0) {
            const int myblk = lane / GROUP;
            // the divisions target/env of the blocks of this pass are independent of the gain
            // recurrence: issue them together, then run the (cheap) recurrence
            float dsr[64 / GROUP];
            // every lane divides for its own block's envelope (one division sequence for the whole
            // wavefront instead of one per block), then the per-block results are broadcast
            const float mine_d = agc_desired(p.agcp, m);
#pragma unroll
            for (int b = 0; b < 64 / GROUP; ++b)
                dsr[b] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine_d), b * GROUP));
#pragma unroll
            for (int b = 0; b < 64 / GROUP; ++b) {
                const float gn = agc_step(p.agcp, g, dsr[b]);
                g = b < nvb ? gn : g;                             // blocks past the end of the call leave the gain alone
                mine = (b == myblk) ? g : mine;
            }
        } else {
            const int myblk = lane / group;
            const int nblk = min(64 / group, nvb);
            for (int b = 0; b < nblk; ++b) {
                const float env = __shfl(m, b * group, 64);
                g = agc_update<0>(p.agcp, g, env);
                if (b == myblk) mine = g;
            }
        }
        gain = g;
#pragma unroll
        for (int r = 0; r < 4; ++r) au[r] = au[r] * mine;
    }
    const bool live = lane < nvb * (GROUP ? GROUP : group);       // this lane's four samples exist
    {   // ARM_MATH_NANINF: x * 0 is NaN iff x is not finite
        const float z = __builtin_fmaf(au[3], 0.0f, __builtin_fmaf(au[2], 0.0f, __builtin_fmaf(au[1], 0.0f, au[0] * 0.0f)));
        nonfinite = nonfinite || (live && z != z);
    }
    const size_t o = out_index + 4 * lane;
    if (live) {
        // (non-temporal: the audio is written once and never read by the chain -- the caches are left to the streaming state)
        if constexpr (sizeof(TOut) == 4) {
            v4f *at = reinterpret_cast<v4f *>(reinterpret_cast<float *>(dst) + o);
            // (the non-temporal store as the instruction itself: __builtin_nontemporal_store of a 16-byte vector came out as a plain
            // global_store_dwordx4 -- and merged with the cached store of the other branch -- so the f32 audio of every launch of this kernel
            // went through the caches until round 5)
            const v4f av = { au[0], au[1], au[2], au[3] };
            if (p.out_cached) *at = av;                                       // global gain, phase 1: the gain pass reads it back
            else asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" :: "v"(at), "v"(av) : "memory");      // (s_nop: the wait states a VALU write of the data registers needs behind a store wider than 64 bits -- the compiler does not see into the asm)
        } else {
            typedef uint32_t w2v __attribute__((ext_vector_type(2)));
            uint32_t w0, w1;
            float4_to_q15(au[0], au[1], au[2], au[3], p.q15_round, w0, w1);
            __builtin_nontemporal_store(w2v{ w0, w1 }, reinterpret_cast<w2v *>(reinterpret_cast<int16_t *>(dst) + o));
        }
    }
}

// NCO flavour (fa.nco: 0 off, 1 per-channel per sample, 2 shared table, 4 per-channel periodic) and demodulator (fa.am) are RUN-TIME
// switches, wave-uniform, outside the hot loops (round 4): one kernel per arithmetic, shape and slot format -- the sixteen
// instantiations per shape this replaced were most of a 35 MB library and of its four-minute build.
// The kernel body is a function of its own: k_ssb_fused runs it over the channels of its grid (or, as the rerun pass, over the dense list);
// the matrix kernels of rx_split16_kernels.h call it for ONE channel they recompute themselves (INL: channel inl.c, whose word -- as the
// rerun pass would find it -- is inl.word; p.chan_flags is set, the list and its counters are not looked at).
struct FusedInl { uint32_t c, word; };
template <int ARITH, int ND, int M, int NH, typename TIn, typename TOut, int DENSE, bool INL>
__device__ __forceinline__ void ssb_fused_body(RxParams p, FusedArgs fa, const TIn *__restrict__ src, TOut *__restrict__ dst, FusedInl inl)
{
    using G = Geo<ND, M, NH>;
    const uint32_t NCO = fa.nco;                         // wave-uniform
    constexpr int AM = 2;                                // demod_agc_store: look at fa.am
    // Round 4: the decimator of the INSTANCE may be shorter than the kernel's (p.nd <= ND: the host picks the smallest instantiated
    // shape that holds it and pads the taps with zeros in front -- older samples times +0.0f leave a finite accumulator alone, the
    // structural-zero argument of DESIGN.md section 3).  What changes is the state: p.nd - 1 samples per rail, sitting Fr slots into the
    // kernel's history.
    const int ndr = ND > 0 ? (int)p.nd : 0, Fr = ND > 0 ? G::HQ4 * M + 1 - ndr : 0;
    // ... and so may the FIR pair (DENSE instantiations: p.nh <= NH taps, padded in front): p.nh - 1 history samples per rail
    const int hhr = NH > 0 ? (int)p.nh - 1 : 0, FHr = G::HH4 - hhr;
    using R = BRaw<TIn>;
    static_assert(ND == 0 ? M == 1 : (M == 2 || M == 4 || M == 8), "fused kernel: no decimator, or decimate by 2, 4 or 8");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    // Passes of VARIABLE length (round 3): a full pass produces pq = fa.pass_out audio samples -- the largest whole number of
    // DSP blocks in 256 (256 itself when block / M divides 256; 240 = 10 blocks of the firmware's 96-frame geometry by 4,
    // dsp_if.h:69-73) -- and the last pass of a call whatever is left (a call is a whole number of DSP blocks, not of
    // passes).  The arithmetic always covers the whole 256-output tile: input beyond the call reads as zeros (buffer range
    // check), outputs beyond the pass are not stored and do not move the AGC, and the history copies take the samples behind
    // the last one that exists.  Per output the operation order is the reference's in every case.
    const uint32_t pq = fa.pass_out, tq = pq * M;
    float *tab = lds + G::oTab;
    float *S = lds + G::oS;
    float *D = lds + G::oD;
    float *dI = D, *dQ = D + G::DLEN;
    constexpr int NLD = G::T / 128;                      // raw loads per lane per pass
    bool nonfinite = false;                              // any audio sample of this workgroup NaN / Inf
    // One channel per workgroup, c = blockIdx.x -- or, as the rerun pass of SELENITE_ARITH_AUTO (p.chan_flags: the channel words, whose
    // rerun bit the split16 kernel of the same call raised for the channels under the parity guard and the exact kernel keeps up for
    // the channels it holds), entries blockIdx.x, blockIdx.x + gridDim.x, ... of the dense list k_hist_exact made of them: which
    // channels, and how many, is only known on the device; every workgroup gets an even share.
    uint32_t li = INL ? 0u : blockIdx.x;
    const uint32_t ln = INL ? 1u : (p.chan_flags ? *p.chan_count : 0u);
    if (!INL && p.chan_flags && p.rerun_seen && blockIdx.x == 0 && lane == 0) __hip_atomic_store(p.rerun_seen, ln, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (p.chan_flags && li >= ln) return;                // rerun pass: nothing on the list for this workgroup (every workgroup, in the steady state of a clean workload)
    // what does not depend on the channel, once per workgroup: sine table, decimator taps (lane-distributed), Hilbert taps
    if (NCO == 1u || NCO == 4u)
        for (int i = lane; i < 513; i += kWave) tab[i] = p.sintab[i];
    float creg[G::NCR > 0 ? G::NCR : 1];
    if constexpr (ND > 0) {
#pragma unroll
        for (int v = 0; v < G::NCR; ++v) creg[v] = fa.cq[64 * v + lane];
    }
    float hreg[(NH + 63) / 64 ? (NH + 63) / 64 : 1];
#pragma unroll
    for (int v = 0; v < (NH + 63) / 64; ++v) hreg[v] = (DENSE == 0 && 64 * v + lane < NH) ? p.hilb_c[64 * v + lane] : 0.0f;     // (DENSE: p.hilb_c holds p.nh <= NH taps and is read from LDS)
    if constexpr (DENSE != 0) {                          // the FIR pair's tap tables (both rails) behind the kernel's own LDS image
        float *pt = lds + G::total;
        for (int i = lane; i < 2 * DenseTab<NH>::LEN; i += kWave) pt[i] = fa.ptab[i];
        fa.ptab_lds = pt;
    }
    auto in_rsrc = [&](uint32_t ch, bool valid) { return make_rsrc(src + (size_t)ch * p.in_stride * 2, valid ? p.block_size * (R::kBytes / 2) : 0u); };
    // the first pass of a channel is in flight before the channel starts: loaded here for the first one, under the last pass of the
    // channel before it for the others (rerun pass: the list says which channel comes next)
    uint32_t c_cur = INL ? inl.c : blockIdx.x;
    if (!INL && p.chan_flags) c_cur = li < ln ? p.chan_list[li] : 0u;
    typename R::type raw[NLD];
    {
        const __amdgpu_buffer_rsrc_t rs0 = in_rsrc(c_cur, !p.chan_flags || li < ln);
#pragma unroll
        for (int i = 0; i < NLD; ++i) raw[i] = R::load(rs0, lane * R::kBytes + i * 64 * R::kBytes, 0);
    }
  for (;;) {
    const uint32_t c = c_cur;
    uint32_t c_nxt = 0u;
    bool has_nxt = false;
    if (p.chan_flags) {
        if (li >= ln) break;
        li += INL ? 1u : gridDim.x;
        has_nxt = li < ln;
        c_nxt = has_nxt ? p.chan_list[li] : 0u;
    }

    const size_t out_base = (size_t)c * p.out_stride;
    const uint32_t npass = (p.nout + pq - 1) / pq;
    // rerun pass of SELENITE_ARITH_AUTO: the parity guard is evaluated here too (GuardEx); a channel that came in HELD (not raised by
    // the matrix kernel of this call, which skipped it) gets its guard counters from this kernel
    const bool rerun_pass = p.chan_flags != nullptr;                 // wave-uniform
    const uint32_t word_in = INL ? inl.word : (rerun_pass ? p.chan_flags[c] : 0u);
    const bool held_in = (word_in & kFlagHold) != 0u;
    GuardEx gx{ 0.0f, 0.0f, 0u, 0u };
    float hmax = 0.0f;                                               // largest |component| of the FIR history the channel came in with
    const __amdgpu_buffer_rsrc_t rs_in = in_rsrc(c, true);
    const __amdgpu_buffer_rsrc_t rs_next = in_rsrc(c_nxt, has_nxt);      // (no next channel: an empty range -- zeros, no traffic)
    const __amdgpu_buffer_rsrc_t rs_lo = make_rsrc(p.lo, NCO == 2u ? p.block_size * 8u : 0u);

    // ---- prologue: streaming state into LDS / registers ----
    if constexpr (ND > 0) {
        // history element (phase pp, index m) holds sample s = (m*M + pp) - F of the CMSIS state
        // (oldest first); slots before the state (s < 0) only ever meet zero-padded taps
        batched_fill<2 * M * G::HQ4>(lane, p.dec_state + (size_t)c * 2 * (ndr - 1),
            [&](int i) {
                const int rail = i / (M * G::HQ4), sidx = i % (M * G::HQ4) - Fr;
                return sidx >= 0 ? rail * (ndr - 1) + sidx : -1;
            },
            [&](int i, float v) {
                const int rail = i / (M * G::HQ4), rem = i % (M * G::HQ4);
                S[(rem % M) * G::PSF + G::elem(rem / M) + rail] = v;
                hmax = fmaxf(hmax, fabsf(v));
            });
    }
    if constexpr (NH > 0) {
        batched_fill<2 * G::HH4>(lane, p.fir_state + (size_t)c * 2 * hhr,
            [&](int i) {
                const int rail = i / G::HH4, sidx = i % G::HH4 - FHr;
                return sidx >= 0 ? rail * hhr + sidx : -1;
            },
            [&](int i, float v) { D[(i / G::HH4) * G::DLEN + i % G::HH4] = v; if (ND == 0) hmax = fmaxf(hmax, fabsf(v)); });
    }
    float pm_prev = __uint_as_float(wave_umax_bits(hmax));           // what "the pass before" pass 0 held: the history
    const uint32_t ph0 = NCO ? p.phase[c] : 0u;
    const uint32_t step = NCO ? p.step[c] : 0u;
    float gain = p.agc ? p.gain[c] : 1.0f;
    const int group = (int)fa.group;
    wave_lds_sync();
    // NCO == 4 (round 3; as in k_ssb_split16): the channel's own step is a multiple of 2^24, so its LO repeats every 256 samples
    // whatever its phase, and a pass (256 M inputs: the host selects this flavour only with 256-output passes) is a whole number
    // of periods: load i of any pass multiplies by LO[(128 i + 2 lane, + 1) mod 256] -- two register quads, computed once per
    // channel and call with the arithmetic of the per-sample flavour (same phases modulo 2^32: same bits)
    lo_v2f lo_per[4] = { { 1.0f, 0.0f }, { 1.0f, 0.0f }, { 1.0f, 0.0f }, { 1.0f, 0.0f } };
    if (NCO == 4u) {
        const uint32_t pe = ph0 + 2u * lane * step;
        nco_lo_pair(tab, pe, pe + step, lo_per[0], lo_per[1]);
        nco_lo_pair(tab, pe + 128u * step, pe + 129u * step, lo_per[2], lo_per[3]);
    }

    for (uint32_t pass = 0; pass < npass; ++pass) {
        const uint32_t n0 = pass * tq;
        const uint32_t cur = (pass + 1 == npass) ? p.nout - pass * pq : pq;      // audio samples of this pass (whole DSP blocks)
        // ---- 1. NCO mix of the prefetched samples, scatter into the LDS image ----
        // the LO of a chunk of loads first -- one wave-uniform branch per flavour, outside the loop that mixes and scatters --, then one
        // branch-free loop (a branch inside it splits the pass into small basic blocks: measured 20 % on the rerun pass)
        float mx = 0.0f;                                              // rerun pass: largest |component| of this pass's mixed samples
        constexpr int CH = NLD < 8 ? NLD : 8;                         // loads per chunk (decimation by 8: two chunks -- 16 LO pairs at once spilled)
        static_assert(NLD % CH == 0, "whole chunks");
        const bool mixing = NCO != 0u;                                // wave-uniform: two copies of the mix loop, one without the multiply
#pragma unroll
        for (int ch = 0; ch < NLD / CH; ++ch) {
        lo_v2f la[CH], lb[CH];
        if (NCO == 2u) {                                              // shared LO table (L2 resident): all loads of the chunk in flight at once
            u4v lo4[CH];
#pragma unroll
            for (int j = 0; j < CH; ++j)
                lo4[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_lo, lane * 16 + (ch * CH + j) * 1024, (int)(n0 * 8u), 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                la[j] = lo_v2f{ __uint_as_float(lo4[j].x), __uint_as_float(lo4[j].y) };
                lb[j] = lo_v2f{ __uint_as_float(lo4[j].z), __uint_as_float(lo4[j].w) };
            }
        } else if (NCO == 1u) {                                       // arm_sin/cos_f32 restated for the vector ALU: same bits (rx_device.h)
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const uint32_t pe = ph0 + (n0 + 128u * (ch * CH + j) + 2u * lane) * step;
                nco_lo_pair(tab, pe, pe + step, la[j], lb[j]);
            }
        } else {                                                      // per-channel periodic LO (registers); NCO off: not used
#pragma unroll
            for (int j = 0; j < CH; ++j) { la[j] = lo_per[2 * (j & 1)]; lb[j] = lo_per[2 * (j & 1) + 1]; }
        }
        auto mix_scatter = [&](auto mixc) {
            constexpr bool MIX = decltype(mixc)::value;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int i = ch * CH + j;
            const uint32_t n = 128u * i + 2u * lane;                  // even sample index in the pass
            float2 a, b;
            {
                v2f va, vb;
                R::unpack(raw[i], va, vb);
                a = make_float2(va.x, va.y); b = make_float2(vb.x, vb.y);
            }
            if constexpr (MIX) {
                a = cmul<0>(a, make_float2(la[j].x, la[j].y));
                b = cmul<0>(b, make_float2(lb[j].x, lb[j].y));
            }
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(a.x), fabsf(a.y))), fmaxf(fabsf(b.x), fabsf(b.y)));      // (unconditional: no branch in the mix stage)
            if constexpr (ND > 0) {
                const int m = G::HQ4 + (int)(n / M), pp = (int)(n % M);   // n even: pp in {0,2}
                float *d = S + pp * G::PSF + G::elem(m);
                *reinterpret_cast<float2 *>(d) = a;
                *reinterpret_cast<float2 *>(d + G::PSF) = b;
            } else {
                *reinterpret_cast<float2 *>(dI + G::HH4 + n) = make_float2(a.x, b.x);
                *reinterpret_cast<float2 *>(dQ + G::HH4 + n) = make_float2(a.y, b.y);
            }
        }
        };
        if (mixing) mix_scatter(std::true_type{});
        else mix_scatter(std::false_type{});
        }
        {
            // the matrix kernel's guard compares a block's envelope with the largest sample its pass's product saw (new samples and
            // the decimator history) and, for the first blocks, the pass before; here: this pass and the one before it, for every block
            // (evaluated in every launch -- a dozen instructions per pass --, used by the rerun pass only)
            const float pm = __uint_as_float(wave_umax_bits(mx));
            const float lvl = fmaxf(pm, pm_prev);
            gx.thr = lvl * p.guard_ratio;
            gx.thr2 = gx.thr * 1.25f;
            pm_prev = pm;
        }
        wave_lds_sync();
        // ---- prefetch the next pass while this one computes (the last pass: the first pass of the workgroup's next channel) ----
        {
            const bool last = pass + 1 == npass;                      // wave-uniform
            const __amdgpu_buffer_rsrc_t rs_pf = last ? rs_next : rs_in;
            const int so = last ? 0 : (int)((n0 + tq) * (R::kBytes / 2));
#pragma unroll
            for (int i = 0; i < NLD; ++i) raw[i] = R::load(rs_pf, lane * R::kBytes + i * 64 * R::kBytes, so);
        }
        // ---- 2. arm_fir_decimate_f32 on both rails, 4 adjacent outputs per lane ----
        if constexpr (ND > 0) {
            if (ARITH == 0 && M == 4 && DENSE == 0 && cur <= 64u) {     // wave-uniform: a short pass -- only the outputs that exist (decim_spread; the bit-exact /4 kernels: what AUTO's short calls run on)
                v2f a1[1] = { { 0.0f, 0.0f } };
                decim_spread<ARITH, ND, M, NH, 1>(S, lane, creg, a1);
                dI[G::HH4 + lane] = a1[0].x; dQ[G::HH4 + lane] = a1[0].y;
                if (lane >= 16) {                                     // the rest of the tile: not computed, never stored, in no DSP block the AGC looks at -- but read by the demodulator: zeros
                    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    *reinterpret_cast<float4 *>(dI + G::HH4 + 4 * lane) = z4;
                    *reinterpret_cast<float4 *>(dQ + G::HH4 + 4 * lane) = z4;
                }
            } else {
                v2f acc[4] = { { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f } };
                decim_quad<ARITH, ND, M, NH>(S, lane, creg, acc);
                *reinterpret_cast<float4 *>(dI + G::HH4 + 4 * lane) = make_float4(acc[0].x, acc[1].x, acc[2].x, acc[3].x);
                *reinterpret_cast<float4 *>(dQ + G::HH4 + 4 * lane) = make_float4(acc[0].y, acc[1].y, acc[2].y, acc[3].y);
            }
            wave_lds_sync();
        }
        // ---- 3-5. Hilbert pair + sideband, AGC, store ----
        const int nvb = (int)(cur / (4u * (uint32_t)group));          // DSP blocks of this pass
        // (rerun pass of AUTO inside a global-gain call whose split16 kernel emitted block maxima: refresh this channel's row)
        float *env_row = (p.chan_flags && p.env_part) ? p.env_part + (size_t)c * (p.block_size / p.block) + (size_t)pass * (pq / (4u * (uint32_t)group)) : nullptr;
        if (group == 16)
            demod_agc_store<ARITH, 16, ND, M, NH, TOut, AM, DENSE>(p, fa, dI, dQ, lane, group, hreg, gain, dst, out_base + (size_t)pass * pq, nonfinite, nvb, env_row, &gx);
        else if (group == 64)
            demod_agc_store<ARITH, 64, ND, M, NH, TOut, AM, DENSE>(p, fa, dI, dQ, lane, group, hreg, gain, dst, out_base + (size_t)pass * pq, nonfinite, nvb, env_row, &gx);
        else
            demod_agc_store<ARITH, 0, ND, M, NH, TOut, AM, DENSE>(p, fa, dI, dQ, lane, group, hreg, gain, dst, out_base + (size_t)pass * pq, nonfinite, nvb, env_row, &gx);
        wave_lds_sync();
        // ---- 6. history copy-back (arm_fir_decimate_f32.c:396-426, arm_fir_f32.c:947-978) ----
        if constexpr (ND > 0) {
            constexpr int NG = M * (G::HQ4 / 4);                      // 48-byte groups to move
            constexpr int NK = (NG + 63) / 64;
            float4 t0[NK], t1[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i = k * 64 + lane;
                if (i < NG) {                                         // the HQ4 phase-samples behind the last one that exists
                    const float *sp = S + (i / (G::HQ4 / 4)) * G::PSF + 12 * (cur / 4 + i % (G::HQ4 / 4));
                    t0[k] = lds_ld4f(sp);
                    t1[k] = lds_ld4f(sp + 4);
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i = k * 64 + lane;
                if (i < NG) {
                    float *dp = S + (i / (G::HQ4 / 4)) * G::PSF + 12 * (i % (G::HQ4 / 4));
                    *reinterpret_cast<float4 *>(dp) = t0[k];
                    *reinterpret_cast<float4 *>(dp + 4) = t1[k];
                }
            }
        }
        if constexpr (NH > 0) {
            constexpr int NV = 2 * (G::HH4 / 4);
            static_assert(NV <= 64, "Hilbert history move assumes <= 64 float4");
            float4 tmp;
            const int rail = lane / (G::HH4 / 4), v = lane % (G::HH4 / 4);
            if (lane < NV) tmp = lds_ld4f(D + rail * G::DLEN + cur + 4 * v);
            wave_lds_sync();
            if (lane < NV) *reinterpret_cast<float4 *>(D + rail * G::DLEN + 4 * v) = tmp;
        }
        wave_lds_sync();
    }

    // ---- epilogue: streaming state back to HBM ----
    if constexpr (ND > 0) {
        for (int i = lane; i < 2 * M * G::HQ4; i += kWave) {
            const int rail = i / (M * G::HQ4), rem = i % (M * G::HQ4);
            const int s = rem - Fr, pp = rem % M, m = rem / M;
            if (s >= 0) p.dec_state[((size_t)c * 2 + rail) * (ndr - 1) + s] = S[pp * G::PSF + G::elem(m) + rail];
        }
    }
    if constexpr (NH > 0) {
        if (fa.am != 1u) {                                            // AM never ran the Hilbert pair: its state stays (FM keeps the delay lines running)
            for (int i = lane; i < 2 * G::HH4; i += kWave) {
                const int rail = i / G::HH4, m = i % G::HH4, s = m - FHr;
                if (s >= 0) p.fir_state[((size_t)c * 2 + rail) * hhr + s] = D[rail * G::DLEN + m];
            }
        }
    }
    if (lane == 0) {
        if (NCO != 0u) p.phase[c] = ph0 + p.block_size * step;
        if (p.agc) p.gain[c] = gain;
        // SELENITE_ARITH_AUTO: the state this kernel leaves is exact (kProvExact) -- as the rerun pass, and as a call without a matrix
        // kernel; k_ssb_split16 reads the word at the channel's next call.  (AM, not FM, leaves the Hilbert-pair history alone: its
        // provenance stays what it was -- exact in practice, k_hist_exact having run in front of the AM call; "with samples" would
        // degrade to "without", the decimator state having moved on without them.)
        // Rerun pass (round 4): the channel is HELD on this kernel (kFlagRerun | kFlagHold: the matrix kernel skips it from the next
        // call on) while any block of the call sits under 1.25 x the guard ratio; the second call in a row without one hands it back (word 0).
        uint32_t *w = p.chan_flags ? p.chan_flags + c : (p.rerun_flag ? p.rerun_flag + c : nullptr);
        if (w) {
            uint32_t nw = 0u;
            if (fa.am == 1u) {
                const uint32_t prov = (*w >> kProvShift) & kProvMask;
                nw = prov == kProvExact ? 0u : ((kProvSplit << kProvShift) | (*w & (1u << kExtBufShift)));
            }
            if (rerun_pass && (nw >> kProvShift) == 0u) {
                if (gx.n2 != 0u) nw = kFlagRerun | kFlagHold;
                else if (!(held_in && (word_in & kFlagClean1) != 0u)) nw = kFlagRerun | kFlagHold | kFlagClean1;
            }
            *w = nw;
        }
        if (held_in && p.guard_ch) {                                  // (a channel the matrix kernel raised in this call was counted there)
            if (gx.n) p.guard_ch[c] = p.guard_ch[c] > 0xFFFFFFFFu - gx.n ? 0xFFFFFFFFu : p.guard_ch[c] + gx.n;
            if (p.guard_calls[c] != 0xFFFFFFFFu) p.guard_calls[c] += 1u;
        }
    }
    if (!p.chan_flags) break;
    c_cur = c_nxt;
    wave_lds_sync();                                     // the state reads above before the next channel's prologue fills
  }
    if (nonfinite) p.flags[kFlagNanInf] = 1u;            // ARM_MATH_NANINF, read by selenite_rx_sync
}

template <int ARITH, int ND, int M, int NH, typename TIn, typename TOut, int DENSE = 0>
__global__ __launch_bounds__(64, 2) void k_ssb_fused(RxParams p, FusedArgs fa, const TIn *__restrict__ src,
                                                     TOut *__restrict__ dst)
{
    ssb_fused_body<ARITH, ND, M, NH, TIn, TOut, DENSE, false>(p, fa, src, dst, FusedInl{ 0u, 0u });
}

template <int ARITH, int ND, int M, int NH, typename TIn, typename TOut, int DENSE = 0>
static hipError_t launch_one(const RxParams &p, const FusedArgs &fa, const void *src, void *dst, hipStream_t st)
{
    using G = Geo<ND, M, NH>;
    constexpr size_t lds = ((size_t)G::total + (DENSE ? 2 * DenseTab<NH>::LEN : 0)) * sizeof(float);
    if (fa.nco == 3u || (fa.nco == 4u && fa.pass_out != 256u)) return hipErrorNotSupported;      // (rx_select.h: fused_nco)
    auto k = k_ssb_fused<ARITH, ND, M, NH, TIn, TOut, DENSE>;
    if constexpr (lds > 48 * 1024) {                      // per device and per kernel: set on every launch (cheap)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // (rerun pass of SELENITE_ARITH_AUTO: which channels are flagged is only known on the device -- a resident-sized grid strides
    // over the dense list of them)
    // 2048 workgroups when the last call's list was short (the empty pass of a clean workload costs ~3 us; 16 384 would cost 8), 16 384
    // when it held more than an eighth of the channels: more workgroups than the device keeps resident let the dispatcher even the load
    // out -- 3-6 % on a call that recomputes 80 % of the channels (profiles/r4/rerun_grid_sweep.txt).  The count is the one the LAST
    // rerun pass wrote into a page-locked host word, read here without synchronising: a hint, never a result.
    uint32_t rerun_grid = plan_option(SELENITE_RX_OPT_RERUN_GRID);        // (the tests pin it: selenite_rx_set_plan_option)
    if (!rerun_grid) {
        const uint32_t seen = p.rerun_seen ? __atomic_load_n(p.rerun_seen, __ATOMIC_RELAXED) : 0u;
        rerun_grid = seen > p.channels / 8u ? 16384u : 2048u;
    }
    const uint32_t grid = p.chan_flags ? (p.channels < rerun_grid ? p.channels : rerun_grid) : p.channels;
    hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, st, p, fa, static_cast<const TIn *>(src),
                       static_cast<TOut *>(dst));
    return hipGetLastError();
}

// (the instantiated shapes, SRX_SHAPES and SRX_DENSE_SHAPES: rx_select.h)
hipError_t launch_exact_dense(int nd, int m, bool q15, bool delay_impulse, const RxParams &p, const FusedArgs &fa, const void *src, void *dst, hipStream_t st);

// the CMSIS-arithmetic instantiations live in rx_fused_exact.hip
hipError_t launch_exact(int nd, int m, int nh, bool q15, const RxParams &p, const FusedArgs &fa, const void *src, void *dst,
                        hipStream_t st);

}  // namespace srx
