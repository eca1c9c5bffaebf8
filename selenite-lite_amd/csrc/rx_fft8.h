// rx_fft8.h -- arm_cfft_f32 for the pure radix-8 lengths (64, 512), one transform of 512 (or eight of 64) per wave: the reference's twiddle
// table regenerated on the host, the eight-point butterfly of arm_radix8_butterfly_f32 (TransformFunctions/arm_cfft_radix8_f32.c:45-285), its
// twiddle multiplies, the twiddles a lane needs (fft8_twiddles) and the passes over the wave with their LDS exchanges (fft8_passes).  The
// spectrum tap (rx_spectrum.hip), the polyphase channeliser (chan.hip) and the combiner (comb.hip) run this one transform.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace srx {

// twiddleCoef_N (CommonTables/arm_common_tables.c) regenerated on the host, as host_sin_table() does for sinTable_f32: the source holds every
// entry as a nine-decimal literal of cos / sin(2 pi i / N), so entry i = float("%.9f" % cos), float("%.9f" % sin) -- signs of the zeros
// included (a tiny negative value prints as -0.000000000).  The plain (float)cos differs in 3 / 19 entries of the 64 / 512 table.
inline void spec_twiddles(float *tw, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) {
        const double a = 2.0 * 3.14159265358979323846 * (double)i / (double)n;
        char buf[32];
        std::snprintf(buf, sizeof buf, "%.9f", std::cos(a));
        tw[2 * i] = std::strtof(buf, nullptr);
        std::snprintf(buf, sizeof buf, "%.9f", std::sin(a));
        tw[2 * i + 1] = std::strtof(buf, nullptr);
    }
}

constexpr float kC81 = 0.70710678118f;      // arm_cfft_radix8_f32.c:62, as the reference writes it

// arm_radix8_butterfly_f32's eight-point butterfly without the twiddle multiplies: a[m] = element i1 + m * n2 (:74-132 / :175-251)
__device__ __forceinline__ void bfly8(float2 (&a)[8])
{
    float r1 = a[0].x + a[4].x, r5 = a[0].x - a[4].x;
    float r2 = a[1].x + a[5].x, r6 = a[1].x - a[5].x;
    float r3 = a[2].x + a[6].x, r7 = a[2].x - a[6].x;
    float r4 = a[3].x + a[7].x, r8 = a[3].x - a[7].x;
    float t1 = r1 - r3;
    r1 = r1 + r3;
    r3 = r2 - r4;
    r2 = r2 + r4;
    float s1 = a[0].y + a[4].y, s5 = a[0].y - a[4].y;
    float s2 = a[1].y + a[5].y, s6 = a[1].y - a[5].y;
    float s3 = a[2].y + a[6].y, s7 = a[2].y - a[6].y;
    float s4 = a[3].y + a[7].y, s8 = a[3].y - a[7].y;
    float t2 = s1 - s3;
    s1 = s1 + s3;
    s3 = s2 - s4;
    s2 = s2 + s4;
    a[0] = make_float2(r1 + r2, s1 + s2);
    a[4] = make_float2(r1 - r2, s1 - s2);
    a[2] = make_float2(t1 + s3, t2 - r3);
    a[6] = make_float2(t1 - s3, t2 + r3);
    const float q1 = (r6 - r8) * kC81;
    r6 = (r6 + r8) * kC81;
    const float q2 = (s6 - s8) * kC81;
    s6 = (s6 + s8) * kC81;
    t1 = r5 - q1;
    r5 = r5 + q1;
    r8 = r7 - r6;
    r7 = r7 + r6;
    t2 = s5 - q2;
    s5 = s5 + q2;
    s8 = s7 - s6;
    s7 = s7 + s6;
    a[1] = make_float2(r5 + s7, s5 - r7);
    a[7] = make_float2(r5 - s7, s5 + r7);
    a[5] = make_float2(t1 + s8, t2 - r8);
    a[3] = make_float2(t1 - s8, t2 + r8);
}

// the twiddled form's tail (:214-275): element m times (co, si) of index m * id -- p1 = co * r, p2 = si * s, p3 = co * s, p4 = si * r
__device__ __forceinline__ void twiddle7(float2 (&a)[8], const float2 (&w)[7])
{
#pragma unroll
    for (int m = 1; m < 8; ++m) {
        const float p1 = w[m - 1].x * a[m].x, p2 = w[m - 1].y * a[m].y;
        const float p3 = w[m - 1].x * a[m].y, p4 = w[m - 1].y * a[m].x;
        a[m] = make_float2(p1 + p2, p3 - p4);
    }
}

// the lane's twiddles of the two twiddled passes.  Pass n2 = 64 (N = 512 only; twidCoefModifier 1): ia_k = k * j, j = lane; pass n2 = 8
// (modifier N / 64): ia_k = k * j * N / 64, j = lane & 7 (arm_cfft_radix8_f32.c:146-168).  tw is spec_twiddles' table of N entries.
template <int N>
__device__ __forceinline__ void fft8_twiddles(const float *tw, uint32_t lane, float2 (&tw1)[7], float2 (&tw2)[7])
{
    static_assert(N == 64 || N == 512, "the pure radix-8 lengths a wave holds");
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        if (N == 512) tw1[k - 1] = reinterpret_cast<const float2 *>(tw)[k * lane];
        tw2[k - 1] = reinterpret_cast<const float2 *>(tw)[(N / 64) * k * (lane & 7u)];
    }
}

// The radix-8 passes of arm_cfft_f32 over one single-wave workgroup: in, a[m] is element e0 + es * m of the load layout (N = 512: e0 = lane,
// es = 64; N = 64: eight transforms per wave, lane 8 f + j holds elements j + 8 m of transform slot f); out, a[m] is position 8 * lane + m of
// the butterflies' output (N = 64: position 8 * (lane & 7) + m of slot lane >> 3), which arm_bitreversal_32 -- the base-8 digit reversal --
// makes bin 64 m + 8 (lane & 7) + (lane >> 3) (N = 64: bin 8 m + (lane & 7)).  fs is the caller's exchange buffer: 512 elements + the padding of
// either exchange.
//
// The reference has two butterfly forms: the j = 0 column of a pass and the whole last pass store the sums as they are (:72-135), the other
// columns multiply them by the twiddles (:143-281).  Both compute the same sums in the same order, so bfly8 serves both and the lanes of
// column 0 skip the multiplies (1 * x + 0 * y is not x for Inf, NaN and the sign of zero).  A pass of 512 points is 64 butterflies, one per lane:
//   pass 1  lane j owns elements j + 64 m: the caller's loads put them straight into registers -- no LDS in front of pass 1;
//   pass 2  lane 8 g + j owns 64 g + j + 8 m: exchanged through LDS at index e + 8 (e >> 6): the eight groups of a wave would otherwise sit
//           512 bytes apart, on the same banks;
//   pass 3  lane b owns 8 b + m: exchanged at index e + (e >> 3) (stride 9 instead of 8 between lanes).
// Both exchanges are conflict-free in writes and reads (64-bit accesses, 32 lanes per LDS cycle covering the 64 banks once).  N = 64 is
// passes 2 and 3 alone.  The barriers order the LDS traffic across the lanes of the one wave for the compiler; the first of an exchange also
// keeps it behind whatever the caller last read from fs.
template <int N>
__device__ __forceinline__ void fft8_passes(float2 (&a)[8], const float2 (&tw1)[7], const float2 (&tw2)[7], float2 *fs, uint32_t lane)
{
    const uint32_t j2 = lane & 7u, g = lane >> 3;
    if (N == 512) {
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
    bfly8(a);                                                // n2 = 1: every butterfly is of the twiddle-free form
}

}  // namespace srx
