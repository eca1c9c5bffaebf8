// rx_fft8.h -- the pieces of arm_cfft_f32 for the pure radix-8 lengths (64, 512) that the spectrum tap (rx_spectrum.hip) and the polyphase
// channeliser (chan.hip) share: the reference's twiddle table regenerated on the host, the eight-point butterfly of
// arm_radix8_butterfly_f32 (TransformFunctions/arm_cfft_radix8_f32.c:45-285) and its twiddle multiplies.  How a wave lays a transform of 512
// (or eight of 64) over its lanes, pass by pass, is described at the head of rx_spectrum.hip; both files use that layout.
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

}  // namespace srx
