// route_cases.cpp -- the route of a launch through the RX stages (selenite-lite_amd/csrc/rx_route.h) over the full product of its facts:
// phases, slot formats, global gain, AGC, the four stages in front of the AGC (and the meter's gate), the forced generic path, the kernel
// that serves the launch, a CW chain with biquads, SELENITE_ARITH_AUTO's words -- one line of integers per case, for tests/test_route.py.
// Phase 1 and phase 2 appear only with a global gain: the entry points refuse them otherwise.  Host code only: g++ -std=c++17, no HIP.
#include <cstdio>

#include "../selenite-lite_amd/csrc/rx_route.h"

using namespace srx;

int main()
{
    const Phase phases[] = { kAll, kPhase1, kPhase2 };
    const bool slots[3][2] = { { false, false }, { true, true }, { false, true } };      // (src, dst): f32 -> f32, int16 -> int16, f32 -> int16
    for (Phase phase : phases)
    for (const bool *sd : slots)
    for (int global = 0; global < 2; ++global)
    for (int agc = 0; agc < 2; ++agc)
    for (int stages = 0; stages < 16; ++stages)
    for (int gate = 0; gate < 2; ++gate)
    for (int force = 0; force < 2; ++force)
    for (int kernel = 0; kernel < 3; ++kernel)        // neither, SSB fused, CW fused
    for (int cwbq = 0; cwbq < 2; ++cwbq)
    for (int words = 0; words < 2; ++words) {
        if (phase != kAll && !global) continue;
        RouteFacts f;
        f.phase = phase; f.src_q15 = sd[0]; f.dst_q15 = sd[1];
        f.global = global; f.agc_enable = agc;
        f.on.tones = stages & 1; f.on.afilt = stages & 2; f.on.nr = stages & 4; f.on.meter = stages & 8;
        if (gate && !f.on.meter) continue;            // the gate is the meter's
        f.gate = gate;
        f.force_generic = force; f.ssb_kernels = kernel == 1; f.cw_kernel = kernel == 2;
        f.cw_biquads = cwbq; f.words = words;
        const Route t = route(f);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n",
               (int)phase, (int)f.src_q15, (int)f.dst_q15, global, agc, (int)f.on.tones, (int)f.on.afilt, (int)f.on.nr, (int)f.on.meter, gate, force, kernel,
               cwbq, words,
               (int)t.run.tones, (int)t.run.afilt, (int)t.run.nr, (int)t.run.meter, (int)t.gate, (int)t.mixed, (int)t.ssb_fused, (int)t.cw_fused, (int)t.fused,
               (int)t.unscaled, (int)t.convert_in, (int)t.audio_in_scratch, (int)t.fused_agc_off, (int)t.done_after_fused, (int)t.clear_words,
               (int)t.generic_front, (int)t.biquad, (int)t.env, (int)t.apply, (int)t.agc_generic);
    }
    return 0;
}
