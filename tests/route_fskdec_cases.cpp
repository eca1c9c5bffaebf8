// route_fskdec_cases.cpp -- the route of a launch (selenite-lite_amd/csrc/rx_route.h) over the product of tests/route_cases.cpp, in the same
// order and with the same columns, once with the FSK decoder's flag off and once with it on: two more columns at the end of a line, the
// flag and Route::run.fskdec -- for tests/test_route_fskdec.py.  Host code only: g++ -std=c++17, no HIP.
#include <cstdio>

#include "../selenite-lite_amd/csrc/rx_route.h"

using namespace srx;

int main()
{
    const Phase phases[] = { kAll, kPhase1, kPhase2 };
    const bool slots[3][2] = { { false, false }, { true, true }, { false, true } };      // (src, dst): f32 -> f32, int16 -> int16, f32 -> int16
    for (int fskdec = 0; fskdec < 2; ++fskdec)
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
        if (fskdec) f.on.fskdec = true;                // (off: the flag is left at its default)
        if (gate && !f.on.meter) continue;            // the gate is the meter's
        f.gate = gate;
        f.force_generic = force; f.ssb_kernels = kernel == 1; f.cw_kernel = kernel == 2;
        f.cw_biquads = cwbq; f.words = words;
        const Route t = route(f);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d\n",
               (int)phase, (int)f.src_q15, (int)f.dst_q15, global, agc, (int)f.on.tones, (int)f.on.afilt, (int)f.on.nr, (int)f.on.meter, gate, force, kernel,
               cwbq, words,
               (int)t.run.tones, (int)t.run.afilt, (int)t.run.nr, (int)t.run.meter, (int)t.gate, (int)t.mixed, (int)t.ssb_fused, (int)t.cw_fused, (int)t.fused,
               (int)t.unscaled, (int)t.convert_in, (int)t.audio_in_scratch, (int)t.fused_agc_off, (int)t.done_after_fused, (int)t.clear_words,
               (int)t.generic_front, (int)t.biquad, (int)t.env, (int)t.apply, (int)t.agc_generic, (int)f.on.fskdec, (int)t.run.fskdec);
    }
    return 0;
}
