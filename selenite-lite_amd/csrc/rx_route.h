// rx_route.h -- which stages run in one launch of a call, on which buffer, and what finishes it: ONE function from the facts of a launch to
// a Route that rx_dispatch.hip's run_part executes top to bottom (rx_select.h does the same for the kernel that serves the launch).  No HIP
// in here: plain C++17, so the rule is testable on a CPU over its whole input space (tests/test_route.py).
// A new stage in front of the AGC hooks in with one line here (its flag in StagesOn, and so in `unscaled`) and one in the executor.
#pragma once
#include <stdint.h>

namespace srx {

// all: a whole call; 1 / 2: the two halves of a global-gain call around the exchange of the envelopes (phase 2 only applies the gain)
enum Phase { kAll, kPhase1, kPhase2 };

// The stages in front of the AGC.  Each of them wants the un-scaled f32 audio of the launch: the tone detector, the Morse decoder, the FSK decoder and the level meter read it,
// the audio filter and NLMS run in place on it.
struct StagesOn {
    bool tones = false, afilt = false, nr = false, meter = false, cwdec = false, fskdec = false;
    bool any() const { return tones || afilt || meter || nr || cwdec || fskdec; }
};

struct RouteFacts {
    Phase phase = kAll;
    bool src_q15 = false, dst_q15 = false;   // slot formats as the launch finds them (behind the I/Q correction: f32 in, int16 out)
    bool agc_enable = false, global = false; // global: agc_enable && agc_global
    StagesOn on;                             // what the instance has switched on ...
    bool gate = false;                       // ... and the meter's gate (meter on and gate set)
    bool force_generic = false;
    bool ssb_kernels = false;                // the instance is on the SSB fused kernels (on_ssb_fused)
    bool cw_kernel = false;                  // the fused CW kernel takes this call (cw_fused_ok && cw_strides_ok)
    bool cw_biquads = false;                 // a CW chain with biquads: the generic path runs its biquad kernel
    bool words = false;                      // SELENITE_ARITH_AUTO's per-channel words exist
};

struct Route {
    StagesOn run;                // the stages of this launch: phase 2 runs none (its phase 1 did)
    bool gate = false;           // the meter's gate behind the AGC: not in phase 1
    bool mixed = false;          // f32 in, int16 out
    bool ssb_fused = false, cw_fused = false, fused = false;
    bool unscaled = false;       // THE definition: something in front of the AGC -- or the global gain, or the int16 store behind f32 input --
                                 // wants un-scaled f32 audio, so a fused kernel runs with its own AGC off and the tail finishes the call
    bool convert_in = false;     // int16 input converted to f32 up front (the fused kernels convert in and out symmetrically)
    bool audio_in_scratch = false;   // the un-scaled audio lives in the instance's f32 scratch, not in dst
    bool fused_agc_off = false;  // the fused kernel leaves un-scaled f32 audio (and, where Decision::env_part says so, the block maxima)
    bool done_after_fused = false;   // the fused kernel wrote dst: nothing follows
    bool clear_words = false;    // not on the SSB fused kernels: every channel's state stays exact -- repair the histories, clear the words
    bool generic_front = false, biquad = false;   // the generic kernels in front of the stages
    bool env = false, apply = false;   // the tail with a global gain: the envelope (not in phase 2), the gain pass (not in phase 1) ...
    bool agc_generic = false;    // ... and without one: k_agc_generic, which also stores int16
};

inline Route route(const RouteFacts &f)
{
    Route t;
    const bool front = f.phase != kPhase2;          // phase 2 reads the audio its phase 1 left
    if (front) t.run = f.on;
    t.gate = f.gate && f.phase != kPhase1;
    t.mixed = !f.src_q15 && f.dst_q15;
    t.ssb_fused = front && !f.force_generic && f.ssb_kernels;
    t.cw_fused = front && !f.force_generic && f.cw_kernel;
    t.fused = t.ssb_fused || t.cw_fused;
    t.unscaled = f.global || t.run.any() || t.mixed;
    t.convert_in = t.unscaled && f.src_q15 && t.fused;
    t.audio_in_scratch = f.dst_q15 && (t.unscaled || !t.fused);
    t.fused_agc_off = t.fused && t.unscaled;
    t.done_after_fused = t.fused && !t.unscaled;
    t.clear_words = front && f.words && !t.ssb_fused;
    t.generic_front = front && !t.fused;
    t.biquad = t.generic_front && f.cw_biquads;
    t.env = f.global && front;
    t.apply = f.global && f.phase != kPhase1;
    t.agc_generic = !f.global && (f.agc_enable || f.dst_q15);
    return t;
}

}  // namespace srx
