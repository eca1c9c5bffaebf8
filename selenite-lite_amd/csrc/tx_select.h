// tx_select.h -- which TX kernel, in which NCO flavour, serves a call: ONE function from (config, what selenite_tx_init fixed, the facts of
// this call) to a decision that the launchers execute (tx_api.hip: run, tx_cw.hip: run_key, tx_in.hip: frames_call_ok).  No HIP in here:
// plain C++17, so the rule is testable on a CPU (tests/test_tx_select.py), like rx_select.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/selenite_tx.h"

namespace srx {

// the one shape of the matrix kernels (tx_fused.hip checks its constants against these): ALC block, L, interpolator and Hilbert-pair
// taps, audio samples of a pass
constexpr uint32_t kTxFusedBlock = 64, kTxFusedL = 4, kTxFusedNI = 256, kTxFusedNH = 63, kTxFusedPass = 256;
// dynamic LDS a single-wave workgroup of the any-shape kernels may ask for
constexpr size_t kTxLdsLimit = 64 * 1024;

// What is fixed per instance.  delay_is_impulse && hilb_odd_only: a unit-impulse delay FIR and a type-III Hilbert, what k_tx_fused and
// k_tx_split16 are written for.
struct TxSelPlan {
    bool delay_is_impulse = false, hilb_odd_only = false;
    bool table = false;                                   // the split-precision operand exists (selenite_tx_instance::d_ttab16)
    bool force_generic = false, no_periodic_lo = false;   // the two plan options (selenite_rx_set_plan_option)
    bool steps_same = true;                               // every channel has the NCO step of channel 0,
    uint32_t step0 = 0;                                   // which is this
};

// The facts of one call.  The any-shape kernels keep their LDS layouts next to themselves; the rule gets the byte counts as numbers.
struct TxSelCall {
    uint32_t block_size = 0;
    bool key = false;                  // a key call (selenite_tx_process_key_*): k_tx_cw whatever else holds
    bool phase_uniform = false;        // every channel's NCO is at the host's phase (selenite_tx_instance::phase_uniform)
    size_t lds_generic = 0, lds_fm = 0, lds_cw = 0;
};

enum TxKernel : uint8_t { kTxGeneric, kTxFused, kTxSplit16, kTxFm, kTxCw };

struct TxDecision {
    TxKernel kernel = kTxGeneric;
    uint32_t nco = 0;                  // as the kernel templates number it: 0 off, 1 per channel, 2 shared table, 3 shared periodic LO in registers (k_tx_split16 only)
    uint32_t lo_n = 0;                 // samples the shared LO table must hold (block_size * interp), 0: no table
    bool clears_uniform = false;       // the kernel moves every channel's phase on its own (FM, key calls): no shared LO behind it until reset or set_state
    bool refused = false;              // the serving any-shape kernel's layout exceeds kTxLdsLimit: nothing is launched, no state moves
};

inline bool tx_fused_ok(const selenite_tx_config &g, bool delay_is_impulse, bool hilb_odd_only, uint32_t block_size)
{
    return g.interp == kTxFusedL && g.ni_taps == kTxFusedNI && g.nh_taps == kTxFusedNH && g.block == kTxFusedBlock && delay_is_impulse &&
           hilb_odd_only && block_size % kTxFusedPass == 0;
}

inline TxDecision tx_select(const selenite_tx_config &g, const TxSelPlan &sp, const TxSelCall &c)
{
    TxDecision d;
    d.nco = g.nco_enable ? 1u : 0u;
    if (c.key || g.mode == SELENITE_MODE_FM) {
        // the phase accumulator carries the modulation (FM) or the carrier offset (CW): every channel's phase is its own from here on
        d.kernel = c.key ? kTxCw : kTxFm;
        d.clears_uniform = true;
        d.refused = (c.key ? c.lds_cw : c.lds_fm) > kTxLdsLimit;
        return d;
    }
    if (sp.force_generic || !tx_fused_ok(g, sp.delay_is_impulse, sp.hilb_odd_only, c.block_size)) {
        d.refused = c.lds_generic > kTxLdsLimit;
        return d;
    }
    d.kernel = g.arith == SELENITE_ARITH_SPLIT16 && sp.table ? kTxSplit16 : kTxFused;
    if (g.nco_enable && sp.steps_same && c.phase_uniform) {
        // every channel shares step and phase: one LO per call in a table, read from L2 by every wavefront.  On the fs / 256 grid (step a
        // multiple of 2^24) it repeats every 256 output samples, and k_tx_split16 keeps one period in registers
        d.nco = d.kernel == kTxSplit16 && (sp.step0 & 0x00FFFFFFu) == 0 && !sp.no_periodic_lo ? 3u : 2u;
        d.lo_n = c.block_size * g.interp;
    }
    return d;
}

// The call selenite_tx_kernel_name answers for: one whole pass, so no matrix kernel is ruled out by the length.  Mode and force_generic
// are the only call-independent inputs besides the plan.
inline TxSelCall tx_whole_pass_call() { TxSelCall c; c.block_size = kTxFusedPass; return c; }

// the one place a TX kernel name is spelled
inline const char *tx_kernel_name(const TxDecision &d)
{
    switch (d.kernel) {
    case kTxFused: return "k_tx_fused<4,256,63>";
    case kTxSplit16: return "k_tx_split16<4,256,63>";
    case kTxFm: return "k_tx_fm";
    case kTxCw: return "k_tx_cw";
    default: return "k_tx_generic";
    }
}

// selenite_tx_init's question, asked of the rule itself: would a whole-pass call run on k_tx_split16 if the table existed?
inline bool tx_wants_table(const selenite_tx_config &g, TxSelPlan sp)
{
    sp.table = true;
    return tx_select(g, sp, tx_whole_pass_call()).kernel == kTxSplit16;
}

}  // namespace srx
