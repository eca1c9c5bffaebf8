// select_cases.cpp -- the decision function of the SSB fused path (selenite-lite_amd/csrc/rx_select.h) over the full product of shapes,
// arithmetics, modes, slot formats, DSP blocks, call lengths, LO situations and call facts: one line of integers per case, for
// tests/test_select.py.  `names` as the only argument: one line per (shape, arith, mode, block) with the whole-pass decision's family
// and the kernel name formatted from it.  Host code only: g++ -std=c++17, no HIP.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../selenite-lite_amd/csrc/rx_select.h"

using namespace srx;

struct Shape { int nd, m, nh; bool plain; };      // plain: unit-impulse delay and odd-only Hilbert taps (else the dense flavour serves it)

int main(int argc, char **argv)
{
    const bool names = argc > 1 && !std::strcmp(argv[1], "names");
    std::vector<Shape> shapes;                    // the four lists (a shape two of them name appears once)
    auto add = [&](int nd, int m, int nh, bool plain) {
        for (const Shape &s : shapes) if (s.nd == nd && s.m == m && s.nh == nh && s.plain == plain) return;
        shapes.push_back({ nd, m, nh, plain });
    };
#define X(ND_, M_, NH_, ID_) add(ND_, M_, NH_, true);
    SRX_SHAPES(X)
#undef X
#define X(ND_, M_, NH_, ID_) add(ND_, M_, NH_, false);
    SRX_DENSE_SHAPES(X)
#undef X
#define X(ND_, M_, NH_) add(ND_, M_, NH_, true);
    SRX_SPLIT16_SHAPES(X)
#undef X
#define X(NH_) add(0, 1, NH_, true);
    SRX_HILB16_SHAPES(X)
#undef X
    add(100, 4, 63, true);                        // in range, no instantiation of its own: the 128-tap kernels, taps zero-padded
    add(256, 4, 65, true);                        // a 65-tap pair: the dense flavour
    const uint32_t modes[] = { SELENITE_MODE_USB, SELENITE_MODE_AM, SELENITE_MODE_FM }, blocks[] = { 64, 96, 128, 192, 256 };
    for (const Shape &s : shapes)
    for (uint32_t arith = 0; arith < 4; ++arith)
    for (uint32_t mode : modes)
    for (uint32_t block : blocks) {
        selenite_rx_config g{};
        g.block = block; g.decim = (uint32_t)s.m; g.nd_taps = (uint32_t)s.nd; g.nh_taps = (uint32_t)s.nh; g.arith = arith; g.mode = (uint8_t)mode;
        const SelPlan sp = plan_shape(g, s.plain, s.plain);
        if (!sp.kind) continue;                   // the shape does not admit this DSP block (block / M: 4 .. 256, a multiple of 4)
        if (names) {
            const Decision d = select(g, sp, whole_pass_call(g, sp));
            printf("%d %d %d %d %u %u %u %d %s\n", s.nd, s.m, s.nh, (int)s.plain, arith, mode, block, (int)d.family, kernel_name(g, d).c_str());
            continue;
        }
        const uint32_t p16 = split16_pass_out(block, g.decim);
        const uint32_t pass = (sp.nds > 0 && split16_pass_ok(p16) ? p16 : fused_pass_out(block, g.decim)) * g.decim;
        const uint32_t hs = sp.nd > 0 ? split16_hs(sp.nds > 0 ? sp.nds : sp.nd, s.m == 8 ? 4 : s.m) : 0u;
        const uint32_t under = hs ? (hs - 1) / block : 0u, at = (hs + block - 1) / block;      // blocks that land just under / just at HS
        const uint32_t lens[] = { block, 2 * block, 4 * block, pass, pass + block, 3 * pass, 3 * pass + under * block, 3 * pass + at * block };
        for (uint32_t bs : lens)
        for (int q15 = 0; q15 < 2; ++q15)
        for (int lo = 0; lo < 5; ++lo)            // off, shared table, shared on the fs / 256 grid, per channel on the grid, per channel arbitrary
        for (int unscaled = 0; unscaled < 2; ++unscaled)
        for (int rows = 0; rows < 2; ++rows)
        for (int launches = 1; launches <= 3; launches += 2) {
            g.nco_enable = lo != 0;
            SelCall c;
            c.block_size = bs; c.q15 = q15; c.global_gain = unscaled; c.hist_ext = rows;
            c.steps_uniform = c.phase_uniform = lo == 1 || lo == 2;
            c.steps_grid256 = lo == 2 || lo == 3;
            c.auto_launches = launches;
            c.rerun_words = arith == SELENITE_ARITH_AUTO;
            const Decision d = select(g, sp, c);
            Decision d1;                          // the first part of a cut call, decided as a call of its own
            if (d.first) { c.block_size = d.first; d1 = select(g, sp, c); }
            printf("%d %d %d %d %u %u %u %u %d %d %d %d %d  %d %d %d %d %u  %d %d %u %d %u %u %u %u %u %d %u %d %u  %d %u\n",
                   s.nd, s.m, s.nh, (int)s.plain, arith, mode, block, bs, q15, lo, unscaled, rows, launches,
                   sp.nd, sp.nds, (int)sp.btab16, (int)sp.mfma, sp.ext_len,
                   (int)d.family, (int)d.q15, d.pass_out, (int)d.dec2, d.nco_rx, d.lo_period, d.nco, d.nco_rerun, d.lo_n, (int)d.env_part, d.auto_form,
                   (int)d.repair_all, d.first, (int)d1.family, d1.first);
        }
    }
    return 0;
}
