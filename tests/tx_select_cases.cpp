// tx_select_cases.cpp -- the decision function of the TX direction (selenite-lite_amd/csrc/tx_select.h) over the full product of
// geometries, tap classes, arithmetics, modes, LO situations, plan options, call lengths, key calls and LDS byte counts: one line per case,
// for tests/test_tx_select.py.  A line is one character per input and output (COLS in the test names them in this order), the LO table's
// length as five digits.  `names`: one line per (geometry, tap classes, arith, mode, force_generic, table) with the whole-pass decision's
// kernel and the name spelled from it.  `eval`: decides the calls given on stdin, one per line.  Host code only: g++ -std=c++17, no HIP.
#include <cstdio>
#include <cstring>

#include "../selenite-lite_amd/csrc/tx_select.h"

using namespace srx;

struct Geo { uint32_t block, interp, ni, nh; };
// the fused geometry and one neighbour in each of block, interp, ni_taps, nh_taps
static const Geo kGeos[] = { { 64, 4, 256, 63 }, { 65, 4, 256, 63 }, { 64, 2, 256, 63 }, { 64, 4, 252, 63 }, { 64, 4, 256, 65 } };
static const uint8_t kModes[] = { SELENITE_MODE_LSB, SELENITE_MODE_USB, SELENITE_MODE_CW, SELENITE_MODE_CWR, SELENITE_MODE_AM,
                                  SELENITE_MODE_DIG, SELENITE_MODE_PKT, SELENITE_MODE_FM, SELENITE_MODE_FM };      // FM with and without fm_set
static const uint32_t kBlocks[] = { 1, 3, 4, 8 };
static const size_t kBelow = 64 * 1024, kAbove = 64 * 1024 + 4;      // the largest layout that runs, the smallest that does not

static selenite_tx_config config(const Geo &s, uint32_t arith, uint8_t mode, int nco)
{
    selenite_tx_config g{};
    g.block = s.block; g.interp = s.interp; g.ni_taps = s.ni; g.nh_taps = s.nh; g.arith = (uint8_t)arith; g.mode = mode; g.nco_enable = (uint8_t)nco;
    return g;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "eval")) {
        unsigned block, interp, ni, nh, imp, odd, arith, mode, nco, same, uni, step0, fg, npl, table, bs, key, lg, lf, lc;
        while (scanf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u", &block, &interp, &ni, &nh, &imp, &odd, &arith, &mode, &nco, &same,
                     &uni, &step0, &fg, &npl, &table, &bs, &key, &lg, &lf, &lc) == 20) {
            TxSelPlan sp;
            sp.delay_is_impulse = imp; sp.hilb_odd_only = odd; sp.table = table; sp.force_generic = fg; sp.no_periodic_lo = npl;
            sp.steps_same = same; sp.step0 = step0;
            TxSelCall c;
            c.block_size = bs; c.key = key; c.phase_uniform = uni; c.lds_generic = lg; c.lds_fm = lf; c.lds_cw = lc;
            const selenite_tx_config g = config(Geo{ block, interp, ni, nh }, arith, (uint8_t)mode, (int)nco);
            const TxDecision d = tx_select(g, sp, c);
            printf("%d %u %u %d %d %s\n", (int)d.kernel, d.nco, d.lo_n, (int)d.clears_uniform, (int)d.refused,
                   tx_kernel_name(tx_select(g, sp, tx_whole_pass_call())));
        }
        return 0;
    }
    const bool names = argc > 1 && !std::strcmp(argv[1], "names");
    for (int gi = 0; gi < 5; ++gi)
    for (int imp = 0; imp < 2; ++imp)
    for (int odd = 0; odd < 2; ++odd)
    for (uint32_t arith = 0; arith < 4; ++arith)      // CMSIS, FMA, SPLIT16 and AUTO (which selenite_tx_init refuses: the rule runs it as FMA)
    for (int mi = 0; mi < 9; ++mi)
    for (int fg = 0; fg < 2; ++fg)
    for (int table = 0; table < 2; ++table) {
        TxSelPlan sp;
        sp.delay_is_impulse = imp; sp.hilb_odd_only = odd; sp.force_generic = fg; sp.table = table;
        if (names) {
            const TxDecision d = tx_select(config(kGeos[gi], arith, kModes[mi], 0), sp, tx_whole_pass_call());
            printf("%d %d %d %u %d %d %d %d %s\n", gi, imp, odd, arith, mi, fg, table, (int)d.kernel, tx_kernel_name(d));
            continue;
        }
        for (int nco = 0; nco < 2; ++nco)
        for (int same = 0; same < 2; ++same)
        for (int uni = 0; uni < 2; ++uni)
        for (int grid = 0; grid < 2; ++grid)          // step0 on the fs / 256 grid, and one bit off it
        for (int npl = 0; npl < 2; ++npl)
        for (int bi = 0; bi < 4; ++bi)
        for (int key = 0; key < 2; ++key)
        for (int lds = 0; lds < 8; ++lds) {           // bit 0: k_tx_generic's layout above the limit, bit 1: k_tx_fm's, bit 2: k_tx_cw's
            sp.steps_same = same; sp.no_periodic_lo = npl; sp.step0 = grid ? 0x03000000u : 0x03000001u;
            TxSelCall c;
            c.block_size = kBlocks[bi] * kGeos[gi].block; c.key = key; c.phase_uniform = uni;
            c.lds_generic = lds & 1 ? kAbove : kBelow; c.lds_fm = lds & 2 ? kAbove : kBelow; c.lds_cw = lds & 4 ? kAbove : kBelow;
            const TxDecision d = tx_select(config(kGeos[gi], arith, kModes[mi], nco), sp, c);
            printf("%d%d%d%u%d%d%d%d%d%d%d%d%u%d%d%d%u%05u%d%d\n", gi, imp, odd, arith, mi, fg, table, nco, same, uni, grid, npl, kBlocks[bi], key, lds,
                   (int)d.kernel, d.nco, d.lo_n, (int)d.clears_uniform, (int)d.refused);
        }
    }
    return 0;
}
