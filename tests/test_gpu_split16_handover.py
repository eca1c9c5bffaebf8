"""k_ssb_split16 across a channel switch.

The kernel is persistent: a workgroup runs channels b, b + grid, b + 2 grid, ... and loads the streaming state of its next
channel (dec_state, fir_state, phase, gain, the AUTO word) while the present one is in its last pass, writes the present
channel's state and guard words back, and goes on.  With a few dozen channels every channel is the first and the last of its
workgroup and none of that code is ever between two channels; here a workgroup owns at least three: 6 200 channels, more
than 3 x the 2048-workgroup grid of an MI355X and no multiple of it.

The channels repeat 64 signals (channel c carries signal c % 64, so c, c + 2048 and c + 4096 are copies of one another):
what a channel computes must not depend on its place in its workgroup's sequence, so every channel must give the bits of
its twin in a 64-channel instance, where no workgroup has a second channel."""
import numpy as np
import pytest

import rxcommon as rc
from rxcommon import ARITH_AUTO, ARITH_CMSIS, ARITH_SPLIT16, CpuChain, bits_equal, synth_iq

pytestmark = pytest.mark.gpu

NCH, TWIN = 6200, 64
# workgroups of the persistent launch on an MI355X (256 CUs x 4 SIMDs x 2 waves); GRID % 64 == 0, so the channels of one workgroup are copies
# of one signal.  (On a device with another grid the copies are still copies, only not of one workgroup; the twin comparison covers every
# channel whatever the grid.)
GRID = 2048
# first channels k of a workgroup whose copies k + GRID, k + 2 GRID (, k + 3 GRID) are compared: the first workgroups, the last one that has
# a fourth channel and the first that has not, the last workgroup
COPIES = (0, 1, NCH - 3 * GRID - 1, NCH - 3 * GRID, 63, GRID - 1)
GRID_STEP = 0x01000000                        # NCO step fs / 256
STATE_KEYS = ("dec_state", "fir_state", "nco_phase", "agc_gain")
IDX = np.arange(NCH) % TWIN

_base = {}


def base_iq(pos, bs):
    """the 64 signals, samples [pos, pos + bs): computed once per window"""
    if (pos, bs) not in _base:
        a = synth_iq(0, TWIN, pos, bs)
        a.setflags(write=False)
        _base[(pos, bs)] = a
    return _base[(pos, bs)]


def to_q15(iq):
    return np.clip(np.trunc(iq * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return bits_equal(a, b)
    return a.shape == b.shape and np.array_equal(a, b)


def run_pair(make_spec, bs, ncalls, q15=False, amp=None, kernel="k_ssb_split16"):
    """`ncalls` calls of `bs` samples through an instance of NCH channels and through its 64-channel twin (make_spec(nch, idx):
    idx = the signal of every channel); amp: per-signal-copy scale, amp[c] for the big instance and amp64 for the twin.
    Returns (audio of every call, state) of both."""
    import selenite_rx as sr
    big, twin = sr.Rx(make_spec(NCH, IDX).config()), sr.Rx(make_spec(TWIN, np.arange(TWIN)).config())
    assert big.kernel_name().startswith(kernel) and twin.kernel_name().startswith(kernel), (big.kernel_name(), twin.kernel_name())
    yb, yt = [], []
    for call in range(ncalls):
        b = base_iq(call * bs, bs)
        xb, xt = b[IDX], b
        if amp is not None:
            xb = (xb * amp[0][:, None, None]).astype(np.float32)
            xt = (xt * np.float32(amp[1])).astype(np.float32)
        if q15:
            yb.append(big.process_q15(to_q15(xb))); yt.append(twin.process_q15(to_q15(xt)))
        else:
            yb.append(big.process(xb)); yt.append(twin.process(xt))
    sb, st = big.state(), twin.state()
    return big, twin, yb, yt, sb, st


def assert_twins(yb, yt, sb, st, rows=None):
    """channel c of the big instance == signal c % 64 of the twin, audio of every call and the streaming state, bit for bit
    (rows: only these channels of the big instance)"""
    rows = np.arange(NCH) if rows is None else rows
    for call, (a, b) in enumerate(zip(yb, yt)):
        assert same_bits(a[rows], b[IDX[rows]]), ("audio", call, np.nonzero((a[rows] != b[IDX[rows]]).any(axis=1))[0][:8])
    for key in STATE_KEYS:
        assert same_bits(sb[key][rows], st[key][IDX[rows]]), key


def assert_copies(yb, sb):
    """the copies of a signal -- first, second, third (and fourth) channel of one workgroup -- are equal bit for bit"""
    for k in COPIES:
        assert 0 <= k < GRID and k + 2 * GRID < NCH
        for other in range(k + GRID, NCH, GRID):
            for call, a in enumerate(yb):
                assert same_bits(a[k], a[other]), ("audio", call, k, other)
            for key in STATE_KEYS:
                assert same_bits(sb[key][k], sb[key][other]), (key, k, other)


def cfg3(arith, block=256, decim=4, mode=rc.MODE_USB, **kw):
    kw.setdefault("nco", True)
    if "nco_steps" not in kw:
        kw.setdefault("nco_step_all", GRID_STEP)
    return lambda nch, idx: rc.ChainSpec(nch, block, decim, 256, 63, 0, mode, arith,
                                         **{k: (v[idx] if k == "nco_steps" else v) for k, v in kw.items()})


# 1024: one pass per channel; 2048, 4096: two and four; 2304: a partial last pass of 256 inputs (a whole decimator history);
# 768 in DSP blocks of 96: passes of 240 outputs, the run-time geometry
@pytest.mark.parametrize("q15", [False, True])
@pytest.mark.parametrize("bs,block", [(1024, 256), (2048, 256), (4096, 256), (2304, 256), (768, 96)])
def test_a_channels_bits_do_not_depend_on_its_place_in_the_sequence(bs, block, q15):
    """cfg3 chain, raw SELENITE_ARITH_SPLIT16 (bit-invariant by construction), two calls (the second starts from the state the
    first one wrote behind a channel switch)."""
    big, twin, yb, yt, sb, st = run_pair(cfg3(ARITH_SPLIT16, block), bs, 2, q15)
    assert_copies(yb, sb)
    assert_twins(yb, yt, sb, st)
    big.close(); twin.close()


def test_mixed_neighbours_in_auto():
    """SELENITE_ARITH_AUTO, per-channel NCO steps with three channels in four out of band (guarded, recomputed, then held by the exact
    kernel): held and skipped channels sit between kept ones in every workgroup's sequence.  Four calls of 2048: every DSP block
    within the plain 1e-5 bar of the CMSIS arithmetic, no handover block, and the same bits with the rerun grid pinned to 64
    workgroups (the result does not depend on timing)."""
    import selenite_rx as sr
    steps = np.where(np.arange(NCH) % 4 == 0, GRID_STEP, 0x40000000).astype(np.uint32)
    assert TWIN % 4 == 0                      # the step of a channel is the step of its signal's twin
    bs, ncalls, na = 2048, 4, 64
    orc = CpuChain(rc.ChainSpec(TWIN, 256, 4, 256, 63, 0, rc.MODE_USB, ARITH_CMSIS, nco=True, nco_steps=steps[:TWIN]), "orc")
    want = [orc.process(base_iq(call * bs, bs)).astype(np.float64) for call in range(ncalls)]
    orc.close()
    runs = []
    for grid in (0, 64):
        assert sr.lib().selenite_rx_set_plan_option(sr.OPT_RERUN_GRID, grid) == 0
        try:
            g = sr.Rx(rc.ChainSpec(NCH, 256, 4, 256, 63, 0, rc.MODE_USB, ARITH_AUTO, nco=True, nco_steps=steps).config())
            assert g.kernel_name().startswith("k_ssb_split16"), g.kernel_name()
            ys = [g.process(base_iq(call * bs, bs)[IDX]) for call in range(ncalls)]
            stats, words, state = g.guard_stats(), g.auto_words(), g.state()
            g.close()
        finally:
            sr.lib().selenite_rx_set_plan_option(sr.OPT_RERUN_GRID, 0)
        runs.append((ys, state, words))
        worst = 0.0
        for call, y in enumerate(ys):
            w = want[call][IDX]
            d = np.abs(y.astype(np.float64) - w).reshape(NCH, -1, na).max(axis=2)
            m = np.abs(w).reshape(NCH, -1, na).max(axis=2)
            worst = max(worst, float((d / np.maximum(m, 1e-30)).max()))
            assert (d <= 1e-5 * m).all(), (grid, call, worst)
        print("rerun grid %d: worst per-block error %.3g of the block maximum (bar 1e-5); %s" % (grid, worst, stats))
        assert stats["handover_blocks"] == 0
        assert stats["rerun_channel_calls"] >= 3 * int((steps != GRID_STEP).sum())      # the out-of-band channels were recomputed (held from the second call on)
    (ya, sa, wa), (yb, sb, wb) = runs
    for call in range(ncalls):
        assert same_bits(ya[call], yb[call]), call
    for key in STATE_KEYS:
        assert same_bits(sa[key], sb[key]), key
    assert np.array_equal(wa, wb)


@pytest.mark.parametrize("scale", [1e-6, 1e+6])
def test_level_step_at_the_channel_switch(scale):
    """Loud channels k, then channels k + 2048 at `scale` times their level, then loud ones again, raw SPLIT16, three calls of one
    pass: block exponents, guard thresholds or gain leaking across the switch would show.  Bar: 1e-5 of the block maximum per DSP
    block against the CMSIS arithmetic (tests/test_gpu_dynamic_range.py); the scaled channels equal their 64-channel twins bit for bit."""
    amp = np.ones(NCH, np.float32)
    amp[GRID:2 * GRID] = np.float32(scale)
    bs, ncalls, na = 1024, 3, 64
    big, twin, yb, yt, sb, st = run_pair(cfg3(ARITH_SPLIT16), bs, ncalls, amp=(amp, scale))
    assert_twins(yb, yt, sb, st, rows=np.arange(GRID, 2 * GRID))
    for level in (1.0, scale):
        orc = CpuChain(cfg3(ARITH_CMSIS)(TWIN, np.arange(TWIN)), "orc")
        rows = np.nonzero(amp == np.float32(level))[0]
        for call in range(ncalls):
            w = orc.process((base_iq(call * bs, bs) * np.float32(level)).astype(np.float32)).astype(np.float64)[IDX[rows]]
            d = np.abs(yb[call][rows].astype(np.float64) - w).reshape(len(rows), -1, na).max(axis=2)
            m = np.abs(w).reshape(len(rows), -1, na).max(axis=2)
            assert (d <= 1e-5 * m).all(), (level, call, float((d / np.maximum(m, 1e-30)).max()))
        orc.close()
    big.close(); twin.close()


@pytest.mark.parametrize("flavour", ["am", "fm", "by8"])
def test_further_flavours(flavour):
    """AM (the Hilbert-pair state stays), FM (the AM instantiation with the delay lines running; SELENITE_ARITH_AUTO only) and
    decimation by 8 (its own instantiation): the same twin comparison, two calls of 2048."""
    make = {"am": cfg3(ARITH_SPLIT16, mode=rc.MODE_AM), "fm": cfg3(ARITH_AUTO, mode=rc.MODE_FM), "by8": cfg3(ARITH_SPLIT16, decim=8)}[flavour]
    big, twin, yb, yt, sb, st = run_pair(make, 2048, 2)
    assert_copies(yb, sb)
    assert_twins(yb, yt, sb, st)
    if flavour == "fm":
        assert np.array_equal(big.auto_words(), twin.auto_words()[IDX])
    big.close(); twin.close()
