"""k_tx_split16 across a channel switch.

The kernel (csrc/tx_fused.hip, SELENITE_ARITH_SPLIT16 for TX) is persistent: launch_s16 sizes the grid to what the device keeps
resident (8 single-wave workgroups x 256 CUs = 2048 on an MI355X, at most 2304 if the LDS were the limit) and a workgroup runs
channels b, b + grid, b + 2 grid, ...  Between two channels it loads the next channel's streaming state into registers right
after installing the present one, prefetches the next channel's first 256 audio samples in the present channel's last pass,
writes the present channel's state back, installs the Hilbert-pair and interpolator histories into LDS again, resets the block
exponent, and carries on with the Toeplitz fragments, the Hilbert taps, the periodic LO registers and the zeroed image slack of
the workgroup.  With a few dozen channels every channel is the first and the last of its workgroup and none of that code is
ever between two channels; here a workgroup owns three or four: 6 200 channels, more than twice any grid the launch can choose
and no multiple of it.

The channels repeat 64 signals (channel c carries signal c % 64; every possible grid is a multiple of 64, so the channels of one
workgroup are copies of one signal).  What a channel computes depends on its own samples and state only -- the block exponent
comes from its own wave's data -- so every channel must give the bits of its twin in a 64-channel instance of the same spec,
where no workgroup has a second channel: the output of every call and the four state arrays, whatever the grid is (it is neither
pinned nor read here).

A batch of this size is also the first in the suite that puts two of this kernel's waves on one SIMD.  That, not the hand-over, is what
these cases caught first: the up-mix behind the transpose, packed by the compiler into v_pk_mul_f32 / v_pk_add_f32, left the first
product alone in I of a store's second output, lanes 48 to 63, in up to 70 channels of 6 200 per call and at any place of the sequence
(13 of these 19 cases failed; cmul_np in csrc/tx_fused.hip, profiles/tx_handover/README.md)."""
import numpy as np
import pytest

import rxcommon as rc
from rxcommon import ARITH_CMSIS, ARITH_FMA, ARITH_SPLIT16, bits_equal

pytestmark = pytest.mark.gpu

NCH, TWIN = 6200, 64
# workgroups of the persistent launch on an MI355X; the copies k, k + GRID, k + 2 GRID (, k + 3 GRID) are then the channels of one
# workgroup (on a device with another grid they are still copies, and the twin comparison covers every channel whatever the grid)
GRID = 2048
# the first workgroups, the last one that has a fourth channel and the first that has not (6200 - 3 * 2048 = 56), the last signal,
# the last workgroup
COPIES = (0, 1, 55, 56, 63, 2047)
PAST = 2100                                   # a batch just past the grid: 52 workgroups run a second channel, the rest end after one
KERNEL = "k_tx_split16<4,256,63>"
STATE_KEYS = ("fir_state", "interp_state", "alc_gain", "nco_phase")
TOL = 1e-5                                    # of the block maximum per 256 complex output samples (tests/test_gpu_tx.py)
ODD_STEP = 0x0FEDCBA9                         # a shared LO that is not periodic in 256: the per-call table
# per-channel NCO: the step of a channel is the step of its signal
STEPS64 = (np.arange(TWIN, dtype=np.uint64) * 0x00100101 + 0x00400000).astype(np.uint32)
NCO = {"off": dict(nco=False), "periodic": dict(), "table": dict(nco_step_all=ODD_STEP), "per_channel": dict(nco_steps=STEPS64)}

_base = {}


def base_audio(pos, bs):
    """the 64 signals, samples [pos, pos + bs): computed once per window"""
    if (pos, bs) not in _base:
        a = rc.synth_audio(0, TWIN, pos, bs)
        a.setflags(write=False)
        _base[(pos, bs)] = a
    return _base[(pos, bs)]


def to_q15(a):
    return np.clip(np.trunc(a * 32768.0), -32768, 32767).astype(np.int16)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return bits_equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def differing(a, b):
    """the first few rows of a and b that differ in some bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0][:8]


def spec_of(arith=ARITH_SPLIT16, **kw):
    """make(nch, idx): the TxSpec of an instance whose channel c carries signal idx[c] (default shape: block 64, interpolate by 4,
    256 taps, 63-tap Hilbert pair)"""
    return lambda nch, idx: rc.TxSpec(nch, arith=arith, **{k: (v[idx] if k == "nco_steps" else v) for k, v in kw.items()})


def run_pair(make, bs, ncalls, q15=False, nch=NCH, amp=None, start=None):
    """`ncalls` calls of `bs` samples through an instance of `nch` channels and through its 64-channel twin.  amp: (per-channel scale
    of the big instance, per-signal scale of the twin); start: the streaming state of the 64 signals before the first call.
    Returns both instances, the output of every call and the state of both, and the twin's input of every call."""
    import selenite_rx as sr
    idx = np.arange(nch) % TWIN
    big, twin = sr.Tx(make(nch, idx).config()), sr.Tx(make(TWIN, np.arange(TWIN)).config())
    assert big.kernel_name() == KERNEL and twin.kernel_name() == KERNEL, (big.kernel_name(), twin.kernel_name())
    if start is not None:
        big.set_state({k: v[idx] for k, v in start.items()})
        twin.set_state(start)
    yb, yt, xs = [], [], []
    for call in range(ncalls):
        xt = base_audio(call * bs, bs)
        xb = xt[idx]
        if amp is not None:
            xb = (xb * amp[0][:, None]).astype(np.float32)
            xt = (xt * amp[1][:, None]).astype(np.float32)
        xs.append(xt)
        if q15:
            yb.append(big.process_q15(to_q15(xb))); yt.append(twin.process_q15(to_q15(xt)))
        else:
            yb.append(big.process(xb)); yt.append(twin.process(xt))
        assert big.kernel_name() == KERNEL and twin.kernel_name() == KERNEL, (call, big.kernel_name(), twin.kernel_name())
    return big, twin, yb, yt, big.state(), twin.state(), xs


def assert_twins(yb, yt, sb, st, rows=None):
    """channel c of the big instance == signal c % 64 of the twin: the output of every call and the streaming state, bit for bit
    (rows: only these channels of the big instance)"""
    rows = np.arange(len(yb[0])) if rows is None else rows
    idx = rows % TWIN
    for call, (a, b) in enumerate(zip(yb, yt)):
        assert same_bits(a[rows], b[idx]), ("output", call, "channels", rows[differing(a[rows], b[idx])])
    for key in STATE_KEYS:
        assert same_bits(sb[key][rows], st[key][idx]), (key, "channels", rows[differing(sb[key][rows], st[key][idx])])


def assert_copies(yb, sb, copies=COPIES):
    """the copies of a signal -- first, second, third (and fourth) channel of one workgroup of a 2048 grid -- are equal bit for bit"""
    nch = len(yb[0])
    for k in copies:
        assert 0 <= k < GRID and k + GRID < nch
        for other in range(k + GRID, nch, GRID):
            for call, a in enumerate(yb):
                assert same_bits(a[k], a[other]), ("output", call, k, other)
            for key in STATE_KEYS:
                assert same_bits(sb[key][k], sb[key][other]), (key, k, other)


def block_error(y, want):
    """(worst error of y against want as a part of the block maximum, every block within TOL), blocks of 256 complex output samples"""
    y, want = y.astype(np.float64), want.astype(np.float64)
    nb = want.shape[1] // 256
    d = np.abs(y - want).reshape(len(want), nb, -1).max(axis=2)
    m = np.abs(want).reshape(len(want), nb, -1).max(axis=2)
    return float((d / np.maximum(m, 1e-30)).max()), bool((d <= TOL * m).all())


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("nco", sorted(NCO))
def test_every_nco_instantiation_both_slot_types(nco, q15):
    """NCO off, the periodic shared LO in registers, the shared LO from the per-call table, the per-channel NCO; f32 and int16 slots.
    Two calls of 512 = two passes each: the next channel's samples are prefetched in a pass that is not the first, and the second
    call starts from the state the first one wrote behind a channel switch.

    The periodic-LO f32 case also anchors the twin to the oracle (the assertions of test_tx_split16_interpolator_on_the_matrix_pipe):
    ALC gain, NCO phase and Hilbert-pair state of the CMSIS arithmetic and the interpolator state of the FMA arithmetic bit for bit,
    the output within 1e-5 of the block maximum per 256 output samples -- and through the twin equality so do all 6 200 channels."""
    bs, ncalls = 512, 2
    big, twin, yb, yt, sb, st, xs = run_pair(spec_of(**NCO[nco]), bs, ncalls, q15)
    assert_copies(yb, sb)
    assert_twins(yb, yt, sb, st)
    if nco == "periodic" and not q15:
        every = np.arange(TWIN)
        assert twin.cfg.nco_step_all & 0x00FFFFFF == 0
        oc, of = rc.TxCpuChain(spec_of(ARITH_CMSIS)(TWIN, every), "orc"), rc.TxCpuChain(spec_of(ARITH_FMA)(TWIN, every), "orc")
        worst = 0.0
        for call in range(ncalls):
            want = oc.process(xs[call])
            of.process(xs[call])
            err, ok = block_error(yt[call], want)
            worst = max(worst, err)
            assert np.isfinite(yt[call]).all() and ok, (call, err)
        print("tx hand-over, twin against the CMSIS arithmetic: worst per-block error %.3g of the block maximum (bar %g)" % (worst, TOL))
        so, sf = oc.state(), of.state()
        assert bits_equal(st["alc_gain"], so["alc_gain"]) and np.array_equal(st["nco_phase"], so["nco_phase"])
        assert bits_equal(st["fir_state"], so["fir_state"])
        assert bits_equal(st["interp_state"], sf["interp_state"])
    big.close(); twin.close()


@pytest.mark.parametrize("bs", [256, 1024])
def test_passes_per_channel(bs):
    """256: one pass, the prefetch of the next channel's samples and the install of its state share the channel's only pass;
    1024: four passes.  Periodic LO, f32, two calls."""
    big, twin, yb, yt, sb, st, _ = run_pair(spec_of(), bs, 2)
    assert_copies(yb, sb)
    assert_twins(yb, yt, sb, st)
    big.close(); twin.close()


@pytest.mark.parametrize("flavour", ["no_alc", "am", "lsb"])
def test_flavours_of_the_body(flavour):
    """ALC off (the gain register stays 1), AM (carrier, no Q rail), LSB (the Q rail's sign): two calls of 512, f32."""
    kw = {"no_alc": dict(alc=False), "am": dict(mode=rc.MODE_AM), "lsb": dict(mode=rc.MODE_LSB)}[flavour]
    big, twin, yb, yt, sb, st, _ = run_pair(spec_of(**kw), 512, 2)
    assert_copies(yb, sb)
    assert_twins(yb, yt, sb, st)
    big.close(); twin.close()


def test_a_channel_installs_its_own_row_of_a_non_uniform_start():
    """set_state before the first call: per-signal NCO phase, ALC gain away from 1 inside [gain_min, gain_max], random finite filter
    histories; per-channel NCO.  A channel that installed a neighbour's row (or its predecessor's registers) would differ from its twin."""
    rng = np.random.default_rng(0x7A11)
    make = spec_of(**NCO["per_channel"])
    spec = make(TWIN, np.arange(TWIN))
    start = spec.state_arrays()
    lo, hi = spec.alc_params["gain_min"], spec.alc_params["gain_max"]
    start["fir_state"][:] = rng.uniform(-0.9, 0.9, start["fir_state"].shape)
    start["interp_state"][:] = rng.uniform(-0.9, 0.9, start["interp_state"].shape)
    start["alc_gain"][:] = np.exp(rng.uniform(np.log(2 * lo), np.log(hi / 2), TWIN))
    start["nco_phase"][:] = rng.integers(1, 2 ** 32, TWIN, dtype=np.uint64).astype(np.uint32)
    assert ((start["alc_gain"] >= lo) & (start["alc_gain"] <= hi) & (start["alc_gain"] != 1.0)).all() and (start["nco_phase"] != 0).all()
    assert len(np.unique(start["nco_phase"])) == TWIN and len(np.unique(start["alc_gain"])) == TWIN
    big, twin, yb, yt, sb, st, _ = run_pair(make, 512, 2, start=start)
    assert_copies(yb, sb)
    assert_twins(yb, yt, sb, st)
    big.close(); twin.close()


@pytest.mark.parametrize("alc", [False, True], ids=["alc_off", "alc_on"])
@pytest.mark.parametrize("scale", [1e-6, 1e+6])
def test_level_step_at_the_channel_switch(scale, alc):
    """Loud channels k, then channels k + 2048 at `scale` times their level, then loud ones again; three calls of one pass.  A block
    exponent or a gain that leaked across the switch would show: the scaled channels equal a 64-channel twin fed the scaled signals
    bit for bit (and the loud ones a twin fed the loud signals), and every channel of both levels stays within 1e-5 of the block
    maximum per 256 output samples of the CMSIS arithmetic (test_tx_amplitude_sweep: the kernel holds that from 1e-30 to 1e6)."""
    import selenite_rx as sr
    bs, ncalls = 256, 3
    amp = np.ones(NCH, np.float32)
    amp[GRID:2 * GRID] = np.float32(scale)
    quiet, loud = np.arange(GRID, 2 * GRID), np.nonzero(amp == np.float32(1.0))[0]
    assert len(quiet) + len(loud) == NCH
    big, twin, yb, yt, sb, st, xs = run_pair(spec_of(alc=alc), bs, ncalls, amp=(amp, np.full(TWIN, scale, np.float32)))
    assert_twins(yb, yt, sb, st, rows=quiet)
    ref = sr.Tx(spec_of(alc=alc)(TWIN, np.arange(TWIN)).config())      # the loud signals' twin
    yl = [ref.process(base_audio(call * bs, bs)) for call in range(ncalls)]
    assert ref.kernel_name() == KERNEL
    assert_twins(yb, yl, sb, ref.state(), rows=loud)
    for level, rows, x in ((1.0, loud, [base_audio(call * bs, bs) for call in range(ncalls)]), (scale, quiet, xs)):
        orc = rc.TxCpuChain(spec_of(ARITH_CMSIS, alc=alc)(TWIN, np.arange(TWIN)), "orc")
        worst = 0.0
        for call in range(ncalls):
            want = orc.process(x[call])[rows % TWIN]
            err, ok = block_error(yb[call][rows], want)
            worst = max(worst, err)
            assert np.isfinite(yb[call][rows]).all() and ok, (level, call, err)
        print("tx hand-over, level step %g, alc %d, channels at level %g: worst per-block error %.3g of the block maximum (bar %g)"
              % (scale, alc, level, worst, TOL))
    big.close(); twin.close(); ref.close()


def test_a_batch_just_past_the_grid():
    """2 100 channels: on the 2048 grid 52 workgroups run a second channel while the rest end after one -- the `cn == c` re-read of
    a channel's own state and samples right beside a real hand-over.  Two calls of one pass."""
    big, twin, yb, yt, sb, st, _ = run_pair(spec_of(), 256, 2, nch=PAST)
    assert_copies(yb, sb, copies=(0, 1, PAST - GRID - 1))
    assert_twins(yb, yt, sb, st)
    big.close(); twin.close()
