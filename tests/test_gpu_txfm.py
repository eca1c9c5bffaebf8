"""GPU: the FM transmit mode of the TX chain (include/selenite_tx_fm.h, k_tx_fm in csrc/tx_fm.hip) through the C-ABI against the fixture made
from the reference's CMSIS-DSP functions (tests/golden/txfm.npz) and against the oracle (tests/txfm_oracle.py over oracle/tx_oracle.c).
Every comparison is on bits -- output, fir_state, interp_state, alc_gain, nco_phase, tone_phase -- in SELENITE_ARITH_CMSIS and _FMA: the
running sum of the mode is a 32-bit integer, so the kernel's prefix scan and the sequential loop agree exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import rxcommon as rc
import txfm_oracle as fo
from rxcommon import ARITH_CMSIS, ARITH_FMA

pytestmark = pytest.mark.gpu
f32 = np.float32
ARITHS = [ARITH_CMSIS, ARITH_FMA]
FM = rc.MODE_FM


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def gpu_tx(spec):
    import selenite_rx as sr
    return sr.Tx(spec.config())


def fm_pair(spec, dev, amp=1.0, tone_level=0.0, tsteps=None):
    """a GPU instance and the oracle, both configured for FM and switched to it"""
    g = gpu_tx(spec)
    assert g.set_fm(dev, amp, tone_level, tsteps) == 0 and g.set_mode(FM) == 0
    assert g.kernel_name() == "k_tx_fm"
    o = fo.TxFmOracle(spec, dev, amp, tone_level, tsteps)
    o.set_mode(FM)
    return g, o


def full_state(g):
    st = g.state()
    st["tone_phase"] = g.fm_state()["tone_phase"]
    return st


def assert_state_equal(g, o, nan_ok=False):
    sg, so = full_state(g), o.state()
    assert set(sg) == set(so)
    for k in so:
        a, b = sg[k], so[k]
        if nan_ok and a.dtype == np.float32:
            assert np.array_equal(np.isnan(a), np.isnan(b)), "state %s: NaN positions differ" % k
            a, b = np.where(np.isnan(a), f32(0), a), np.where(np.isnan(b), f32(0), b)
        assert same_bits(a, b), "state %s differs" % k


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "txfm.npz")) as z:
        return {k: z[k] for k in z.files}


def tail_instance(gold, name, arith, q15_rounding=False):
    """interp = 1, nh_taps = 0, ALC off: u is the audio.  Three channels with the same stream (every channel must give the fixture)."""
    par, ipar = gold[name + "/par"], gold[name + "/ipar"]
    step, phase0, tone_on, tstep, tphase0 = (int(v) for v in ipar)
    spec = rc.TxSpec(3, block=64, interp=1, ni_taps=0, nh_taps=0, mode=rc.MODE_USB, arith=arith, nco=step != 0, nco_step_all=step, alc=False,
                     q15_rounding=q15_rounding)
    g = gpu_tx(spec)
    assert g.set_fm(float(par[0]), float(par[1]), float(par[2]), tstep if tone_on else None) == 0 and g.set_mode(FM) == 0
    st = g.state()
    st["nco_phase"][:] = phase0
    g.set_state(st)
    g.set_fm_state({"tone_phase": np.full(3, tphase0, np.uint32)})
    return g


NAMES = ("negfrac", "q15", "q15_t", "saturate", "saturate_t", "speech", "speech_t", "zero_if", "zeros", "zeros_t")


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", NAMES)
def test_fixture_tail_f32(gold, name, arith):
    g = tail_instance(gold, name, arith)
    u, want = gold[name + "/u"], gold[name + "/out"]
    got = np.concatenate([g.process(np.tile(u[a:b], (3, 1))) for a, b in ((0, 64), (64, 256))], axis=1)      # the phase carries across calls
    for c in range(3):
        assert same_bits(got[c], want), "channel %d" % c
    assert (g.state()["nco_phase"] == gold[name + "/phase"][-1]).all()
    if gold[name + "/ipar"][2]:
        assert (g.fm_state()["tone_phase"] == gold[name + "/tone_phase"]).all()
    g.close()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("rounding", [False, True])
@pytest.mark.parametrize("name", ["q15", "q15_t"])
def test_fixture_tail_int16(gold, name, rounding, arith):
    g = tail_instance(gold, name, arith, q15_rounding=rounding)
    u = gold[name + "/u"]
    aq = np.round(u.astype(np.float64) * 32768.0).astype(np.int16)
    assert same_bits(aq.astype(f32) / f32(32768.0), u)
    got = g.process_q15(np.tile(aq, (3, 1)))
    want = gold[name + ("/q15_round" if rounding else "/q15_trunc")]
    for c in range(3):
        assert same_bits(got[c], want), "channel %d" % c
    assert (g.state()["nco_phase"] == gold[name + "/phase"][-1]).all()
    g.close()


# 16 outputs (a partial slice) / exactly 64 / one slice per block without filters / 500 = seven slices and a ragged one / the BASELINE-like
# shape, 256 / 96 with L = 3 (output pairs of different interpolator phases)
GEOMETRY = [(8, 2, 2, 1), (16, 4, 16, 0), (64, 1, 0, 0), (100, 5, 35, 3), (64, 4, 256, 63), (32, 3, 45, 15)]
NCO_STEPS = np.array([0x3A5F1C27, 0xC0000001, 0xFFFFFFFF, 0x80000000, 0x7FFFFF01], np.uint32)
TONE_STEPS = np.array([0x0B4E81B5, 0x80000001, 0xFFFFFF01, 0x40000003, 0x00000001], np.uint32)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("block,L,ni,nh", GEOMETRY)
def test_scan_geometry(block, L, ni, nh, arith):
    spec = rc.TxSpec(5, block=block, interp=L, ni_taps=ni, nh_taps=nh, mode=rc.MODE_LSB, arith=arith, nco_steps=NCO_STEPS)
    g, o = fm_pair(spec, 2.5, 0.8, 0.3, TONE_STEPS)
    sat = 0
    for k in range(3):
        a = rc.synth_audio(3, 5, k * 3 * block, 3 * block)
        assert same_bits(g.process(a), o.process(a)), "call %d" % k
        sat += int((o.last_d == 0x7FFFFFFF).sum() + (o.last_d == -0x80000000).sum())
    assert sat > 0, "some v must saturate"
    assert_state_equal(g, o)
    st = o.state()
    assert (st["nco_phase"] != 0).all() and (st["tone_phase"] != 0).all()
    g.close()


@pytest.mark.parametrize("arith", ARITHS)
def test_call_partition(arith):
    block = 32
    spec = rc.TxSpec(5, block=block, interp=3, ni_taps=45, nh_taps=15, arith=arith, nco_steps=NCO_STEPS)
    audio = rc.synth_audio(0, 5, 0, 6 * block)
    runs = []
    for cut in ((1,) * 6, (2, 4), (6,)):
        g = gpu_tx(spec)
        assert g.set_fm(0.7, 0.9, 0.2, TONE_STEPS) == 0 and g.set_mode(FM) == 0
        at, ys = 0, []
        for nb in cut:
            ys.append(g.process(audio[:, at * block:(at + nb) * block]))
            at += nb
        runs.append((np.concatenate(ys, axis=1), full_state(g)))
        g.close()
    for y, st in runs[1:]:
        assert same_bits(y, runs[0][0])
        for k in st:
            assert same_bits(st[k], runs[0][1][k]), k
    o = fo.TxFmOracle(spec, 0.7, 0.9, 0.2, TONE_STEPS)
    o.set_mode(FM)
    assert same_bits(runs[0][0], o.process(audio))


def raw_fm_config(**kw):
    import selenite_rx as sr
    g = sr.TxFmConfig()
    g.struct_size, g.deviation, g.amplitude, g.tone_enable, g.tone_level, g.tone_step_all, g.reserved = C.sizeof(sr.TxFmConfig), 0.3, 1.0, 1, 0.1, 0x01234567, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("arith", ARITHS)
def test_mode_switching_state_and_errors(arith):
    import selenite_rx as sr
    nch, bs = 37, 256
    steps = (np.arange(nch, dtype=np.uint64) * 0x00131313 + 0x00800000).astype(np.uint32)
    tsteps = (np.arange(nch, dtype=np.uint64) * 0x01010101 + 0x00345678).astype(np.uint32)
    spec = rc.TxSpec(nch, block=64, interp=4, ni_taps=256, nh_taps=63, mode=rc.MODE_USB, arith=arith, nco_steps=steps)
    g = gpu_tx(spec)
    assert g.set_mode(FM) == rc.ARGUMENT_ERROR and g.kernel_name() != "k_tx_fm"              # FM before set_fm: refused, mode kept
    with pytest.raises(sr.RxError):
        g.fm_state()
    assert g.set_fm(0.4, 0.9, 0.15, tsteps) == 0
    o = fo.TxFmOracle(spec, 0.4, 0.9, 0.15, tsteps)
    for k, mode in enumerate((rc.MODE_USB, FM, rc.MODE_AM, FM, rc.MODE_USB)):
        assert g.set_mode(mode) == 0
        o.set_mode(mode)
        assert g.kernel_name() == ("k_tx_fm" if mode == FM else "k_tx_fused<4,256,63>")
        a = rc.synth_audio(0, nch, k * bs, bs)
        assert same_bits(g.process(a), o.process(a)), "call %d (mode %d)" % (k, mode)
        assert_state_equal(g, o)
    # checkpoint / resume in FM
    assert g.set_mode(FM) == 0
    o.set_mode(FM)
    snap, a = full_state(g), rc.synth_audio(0, nch, 5 * bs, bs)
    y = g.process(a)
    assert same_bits(y, o.process(a))
    after = full_state(g)
    g.set_state({k: snap[k] for k in ("fir_state", "interp_state", "alc_gain", "nco_phase")})
    g.set_fm_state(snap)
    assert same_bits(g.process(a), y)
    for k in after:
        assert same_bits(full_state(g)[k], after[k]), k
    # a second set_fm retunes and keeps tone_phase; NULL is refused while the mode is FM
    tp = g.fm_state()["tone_phase"]
    assert tp.any()
    assert g.set_fm(0.2, 0.5, 0.05, tsteps[::-1].copy()) == 0
    o.set_fm(0.2, 0.5, 0.05, tsteps[::-1].copy())
    assert same_bits(g.fm_state()["tone_phase"], tp)
    assert g.clear_fm() == rc.ARGUMENT_ERROR and g.kernel_name() == "k_tx_fm"
    # every bad field: ARGUMENT_ERROR, the old setting still active
    L = sr.lib()
    bad = [raw_fm_config(struct_size=36), raw_fm_config(struct_size=0), raw_fm_config(deviation=0.0), raw_fm_config(deviation=-0.3),
           raw_fm_config(deviation=float("nan")), raw_fm_config(deviation=float("inf")), raw_fm_config(amplitude=float("nan")),
           raw_fm_config(amplitude=float("-inf")), raw_fm_config(tone_level=float("nan")), raw_fm_config(tone_level=float("inf")),
           raw_fm_config(tone_enable=2), raw_fm_config(reserved=1)]
    for b in bad:
        assert L.selenite_tx_set_fm(g.h, C.byref(b)) == rc.ARGUMENT_ERROR
    assert g.sync() == 0
    a = rc.synth_audio(0, nch, 6 * bs, bs)
    assert same_bits(g.process(a), o.process(a))
    assert_state_equal(g, o)
    # reset clears both phases; the mode and the FM setting stay
    assert g.reset() == 0
    st = full_state(g)
    assert not st["nco_phase"].any() and not st["tone_phase"].any() and g.kernel_name() == "k_tx_fm"
    o2 = fo.TxFmOracle(spec, 0.2, 0.5, 0.05, tsteps[::-1].copy())
    o2.set_mode(FM)
    assert same_bits(g.process(a), o2.process(a))
    assert_state_equal(g, o2)
    # out of FM, FM off, refused again; on again starts the tone at phase 0
    assert g.set_mode(rc.MODE_USB) == 0 and g.clear_fm() == 0 and g.set_mode(FM) == rc.ARGUMENT_ERROR
    assert g.set_fm(0.2, 0.5, 0.05, tsteps) == 0 and not g.fm_state()["tone_phase"].any()
    g.close()


@pytest.mark.parametrize("arith", ARITHS)
def test_zero_if_int16_and_host_entries_equal_device_entries(arith):
    import selenite_rx as sr
    nch, block, L = 3, 32, 3
    tsteps = TONE_STEPS[:nch].copy()
    for rounding in (False, True):
        spec = rc.TxSpec(nch, block=block, interp=L, ni_taps=45, nh_taps=15, arith=arith, nco=False, q15_rounding=rounding)     # zero-IF FM
        g, o = fm_pair(spec, 0.6, 0.95, 0.2, tsteps)
        gd, _ = fm_pair(spec, 0.6, 0.95, 0.2, tsteps)
        bs = 3 * block
        d_a, d_iq = sr.DeviceBuffer(nch * bs * 4), sr.DeviceBuffer(nch * bs * L * 8)
        for k in range(2):
            a = rc.synth_audio(0, nch, k * bs, bs)
            aq = np.clip(np.trunc(a * 32768.0), -32768, 32767).astype(np.int16)
            if k == 0:
                want = o.process(a)
                assert same_bits(g.process(a), want)
                d_a.upload(a)
                gd.process_device(d_a.ptr, d_iq.ptr, bs)
                assert gd.sync() == 0
                assert same_bits(d_iq.download((nch, bs * L, 2), np.float32), want)
            else:
                want = o.process_q15(aq)
                assert same_bits(g.process_q15(aq), want)
                d_a.upload(aq)
                gd.L.selenite_tx_process_q15_device(gd.h, d_a.ptr, d_iq.ptr, bs)
                assert gd.sync() == 0
                assert same_bits(d_iq.download((nch, bs * L, 2), np.int16), want)
        assert o.state()["nco_phase"].any(), "the phase accumulator runs without the NCO"
        assert_state_equal(g, o)
        assert_state_equal(gd, o)
        g.close()
        gd.close()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("block,L,ni,nh", [(64, 1, 0, 0), (32, 3, 45, 15)])
def test_nan_audio_gives_d_zero_and_raises_nothing(block, L, ni, nh, arith):
    spec = rc.TxSpec(2, block=block, interp=L, ni_taps=ni, nh_taps=nh, arith=arith, nco_step_all=0x0FEDCBA9, alc=False)
    g, o = fm_pair(spec, 0.5, 1.0, 0.1, TONE_STEPS[:2].copy())
    a = rc.synth_audio(0, 2, 0, 2 * block).copy()
    a[0, 5], a[1, block + 7] = np.nan, np.nan
    got, want = g.process(a), o.process(a)
    assert np.isfinite(got).all() and same_bits(got, want)
    reached = np.isnan(fo.TxFmOracle(spec, 0.5).b.process(a)[:, :, 0])              # where the NaN arrives behind the filters
    assert reached.any() and (o.last_d[reached] == 0).all()
    assert g.sync() == 0
    g.check()
    assert_state_equal(g, o, nan_ok=True)
    g.close()


def test_scale_sampled_channels_and_ctcss_read_back_by_the_gpu_receiver():
    """4 099 channels (past any multiple of a workgroup packing), calls of 256 audio samples; sampled channels against the oracle on every
    call; the GPU RX chain in FM mode with the tone detector reads the CTCSS tone sent on three channels (the device form of
    tests/test_txfm_oracle.py::test_ctcss_loopback_reads_the_tone_that_was_sent: 12 kHz audio, frames of 38 x 64 = 2 432 samples)."""
    import selenite_rx as sr
    nch, bs, L, ncalls = 4099, 256, 4, 11
    chans = [0, 1, 63, 64, 4095, 4098]
    hz = sr.ctcss_hz()
    sent = {1: 0, 64: 24, 4098: 49}
    step = 0x01000000
    rng = np.random.default_rng(0x7F4D)
    tsteps = rng.integers(0, 1 << 32, nch, dtype=np.uint64).astype(np.uint32)
    for c, k in sent.items():
        tsteps[c] = sr.tone_step(hz[k], 12000.0 * L)
    audio = rng.uniform(-0.3, 0.3, (nch, ncalls * bs)).astype(f32)
    spec = rc.TxSpec(nch, alc=False, nco_step_all=step)
    g = gpu_tx(spec)
    assert g.set_fm(0.05, 1.0, 0.1, tsteps) == 0 and g.set_mode(FM) == 0
    o = fo.TxFmOracle(rc.TxSpec(len(chans), alc=False, nco_step_all=step), 0.05, 1.0, 0.1, tsteps[chans])
    o.set_mode(FM)
    rx = sr.Rx(rc.ChainSpec(nch, 256, 4, 256, 63, 0, rc.MODE_FM, ARITH_CMSIS, nco=True, nco_step_all=step, agc=False).config())
    d_a, d_iq, d_y = sr.DeviceBuffer(nch * bs * 4), sr.DeviceBuffer(nch * bs * L * 8), sr.DeviceBuffer(nch * bs * 4)
    for k in range(ncalls):
        a = np.ascontiguousarray(audio[:, k * bs:(k + 1) * bs])
        d_a.upload(a)
        g.process_device(d_a.ptr, d_iq.ptr, bs)
        assert g.sync() == 0
        iq = d_iq.download((nch, bs * L, 2), np.float32)
        assert same_bits(iq[chans], o.process(a[chans])), "call %d" % k
        if k == 1:                                               # the receiver's filters are full: frames count from here
            rx.set_tones(sr.design_tones(hz / 12000.0), frame_blocks=38, confirm=1, release=1, ratio=0.02, min_power=0.0)
        rx.process_device(d_iq.ptr, d_y.ptr, bs * L)
        rx.sync()
        rx.check()
    st, so = full_state(g), o.state()
    for key in so:
        assert same_bits(st[key][chans], so[key]), key
    tone, _, frames = rx.tones()
    assert frames == 1
    assert [int(tone[c]) for c in sent] == list(sent.values())
    g.close()
    rx.close()
