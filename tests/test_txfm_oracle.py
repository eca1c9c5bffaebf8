"""CPU: the numpy restatement of the TX chain's FM mode (tests/txfm_oracle.py) against the fixture made from the reference's CMSIS-DSP
functions (tests/golden/txfm.npz, tests/golden/make_txfm_golden.py), and what the mode is for: this chain's own FM demodulator gives the
modulating signal back, and its tone detector reads the CTCSS tone that was sent."""
import copy
import os

import numpy as np
import pytest

import gain_law_cases as gl
import rxcommon as rc
import selenite_rx as sr
import tones_oracle as to
import tx_fuzz_cases as fz
import txfm_oracle as fo

f32 = np.float32
NAMES = ("negfrac", "q15", "q15_t", "saturate", "saturate_t", "speech", "speech_t", "zero_if", "zeros", "zeros_t")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "txfm.npz")) as z:
        return {k: z[k] for k in z.files}


def stream(gold, name):
    g = {k: gold[name + "/" + k] for k in ("u", "par", "ipar", "d", "phase", "out", "q15_trunc", "q15_round", "tone_phase")}
    par, ipar = g["par"], g["ipar"]
    g["kw"] = dict(phase=ipar[1], step=ipar[0], deviation=par[0], amplitude=par[1], tone_phase=ipar[4], tone_step=ipar[3], tone_on=bool(ipar[2]),
                   tone_level=par[2])
    return g


def test_fixture_holds_the_issue_cases(gold):
    assert tuple(gold["names"]) == NAMES
    for name in NAMES:
        g = stream(gold, name)
        assert np.isfinite(g["u"]).all() and np.isfinite(g["out"]).all() and g["u"].dtype == f32 and g["d"].dtype == np.int32
    z = stream(gold, "zeros")["u"]
    assert ((z == 0) & ~np.signbit(z)).any() and ((z == 0) & np.signbit(z)).any()
    assert ((z != 0) & (np.abs(z) < f32(1.1754944e-38))).any(), "denormals"
    s = stream(gold, "saturate")
    v = s["u"] * s["par"][0]
    assert (s["d"] == 0x7FFFFFFF).any() and (s["d"] == -0x80000000).any()
    assert ((v < 1) & (v > f32(0.9999))).any() and ((v > 1) & (v < f32(1.0001))).any() and ((v > -1) & (v < f32(-0.9999))).any() and \
        ((v < -1) & (v > f32(-1.0001))).any(), "just under and over +-1"
    n = stream(gold, "negfrac")
    x = n["u"].astype(np.float64) * 2147483648.0
    neg = x < 0
    assert neg.any() and (x[neg] != np.floor(x[neg])).all()
    assert np.array_equal(n["d"][neg], np.trunc(x[neg]).astype(np.int32)) and (n["d"][neg] == np.floor(x[neg]).astype(np.int32) + 1).all(), "toward zero"
    for name, key, step in (("speech", "phase", 0), ("speech_t", "phase", 0)):
        assert (np.diff(stream(gold, name)[key].astype(np.int64)) < 0).sum() >= 3, "the phase wraps several times"
    t = stream(gold, "speech_t")
    assert 256 * int(t["ipar"][3]) + int(t["ipar"][4]) >= 3 << 32, "tone_phase wraps several times"
    assert {bool(stream(gold, k)["ipar"][2]) for k in NAMES} == {False, True}
    assert os.path.getsize(os.path.join(rc.GOLDEN_DIR, "txfm.npz")) < 100 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference_on_bits(gold, name):
    g = stream(gold, name)
    r = fo.fm_tail(g["u"], **g["kw"])
    assert rc.identical(r["d"], g["d"])
    assert rc.identical(r["phase"], g["phase"])
    assert rc.identical(r["out"], g["out"])
    assert int(r["tone_phase"]) == int(g["tone_phase"])
    assert rc.identical(fo.float_to_q15(r["out"], 0), g["q15_trunc"]) and rc.identical(fo.float_to_q15(r["out"], 1), g["q15_round"])
    s = fo.fm_tail_sequential(g["u"][:70], **g["kw"])              # the prefix sums are the sequential loop
    assert rc.identical(s["d"], g["d"][:70]) and rc.identical(s["phase"], g["phase"][:70]) and rc.identical(s["out"], g["out"][:70])


@pytest.mark.parametrize("name", NAMES)
def test_the_final_phase_is_the_integer_sum(gold, name):
    g = stream(gold, name)
    r = fo.fm_tail(g["u"], **g["kw"])
    total = int(g["ipar"][1]) + sum(int(d) for d in r["d"]) + len(r["d"]) * int(g["ipar"][0])
    assert int(r["phase"][-1]) == total % (1 << 32) == int(g["phase"][-1])


def fm_spec(ch, block, L, ni, nh, arith=rc.ARITH_CMSIS, **kw):
    return rc.TxSpec(ch, block=block, interp=L, ni_taps=ni, nh_taps=nh, mode=rc.MODE_USB, arith=arith, **kw)


def states_identical(a, b):
    return all(rc.identical(a[k], b[k]) for k in a) and set(a) == set(b)


@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_FMA])
def test_calls_of_any_cut_give_the_same_output_and_state(arith):
    ch, block, L = 3, 32, 3
    steps = np.array([0x3A5F1C27, 0xC0000001, 0x00000000], np.uint32)
    tsteps = np.array([0x0B4E81B5, 0x80000001, 0xFFFFFF01], np.uint32)
    audio = rc.synth_audio(0, ch, 0, 6 * block)
    runs = []
    for cut in ((1,) * 6, (2, 4), (6,)):
        o = fo.TxFmOracle(fm_spec(ch, block, L, 45, 15, arith, nco_steps=steps), 0.7, 0.9, 0.2, tsteps)
        o.set_mode(rc.MODE_FM)
        at, ys = 0, []
        for nb in cut:
            ys.append(o.process(audio[:, at * block:(at + nb) * block]))
            at += nb
        runs.append((np.concatenate(ys, axis=1), o.state()))
    for y, st in runs[1:]:
        assert rc.identical(y, runs[0][0]) and states_identical(st, runs[0][1])
    assert (runs[0][1]["nco_phase"] != 0).all() and (runs[0][1]["tone_phase"] != 0).all()


# ---- the oracle's face for call sequences (tests/test_gpu_tx_fuzz.py), on the fuzz generator's own shapes ----
PIN_CASES = 40


def pin_specs():
    """the fuzz generator's first 40 specs (taps overwritten as the cases say: moved impulse, odd-distance values, dense FIRs),
    each with the NCO, q15_rounding and arithmetic the case drew -- SPLIT16 runs as FMA here"""
    out = []
    for case in fz.cases(fz.SEED, PIN_CASES // 2, None):
        if case["kind"] == "FM":
            continue
        spec = fz.build_spec(case)
        if spec.arith == rc.ARITH_SPLIT16:
            spec.arith = rc.ARITH_FMA
        if spec.channels > 5:                      # channels are independent streams: five of them, to keep this a quick CPU test
            spec.channels = 5
            spec.nco_steps = None if spec.nco_steps is None else spec.nco_steps[:5].copy()
        out.append((case, spec))
    assert len(out) == PIN_CASES
    return out


def pin_audio(case, spec, k, q15):
    a = rc.synth_audio(k, spec.channels, 100 * k, (3 - k) * spec.block)
    return gl.to_q15(a) if q15 else a


def test_pin_specs_cover_both_values_of_every_switch():
    specs = [s for _, s in pin_specs()]
    assert {s.nco for s in specs} == {False, True} and {s.q15_rounding for s in specs} == {False, True}
    assert {s.arith for s in specs} == {rc.ARITH_CMSIS, rc.ARITH_FMA} and {s.alc for s in specs} == {False, True}
    assert any(s.nco_steps is not None for s in specs) and any(s.interp == 1 for s in specs) and any(s.nh_taps == 0 for s in specs)
    taps = {c["taps"][k][0] for c, _ in pin_specs() for k in ("delay", "hilb", "ic")}
    assert taps >= {"designed", "impulse", "odd", "dense"}


@pytest.mark.parametrize("mode", fz.MODES)
def test_every_other_mode_equals_the_tx_oracle_on_bits(mode):
    """TxFmOracle without an FM setting is rc.TxCpuChain(spec, "orc"): the restated up-mix, the q15 composition and the state, when the
    mode is the spec's own and when set_mode brings it"""
    for case, spec in pin_specs():
        for created_in_mode in (True, False):
            s = copy.copy(spec)
            if created_in_mode:
                s.mode = mode
            o, t = fo.TxFmOracle(s), rc.TxCpuChain(s, "orc")
            assert t.ok() and o.set_mode(rc.MODE_FM) == rc.ARGUMENT_ERROR and o.mode == s.mode
            if not created_in_mode:
                a = pin_audio(case, s, 2, False)
                assert rc.identical(o.process(a), t.process(a))
                assert o.set_mode(mode) == 0 and t.set_mode(mode) == 0
            for k, q15 in enumerate((False, True)):
                a = pin_audio(case, s, k, q15)
                got, want = (o.process_q15(a), t.process_q15(a)) if q15 else (o.process(a), t.process(a))
                assert rc.identical(got, want), (case, mode, k)
            so, st = o.state(), t.state()
            assert not so.pop("tone_phase").any()
            assert states_identical(so, st), (case, mode)


@pytest.mark.parametrize("fm", [False, True])
def test_reset_equals_a_fresh_oracle_on_bits(fm):
    tsteps = np.array([0x0B4E81B5, 0x80000001, 0xFFFFFF01], np.uint32)
    for arith in (rc.ARITH_CMSIS, rc.ARITH_FMA):
        spec = fm_spec(3, 32, 3, 45, 15, arith, nco_steps=np.array([0x3A5F1C27, 0xC0000001, 0], np.uint32), alc_params=gl.SETS["odd"])
        used, fresh = (fo.TxFmOracle(spec, 0.7, 0.9, 0.2, tsteps) for _ in range(2))
        for o in (used, fresh):
            assert o.set_mode(rc.MODE_FM if fm else rc.MODE_LSB) == 0
        used.process(rc.synth_audio(0, 3, 0, 96))
        st = used.state()
        assert st["nco_phase"].any() and (st["alc_gain"] != f32(gl.SETS["odd"]["gain_init"])).all() and st["tone_phase"].any() == fm
        assert used.reset() == 0 and used.mode == fresh.mode and used.fm_set
        assert states_identical(used.state(), fresh.state())
        a = rc.synth_audio(0, 3, 96, 64)
        assert rc.identical(used.process(a), fresh.process(a)) and states_identical(used.state(), fresh.state())


def test_fm_is_optional_and_the_first_setting_starts_the_tone_at_zero():
    spec = fm_spec(2, 16, 2, 2, 1)
    o = fo.TxFmOracle(spec)
    assert not o.fm_set and o.set_mode(rc.MODE_FM) == rc.ARGUMENT_ERROR and o.mode == rc.MODE_USB
    assert o.set_fm(0.3, 1.0, 0.1, 0x01234567) == 0 and o.set_mode(rc.MODE_FM) == 0
    o.process(rc.synth_audio(0, 2, 0, 32))
    tp = o.state()["tone_phase"]
    assert tp.all() and o.clear_fm() == rc.ARGUMENT_ERROR and o.fm_set
    o.set_fm(0.2, 1.0, 0.1, 0x01234567)
    assert rc.identical(o.state()["tone_phase"], tp), "a retune keeps the tone's phase"
    assert o.set_mode(rc.MODE_USB) == 0 and o.clear_fm() == 0 and o.set_mode(rc.MODE_FM) == rc.ARGUMENT_ERROR
    o.set_fm(0.2, 1.0, 0.1, 0x01234567)
    assert not o.state()["tone_phase"].any()


# ---- what the mode is for ---------------------------------------------------------------------------------------------------------------
# The receiver of both loop-backs: NCO at the transmitter's step, a 255-tap decimator by L = 4 (group delay 127 output samples: decimated sample m sits
# on output sample 4 m - 127, and the decimator is full from m = 64 on), the FM demodulator.  The discriminator works on the decimated samples: it
# returns the phase advance of L output samples in half turns -- the sum of L consecutive v = deviation * w -- so at L = 1 it is deviation * w itself and at L = 4 four times its
# mean over the L samples.
L_LOOP, ND_LOOP, DELAY, LAG = 4, 255, 127, 32        # LAG: DELAY in audio samples, rounded up


def rx_fm(ch, block, step):
    spec = rc.ChainSpec(ch, block * L_LOOP, L_LOOP, ND_LOOP, 63, 0, rc.MODE_FM, rc.ARITH_CMSIS, nco=True, nco_step_all=int(step), agc=False)
    rx = rc.CpuChain(spec, "orc")
    assert rx.ok()
    return rx


# measured here, on the CPU oracle pair, with the inputs of the test below: max |audio - expected| = 9.79e-4 at a signal peak of 0.128.  It holds the
# 24-bit phase (1.2e-7 of a half turn), the table sine and cosine (513 entries, linear interpolation: ~5e-6 of the amplitude), the 9-term arctangent
# (~1e-6 rad) and, the largest term by far, what the receiver's 255-tap decimator does to a carrier modulated over a tenth of its pass band.
# The bound is the measured value with a factor 2.
LOOPBACK_BOUND = 2.0e-3


def test_loopback_through_the_rx_oracle_returns_the_modulating_signal():
    ch, block, nblk = 2, 64, 12
    step = 0x01000000
    dev = 0.04
    t = np.arange(block * nblk)
    audio = np.stack([0.5 * np.sin(2 * np.pi * 0.011 * t) + 0.3 * np.sin(2 * np.pi * 0.031 * t + 0.5),
                      0.6 * np.sin(2 * np.pi * 0.02 * t + 1.0)]).astype(f32)
    o = fo.TxFmOracle(fm_spec(ch, block, L_LOOP, 256, 63, alc=False, nco_step_all=step), dev, 1.0)
    o.set_mode(rc.MODE_FM)
    iq = o.process(audio)
    y = rx_fm(ch, block, step).process(iq)
    v = o.last_d.astype(np.float64) / 2147483648.0
    csum = np.cumsum(v, axis=1)
    m = np.arange(66, y.shape[1])
    want = csum[:, L_LOOP * m - DELAY] - csum[:, L_LOOP * (m - 1) - DELAY]
    err = np.abs(y[:, m].astype(np.float64) - want).max()
    print("FM loop-back: max |audio - sum of L deviations| = %.3e (bound %.1e), signal peak %.3f" % (err, LOOPBACK_BOUND, np.abs(want).max()))
    assert np.abs(want).max() > 0.1
    assert err <= LOOPBACK_BOUND


FS_AUDIO, FRAME = 12000.0, 2400          # tests/test_tones_oracle.py: test_the_50_ctcss_tones_under_noise, N = 2400


@pytest.mark.parametrize("tone_on", [True, False])
def test_ctcss_loopback_reads_the_tone_that_was_sent(tone_on):
    hz = sr.ctcss_hz()
    sent = [0, 24, 49]
    block = 100
    step = 0x01000000
    tsteps = np.array([sr.tone_step(hz[k], FS_AUDIO * L_LOOP) for k in sent], np.uint32)
    rng = np.random.default_rng(0xC7C55F)
    audio = rng.uniform(-0.3, 0.3, (3, FRAME + LAG + 9 + (-(FRAME + LAG + 9)) % block)).astype(f32)
    o = fo.TxFmOracle(fm_spec(3, block, L_LOOP, 256, 63, alc=False, nco_step_all=step), 0.05, 1.0, 0.1, tsteps if tone_on else None)
    o.set_mode(rc.MODE_FM)
    y = rx_fm(3, block, step).process(o.process(audio))
    bank = to.Tones(3, FRAME, sr.design_tones(hz / FS_AUDIO), frame_blocks=1, confirm=1, release=1, ratio=0.02, min_power=0.0)
    bank.process(y[:, LAG + 1:LAG + 1 + FRAME])
    if tone_on:
        assert list(bank.tone) == sent
    else:
        assert list(bank.tone) == [to.NONE] * 3 and (bank.changes == 0).all()


def test_tone_step_is_rounded_once_in_double():
    assert sr.tone_step(0.0, 48000.0) == 0 and sr.tone_step(12000.0, 48000.0) == 0x40000000 and sr.tone_step(48000.0, 48000.0) == 0
    assert sr.tone_step(-12000.0, 48000.0) == 0xC0000000
    for hz in sr.ctcss_hz():
        assert sr.tone_step(hz, 48000.0) == int(round(hz / 48000.0 * 4294967296.0))
    assert sr.tone_step(float("nan"), 48000.0) == 0 and sr.tone_step(100.0, 0.0) == 0 and sr.tone_step(100.0, float("inf")) == 0
