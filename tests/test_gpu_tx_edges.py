"""GPU: directed cases of the TX chain that the fuzz (tests/test_gpu_tx_fuzz.py) must not be relied on to hit, each against the oracle
(tests/txfm_oracle.py) through tests/tx_fuzz_runner.py -- output and every state array on bits (k_tx_split16's output: the 1e-5 bar):

  - the ALC law inside k_tx_fm away from its defaults (gain_law_cases.SETS, the six-call level plan of test_gpu_gain_law.py);
  - an instance with one NCO step for all channels (the shared LO of k_tx_fused / k_tx_split16) around FM calls: FM leaves every channel
    with a phase of its own, reset and set_state with one phase for all bring the shared LO back, at the restored phase;
  - dynamic LDS between 48 KB and 64 KB in k_tx_generic and k_tx_fm, and the refusal above 64 KB, which must leave the output and the
    state as they were;
  - a unit-impulse delay FIR whose 1.0 is not at the centre, across a call boundary;
  - slot formats and entry points alternating on one instance of every kernel family."""
import ctypes as C
import functools

import numpy as np
import pytest

import gain_law_cases as gl
import rxcommon as rc
import tx_fuzz_cases as fz
import tx_fuzz_runner as fr
from rxcommon import ARITH_CMSIS, ARITH_FMA, ARITH_SPLIT16

pytestmark = pytest.mark.gpu
f32 = np.float32
FM = rc.MODE_FM
LDS_MESSAGE = "filter lengths exceed the LDS budget of the TX kernel"


def tone_steps(channels):
    return (np.arange(channels, dtype=np.uint64) * 0x01010101 + 0x00345678).astype(np.uint32)


# ---- FM in the ALC grid ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def tx_plan(channels, q15):
    return gl.plan(channels, 64, gl.CALLS, q15, audio=True, **gl.run_kw("tx", channels, q15))


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("channels", gl.CHANNELS)
@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_fm_alc_away_from_its_defaults(name, channels, q15):
    """k_tx_fm through the plan of test_gpu_gain_law.py::test_tx_kernel_forms: the oracle with the same alc_params on bits, output and
    state (alc_gain among it) behind every call"""
    spec = rc.TxSpec(channels, alc_params=gl.SETS[name], nco_step_all=0x0FEDCBA9)
    p = fr.Pair(spec, (0.3, 0.9, 0.1, tone_steps(channels)), kernel=fz.FUSED)
    p.set_mode(FM, fz.KFM)
    gains = []
    for i, x in enumerate(tx_plan(channels, q15)):
        p.call(x, served="fm", what="%s x %d call %d" % (name, channels, i))
        gains.append(p.o.state()["alc_gain"])
    assert not fr.same_bits(gains[0], gains[-1]), "the gain moves over the plan"
    p.close()


@pytest.mark.parametrize("name", gl.SET_NAMES)
def test_fm_reset_returns_to_the_configured_gain(name):
    ch, prm = 65, gl.SETS[name]
    p = fr.Pair(rc.TxSpec(ch, alc_params=prm), (0.3, 0.9, 0.1, tone_steps(ch)))
    p.set_mode(FM, fz.KFM)
    init = np.full(ch, prm["gain_init"], f32)
    fr.assert_bits(p.g.state()["alc_gain"], init, "alc_gain of a new instance")
    calls = tx_plan(ch, False)[:3]
    first = [p.call(x, served="fm", what="call %d" % i) for i, x in enumerate(calls)]
    assert not (p.g.state()["alc_gain"] == init).any()
    p.reset()
    fr.assert_bits(p.g.state()["alc_gain"], init, "alc_gain behind reset()")
    for i, x in enumerate(calls):
        fr.assert_bits(p.call(x, served="fm", what="replayed call %d" % i), first[i], "call %d replayed behind reset()" % i)
    p.close()


# ---- one NCO step for all channels, around FM ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0x03000000, 0x0FEDCBA9], ids=["periodic", "odd"])
@pytest.mark.parametrize("arith", [ARITH_CMSIS, ARITH_SPLIT16], ids=["cmsis", "split16"])
def test_shared_lo_instance_around_fm(arith, step):
    ch = 37
    spec = rc.TxSpec(ch, arith=arith, nco_step_all=step)
    kernel = fz.SPLIT16 if arith == ARITH_SPLIT16 else fz.FUSED
    fam = fz.FAMILY[kernel]
    at = [0]

    def call(p, n, what, served):
        x = rc.synth_audio(0, ch, at[0], n)
        at[0] += n
        return p.call(x, served=served, what=what)

    def phases(p):
        return p.g.state()["nco_phase"]

    p = fr.Pair(spec, (0.4, 0.9, 0.15, tone_steps(ch)), kernel=kernel)
    call(p, 512, "USB on the shared LO", fam)
    call(p, 256, "USB, a shorter call on the LO table of the longer one", fam)
    assert len(set(phases(p))) == 1
    p.set_mode(FM, fz.KFM)
    call(p, 256, "FM", "fm")
    assert len(set(phases(p))) == ch, "FM leaves every channel at a phase of its own"
    p.set_mode(rc.MODE_USB, kernel)
    call(p, 256, "USB behind FM: per-channel phases", fam)
    call(p, 512, "USB behind FM, second call", fam)
    p.reset()
    assert not phases(p).any()
    call(p, 256, "USB behind reset: the shared LO again, from phase 0", fam)
    call(p, 512, "USB behind reset, a longer call", fam)
    assert len(set(phases(p))) == 1
    p.close()
    # FM, then set_state with one phase for all: the shared LO starts at the restored phase (the LO table is rebuilt there)
    p = fr.Pair(spec, (0.4, 0.9, 0.15, None), kernel=kernel)
    call(p, 256, "USB: the LO table from phase 0", fam)
    p.set_mode(FM, fz.KFM)
    call(p, 192, "FM", "fm")
    p.set_phase(0x3456789A)
    p.set_mode(rc.MODE_USB, kernel)
    call(p, 256, "USB behind set_state(uniform)", fam)
    assert len(set(phases(p))) == 1 and phases(p)[0] == (0x3456789A + 1024 * step) & 0xFFFFFFFF
    call(p, 512, "USB behind set_state(uniform), second call", fam)
    p.set_phase(0)                                                  # back where the first table was built
    call(p, 256, "USB from phase 0 again", fam)
    p.close()


# ---- dynamic LDS between 48 KB and 64 KB, and the refusal above -----------------------------------------------------------------------------
# one ALC block per workgroup: (block, L, ni, nh).  k_tx_generic keeps (I, Q) pairs of the block twice, k_tx_fm single floats: a block of
# 3 500 without filters is 58 064 bytes there, a block of 6 144 behind a 3-tap pair 51 248 bytes here (fz.tx_lds_bytes, fz.fm_lds_bytes
# restate tx_layout and fm_layout)
BIG_GENERIC, BIG_FM = (3500, 1, 0, 0), (6144, 1, 0, 3)


def big_spec(shape, arith, **kw):
    block, L, ni, nh = shape
    return rc.TxSpec(2, block=block, interp=L, ni_taps=ni, nh_taps=nh, arith=arith, nco_step_all=0x0FEDCBA9, **kw)


@pytest.mark.parametrize("arith", [ARITH_CMSIS, ARITH_FMA], ids=["cmsis", "fma"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_lds_between_48_and_64_kb(q15, arith):
    assert 48 * 1024 < fz.tx_lds_bytes(*BIG_GENERIC) < 64 * 1024 and 48 * 1024 < fz.fm_lds_bytes(*BIG_FM) < 64 * 1024
    for shape, fm in ((BIG_GENERIC, False), (BIG_FM, True)):
        p = fr.Pair(big_spec(shape, arith), (0.3, 0.9, 0.1, tone_steps(2)), kernel=fz.GENERIC)
        if fm:
            p.set_mode(FM, fz.KFM)
        x = rc.synth_audio(0, 2, 0, shape[0])
        p.call(gl.to_q15(x) if q15 else x, served="fm" if fm else "generic", what="block %d" % shape[0])
        p.close()


def smallest_refused(lds_bytes, L, ni, nh):
    block = 1
    while lds_bytes(block, L, ni, nh) <= 64 * 1024:
        block += 1
    return block


@pytest.mark.parametrize("fm", [False, True], ids=["generic", "fm"])
def test_lds_above_64_kb_is_refused_and_changes_nothing(fm):
    import selenite_rx as sr
    L, ni, nh = 2, 8, 3
    block = smallest_refused(fz.fm_lds_bytes if fm else fz.tx_lds_bytes, L, ni, nh)
    lds = (fz.fm_lds_bytes if fm else fz.tx_lds_bytes)(block, L, ni, nh)
    assert 64 * 1024 < lds <= 64 * 1024 + 64, "just above the bound"
    spec = big_spec((block, L, ni, nh), ARITH_CMSIS)
    rng = np.random.default_rng(0x1D5)
    for q15 in (False, True):
        for device in (False, True):
            g = sr.Tx(spec.config())
            if fm:
                assert g.set_fm(0.3, 0.9, 0.1, tone_steps(2)) == 0 and g.set_mode(FM) == 0
            st = g.state()
            for k in ("fir_state", "interp_state", "alc_gain"):
                st[k][...] = rng.uniform(0.1, 1.0, st[k].shape).astype(f32)
            st["nco_phase"][:] = [0x3456789A, 0x00C0FFEE]
            g.set_state(st)
            if fm:
                g.set_fm_state({"tone_phase": np.array([7, 0x89ABCDEF], np.uint32)})
            dt = np.int16 if q15 else f32
            x = gl.to_q15(rc.synth_audio(0, 2, 0, block)) if q15 else rc.synth_audio(0, 2, 0, block)
            sentinel = np.full((2, block * L, 2), 0x5A5A if q15 else -12345.5, dt)
            entry = getattr(g.L, "selenite_tx_process_%s%s" % ("q15" if q15 else "f32", "_device" if device else ""))
            if device:
                d_in, d_out = sr.DeviceBuffer(x.nbytes), sr.DeviceBuffer(sentinel.nbytes)
                d_in.upload(x)
                d_out.upload(sentinel)
                entry(g.h, d_in.ptr, d_out.ptr, block)
                out = d_out.download(sentinel.shape, dt)
            else:
                out = sentinel.copy()
                entry(g.h, x.ctypes.data, out.ctypes.data, block)
            what = "%s entry, %s" % ("device" if device else "host", "int16" if q15 else "f32")
            assert g.L.selenite_tx_status(g.h) == rc.LENGTH_ERROR, what
            assert g.L.selenite_tx_error_string(g.h).decode() == LDS_MESSAGE, what
            with pytest.raises(sr.RxError) as e:
                g.check()
            assert e.value.code == rc.LENGTH_ERROR
            fr.assert_bits(out, sentinel, what + ": the output buffer")
            after = g.state()
            for k in st:
                fr.assert_bits(after[k], st[k], "%s: state %s" % (what, k))
            if fm:
                fr.assert_bits(g.fm_state()["tone_phase"], np.array([7, 0x89ABCDEF], np.uint32), what + ": tone_phase")
            g.close()


# ---- the unit impulse of the delay FIR away from the centre ---------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [ARITH_CMSIS, ARITH_FMA, ARITH_SPLIT16], ids=["cmsis", "fma", "split16"])
@pytest.mark.parametrize("index", [0, 1, 31, 61, 62])
def test_moved_impulse_of_the_delay_fir(index, arith):
    """selenite_tx_init hands the index of the 1.0 to k_tx_fused and k_tx_split16 as delay_index; two calls, so that the delay line
    crosses the call boundary (index 0: the I rail is 62 samples behind the audio; index 62: not at all)"""
    ch = 5
    spec = rc.TxSpec(ch, arith=arith)
    spec.delay = np.zeros(63, f32)
    spec.delay[index] = 1.0
    kernel = fz.SPLIT16 if arith == ARITH_SPLIT16 else fz.FUSED
    p = fr.Pair(spec, kernel=kernel)
    for k in range(2):
        p.call(rc.synth_audio(0, ch, 256 * k, 256), served=fz.FAMILY[kernel], what="impulse at %d, call %d" % (index, k))
    p.set_mode(rc.MODE_AM, kernel)
    p.call(gl.to_q15(rc.synth_audio(0, ch, 512, 256)), device=True, served=fz.FAMILY[kernel], what="impulse at %d, AM, int16" % index)
    p.close()


# ---- slot formats and entries in turn on one instance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["generic", "fused", "split16", "fm"])
def test_slot_formats_and_entries_alternate_on_one_instance(family):
    ch = 65
    if family == "generic":
        spec, kernel, n = rc.TxSpec(ch, block=32, interp=3, ni_taps=45, nh_taps=15, nco_step_all=0x0FEDCBA9), fz.GENERIC, 96
    else:
        spec, kernel, n = rc.TxSpec(ch, arith=ARITH_SPLIT16 if family == "split16" else ARITH_FMA), (fz.SPLIT16 if family == "split16" else fz.FUSED), 256
    p = fr.Pair(spec, (0.4, 0.9, 0.15, tone_steps(ch)), kernel=kernel)
    if family == "fm":
        p.set_mode(FM, fz.KFM)
    for k, (q15, device) in enumerate(((False, False), (True, True), (False, True), (True, False), (False, False))):
        x = rc.synth_audio(0, ch, n * k, n)
        p.call(gl.to_q15(x) if q15 else x, device=device, served=family,
               what="call %d, %s, %s entry" % (k, "int16" if q15 else "f32", "device" if device else "host"))
    p.close()
