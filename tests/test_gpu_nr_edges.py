"""GPU: the NLMS stage (csrc/rx_nlms.hip, selenite_rx_set_nr) where tests/test_gpu_nr.py never takes it -- the firmware's slot geometry, the
forms and the mixed reruns of SELENITE_ARITH_AUTO, the other chain shapes, the edges of the float32 range, a second workgroup at N = 64 / 8.
Same method and same helpers as test_gpu_nr.py: bit for bit against the oracle chain with its AGC off + the numpy restatement of
arm_lms_norm_f32 (tests/nr_oracle.py; pinned to the reference's code at these edges by tests/golden/lms_norm.npz), or, behind the
split-precision kernels, against the restatement fed the same instance's own pre-stage audio.

k_nlms works in tiles of 32 audio samples and batches of 8.  Which case of GEOMETRY reaches which of its branches (nout: audio samples of a call):
  - the call's last, partial batch (nout % 8 != 0):       b48d4-*  (calls of 12, 36, 60, 132 samples), b16d4-* (4, 12, 20, 44)
  - a partial last tile, whole batches (nout % 32 != 0):  b96d4-*  (24, 48, 72, 120, 264), b96d2-* (48, 144, 240)
  - a call shorter than the delay line (nout < D):        b96d4-*-D64 / -D25 (24 < 25), b48d4-*-D64 / -D63 / -D25 / -D24 / -D23 (12), b16d4-*-D5 (4)
  - nout == D, nout == D + 1:                              b96d4-*-D24 and b48d4-*-D24 (24), b96d4-*-D23 and b48d4-*-D23 (24)
  - a call shorter than one batch (nout < 8):              b16d4-*  (4)
  - tiles that do not line up with the DSP blocks, whole:  b96d1-*, cw96-*  (96, 192, 288 ...)
The AUTO tests prove what they reach by the guard counters they assert.
"""
import numpy as np
import pytest

import nr_oracle as nro
import rxcommon as rc
import selenite_rx as sr
from test_gpu_nr import Expect, GlobalGain, assert_bits, oracle_chain, own_pre_stage, spec_of, to_q15

pytestmark = pytest.mark.gpu
both_auto_forms = pytest.mark.usefixtures("auto_form")          # SELENITE_ARITH_AUTO in its one-launch and its three-launch form (conftest.py)

TINY = float(np.finfo(np.float32).tiny)                          # 1.18e-38: below it a float32 is a denormal


def mu_of(n):
    return 0.05 if n < 64 else 0.5


def assert_state(rx, exp):
    st = rx.nr_state()
    for k, v in exp.nlms.state().items():
        assert_bits(st[k], v, k)


def run_exact(spec, kind, n, d, mu, inputs, q15=False):
    """an instance of `spec` (exact arithmetic) with the stage against oracle_chain(spec) + restatement, call by call, then nr_state()"""
    rx = sr.Rx(spec.config())
    rx.set_nr(kind, num_taps=n, delay=d, mu=mu)
    orc, exp = oracle_chain(spec), Expect(spec, kind, n, d, mu)
    for i, iq in enumerate(inputs):
        if q15:
            qi = to_q15(iq)
            got = rx.process_q15(qi)
            want = exp.after(orc.process(qi.astype(np.float32) / np.float32(32768.0)), q15=True)
        else:
            got, want = rx.process(iq), exp.after(orc.process(iq))
        assert_bits(got, want, "call %d (%d samples)" % (i, iq.shape[1]))
    assert_state(rx, exp)
    rx.close()
    return exp


def stream(ch, lengths):
    at = 0
    for bs in lengths:
        yield rc.synth_iq(0, ch, at, bs)
        at += bs


# ---- a. the firmware's slot geometry, exact arithmetic end to end ------------------------------------------------------------------
# chain: (nd_taps, decim, nh_taps, n_biquad, DSP block) -> audio samples per DSP block
CHAINS = {
    "b96d4": (256, 4, 63, 0, 96),        # 24: the firmware's slot behind the /4 decimator
    "b48d4": (256, 4, 63, 0, 48),        # 12
    "b96d2": (128, 2, 63, 0, 96),        # 48
    "b96d1": (0, 1, 63, 0, 96),          # 96
    "cw96": (0, 1, 0, 4, 96),            # 96, CW: four biquads
    "b16d4": (32, 4, 63, 0, 16),         # 4: fewer than one batch of the stage
}
BLOCKS = [1, 2, 10, 3, 11, 1, 5, 50, 2]      # DSP blocks per call


def chain_spec(name, ch, arith, agc=True, q15_rounding=False, **kw):
    nd, m, nh, nbiq, block = CHAINS[name]
    kw.setdefault("nco", True)
    kw.setdefault("nco_step_all", 0x00800000 if nbiq else 0x01000000)
    return rc.ChainSpec(ch, block, m, nd, nh, nbiq, rc.MODE_CW if nbiq else rc.MODE_USB, arith, agc=agc, q15_rounding=q15_rounding, **kw)


# (chain, arith, kind, N, D, int16 slots, rounding, agc, channels)
GEOMETRY = [
    ("b96d4", rc.ARITH_CMSIS, sr.NR_DENOISE, 32, 24, False, False, True, 70),
    ("b96d4", rc.ARITH_FMA, sr.NR_NOTCH, 16, 64, True, False, True, 7),
    ("b96d4", rc.ARITH_CMSIS, sr.NR_NOTCH, 64, 23, False, False, False, 70),
    ("b96d4", rc.ARITH_FMA, sr.NR_DENOISE, 8, 25, True, True, True, 130),
    ("b96d4", rc.ARITH_CMSIS, sr.NR_NOTCH, 8, 24, True, True, False, 70),
    ("b48d4", rc.ARITH_CMSIS, sr.NR_NOTCH, 8, 64, False, False, True, 70),
    ("b48d4", rc.ARITH_FMA, sr.NR_DENOISE, 16, 5, True, True, False, 7),
    ("b48d4", rc.ARITH_CMSIS, sr.NR_DENOISE, 32, 63, True, False, True, 130),
    ("b48d4", rc.ARITH_FMA, sr.NR_NOTCH, 64, 24, False, False, True, 70),
    ("b48d4", rc.ARITH_CMSIS, sr.NR_DENOISE, 64, 1, False, False, False, 7),
    ("b48d4", rc.ARITH_CMSIS, sr.NR_DENOISE, 16, 23, False, False, True, 130),
    ("b48d4", rc.ARITH_FMA, sr.NR_NOTCH, 8, 25, True, False, False, 70),
    ("b48d4", rc.ARITH_CMSIS, sr.NR_NOTCH, 16, 24, False, False, True, 7),
    ("b96d2", rc.ARITH_CMSIS, sr.NR_DENOISE, 16, 63, False, False, True, 70),
    ("b96d2", rc.ARITH_FMA, sr.NR_NOTCH, 32, 1, True, False, False, 130),
    ("b96d1", rc.ARITH_CMSIS, sr.NR_NOTCH, 8, 5, False, False, True, 7),
    ("b96d1", rc.ARITH_FMA, sr.NR_DENOISE, 32, 64, True, True, True, 70),
    ("cw96", rc.ARITH_CMSIS, sr.NR_NOTCH, 16, 25, False, False, True, 70),
    ("cw96", rc.ARITH_FMA, sr.NR_DENOISE, 8, 23, True, False, False, 130),
    ("b16d4", rc.ARITH_CMSIS, sr.NR_DENOISE, 16, 5, False, False, True, 70),
    ("b16d4", rc.ARITH_FMA, sr.NR_NOTCH, 64, 64, True, False, True, 7),
    ("b16d4", rc.ARITH_CMSIS, sr.NR_NOTCH, 8, 1, False, False, False, 130),
    ("b16d4", rc.ARITH_CMSIS, sr.NR_DENOISE, 32, 24, True, True, True, 70),
]


@pytest.mark.parametrize("case", GEOMETRY, ids=lambda c: "%s-a%d-k%d-N%d-D%d-%s-r%d-agc%d-c%d" % (c[0], c[1], c[2], c[3], c[4], "q15" if c[5] else "f32", c[6], c[7], c[8]))
def test_slot_geometry_bit_exact_against_oracle_chain_and_restatement(case):
    """Calls of 1, 2, 3, 5, 10, 11 and 50 DSP blocks of 96 (48, 16) frames: 24 (12, 48, 96, 4) audio samples per block, so the stage's calls are
    neither whole batches nor whole tiles, shorter than its delay line, as long as it, one longer (the module docstring says which case is which)."""
    name, arith, kind, n, d, q15, rnd, agc, ch = case
    spec = chain_spec(name, ch, arith, agc=agc, q15_rounding=rnd)
    run_exact(spec, kind, n, d, mu_of(n), stream(ch, [k * spec.block for k in BLOCKS]), q15=q15)


@pytest.mark.parametrize("n,d", [(32, 24), (64, 64), (8, 5)])
def test_one_call_equals_45_slots(n, d):
    """4320 frames at once (1080 audio samples: 33 tiles and 24 samples) against the same frames in 45 slots of 96 (24 audio samples each)"""
    spec = chain_spec("b96d4", 70, rc.ARITH_CMSIS)
    one, many = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (one, many):
        r.set_nr(sr.NR_NOTCH, num_taps=n, delay=d, mu=0.2)
    iq = rc.synth_iq(0, 70, 0, 4320)
    whole = one.process(iq)
    parts = np.concatenate([many.process(iq[:, a:a + 96]) for a in range(0, 4320, 96)], axis=1)
    assert_bits(parts, whole)
    s1, s2 = one.nr_state(), many.nr_state()
    for k in s1:
        assert_bits(s1[k], s2[k], k)
    assert np.abs(whole).max() > 0


# ---- b. SELENITE_ARITH_AUTO with the stage, both forms -----------------------------------------------------------------------------------
def shape_spec(shape, ch, arith, agc=True, block=256, **kw):
    nd, m, nh = shape
    return rc.ChainSpec(ch, block, m, nd, nh, 0, rc.MODE_USB, arith, agc=agc, **kw)


@both_auto_forms
@pytest.mark.parametrize("shape", [(256, 4, 63), (0, 1, 127)])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_auto_with_every_channel_rerun_is_the_exact_chain_with_the_stage(shape, q15):
    """guard ratio +inf: every channel is recomputed in exact arithmetic inside the call, in front of the stage -- the whole instance is the
    oracle chain + restatement bit for bit, and every channel-call was a rerun"""
    nch = 77
    steps = (np.arange(nch, dtype=np.uint64) * 0x9E3779B1 % (1 << 32)).astype(np.uint32)
    spec = shape_spec(shape, nch, rc.ARITH_AUTO, nco=True, nco_steps=steps)
    rx = sr.Rx(spec.config())
    assert "split16" in rx.kernel_name() and "exact rerun" in rx.kernel_name()
    rx.set_guard_ratio(float("inf"))
    rx.set_nr(sr.NR_DENOISE, num_taps=32, delay=16, mu=0.05)
    orc, exp = oracle_chain(spec), Expect(spec, sr.NR_DENOISE, 32, 16, 0.05)
    for call, iq in enumerate(stream(nch, (1024, 2048, 1024, 4096))):
        if q15:
            qi = to_q15(iq)
            got, want = rx.process_q15(qi), exp.after(orc.process(qi.astype(np.float32) / np.float32(32768.0)), q15=True)
        else:
            got, want = rx.process(iq), exp.after(orc.process(iq))
        assert_bits(got, want, "call %d" % call)
    assert_state(rx, exp)
    st = rx.guard_stats()
    assert st["rerun_channel_calls"] == 4 * nch and st["channel_calls"] == 4 * nch and st["handover_blocks"] == 0
    rx.close()


@both_auto_forms
@pytest.mark.parametrize("shape", [(256, 4, 63), (0, 1, 127)])
def test_auto_with_some_channels_rerun_and_others_not(shape):
    """Every channel its own random NCO step (most pass bands empty): after the start-up call some channels are recomputed and others stay on
    the matrix kernel.  A (stage, AGC) is the restatement of B's audio (the same instance without stage and AGC), and both guard the SAME
    channels in every call: what follows the demodulator has no say in the guard's decision."""
    nch = 192
    steps = np.random.default_rng(5).integers(0, 1 << 32, nch, dtype=np.uint64).astype(np.uint32)
    kw = dict(nco=True, nco_steps=steps)
    sa, sb = shape_spec(shape, nch, rc.ARITH_AUTO, **kw), shape_spec(shape, nch, rc.ARITH_AUTO, agc=False, **kw)
    a, b = sr.Rx(sa.config()), sr.Rx(sb.config())
    a.set_nr(sr.NR_NOTCH, num_taps=16, delay=23, mu=0.05)
    exp = Expect(sa, sr.NR_NOTCH, 16, 23, 0.05)
    rerun_any = np.zeros(nch, bool)
    for call, iq in enumerate(stream(nch, (4096, 4096, 4096))):
        before = a.guard_channels()
        assert_bits(a.process(iq), exp.after(b.process(iq)), "call %d" % call)
        ga, gb = a.guard_channels(), b.guard_channels()
        assert np.array_equal(ga, gb), "call %d: channels %s" % (call, np.flatnonzero(ga != gb)[:8])
        if call > 0:                    # (the first call from the zero state guards everybody: the filters ramp up through its first blocks)
            rerun_any |= ga > before
    assert_state(a, exp)
    assert 0 < rerun_any.sum() and (shape[0] == 0 or rerun_any.sum() < nch), rerun_any.sum()
    for r in (a, b):
        st = r.guard_stats()
        assert st["handover_blocks"] == 0 and st["rerun_channel_calls"] == st["channel_calls"] > 0
    assert a.guard_stats() == b.guard_stats()
    a.close(); b.close()


# ---- c. the other chain shapes behind the split-precision kernels ----------------------------------------------------------------------
def own_audio(mk, calls, kind, n, d, mu, q15=False):
    """test_gpu_nr.own_pre_stage for a chain that has no name: mk(agc) gives the spec; A has the stage, B has neither stage nor AGC"""
    sa, sb = mk(True), mk(False)
    a, b = sr.Rx(sa.config()), sr.Rx(sb.config())
    a.set_nr(kind, num_taps=n, delay=d, mu=mu)
    exp = Expect(sa, kind, n, d, mu)
    for call, iq in enumerate(stream(sa.channels, calls)):
        if q15:
            qi = to_q15(iq)
            got, want = a.process_q15(qi), exp.after(b.process(qi.astype(np.float32) / np.float32(32768.0)), q15=True)
        else:
            got, want = a.process(iq), exp.after(b.process(iq))
        assert_bits(got, want, "call %d" % call)
    assert_state(a, exp)
    name = a.kernel_name()
    a.close(); b.close()
    return name


@pytest.mark.parametrize("arith", [rc.ARITH_SPLIT16, rc.ARITH_AUTO], ids=["split16", "auto"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("name,ch,calls", [("cfg3", 70, [1280, 4096 + 256]),             # whole passes + a tail cut off as a call of its own (rx_select.h)
                                           ("cfg3_by8", 64, [1024 + 256, 4096 + 256, 256]),
                                           ("cfg2_48k128", 130, [128 * 5, 128, 128 * 8]),
                                           ("cfg2_48k", 96, [192 * 5, 192, 192 * 4])])
def test_named_shapes_given_own_pre_stage_audio(arith, q15, name, ch, calls):
    own_pre_stage(name, ch, arith, calls, q15=q15, rnd=q15, kind=sr.NR_NOTCH if q15 else sr.NR_DENOISE, n=16 if q15 else 32, d=24)


@pytest.mark.parametrize("arith", [rc.ARITH_SPLIT16, rc.ARITH_AUTO], ids=["split16", "auto"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_decimation_by_2_given_own_pre_stage_audio(arith, q15):
    mk = lambda agc: shape_spec((128, 2, 63), 100, arith, agc=agc, nco=True, nco_step_all=0x01000000)
    name = own_audio(mk, [512 * 2 + 256, 4096 + 256, 256], sr.NR_DENOISE, 8, 63, 0.05, q15=q15)
    assert name.startswith("k_ssb_split16<128,2,63>"), name


@pytest.mark.parametrize("arith", [rc.ARITH_SPLIT16, rc.ARITH_AUTO], ids=["split16", "auto"])
def test_global_gain_on_int16_slots_given_own_pre_stage_audio(arith):
    """int16 slots with a global gain and the stage: the input converted once up front, the fused kernel, the stage, the envelope over all
    channels, the gain pass storing int16 (selenite_rx_process_q15: both phases in one call)"""
    ch = 96
    sa = rc.baseline_spec("cfg3", ch, arith, agc_global=True)
    a, b = sr.Rx(sa.config()), sr.Rx(spec_of("cfg3", ch, arith, agc=False).config())
    a.set_nr(sr.NR_DENOISE, num_taps=32, delay=16, mu=0.05)
    nl, gg = nro.Nlms(ch, 32, 0.05, delay=16), GlobalGain(sa)
    for call, iq in enumerate(stream(ch, (1024, 2048, 1024))):
        qi = to_q15(iq)
        y = nl.process(b.process(qi.astype(np.float32) / np.float32(32768.0)), sr.NR_DENOISE)
        assert_bits(a.process_q15(qi), nro.float_to_q15(gg.process(y)), "call %d" % call)
    a.close(); b.close()


# ---- d. levels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mu,d,kind,gap,silent_call,agc", [
    (8, 0.05, 16, sr.NR_DENOISE, (3000, 8000), 0, False),          # both edges inside a call
    (32, 0.5, 16, sr.NR_NOTCH, (3000, 8192), 1, False),            # the signal comes back on a call boundary
    (64, 1.5, 16, sr.NR_DENOISE, (4096, 8192), 1, False),          # both edges on call boundaries; N = 64 overshoots to |y| ~ 1e7 and stays finite
    (32, 0.5, 64, sr.NR_DENOISE, (3000, 8000), 0, True),
], ids=["N8", "N32-boundary", "N64-boundaries", "N32-agc"])
def test_burst_silence_and_the_signal_back(n, mu, d, kind, gap, silent_call, agc):
    """The cfg3 chain, three calls of 4096 frames, the input exactly zero over `gap`: the chain's audio is exactly zero by the end of call
    `silent_call`, and `energy` is then what the roundings of energy -= x0*x0, += in*in left behind -- NEGATIVE in some channels, so
    energy + eps is negative when the signal returns.  That is the reference's law; the kernel reproduces it bit for bit."""
    ch = 70
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS, agc=agc)
    rx = sr.Rx(spec.config())
    rx.set_nr(kind, num_taps=n, delay=d, mu=mu)
    orc, exp = oracle_chain(spec), Expect(spec, kind, n, d, mu)
    iq = rc.synth_iq(0, ch, 0, 3 * 4096)
    iq[:, gap[0]:gap[1]] = 0
    negative = False
    for call in range(3):
        part = np.ascontiguousarray(iq[:, call * 4096:(call + 1) * 4096])
        audio = orc.process(part)
        assert_bits(rx.process(part), exp.after(audio), "call %d" % call)
        if call == silent_call:
            assert not audio[:, -(n + d + 2):].any()                    # the input condition: silence has reached the whole window
            assert (exp.nlms.energy < 0).any()                          # ... and left a negative energy (the restatement's)
            e = rx.nr_state()["energy"]
            assert_bits(e, exp.nlms.energy, "energy")
            negative = bool((e < 0).any())
    assert negative
    assert_state(rx, exp)
    rx.close()


def scaled_stream(ch, level, calls):
    lv = np.broadcast_to(np.asarray(level, np.float32), (ch,))[:, None, None]
    for iq in stream(ch, calls):
        yield iq * lv


def run_levels(ch, level, agc):
    """cfg3 chain, exact arithmetic, three calls at `level` (one per channel, or one for all); the restatement's output must be finite"""
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS, agc=agc)
    rx = sr.Rx(spec.config())
    rx.set_nr(sr.NR_NOTCH, num_taps=32, delay=16, mu=0.5)
    orc, exp = oracle_chain(spec), Expect(spec, sr.NR_NOTCH, 32, 16, 0.5)
    for call, iq in enumerate(scaled_stream(ch, level, (1024, 1024, 1024))):
        want = exp.after(orc.process(iq))
        assert np.isfinite(want).all()
        assert_bits(rx.process(iq), want, "call %d" % call)
    assert_state(rx, exp)
    rx.close()
    return exp.nlms


def test_levels_from_1e_30_to_1e18_in_one_workgroup():
    """The lanes of one wave at levels 48 decades apart (a second, partial workgroup beside it): below 1e-19 in*in and `energy` are denormals
    or zero while the outputs are normal numbers -- a kernel that flushed denormals to zero would differ here and nowhere else"""
    ch = 70
    lv = (10.0 ** np.linspace(-30, 18, ch)).astype(np.float32)[np.random.default_rng(7).permutation(ch)]
    nl = run_levels(ch, lv, False)
    e = np.abs(nl.energy)
    assert ((e > 0) & (e < TINY)).any() and (e[lv < 1e-28] == 0).all() and (e[lv > 1e-17] > TINY).all() and np.isfinite(nl.coeffs).all()


@pytest.mark.parametrize("level,agc", [(1e-30, False), (1e-22, False), (1e-22, True), (1e-19, False), (1e18, False), (1e18, True)])
def test_one_level_per_instance(level, agc):
    nl = run_levels(7, level, agc)
    e = np.abs(nl.energy)
    if level == 1e-22:
        assert ((e > 0) & (e < TINY)).all()                             # denormal
    if level == 1e-30:
        assert not e.any() and not nl.coeffs.any()                      # in*in and w * px underflow to 0


def test_overflow_in_some_channels_raises_naninf_and_leaves_the_others_exact():
    """Levels of 1e17 ... 3e20 across the channels: the chain's audio is finite everywhere, `energy` overflows in the loud third of the channels
    and their output turns into NaN some hundred samples into the call.  SELENITE_RX_NANINF is raised; through the device entry point the
    output is there to be read: finite channels bit-exact, poisoned ones bit-exact wherever the restatement is finite, non-finite where it is not."""
    ch, bs = 70, 2048
    lv = (10.0 ** np.linspace(17, 20.5, ch)).astype(np.float32)[np.random.default_rng(8).permutation(ch)]
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS, agc=False)
    iq = next(scaled_stream(ch, lv, (bs,)))
    with np.errstate(all="ignore"):
        audio = oracle_chain(spec).process(iq)
        want = nro.Nlms(ch, 32, 0.5, delay=16).process(audio, sr.NR_NOTCH)
    assert np.isfinite(audio).all()
    poisoned = ~np.isfinite(want).all(axis=1)
    assert 0 < poisoned.sum() < ch                                          # the input condition: some channels only
    rx = sr.Rx(spec.config())
    rx.set_nr(sr.NR_NOTCH, num_taps=32, delay=16, mu=0.5)
    d_in, d_out = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * (bs // 4) * 4)
    d_in.upload(iq)
    rx.process_device(d_in.ptr, d_out.ptr, bs)
    with pytest.raises(sr.RxError) as ei:
        rx.sync()
    assert ei.value.code == sr.NANINF
    got = d_out.download((ch, bs // 4), np.float32)
    assert_bits(got[~poisoned], want[~poisoned], "finite channels")
    fin = np.isfinite(want)
    assert np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin])
    assert not np.isfinite(got[~fin]).any()
    host = sr.Rx(spec.config())                                             # the host-pointer call reports it itself
    host.set_nr(sr.NR_NOTCH, num_taps=32, delay=16, mu=0.5)
    with pytest.raises(sr.RxError) as ei:
        host.process(iq)
    assert ei.value.code == sr.NANINF


# ---- e. scale and reconfiguration ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(64, 64), (8, 23)])
def test_65_workgroups_at_the_slot_geometry(n, d):
    """4096 + 37 channels (64 whole workgroups and a partial one) at N = 64 -- the instantiation that spills into the accumulation registers --
    and N = 8: a call of 240 audio samples (seven tiles and a half) and one slot of 24, every channel against the restatement"""
    ch = 4096 + 37
    spec = chain_spec("b96d4", ch, rc.ARITH_CMSIS)
    run_exact(spec, sr.NR_DENOISE, n, d, mu_of(n), stream(ch, (960, 96)))


def test_set_nr_between_calls_starts_a_fresh_stage():
    """selenite_rx_set_nr with another N, D and kind between calls: from that call on the stage is a fresh restatement; the chain and its AGC go on"""
    ch = 70
    spec = chain_spec("b96d4", ch, rc.ARITH_CMSIS)
    rx, orc = sr.Rx(spec.config()), oracle_chain(spec)
    agc, at = None, 0
    for kind, n, d, calls in ((sr.NR_DENOISE, 32, 16, (960, 96)), (sr.NR_NOTCH, 8, 63, (96, 480, 96)), (sr.NR_DENOISE, 64, 5, (96, 96, 1056)),
                              (sr.NR_NOTCH, 16, 64, (192,))):
        rx.set_nr(kind, num_taps=n, delay=d, mu=mu_of(n))
        exp = Expect(spec, kind, n, d, mu_of(n))
        if agc is not None:
            exp.agc = agc
        for bs in calls:
            iq = rc.synth_iq(0, ch, at, bs)
            assert_bits(rx.process(iq), exp.after(orc.process(iq)), "N %d D %d call at %d" % (n, d, at))
            at += bs
        assert_state(rx, exp)
        agc = exp.agc
    rx.close()
