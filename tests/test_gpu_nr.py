"""GPU: the NLMS noise reduction / automatic notch stage (selenite_rx_set_nr, csrc/rx_nlms.hip) against the numpy restatement of
arm_lms_norm_f32 + the AGC + arm_float_to_q15 (tests/nr_oracle.py), composed behind the oracle chain with its AGC off
(_CMSIS / _FMA: bit-exact end to end) or behind the GPU's own pre-stage audio (_SPLIT16 / _AUTO: the same instance with the stage and
the AGC off -- the stage is bit-exact given its input)."""
import copy
import ctypes as C

import numpy as np
import pytest

import nr_oracle as nro
import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu


def spec_of(name, ch, arith, mode=None, agc=True, q15_rounding=False):
    s = rc.baseline_spec(name, ch, arith, agc=agc, q15_rounding=q15_rounding)
    if mode is not None:
        s.mode = mode
    return s


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


class Expect:
    """What an instance of `spec` with the stage (kind, n, d, mu) gives, from the un-scaled audio of its chain: stage, AGC, int16."""

    def __init__(self, spec, kind, n, d, mu, coeffs_init=None):
        self.spec, self.kind = spec, kind
        self.nlms = nro.Nlms(spec.channels, n, mu, coeffs_init, delay=d)
        self.agc = nro.Agc(spec.channels, spec.block // spec.decim, spec.agc_params) if spec.agc else None

    def after(self, audio, q15=False):
        y = self.nlms.process(audio, self.kind)
        if self.agc is not None:
            y = self.agc.process(y)
        return nro.float_to_q15(y, self.spec.q15_rounding) if q15 else y


def oracle_chain(spec):
    """the oracle chain of `spec` with its AGC off: the un-scaled audio the stage sees (_SPLIT16 / _AUTO: the CMSIS chain)"""
    s = copy.copy(spec)
    s.agc = False
    if s.arith in (rc.ARITH_SPLIT16, rc.ARITH_AUTO):
        s.arith = rc.ARITH_CMSIS
    return rc.CpuChain(s, "orc")


class GlobalGain:
    """The AGC law of nr_oracle.Agc with ONE gain for all channels: per DSP block the envelope is taken over every channel (agc_global)."""

    def __init__(self, spec):
        self.p = {k: np.float32(v) for k, v in spec.agc_params.items()}
        self.g, self.na = self.p["gain_init"], spec.block // spec.decim

    def process(self, y):
        p, g, na = self.p, self.g, self.na
        want = np.empty_like(y)
        for b0 in range(0, y.shape[1], na):                    # one gain from the envelope over ALL channels
            env = np.float32(np.max(np.abs(y[:, b0:b0 + na])))
            e = p["env_floor"] if env < p["env_floor"] else env
            dd = np.float32(p["target"] / e)
            dd = p["gain_max"] if dd > p["gain_max"] else dd
            dd = p["gain_min"] if dd < p["gain_min"] else dd
            diff = np.float32(dd - g)
            g = np.float32(g + np.float32((p["attack"] if diff < 0 else p["decay"]) * diff))
            want[:, b0:b0 + na] = y[:, b0:b0 + na] * g
        self.g = g
        return want


def assert_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


# (shape, arith, mode, kind, N, D, q15, q15_rounding, agc, channels, calls x samples)
CASES = [
    ("cfg1", rc.ARITH_CMSIS, sr.MODE_USB, sr.NR_DENOISE, 32, 16, False, False, True, 70, [512, 256]),
    ("cfg1", rc.ARITH_FMA, sr.MODE_LSB, sr.NR_NOTCH, 16, 1, False, False, True, 64, [256, 768]),
    ("cfg1", rc.ARITH_CMSIS, sr.MODE_AM, sr.NR_NOTCH, 8, 64, False, False, True, 33, [512, 512]),
    ("cfg1", rc.ARITH_CMSIS, sr.MODE_FM, sr.NR_DENOISE, 64, 16, False, False, False, 16, [768]),
    ("cfg1", rc.ARITH_FMA, sr.MODE_USB, sr.NR_DENOISE, 64, 64, True, False, True, 40, [256, 512]),
    ("cfg1", rc.ARITH_CMSIS, sr.MODE_LSB, sr.NR_NOTCH, 32, 1, True, True, True, 64, [1024]),
    ("cfg3", rc.ARITH_CMSIS, sr.MODE_USB, sr.NR_DENOISE, 32, 16, False, False, True, 96, [1024, 2048]),
    ("cfg3", rc.ARITH_FMA, sr.MODE_USB, sr.NR_NOTCH, 16, 64, True, False, True, 80, [1024, 1024]),
    ("cfg3", rc.ARITH_CMSIS, sr.MODE_AM, sr.NR_DENOISE, 8, 1, True, True, False, 65, [2048]),
    ("cfg3", rc.ARITH_FMA, sr.MODE_LSB, sr.NR_DENOISE, 64, 16, False, False, False, 64, [1024, 1024, 1024]),
    ("cfg4", rc.ARITH_CMSIS, sr.MODE_CW, sr.NR_NOTCH, 16, 16, False, False, True, 100, [512, 256]),
    ("cfg4", rc.ARITH_FMA, sr.MODE_CW, sr.NR_DENOISE, 32, 64, True, True, True, 64, [256, 256, 512]),
    ("cfg4", rc.ARITH_CMSIS, sr.MODE_CW, sr.NR_DENOISE, 64, 1, True, False, False, 7, [1024]),
    ("cfg4", rc.ARITH_FMA, sr.MODE_CW, sr.NR_NOTCH, 8, 16, False, False, True, 96, [768]),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-a%d-m%d-k%d-N%d-D%d-%s-r%d-agc%d" % (c[0], c[1], c[2], c[3], c[4], c[5], "q15" if c[6] else "f32", c[7], c[8]))
def test_bit_exact_against_oracle_chain_and_restatement(case):
    name, arith, mode, kind, n, d, q15, rnd, agc, ch, calls = case
    spec = spec_of(name, ch, arith, mode if name != "cfg4" else None, agc=agc, q15_rounding=rnd)
    rx = sr.Rx(spec.config())
    rx.set_nr(kind, num_taps=n, delay=d, mu=0.05 if n < 64 else 0.5)
    orc, exp = oracle_chain(spec), Expect(spec, kind, n, d, 0.05 if n < 64 else 0.5)
    at = 0
    for bs in calls:
        iq = rc.synth_iq(0, ch, at, bs)
        if q15:
            qi = to_q15(iq)
            got = rx.process_q15(qi)
            want = exp.after(orc.process(qi.astype(np.float32) / np.float32(32768.0)), q15=True)
        else:
            got = rx.process(iq)
            want = exp.after(orc.process(iq))
        assert_bits(got, want, "call at %d" % at)
        at += bs
    st = rx.nr_state()
    for k, v in exp.nlms.state().items():
        assert_bits(st[k], v, k)


def test_96_frame_slot_geometry_several_calls():
    """DSP blocks of 96 frames (the firmware's slot), no decimator: tiles of the stage do not line up with the blocks"""
    spec = rc.ChainSpec(48, 96, 1, 0, 31, 0, sr.MODE_USB, rc.ARITH_CMSIS)
    rx = sr.Rx(spec.config())
    rx.set_nr(sr.NR_NOTCH, num_taps=16, delay=5, mu=0.1)
    orc, exp = oracle_chain(spec), Expect(spec, sr.NR_NOTCH, 16, 5, 0.1)
    at = 0
    for bs in (96, 96 * 3, 96, 96 * 7):
        iq = rc.synth_iq(0, 48, at, bs)
        assert_bits(rx.process(iq), exp.after(orc.process(iq)), "call at %d" % at)
        at += bs


def own_pre_stage(name, ch, arith, calls, mode=None, q15=False, rnd=False, kind=sr.NR_DENOISE, n=32, d=16, mu=0.05, agc=True):
    """the stage given the GPU's own pre-stage audio: instance A with the stage, instance B without it and with the AGC off"""
    sa = spec_of(name, ch, arith, mode, agc=agc, q15_rounding=rnd)
    sb = spec_of(name, ch, arith, mode, agc=False)
    a, b = sr.Rx(sa.config()), sr.Rx(sb.config())
    a.set_nr(kind, num_taps=n, delay=d, mu=mu)
    exp = Expect(sa, kind, n, d, mu)
    at = 0
    for bs in calls:
        iq = rc.synth_iq(0, ch, at, bs)
        if q15:
            qi = to_q15(iq)
            got = a.process_q15(qi)
            want = exp.after(b.process(qi.astype(np.float32) / np.float32(32768.0)), q15=True)
        else:
            got, want = a.process(iq), exp.after(b.process(iq))
        assert_bits(got, want, "call at %d" % at)
        at += bs


@pytest.mark.parametrize("arith", [rc.ARITH_SPLIT16, rc.ARITH_AUTO], ids=["split16", "auto"])
@pytest.mark.parametrize("name,calls", [("cfg3", [4096, 1024 + 256]), ("cfg2", [1024, 768]), ("cfg4", [512, 256])])
def test_split_arith_given_own_pre_stage_audio(arith, name, calls):
    own_pre_stage(name, 64, arith, calls)


def test_auto_int16_rounding_given_own_pre_stage_audio():
    own_pre_stage("cfg3", 64, rc.ARITH_AUTO, [2048, 1024], q15=True, rnd=True, kind=sr.NR_NOTCH, n=16, d=64)


def full_size(name, nsamp, kind, n, d):
    ch = 65536
    sa, sb = spec_of(name, ch, rc.ARITH_AUTO), spec_of(name, ch, rc.ARITH_AUTO, agc=False)
    a, b = sr.Rx(sa.config()), sr.Rx(sb.config())
    a.set_nr(kind, num_taps=n, delay=d, mu=0.05)
    nout = nsamp // sa.decim
    d_in, d_a, d_b = sr.DeviceBuffer(ch * nsamp * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(ch * nout * 4)
    a.synth_device(d_in.ptr, 0, ch, 0, nsamp, rc.SEED)
    a.sync()                            # (b runs on a stream of its own)
    a.process_device(d_in.ptr, d_a.ptr, nsamp)
    b.process_device(d_in.ptr, d_b.ptr, nsamp)
    a.sync(); b.sync()
    got, pre = d_a.download((ch, nout), np.float32), d_b.download((ch, nout), np.float32)
    want = Expect(sa, kind, n, d, 0.05).after(pre)
    assert_bits(got, want, name)
    assert np.isfinite(got).all() and np.abs(got).max() > 0


def test_full_size_cfg3_denoise():
    full_size("cfg3", 4096, sr.NR_DENOISE, 32, 16)


def test_full_size_cfg4_notch():
    full_size("cfg4", 4096, sr.NR_NOTCH, 16, 16)


# ---- state ------------------------------------------------------------------------------------
def test_one_call_equals_several_calls():
    spec = spec_of("cfg3", 64, rc.ARITH_CMSIS)
    one, many = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (one, many):
        r.set_nr(sr.NR_NOTCH, num_taps=32, delay=16, mu=0.2)
    iq = rc.synth_iq(0, 64, 0, 4096)
    whole = one.process(iq)
    parts = np.concatenate([many.process(iq[:, a:b]) for a, b in ((0, 256), (256, 1280), (1280, 1536), (1536, 4096))], axis=1)
    assert_bits(parts, whole)
    s1, s2 = one.nr_state(), many.nr_state()
    for k in s1:
        assert_bits(s1[k], s2[k], k)


def test_state_round_trip_reset_and_second_set_nr():
    spec = spec_of("cfg1", 32, rc.ARITH_CMSIS)
    rx, fresh = sr.Rx(spec.config()), sr.Rx(spec.config())
    init = np.linspace(-0.1, 0.1, 16).astype(np.float32)
    for r in (rx, fresh):
        r.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.3, coeffs_init=init)
    s0 = rx.nr_state()
    assert_bits(s0["coeffs"], np.tile(init, (32, 1)))
    assert not any(s0[k].any() for k in ("window", "delay", "energy", "x0"))
    rx.process(rc.synth_iq(0, 32, 0, 512))
    st, g = rx.nr_state(), rx.state()
    nxt = rc.synth_iq(0, 32, 512, 512)
    y1 = rx.process(nxt)
    fresh.set_state(g)
    fresh.set_nr_state(st)
    assert_bits(fresh.process(nxt), y1, "after set_nr_state")
    assert rx.reset() == 0
    s = rx.nr_state()
    assert_bits(s["coeffs"], np.tile(init, (32, 1)))
    assert not any(s[k].any() for k in ("window", "delay", "energy", "x0"))
    rx.process(nxt)
    rx.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.3, coeffs_init=init)
    other = sr.Rx(spec.config())
    other.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.3, coeffs_init=init)
    other.set_state(rx.state())
    iq = rc.synth_iq(0, 32, 5000, 512)
    assert_bits(rx.process(iq), other.process(iq), "second set_nr")


def test_mode_switch_mid_stream_matches_oracle():
    spec = spec_of("cfg1", 40, rc.ARITH_CMSIS)
    rx = sr.Rx(spec.config())
    rx.set_nr(sr.NR_NOTCH, num_taps=32, delay=16, mu=0.05)
    orc, exp = oracle_chain(spec), Expect(spec, sr.NR_NOTCH, 32, 16, 0.05)
    at = 0
    for mode in (sr.MODE_USB, sr.MODE_LSB, sr.MODE_AM, sr.MODE_USB):
        assert rx.set_mode(mode) == 0 and orc.set_mode(mode) == 0
        iq = rc.synth_iq(0, 40, at, 512)
        assert_bits(rx.process(iq), exp.after(orc.process(iq)), "mode %d" % mode)
        at += 512


@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO])
def test_stage_removed_before_any_call_is_no_stage(arith):
    spec = spec_of("cfg3", 64, arith)
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    a.set_nr(sr.NR_DENOISE, num_taps=64, delay=64, mu=1.0)
    a.set_nr(sr.NR_OFF)
    for call in range(2):
        iq = rc.synth_iq(0, 64, call * 2048, 2048)
        assert_bits(a.process(iq), b.process(iq), "call %d" % call)
    with pytest.raises(sr.RxError):
        a.nr_state()
    assert a.L.selenite_rx_get_nr_state(a.h, C.byref(sr.NrStateView())) == sr.ARGUMENT_ERROR


# ---- call paths ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg3", "cfg4"])
def test_host_pointer_calls_equal_device_calls(name):
    ch, bs = 4096, 2048                 # 64 MiB of f32 input: two 32 MiB chunks of the host pipeline, the second one at channel 2048
    spec = spec_of(name, ch, rc.ARITH_AUTO)
    h, dv = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (h, dv):
        r.set_nr(sr.NR_NOTCH, num_taps=16, delay=16, mu=0.05)
    nout = bs // spec.decim
    d_in, d_out = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4)
    for call in range(2):
        iq = rc.synth_iq(0, ch, call * bs, bs)
        d_in.upload(iq)
        dv.process_device(d_in.ptr, d_out.ptr, bs)
        dv.sync()
        assert_bits(h.process(iq), d_out.download((ch, nout), np.float32), "call %d" % call)


def test_global_gain_phase1_phase2_matches_restatement():
    ch, bs = 96, 1024
    sa = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS, agc_global=True)
    sb = spec_of("cfg3", ch, rc.ARITH_CMSIS, agc=False)
    a, b = sr.Rx(sa.config()), sr.Rx(sb.config())
    a.set_nr(sr.NR_DENOISE, num_taps=32, delay=16, mu=0.05)
    nl = nro.Nlms(ch, 32, 0.05, delay=16)
    gg = GlobalGain(sa)
    nout = bs // 4
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(4 * (bs // 256))
    for call in range(2):
        iq = rc.synth_iq(0, ch, call * bs, bs)
        y = nl.process(b.process(iq), sr.NR_DENOISE)
        d_in.upload(iq)
        a.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
        a.global_phase2(d_out.ptr, d_env.ptr, bs)
        a.sync()
        got = d_out.download((ch, nout), np.float32)
        want = gg.process(y)
        assert_bits(got, want, "call %d" % call)


def test_non_finite_stage_output_raises_naninf():
    spec = spec_of("cfg1", 8, rc.ARITH_CMSIS, agc=False)
    rx = sr.Rx(spec.config())
    rx.set_nr(sr.NR_DENOISE, num_taps=8, delay=1, mu=1.0, coeffs_init=np.full(8, 3e38, np.float32))
    iq = rc.synth_iq(0, 8, 0, 256) * np.float32(1e3)
    with pytest.raises(sr.RxError) as ei:
        rx.process(iq)
    assert ei.value.code == sr.NANINF


# ---- validation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("kind", 3), ("num_taps", 12), ("num_taps", 128), ("num_taps", 0), ("delay", 0), ("delay", 65),
                                         ("mu", 0.0), ("mu", 2.0), ("mu", -0.5), ("mu", float("nan")), ("mu", float("inf")),
                                         ("struct_size", 24)])
def test_bad_field_is_argument_error_and_instance_stays_usable(field, value):
    spec = spec_of("cfg1", 16, rc.ARITH_CMSIS)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_nr(sr.NR_NOTCH, num_taps=16, delay=4, mu=0.1)
    iq = rc.synth_iq(0, 16, 0, 512)
    assert_bits(rx.process(iq), ref.process(iq))
    g = sr.NrConfig()
    g.struct_size, g.kind, g.num_taps, g.delay, g.mu = C.sizeof(sr.NrConfig), sr.NR_DENOISE, 32, 16, 0.05
    setattr(g, field, value)
    assert rx.L.selenite_rx_set_nr(rx.h, C.byref(g)) == sr.ARGUMENT_ERROR
    assert rx.status() == 0
    iq = rc.synth_iq(0, 16, 512, 512)
    assert_bits(rx.process(iq), ref.process(iq), "after the refused set_nr")
    with pytest.raises(sr.RxError):
        rx.set_nr(sr.NR_DENOISE, num_taps=32, delay=16, mu=0.05, coeffs_init=np.full(32, np.inf, np.float32))
