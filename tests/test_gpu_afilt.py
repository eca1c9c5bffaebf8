"""GPU: the audio biquad filter stage (selenite_rx_set_afilt, csrc/rx_afilt.hip: k_afilt<NS>) against the reference's own
arm_biquad_cascade_df1_f32 (tests/golden/afilt.npz) and against the numpy restatement (tests/afilt_oracle.py, pinned to that fixture by
tests/test_afilt_oracle.py), by the scheme of tests/test_gpu_nr.py: behind the oracle chain with its AGC off (_CMSIS / _FMA: bit-exact end
to end) or behind the GPU's own pre-stage audio (_SPLIT16 / _AUTO: the stage is bit-exact given its input), then nr_oracle.Agc and
float_to_q15.  Every comparison is on bits; the fixture's Inf streams alone use afilt_oracle.same_bits, which lets any NaN equal any NaN (the
sign of a generated NaN is the implementation's: x86 gives the negative one, gfx950 the positive one)."""
import copy
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import afilt_oracle as afo
import meter_oracle as mo
import nr_oracle as nro
import out_oracle as oo
import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu

KERNEL_TILE = 64          # samples of a channel row per tile of k_afilt (csrc/rx_afilt.hip: kAfTile)
ARITHS = (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO)
ARITH_IDS = ["cmsis", "fma", "split16", "auto"]


def spec_of(name, ch, arith, mode=None, agc=True, q15_rounding=False, **kw):
    s = rc.baseline_spec(name, ch, arith, agc=agc, q15_rounding=q15_rounding, **kw)
    if mode is not None:
        s.mode = mode
    return s


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


def q15_to_f32(q):
    return q.astype(np.float32) / np.float32(32768.0)


def sections(ns, channels=None, seed=1):
    """[ns][5], or [channels][ns][5]: sections from the design helpers with seeded parameters, every one stable and of moderate gain"""
    rng = np.random.default_rng(1000 * seed + ns)
    rows = []
    for _ in range(channels or 1):
        row = []
        for _ in range(ns):
            kind = int(rng.integers(0, 5))
            f0 = float(rng.uniform(0.02, 0.45))
            if kind == 4:
                row.append(sr.design_deemphasis(float(rng.uniform(0.5, 4.0))))
            elif kind in (sr.BIQUAD_NOTCH, sr.BIQUAD_PEAKING):
                row.append(sr.design_biquad(kind, f0, float(rng.uniform(0.5, 8.0)), float(rng.uniform(-9.0, 4.0))))
            else:
                row.append(sr.design_biquad(kind, f0, float(rng.uniform(0.5, 1.2))))
        rows.append(np.stack(row))
    c = np.stack(rows).astype(np.float32)
    return c if channels else c[0]


def assert_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32 if got.itemsize == 4 else np.uint16) != want.view(np.uint32 if want.itemsize == 4 else np.uint16))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


class Expect:
    """What an instance of `spec` with the stage gives, from the un-scaled audio of its chain: stage, AGC, int16."""

    def __init__(self, spec, coeffs, per_channel):
        self.spec = spec
        self.f = afo.Afilt(spec.channels, coeffs, per_channel)
        self.agc = nro.Agc(spec.channels, spec.block // spec.decim, spec.agc_params) if spec.agc else None

    def after(self, audio, q15=False):
        y = self.f.process(audio)
        if self.agc is not None:
            y = self.agc.process(y)
        return nro.float_to_q15(y, self.spec.q15_rounding) if q15 else y


def oracle_chain(spec):
    """the oracle chain of `spec` with its AGC off: the un-scaled audio the stage sees"""
    s = copy.copy(spec)
    s.agc = False
    assert s.arith in (rc.ARITH_CMSIS, rc.ARITH_FMA)
    return rc.CpuChain(s, "orc")


def run_device(rx, data):
    q15 = data.dtype == np.int16
    ch, bs = data.shape[0], data.shape[1]
    vals = rx.out_len(bs)
    d_in, d_out = sr.DeviceBuffer(data.nbytes), sr.DeviceBuffer(ch * vals * data.dtype.itemsize)
    d_in.upload(np.ascontiguousarray(data))
    (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
    rx.sync()
    out = d_out.download((ch, vals), data.dtype)
    d_in.free(); d_out.free()
    return out


def run(rx, data, device=False):
    if device:
        return run_device(rx, data)
    return rx.process_q15(data) if data.dtype == np.int16 else rx.process(data)


# ---- 1. the reference's own vectors through the library -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "afilt.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("ns", range(1, 9))
def test_golden_vectors_through_the_library(gold, ns):
    """an instance whose chain passes the I rail through (no NCO, no decimator, no FIR pair, AGC off, DSP block 1): the fixture's inputs go
    in as I, outputs and state equal the fixture's -- -0.0f, denormals, +-FLT_MAX, +-Inf; n_stages 3 and 5 .. 7 leave stage lanes unused"""
    coeffs, x, y, states = (gold["ns%d/%s" % (ns, k)] for k in ("coeffs", "x", "y", "state"))
    spec = rc.ChainSpec(3, 1, 1, 0, 0, 0, sr.MODE_USB, rc.ARITH_CMSIS, agc=False)
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    a.set_afilt(coeffs, per_channel=True)
    at = 0
    for i, n in enumerate(int(v) for v in gold["lengths"]):
        iq = np.zeros((3, n, 2), np.float32)
        iq[..., 0] = x[:, at:at + n]
        pre = run_device(b, iq)
        assert pre.tobytes() == x[:, at:at + n].tobytes(), "the chain does not pass the I rail through as it is"
        got = run_device(a, iq)
        assert afo.same_bits(got, y[:, at:at + n]), ("audio", ns, at, n)
        assert got[:2].tobytes() == y[:2, at:at + n].tobytes(), ("audio of the finite streams", ns, at, n)
        st = a.afilt_state()
        assert afo.same_bits(st["state"], states[i]), ("state", ns, at, n)
        assert st["state"][:2].tobytes() == states[i][:2].tobytes()
        at += n
    assert_bits(a.afilt_state()["coeffs"], coeffs, "coefficients as configured")


# ---- 2. end to end in _CMSIS and _FMA -----------------------------------------------------------------------------------------------
# (shape, arith, mode, q15, q15_rounding, agc, channels, n_stages, per_channel, calls)
CASES = [
    ("cfg1", rc.ARITH_CMSIS, sr.MODE_USB, False, False, True, 70, 1, False, [512, 256]),
    ("cfg1", rc.ARITH_FMA, sr.MODE_LSB, False, False, True, 33, 2, True, [256, 768]),
    ("cfg1", rc.ARITH_CMSIS, sr.MODE_AM, True, False, True, 100, 3, False, [512, 512]),
    ("cfg1", rc.ARITH_CMSIS, sr.MODE_FM, False, False, False, 7, 1, False, [768, 256]),
    ("cfg1", rc.ARITH_FMA, sr.MODE_USB, True, True, True, 70, 5, True, [256, 512]),
    ("cfg1", rc.ARITH_CMSIS, sr.MODE_LSB, True, False, False, 33, 8, False, [256, 256, 256]),
    ("cfg3", rc.ARITH_CMSIS, sr.MODE_USB, False, False, True, 100, 4, True, [1024, 2048]),
    ("cfg3", rc.ARITH_FMA, sr.MODE_USB, True, False, True, 70, 8, True, [1024, 1024]),
    ("cfg3", rc.ARITH_CMSIS, sr.MODE_AM, True, True, False, 33, 2, False, [2048, 1024]),
    ("cfg3", rc.ARITH_FMA, sr.MODE_FM, False, False, True, 7, 3, True, [1024, 1024, 1024]),
    ("cfg4", rc.ARITH_CMSIS, sr.MODE_CW, False, False, True, 100, 1, True, [512, 256]),
    ("cfg4", rc.ARITH_FMA, sr.MODE_CW, True, True, True, 70, 4, False, [256, 256, 512]),
    ("cfg4", rc.ARITH_CMSIS, sr.MODE_CW, True, False, False, 7, 5, True, [1024, 256]),
    ("cfg4", rc.ARITH_FMA, sr.MODE_CW, False, False, True, 33, 8, False, [768, 256]),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-a%d-m%d-%s-r%d-agc%d-ch%d-ns%d-%s" % (c[0], c[1], c[2], "q15" if c[3] else "f32", c[4], c[5], c[6], c[7], "per" if c[8] else "one"))
def test_bit_exact_against_oracle_chain_and_restatement(case):
    name, arith, mode, q15, rnd, agc, ch, ns, per, calls = case
    spec = spec_of(name, ch, arith, mode if name != "cfg4" else None, agc=agc, q15_rounding=rnd)
    coeffs = sections(ns, ch if per else None)
    rx = sr.Rx(spec.config())
    rx.set_afilt(coeffs, per_channel=per)
    orc, exp = oracle_chain(spec), Expect(spec, coeffs, per)
    at = 0
    for i, bs in enumerate(calls):
        iq = rc.synth_iq(0, ch, at, bs)
        if q15:
            qi = to_q15(iq)
            got, want = run(rx, qi, device=i % 2 == 1), exp.after(orc.process(q15_to_f32(qi)), q15=True)
        else:
            got, want = run(rx, iq, device=i % 2 == 1), exp.after(orc.process(iq))
        assert_bits(got, want, "call at %d" % at)
        at += bs
    assert_bits(rx.afilt_state()["state"], exp.f.state, "state")
    assert np.abs(exp.f.state).max() > 0


# ---- 3. _SPLIT16 and _AUTO: the stage given the GPU's own pre-stage audio -------------------------------------------------------------
def own_pre_stage(spec_a, spec_b, calls, ns, per, q15=False, device=False):
    """instance A with the stage, instance B without it and with the AGC off"""
    ch = spec_a.channels
    coeffs = sections(ns, ch if per else None, seed=2)
    a, b = sr.Rx(spec_a.config()), sr.Rx(spec_b.config())
    a.set_afilt(coeffs, per_channel=per)
    exp = Expect(spec_a, coeffs, per)
    at = 0
    for bs in calls:
        iq = rc.synth_iq(0, ch, at, bs)
        if q15:
            qi = to_q15(iq)
            got, want = run(a, qi, device), exp.after(run(b, q15_to_f32(qi), device), q15=True)
        else:
            got, want = run(a, iq, device), exp.after(run(b, iq, device))
        assert_bits(got, want, "call at %d" % at)
        at += bs
    assert_bits(a.afilt_state()["state"], exp.f.state, "state")
    return a


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", [rc.ARITH_SPLIT16, rc.ARITH_AUTO], ids=["split16", "auto"])
@pytest.mark.parametrize("name,calls,ns,per", [("cfg3", [4096, 1024 + 256], 4, True), ("cfg1", [1024, 768], 3, False)])
def test_split_arith_given_own_pre_stage_audio(arith, name, calls, ns, per, q15):
    own_pre_stage(spec_of(name, 70, arith), spec_of(name, 70, arith, agc=False), calls, ns, per, q15=q15)


# ---- 4. geometry ------------------------------------------------------------------------------------------------------------------------
def against_oracle(spec, calls, ns, per, device=False):
    coeffs = sections(ns, spec.channels if per else None, seed=3)
    rx = sr.Rx(spec.config())
    rx.set_afilt(coeffs, per_channel=per)
    orc, exp = oracle_chain(spec), Expect(spec, coeffs, per)
    at = 0
    for bs in calls:
        iq = rc.synth_iq(0, spec.channels, at, bs)
        assert_bits(run(rx, iq, device), exp.after(orc.process(iq)), "call at %d" % at)
        at += bs
    assert_bits(rx.afilt_state()["state"], exp.f.state, "state")


def test_96_frame_slot_geometry_several_calls():
    """DSP blocks of 96 frames (the firmware's slot), no decimator: calls of 96, 288, 96 and 672 samples -- one and a half, four and a half,
    ten and a half tiles"""
    against_oracle(rc.ChainSpec(48, 96, 1, 0, 31, 0, sr.MODE_USB, rc.ARITH_CMSIS), (96, 96 * 3, 96, 96 * 7), 2, True)


def test_12_samples_per_call_with_8_stages():
    """block 96 by 8: 12 samples per call, n_stages = 8: the 7 fill and 7 drain steps outnumber the samples of the tile"""
    spec = rc.ChainSpec(33, 96, 8, 64, 31, 0, sr.MODE_USB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000)
    against_oracle(spec, (96, 96, 96, 192), 8, True)
    against_oracle(spec, (96, 96), 5, False)


def test_long_call_of_several_tiles_and_a_ragged_last_one():
    """3 channels, one call of 63 DSP blocks of 96 samples = 6048: 94 tiles of KERNEL_TILE samples and one of 32 (47 blocks of 128 = 6016 are
    94 whole tiles of this kernel: that call runs too, and ends on a tile's edge)"""
    n = 63 * 96
    assert n % KERNEL_TILE == 32 and n // KERNEL_TILE == 94
    for ns in (1, 4, 7):
        against_oracle(rc.ChainSpec(3, 96, 1, 0, 31, 0, sr.MODE_USB, rc.ARITH_CMSIS), (n, 96), ns, True, device=True)
    assert 47 * 128 == 94 * KERNEL_TILE
    against_oracle(rc.ChainSpec(3, 128, 1, 0, 31, 0, sr.MODE_USB, rc.ARITH_CMSIS), (47 * 128, 128), 2, True, device=True)


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_call_cut_in_two_under_split16(q15):
    """a call the dispatcher cuts (whole passes and a tail): each part is a launch of its own on the running state, rows `out_stride` apart"""
    mk = lambda agc: rc.ChainSpec(35, 128, 4, 256, 63, 0, sr.MODE_USB, rc.ARITH_SPLIT16, nco=True, nco_step_all=0x01000000, agc=agc)  # noqa: E731
    own_pre_stage(mk(True), mk(False), [1152, 1408, 2176, 128], 3, True, q15=q15, device=True)


# ---- 5. the cut of the stream into calls ----------------------------------------------------------------------------------------------------
def test_one_call_of_2048_equals_eight_calls_of_256():
    spec = spec_of("cfg1", 70, rc.ARITH_CMSIS)
    coeffs = sections(5, 70)
    one, many = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (one, many):
        r.set_afilt(coeffs, per_channel=True)
    iq = rc.synth_iq(0, 70, 0, 2048)
    whole = run_device(one, iq)
    parts = np.concatenate([run_device(many, np.ascontiguousarray(iq[:, a:a + 256])) for a in range(0, 2048, 256)], axis=1)
    assert_bits(parts, whole)
    assert_bits(one.afilt_state()["state"], many.afilt_state()["state"], "state")


# ---- 6. selenite_rx_set_afilt_coeffs ------------------------------------------------------------------------------------------------------
def test_set_afilt_coeffs_between_calls_keeps_the_state():
    ch, ns = 70, 3
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS)
    c0, c1, c2 = sections(ns, ch, seed=4), sections(ns, 20, seed=5), sections(ns, ch, seed=6)
    rx = sr.Rx(spec.config())
    rx.set_afilt(c0, per_channel=True)
    orc, exp = oracle_chain(spec), Expect(spec, c0, True)
    at = 0
    for step in range(3):
        if step == 1:                                   # a sub-range of the channels
            rx.set_afilt_coeffs(c1, first_channel=37)
            exp.f.set_coeffs(c1, 37)
        if step == 2:                                   # all of them
            rx.set_afilt_coeffs(c2)
            exp.f.set_coeffs(c2)
        iq = rc.synth_iq(0, ch, at, 1024)
        assert_bits(rx.process(iq), exp.after(orc.process(iq)), "call %d" % step)
        st = rx.afilt_state()
        assert_bits(st["state"], exp.f.state, "state behind call %d" % step)
        assert_bits(st["coeffs"], exp.f.coeffs, "rows behind call %d" % step)
        at += 1024
    # refused calls leave the stage as it was
    L, p = rx.L, lambda a: a.ctypes.data_as(sr.f32p)  # noqa: E731
    bad = c1.copy()
    bad[3, 1, 2] = np.inf
    assert L.selenite_rx_set_afilt_coeffs(rx.h, 60, 20, p(c1)) == sr.ARGUMENT_ERROR          # past the last channel
    assert L.selenite_rx_set_afilt_coeffs(rx.h, ch, 1, p(c1)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_afilt_coeffs(rx.h, 0, 0, p(c1)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_afilt_coeffs(rx.h, 0, 20, p(bad)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_afilt_coeffs(rx.h, 0, 20, None) == sr.ARGUMENT_ERROR
    assert rx.status() == 0
    iq = rc.synth_iq(0, ch, at, 1024)
    assert_bits(rx.process(iq), exp.after(orc.process(iq)), "behind the refused calls")
    assert_bits(rx.afilt_state()["coeffs"], exp.f.coeffs, "rows behind the refused calls")
    # one set for all channels: the only range is (0, 1)
    sh = sr.Rx(spec.config())
    one, two = sections(ns, None, seed=7), sections(ns, None, seed=8)
    assert sh.L.selenite_rx_set_afilt_coeffs(sh.h, 0, 1, p(one)) == sr.ARGUMENT_ERROR         # the stage is off
    sh.set_afilt(one)
    orc2, exp2 = oracle_chain(spec), Expect(spec, one, False)
    iq = rc.synth_iq(0, ch, 0, 1024)
    assert_bits(sh.process(iq), exp2.after(orc2.process(iq)), "shared set")
    assert sh.L.selenite_rx_set_afilt_coeffs(sh.h, 0, 2, p(np.stack([two, two]))) == sr.ARGUMENT_ERROR
    assert sh.L.selenite_rx_set_afilt_coeffs(sh.h, 1, 1, p(two)) == sr.ARGUMENT_ERROR
    sh.set_afilt_coeffs(two)
    exp2.f.set_coeffs(two)
    iq = rc.synth_iq(0, ch, 1024, 1024)
    assert_bits(sh.process(iq), exp2.after(orc2.process(iq)), "shared set, replaced")


# ---- 7. with the neighbours -----------------------------------------------------------------------------------------------------------------
def test_nlms_meter_and_output_stage_behind_it():
    """afilt -> NLMS -> meter (gate 1) -> AGC -> gate -> output stage (L = 4, stereo), every one by its restatement"""
    ch = 35
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS)
    coeffs, h = sections(4, ch, seed=9), sr.design_interp(32, 4, 0.1)
    par = dict(sense=sr.SQ_ABOVE, gate=1, hang=1, attack=0.5, decay=0.9375, open_level=2e-2, close_level=4e-3, level_init=0.0)
    rx = sr.Rx(spec.config())
    rx.set_afilt(coeffs, per_channel=True)
    rx.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.05)
    rx.set_meter(**par)
    rx.set_out(4, h, sr.OUT_STEREO)
    orc, f = oracle_chain(spec), afo.Afilt(ch, coeffs, True)
    nl, me = nro.Nlms(ch, 16, 0.05, delay=8), mo.Meter(ch, 64, **par)
    agc, out = nro.Agc(ch, 64, spec.agc_params), oo.OutStage(ch, 4, h, sr.OUT_STEREO)
    at = 0
    for i, bs in enumerate((1024, 256, 2048)):
        iq = rc.synth_iq(0, ch, at, bs)
        y = nl.process(f.process(orc.process(iq)), sr.NR_DENOISE)
        bits = me.process(y)
        want = out.process(me.gate_audio(agc.process(y), bits), q15=False, rounding=False)
        got = run(rx, iq, device=i == 1)
        assert_bits(got, np.ascontiguousarray(want, np.float32).reshape(got.shape), "call %d" % i)
        at += bs
    assert_bits(rx.afilt_state()["state"], f.state, "state")
    assert_bits(rx.meter_state()["level"], me.state()["level"], "meter level")


def test_iq_correction_and_blanker_in_front_int16_slots():
    """int16 slots behind the I/Q correction: f32 in, int16 out -- the fused kernel into the f32 scratch, the stage there, k_agc_generic stores"""
    ch = 33
    sa, sb = spec_of("cfg3", ch, rc.ARITH_CMSIS), spec_of("cfg3", ch, rc.ARITH_CMSIS, agc=False)
    coeffs = sections(2, ch, seed=10)
    a, b = sr.Rx(sa.config()), sr.Rx(sb.config())
    for r in (a, b):
        r.set_iqc()
        r.set_nb()
    a.set_afilt(coeffs, per_channel=True)
    exp = Expect(sa, coeffs, True)
    for call in range(3):
        qi = to_q15(rc.synth_iq(0, ch, call * 1024, 1024))
        assert_bits(a.process_q15(qi), exp.after(b.process(q15_to_f32(qi)), q15=True), "call %d" % call)
    assert_bits(a.afilt_state()["state"], exp.f.state, "state")


def test_global_gain_every_entry():
    ch, bs = 35, 1024
    sa, sb = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS, agc_global=True), spec_of("cfg3", ch, rc.ARITH_CMSIS, agc=False)
    coeffs = sections(3, ch, seed=11)
    nout = bs // 4
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(4 * (bs // 256))

    def one_call(rx, iq):
        return rx.process(iq)

    def split(rx, iq):
        d_in.upload(iq)
        rx.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
        rx.global_phase2(d_out.ptr, d_env.ptr, bs)
        rx.sync()
        return d_out.download((ch, nout), np.float32)

    def process_entry(rx, iq):
        rx.L.selenite_rx_global_process_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        d_in.upload(iq)
        assert rx.L.selenite_rx_global_process_f32_device(rx.h, d_in.ptr, d_out.ptr, bs, None) == 0
        rx.sync()
        return d_out.download((ch, nout), np.float32)

    from test_gpu_nr import GlobalGain
    for entry in (one_call, split, process_entry):
        a, b = sr.Rx(sa.config()), sr.Rx(sb.config())
        a.set_afilt(coeffs, per_channel=True)
        f, gg = afo.Afilt(ch, coeffs, True), GlobalGain(sa)
        for call in range(2):
            iq = rc.synth_iq(0, ch, call * bs, bs)
            assert_bits(entry(a, iq), gg.process(f.process(b.process(iq))), "%s, call %d" % (entry.__name__, call))
        assert_bits(a.afilt_state()["state"], f.state, entry.__name__ + ": state")
    d_in.free(); d_out.free(); d_env.free()


# ---- 8. a host-pointer call cut into ragged channel chunks -------------------------------------------------------------------------------
def test_per_channel_rows_across_ragged_channel_chunks():
    """cfg3, 300 channels x 2048 samples with a 1 MiB chunk: 64-channel chunks and a ragged last one of 44; per-channel coefficients: the rows
    and the state of a chunk move with its first channel.  Three host-pointer calls equal the device-pointer result.  (A subprocess: the
    library reads SELENITE_RX_HOST_CHUNK_MB once.)"""
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import rxcommon as rc, selenite_rx as sr, test_gpu_afilt as t
        nch, bs = 300, 2048
        spec = rc.baseline_spec("cfg3", nch, rc.ARITH_AUTO)
        coeffs = t.sections(3, nch, seed=12)
        dev, hst = sr.Rx(spec.config()), sr.Rx(spec.config())
        for r in (dev, hst):
            r.set_afilt(coeffs, per_channel=True)
        for call in range(3):
            iq = rc.synth_iq(0, nch, call * bs, bs)
            t.assert_bits(hst.process(iq), t.run_device(dev, iq), "call %%d" %% call)
        t.assert_bits(hst.afilt_state()["state"], dev.afilt_state()["state"], "state")
        a, b = dev.afilt_state()["state"], dev.afilt_state()["coeffs"]
        assert np.abs(a[250:]).max() > 0 and len({r.tobytes() for r in b}) == nch
        print("OK")
    """ % (os.path.join(rc.ROOT, "tests"), rc.PKG_DIR))
    env = dict(os.environ, SELENITE_RX_HOST_CHUNK_MB="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.stdout[-1000:], out.stderr[-3000:])


# ---- 9. life cycle ------------------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_reset_set_mode_and_the_other_setters():
    ch = 33
    spec = spec_of("cfg1", ch, rc.ARITH_CMSIS)
    coeffs = sections(3, ch, seed=13)
    rx, fresh = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, fresh):
        r.set_afilt(coeffs, per_channel=True)
    assert not rx.afilt_state()["state"].any() and not np.signbit(rx.afilt_state()["state"]).any()
    rx.process(rc.synth_iq(0, ch, 0, 512))
    st, g = rx.afilt_state(), rx.state()
    assert st["state"].any()
    nxt = rc.synth_iq(0, ch, 512, 512)
    y1 = rx.process(nxt)
    fresh.set_state(g)
    fresh.set_afilt_state(st)
    assert_bits(fresh.process(nxt), y1, "after set_afilt_state")
    # set_mode and the other setters keep state and rows
    before = rx.afilt_state()
    assert rx.set_mode(sr.MODE_LSB) == 0
    rx.set_nr(sr.NR_NOTCH, num_taps=16, delay=4, mu=0.1); rx.set_nr(sr.NR_OFF)
    rx.set_meter(); rx.set_meter(sense=None)
    rx.set_out(4, sr.design_interp(32, 4, 0.1), sr.OUT_STEREO); rx.set_out(None)
    rx.set_spectrum(64); rx.set_spectrum(None)
    rx.set_nb(); rx.set_nb(None)
    rx.set_iqc(); rx.set_iqc(None)
    after = rx.afilt_state()
    assert_bits(after["state"], before["state"], "state behind the other setters")
    assert_bits(after["coeffs"], before["coeffs"], "rows behind the other setters")
    # reset clears the state and keeps the rows
    assert rx.reset() == 0
    after = rx.afilt_state()
    assert not after["state"].any() and not np.signbit(after["state"]).any()
    assert_bits(after["coeffs"], coeffs, "rows behind reset")


@pytest.mark.parametrize("field,value", [("n_stages", 0), ("n_stages", 9), ("per_channel", 2), ("reserved", 1), ("struct_size", 20), ("coeffs", None),
                                         ("nan", None), ("inf", None)])
def test_bad_field_is_argument_error_and_the_stage_stays(field, value):
    ch = 16
    spec = spec_of("cfg1", ch, rc.ARITH_CMSIS)
    coeffs = sections(2, None, seed=14)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_afilt(coeffs)
    iq = rc.synth_iq(0, ch, 0, 512)
    assert_bits(rx.process(iq), ref.process(iq))
    new = sections(4, None, seed=15)
    if field in ("nan", "inf"):
        new[2, 3] = np.nan if field == "nan" else -np.inf
    g = sr.AfiltConfig()
    g.struct_size, g.n_stages, g.per_channel, g.reserved, g.coeffs = C.sizeof(sr.AfiltConfig), 4, 0, 0, new.ctypes.data_as(sr.f32p)
    if field not in ("nan", "inf"):
        setattr(g, field, value)
    assert rx.L.selenite_rx_set_afilt(rx.h, C.byref(g)) == sr.ARGUMENT_ERROR
    assert rx.status() == 0
    iq = rc.synth_iq(0, ch, 512, 512)
    assert_bits(rx.process(iq), ref.process(iq), "after the refused set_afilt")
    assert_bits(rx.afilt_state()["state"], ref.afilt_state()["state"])


@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_stage_removed_is_no_stage(arith):
    spec = spec_of("cfg3", 70, arith)
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    a.set_afilt(sections(8, 70), per_channel=True)
    a.set_afilt(None)
    for call in range(2):
        iq = rc.synth_iq(0, 70, call * 2048, 2048)
        assert_bits(a.process(iq), b.process(iq), "call %d" % call)
    with pytest.raises(sr.RxError):
        a.afilt_state()
    assert a.L.selenite_rx_get_afilt_state(a.h, C.byref(sr.AfiltStateView())) == sr.ARGUMENT_ERROR
    assert a.L.selenite_rx_set_afilt_state(a.h, C.byref(sr.AfiltStateView())) == sr.ARGUMENT_ERROR


def test_timing_entry_point_runs_the_stage():
    ch, bs = 35, 1024
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS)
    coeffs = sections(2, ch, seed=16)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_afilt(coeffs, per_channel=True)
    iq = rc.synth_iq(0, ch, 0, bs)
    d_in, d_out = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(ch * (bs // 4) * 4)
    d_in.upload(iq)
    assert rx.time_process(d_in.ptr, d_out.ptr, bs, 3) > 0          # three calls on the same input: the state runs on
    rx.sync()
    got = d_out.download((ch, bs // 4), np.float32)
    for _ in range(3):
        want = ref.process(iq)
    assert_bits(got, want, "audio of the third timed call")
    assert_bits(rx.afilt_state()["state"], ref.afilt_state()["state"], "state")
    d_in.free(); d_out.free()
