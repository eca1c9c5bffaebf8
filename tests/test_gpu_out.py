"""GPU: the audio output stage (selenite_rx_set_out, csrc/rx_out.hip) against the restatement of arm_fir_interpolate_f32 + arm_float_to_q15 +
the stereo frames (tests/out_oracle.py), composed behind the oracle chain (_CMSIS / _FMA: bit-exact end to end) or behind the audio of a second
instance of the same configuration without the stage (_SPLIT16 / _AUTO, NLMS, global gain: the stage is bit-exact given its input).
Every comparison is a bit comparison."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import out_oracle as oo
import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu

INTERPS, PHASES = (1, 2, 4, 8), (1, 3, 8, 13, 64)


def spec_of(name, ch, arith, mode=None, agc=True, q15_rounding=False, **kw):
    s = rc.baseline_spec(name, ch, arith, agc=agc, q15_rounding=q15_rounding, **kw)
    if mode is not None:
        s.mode = mode
    return s


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


def q15_as_f32(qi):
    return np.divide(qi.astype(np.float32), np.float32(32768.0))


def taps(interp, plen, seed=0, gain=1.0):
    """random taps, every phase of about unit gain (x gain): nothing a designed low-pass would hide"""
    rng = np.random.default_rng(1000 * interp + plen + seed)
    return (gain * rng.standard_normal(interp * plen) / np.sqrt(plen)).astype(np.float32)


def assert_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32 if got.dtype == np.float32 else got.dtype) != want.view(np.uint32 if want.dtype == np.float32 else want.dtype))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def run(rx, data, q15=False, device=False):
    """one process call on `data` (f32 or int16 I/Q) through the host-pointer or the device-pointer entry point"""
    if not device:
        return rx.process_q15(data) if q15 else rx.process(data)
    ch, bs = data.shape[0], data.shape[1]
    dt = np.int16 if q15 else np.float32
    vals = rx.out_values(bs)
    d_in, d_out = sr.DeviceBuffer(data.nbytes), sr.DeviceBuffer(ch * vals * np.dtype(dt).itemsize)
    d_in.upload(np.ascontiguousarray(data, dt))
    (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
    rx.sync()
    out = d_out.download((ch, vals), dt)
    d_in.free(); d_out.free()
    return out


def check_state(rx, stage, what="out_state"):
    if stage.P >= 2:
        assert_bits(rx.out_state(), stage.state, what)
    else:
        with pytest.raises(sr.RxError):
            rx.out_state()


# ---- _CMSIS / _FMA end to end ----------------------------------------------------------------------------------------------------
SHAPES = {"cfg1": [512, 256], "cfg2": [256, 768], "cfg3": [1024, 2048], "cfg4": [512, 256]}
SSB_MODES = [sr.MODE_USB, sr.MODE_LSB, sr.MODE_AM, sr.MODE_FM, sr.MODE_DIG, sr.MODE_PKT, sr.MODE_CW, sr.MODE_CWR]
CHANNELS = [70, 33, 100, 7, 65, 40, 97, 130]


def _cases():
    """every (L, P) twice, the other dimensions cycled with co-prime strides: every chain, mode, arithmetic, frame format, slot format,
    rounding, AGC setting and call path appears with several (L, P)"""
    out = []
    for i, (interp, plen) in enumerate(list(itertools.product(INTERPS, PHASES)) * 2):
        p, j = divmod(i, 20)
        name = ("cfg1", "cfg3", "cfg4", "cfg2")[(j + 2 * p) % 4]
        mode = (sr.MODE_CW, sr.MODE_CWR)[(j // 4 + p) % 2] if name == "cfg4" else SSB_MODES[(j // 4 * 3 + j % 4 + 4 * p) % 8]
        arith = (rc.ARITH_CMSIS, rc.ARITH_FMA)[(j // 4 + p) % 2]
        slot = ("f32", "q15", "q15r")[(j + p) % 3]
        out.append((name, mode, arith, interp, plen, (j + j // 5 + p) % 2, slot, j % 5 != 2, (j // 8 + j + p) % 2 == 1, CHANNELS[i % 8]))
    # ... and what the cycling leaves out: the headline stage (L = 4, P = 8) on the headline chain in every format, cfg4 with f32 slots by device pointers
    for k, (frames, slot) in enumerate(itertools.product((0, 1), ("f32", "q15", "q15r"))):
        out.append(("cfg3", sr.MODE_USB, (rc.ARITH_CMSIS, rc.ARITH_FMA)[k % 2], 4, 8, frames, slot, True, k % 2 == 0, 129))
    out.append(("cfg4", sr.MODE_CW, rc.ARITH_CMSIS, 4, 8, 0, "f32", True, True, 100))
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: "%s-m%d-a%d-L%d-P%d-%s-%s-agc%d-%s-c%d" % (
    c[0], c[1], c[2], c[3], c[4], "stereo" if c[5] else "mono", c[6], c[7], "dev" if c[8] else "host", c[9]))
def test_end_to_end_against_oracle_chain_and_restatement(case):
    name, mode, arith, interp, plen, frames, slot, agc, device, ch = case
    q15 = slot != "f32"
    spec = spec_of(name, ch, arith, mode, agc=agc, q15_rounding=slot == "q15r")
    h = taps(interp, plen)
    rx = sr.Rx(spec.config())
    rx.set_out(interp, h, frames)
    exp = oo.StagedChain(spec, interp, h, frames)
    at = 0
    for bs in SHAPES[name]:
        assert rx.out_values(bs) == bs // spec.decim * interp * (2 if frames else 1)
        iq = rc.synth_iq(0, ch, at, bs)
        if q15:
            qi = to_q15(iq)
            got, want = run(rx, qi, True, device), exp.process_q15(qi)
        else:
            got, want = run(rx, iq, False, device), exp.process(iq)
        assert_bits(got, want, "call at %d" % at)
        at += bs
    check_state(rx, exp.stage)


def test_case_list_covers_the_issue():
    cs = _cases()
    assert {(c[0], c[2]) for c in cs} == set(itertools.product(("cfg1", "cfg2", "cfg3", "cfg4"), (rc.ARITH_CMSIS, rc.ARITH_FMA)))
    assert {(c[0], c[6] != "f32", c[8]) for c in cs} == set(itertools.product(("cfg1", "cfg2", "cfg3", "cfg4"), (False, True), (False, True)))
    assert {c[1] for c in cs} >= {sr.MODE_USB, sr.MODE_LSB, sr.MODE_AM, sr.MODE_FM, sr.MODE_CW, sr.MODE_CWR, sr.MODE_DIG, sr.MODE_PKT}
    assert {(c[3], c[4]) for c in cs} == set(itertools.product(INTERPS, PHASES))
    for dim in (5, 7, 8):
        assert {c[dim] for c in cs} == {0, 1}
    assert {c[6] for c in cs} == {"f32", "q15", "q15r"} and all(c[9] % 64 for c in cs)
    for interp in INTERPS:           # every L with both frame formats, both slot formats, both call paths
        assert {(c[5], c[6] != "f32") for c in cs if c[3] == interp} == {(0, False), (0, True), (1, False), (1, True)}
        assert {c[8] for c in cs if c[3] == interp} == {False, True}


def test_frames_only_no_fir():
    """interp 1 without taps: the samples pass as they are (-0.0 included), int16 slots and stereo pairs"""
    spec = spec_of("cfg1", 37, rc.ARITH_CMSIS, q15_rounding=True)
    for frames, q15 in itertools.product((0, 1), (False, True)):
        rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 1, None, frames)
        rx.set_out(1, None, frames)
        for at in (0, 256):
            iq = rc.synth_iq(0, 37, at, 256)
            if q15:
                assert_bits(rx.process_q15(to_q15(iq)), exp.process_q15(to_q15(iq)))
            else:
                assert_bits(rx.process(iq), exp.process(iq))
        with pytest.raises(sr.RxError):
            rx.out_state()


# ---- _SPLIT16 / _AUTO: bit-exact given its input -----------------------------------------------------------------------------------
def given_own_audio(spec, calls, interp, plen, frames, q15=False, ratio=None, prepare=None, ch0=0):
    """instance A with the stage, instance B of the same configuration without it: out_oracle on B's audio equals A's output"""
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (a, b):
        if ratio is not None:
            r.set_guard_ratio(ratio)
        if prepare:
            prepare(r)
    h = taps(interp, plen, seed=7)
    a.set_out(interp, h, frames)
    stage = oo.OutStage(spec.channels, interp, h, frames)
    at = 0
    for bs in calls:
        iq = rc.synth_iq(ch0, spec.channels, at, bs)
        if q15:
            qi = to_q15(iq)
            got = a.process_q15(qi)
            want = stage.process(b.process(q15_as_f32(qi)), q15=True, rounding=spec.q15_rounding)
        else:
            got, want = a.process(iq), stage.process(b.process(iq))
        assert_bits(got, want, "call at %d" % at)
        at += bs
    check_state(a, stage)
    return a, b


@pytest.mark.parametrize("ratio", [None, float("inf")], ids=["default-ratio", "every-channel-rerun"])
@pytest.mark.parametrize("arith", [rc.ARITH_SPLIT16, rc.ARITH_AUTO], ids=["split16", "auto"])
@pytest.mark.parametrize("name,calls", [("cfg3", [4096, 1024 + 256, 2048]), ("cfg2", [1024, 768, 256]), ("cfg4", [512, 256, 256]),
                                        ("cfg3_by8", [2048, 4096])])
def test_split_arith_given_own_audio(arith, name, calls, ratio):
    a, _ = given_own_audio(spec_of(name, 67, arith), calls, 4, 13, oo.OUT_STEREO, ratio=ratio)
    if arith == rc.ARITH_AUTO and ratio is not None and name != "cfg4":
        assert a.guard_stats()["rerun_channel_calls"] > 0


@pytest.mark.parametrize("interp,plen,frames", [(1, 64, 0), (2, 8, 1), (8, 3, 0), (8, 64, 1)])
def test_auto_f32_other_ratios_given_own_audio(interp, plen, frames):
    given_own_audio(spec_of("cfg3", 65, rc.ARITH_AUTO), [2048, 1024, 1024], interp, plen, frames)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def test_firmware_slot_one_slot_per_call_forty_calls():
    """block 96, by 4: 24 audio samples per call under a phase of 64 taps -- every call is shorter than the history, the state shifts"""
    ch = 37
    spec = rc.ChainSpec(ch, 96, 4, 256, 63, 0, sr.MODE_LSB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000)
    h = taps(4, 64)
    rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 4, h, oo.OUT_STEREO)
    rx.set_out(4, h, sr.OUT_STEREO)
    for call in range(40):
        qi = to_q15(rc.synth_iq(0, ch, call * 96, 96))
        got = run(rx, qi, True, device=call % 2 == 1)
        assert got.shape == (ch, 2 * 96)                       # the slot is symmetric: 96 I/Q frames in, 96 L/R frames out
        assert_bits(got, exp.process_q15(qi), "slot %d" % call)
        if call in (0, 1, 2, 39):
            check_state(rx, exp.stage, "state after slot %d" % call)


@pytest.mark.parametrize("decim,nd,block,calls", [(8, 256, 96, [96, 96, 192, 96]), (8, 256, 256, [256, 1024]), (2, 128, 96, [96, 480, 96]),
                                                  (2, 64, 256, [512, 256])])
def test_by8_and_by2_shapes(decim, nd, block, calls):
    """12 audio samples per slot under a 64-tap phase (block 96 by 8); rows of 24 bytes in the int16 mono case at L = 1"""
    ch = 41
    spec = rc.ChainSpec(ch, block, decim, nd, 63, 0, sr.MODE_USB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000, q15_rounding=True)
    for interp, plen, frames, q15 in ((decim, 64, 1, True), (1, 13, 0, True), (decim, 8, 0, False), (1, 3, 1, False)):
        h = taps(interp, plen)
        rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, interp, h, frames)
        rx.set_out(interp, h, frames)
        at = 0
        for bs in calls:
            iq = rc.synth_iq(0, ch, at, bs)
            if q15:
                assert_bits(rx.process_q15(to_q15(iq)), exp.process_q15(to_q15(iq)), "L%d P%d at %d" % (interp, plen, at))
            else:
                assert_bits(rx.process(iq), exp.process(iq), "L%d P%d at %d" % (interp, plen, at))
            at += bs
        check_state(rx, exp.stage)


def test_int16_call_that_is_no_whole_number_of_eight_values():
    """3 channels x 6 frames: 36 int16 values -- the up-front conversion of the int16 slots takes its any-length form, the rows element stores"""
    spec = rc.ChainSpec(3, 6, 2, 8, 3, 0, sr.MODE_USB, rc.ARITH_CMSIS, q15_rounding=True)
    h = taps(2, 3)
    rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 2, h, oo.OUT_MONO)
    rx.set_out(2, h, sr.OUT_MONO)
    for call in range(4):
        qi = to_q15(rc.synth_iq(0, 3, call * 6, 6))
        assert_bits(run(rx, qi, True, device=call % 2 == 0), exp.process_q15(qi), "call %d" % call)
    check_state(rx, exp.stage)


@pytest.mark.parametrize("name", ["cfg2_48k128", "cfg3"])
def test_cfg2_47872_sample_call(name):
    """BASELINE cfg2's second in DSP blocks of 128: 187 passes of 256 outputs in one call (187 whole tiles of the stage per row); the same call
    through the by-4 chain: rows of 11 968 audio samples, 46.75 tiles -- the last one partial"""
    ch = 5
    spec = spec_of(name, ch, rc.ARITH_CMSIS)
    h = taps(2, 13)
    rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 2, h, oo.OUT_MONO)
    rx.set_out(2, h, sr.OUT_MONO)
    for call in range(2):
        iq = rc.synth_iq(0, ch, call * 47872, 47872)
        assert_bits(rx.process(iq), exp.process(iq), "call %d" % call)
    check_state(rx, exp.stage)


@pytest.mark.parametrize("arith", [rc.ARITH_SPLIT16, rc.ARITH_AUTO], ids=["split16", "auto"])
def test_call_cut_by_fused_tail_split(arith):
    """48 000 samples in DSP blocks of 128: the matrix kernel takes 187 passes, the last block runs as a second launch on the same state --
    the stage runs once, behind both"""
    given_own_audio(spec_of("cfg2_48k128", 6, arith), [48000, 48000], 2, 8, oo.OUT_STEREO)


def test_same_stream_cut_three_ways():
    ch = 45
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS)
    h = taps(4, 64)
    iq = rc.synth_iq(0, ch, 0, 6144)
    outs, states = [], []
    for cuts in ([6144], [256] * 24, [256, 1024, 256, 3072, 512, 1024]):
        rx = sr.Rx(spec.config())
        rx.set_out(4, h, sr.OUT_MONO)
        at, parts = 0, []
        for bs in cuts:
            parts.append(rx.process(iq[:, at:at + bs]))
            at += bs
        outs.append(np.concatenate(parts, axis=1))
        states.append(rx.out_state())
    for o, s in zip(outs[1:], states[1:]):
        assert_bits(o, outs[0])
        assert_bits(s, states[0])
    assert_bits(outs[0], oo.StagedChain(spec, 4, h).process(iq))


# ---- composition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [sr.NR_DENOISE, sr.NR_NOTCH], ids=["denoise", "notch"])
@pytest.mark.parametrize("arith,q15", [(rc.ARITH_CMSIS, False), (rc.ARITH_AUTO, True)], ids=["cmsis-f32", "auto-q15"])
def test_behind_the_nlms_stage(kind, arith, q15):
    spec = spec_of("cfg3", 66, arith)
    a, _ = given_own_audio(spec, [1024, 2048, 1024], 4, 8, oo.OUT_STEREO, q15=q15,
                           prepare=lambda r: r.set_nr(kind, num_taps=16, delay=16, mu=0.05))
    before = a.out_state()
    a.set_nr(kind, num_taps=32, delay=8, mu=0.1)             # selenite_rx_set_nr leaves the output stage alone
    assert_bits(a.out_state(), before)


@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_AUTO], ids=["cmsis", "auto"])
def test_behind_the_global_gain(arith):
    """agc_global through process_f32_device and through selenite_rx_global_process_f32_device(comm = NULL); the split phase calls refuse"""
    ch, bs = 96, 1024
    spec = rc.baseline_spec("cfg3", ch, arith, agc_global=True)
    a, g, b = sr.Rx(spec.config()), sr.Rx(spec.config()), sr.Rx(spec.config())
    h = taps(4, 13)
    st_a, st_g = oo.OutStage(ch, 4, h, oo.OUT_STEREO), oo.OutStage(ch, 4, h, oo.OUT_STEREO)
    for r in (a, g):
        r.set_out(4, h, sr.OUT_STEREO)
    fn = a.L.selenite_rx_global_process_f32_device
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    vals = a.out_values(bs)
    d_in, d_out = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * vals * 4)
    for call in range(3):
        iq = rc.synth_iq(0, ch, call * bs, bs)
        pre = b.process(iq)
        assert_bits(run(a, iq, device=True), st_a.process(pre), "process_f32_device, call %d" % call)
        d_in.upload(iq)
        assert fn(g.h, d_in.ptr, d_out.ptr, bs, None) == 0
        g.sync()
        assert_bits(d_out.download((ch, vals), np.float32), st_g.process(pre), "global_process, call %d" % call)
    assert_bits(a.out_state(), st_a.state)
    # the host-pointer call of an agc_global instance is one chunk through the same dispatcher: its output bytes follow selenite_rx_out_values
    iq = rc.synth_iq(0, ch, 3 * bs, bs)
    pre = b.process(iq)
    got = a.process(iq)
    assert got.shape == (ch, vals)
    assert_bits(got, st_a.process(pre), "process_f32 (host pointers)")
    qa, qb = sr.Rx(spec.config()), sr.Rx(spec.config())
    qa.set_out(4, h, sr.OUT_STEREO)
    st_q = oo.OutStage(ch, 4, h, oo.OUT_STEREO)
    qi = to_q15(iq)
    assert_bits(qa.process_q15(qi), st_q.process(qb.process(q15_as_f32(qi)), q15=True), "process_q15 (host pointers)")
    # the split calls exchange audio at the decimated rate: sticky ARGUMENT_ERROR, nothing touched
    mark = np.full((ch, vals), 7.0, np.float32)
    d_env = sr.DeviceBuffer(4 * (bs // 256))
    d_out.upload(mark)
    state, ostate = g.state(), g.out_state()
    g.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
    assert g.status() == sr.ARGUMENT_ERROR
    assert_bits(d_out.download((ch, vals), np.float32), mark)
    s2 = g.state()
    assert all(state[k].tobytes() == s2[k].tobytes() for k in state) and g.out_state().tobytes() == ostate.tobytes()
    a.global_phase2(d_out.ptr, d_env.ptr, bs)
    assert a.status() == sr.ARGUMENT_ERROR
    assert_bits(d_out.download((ch, vals), np.float32), mark)


def test_mode_switch_mid_stream_keeps_the_stage_state():
    ch = 40
    spec = spec_of("cfg1", ch, rc.ARITH_CMSIS)
    h = taps(2, 13)
    rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 2, h, oo.OUT_STEREO)
    rx.set_out(2, h, sr.OUT_STEREO)
    at = 0
    for mode in (sr.MODE_USB, sr.MODE_LSB, sr.MODE_AM, sr.MODE_FM, sr.MODE_USB):
        before = rx.out_state()
        assert rx.set_mode(mode) == 0 and exp.set_mode(mode) == 0
        assert_bits(rx.out_state(), before)
        iq = rc.synth_iq(0, ch, at, 512)
        assert_bits(rx.process(iq), exp.process(iq), "mode %d" % mode)
        at += 512
    check_state(rx, exp.stage)


def test_set_out_mid_stream_clears_only_the_stage():
    ch = 35
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS)
    h1, h2 = taps(4, 8), taps(2, 64)
    rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 4, h1, oo.OUT_MONO)
    rx.set_out(4, h1, sr.OUT_MONO)
    for call in range(2):
        iq = rc.synth_iq(0, ch, call * 1024, 1024)
        assert_bits(rx.process(iq), exp.process(iq))
    chain_state = rx.state()
    rx.set_out(2, h2, sr.OUT_STEREO)
    assert not rx.out_state().any()                              # arm_fir_interpolate_init_f32 clears the state
    after = rx.state()
    assert all(chain_state[k].tobytes() == after[k].tobytes() for k in chain_state)
    exp.stage = oo.OutStage(ch, 2, h2, oo.OUT_STEREO)           # the chain oracle streams on
    for call in range(2, 4):
        iq = rc.synth_iq(0, ch, call * 1024, 1024)
        assert_bits(rx.process(iq), exp.process(iq), "after the second set_out")
    check_state(rx, exp.stage)


def test_state_round_trip_and_reset():
    ch = 34
    spec = spec_of("cfg1", ch, rc.ARITH_CMSIS)
    h = taps(4, 13)
    rx, fresh = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, fresh):
        r.set_out(4, h, sr.OUT_STEREO)
    assert rx.out_state().shape == (ch, 12) and not rx.out_state().any()
    rx.process(rc.synth_iq(0, ch, 0, 512))
    st, g = rx.out_state(), rx.state()
    assert st.any()
    nxt = rc.synth_iq(0, ch, 512, 512)
    y1 = rx.process(nxt)
    fresh.set_state(g)
    fresh.set_out_state(st)
    assert_bits(fresh.out_state(), st)
    assert_bits(fresh.process(nxt), y1, "after set_out_state")
    assert rx.reset() == 0
    assert not rx.out_state().any()
    again = sr.Rx(spec.config())
    again.set_out(4, h, sr.OUT_STEREO)
    iq = rc.synth_iq(0, ch, 0, 512)
    assert_bits(rx.process(iq), again.process(iq), "after reset")


@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_stage_removed_returns_the_instance_to_the_unstaged_bits(arith, q15):
    ch = 64
    spec = spec_of("cfg3", ch, arith)
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    a.set_out(4, taps(4, 8), sr.OUT_STEREO)
    conv = to_q15 if q15 else (lambda x: x)
    # (given its input the chain in front of the stage is the unstaged chain: the two instances stream side by side)
    iq = conv(rc.synth_iq(0, ch, 0, 2048))
    run(a, iq, q15); run(b, iq, q15)
    a.set_out(None)
    assert a.out_values(2048) == 512
    for call in range(1, 3):
        iq = conv(rc.synth_iq(0, ch, call * 2048, 2048))
        assert_bits(run(a, iq, q15), run(b, iq, q15), "call %d" % call)
    with pytest.raises(sr.RxError):
        a.out_state()
    assert a.L.selenite_rx_get_out_state(a.h, np.zeros(ch * 8, np.float32).ctypes.data_as(sr.f32p)) == sr.ARGUMENT_ERROR


def test_stage_set_and_removed_before_any_call_is_no_stage():
    for arith in (rc.ARITH_CMSIS, rc.ARITH_AUTO):
        spec = spec_of("cfg3", 64, arith)
        a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
        a.set_out(8, taps(8, 64), sr.OUT_STEREO)
        a.set_out(None)
        for call in range(2):
            qi = to_q15(rc.synth_iq(0, 64, call * 2048, 2048))
            assert_bits(a.process_q15(qi), b.process_q15(qi), "call %d" % call)


def test_host_pointer_calls_equal_device_calls_across_chunks():
    ch, bs = 4096 + 37, 2048            # > 64 MiB of f32 input: three chunks of the host pipeline, the stage's state follows the chunk's first channel
    spec = spec_of("cfg3", ch, rc.ARITH_AUTO)
    h = taps(4, 13)
    hst, dv = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (hst, dv):
        r.set_out(4, h, sr.OUT_STEREO)
    for call in range(2):
        iq = rc.synth_iq(0, ch, call * bs, bs)
        assert_bits(hst.process(iq), run(dv, iq, device=True), "f32, call %d" % call)
    assert_bits(hst.out_state(), dv.out_state())
    qi = to_q15(rc.synth_iq(0, ch, 2 * bs, bs))
    assert_bits(hst.process_q15(qi), run(dv, qi, True, device=True), "int16")
    assert_bits(hst.out_state(), dv.out_state())


def test_timing_entry_points_run_the_stage():
    ch, bs = 64, 1024
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS)
    h = taps(4, 8)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_out(4, h, sr.OUT_STEREO)
    iq = rc.synth_iq(0, ch, 0, bs)
    vals = rx.out_values(bs)
    d_in, d_out = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(ch * vals * 4)
    d_in.upload(iq)
    rx.time_process(d_in.ptr, d_out.ptr, bs, 1)
    y1 = d_out.download((ch, vals), np.float32)
    assert_bits(y1, ref.process(iq), "selenite_rx_time_process_device")
    rx.time_process_each(d_in.ptr, d_out.ptr, bs, 1)
    assert_bits(d_out.download((ch, vals), np.float32), ref.process(iq), "selenite_rx_time_process_each_device")
    assert rx.algorithmic_bytes(bs) == sr.Rx(spec.config()).algorithmic_bytes(bs)      # the chain alone, as before


# ---- edges -----------------------------------------------------------------------------------------------------------------------------
def test_tiny_input_denormal_products_are_not_flushed():
    """audio of about 1e-30 times taps of about 1e-9: EVERY product and every sum of the stage is a denormal -- a build that flushes them gives zeros"""
    ch = 19
    spec = spec_of("cfg1", ch, rc.ARITH_CMSIS, agc=False)
    h = (taps(4, 13) * np.float32(1e-9)).astype(np.float32)
    rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 4, h, oo.OUT_MONO)
    rx.set_out(4, h, sr.OUT_MONO)
    tiny = np.finfo(np.float32).tiny
    for call in range(2):
        iq = rc.synth_iq(0, ch, call * 512, 512) * np.float32(1e-30)
        want = exp.process(iq)
        assert np.abs(want).max() < tiny and np.count_nonzero(want) > 0.9 * want.size       # denormal outputs, nearly all of them non-zero
        assert float(np.abs(exp.stage.state).max()) * float(np.abs(h).max()) < tiny         # ... from denormal products
        assert_bits(rx.process(iq), want, "call %d" % call)


def test_huge_input_stays_finite():
    ch = 21
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS, agc=False)
    h = taps(4, 8)
    rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 4, h, oo.OUT_STEREO)
    rx.set_out(4, h, sr.OUT_STEREO)
    for call in range(2):
        iq = rc.synth_iq(0, ch, call * 1024, 1024) * np.float32(1e18)
        want = exp.process(iq)
        assert np.isfinite(want).all() and np.abs(want).max() > 1e16
        assert_bits(rx.process(iq), want, "call %d" % call)


@pytest.mark.parametrize("rounding", [False, True], ids=["trunc", "round"])
def test_int16_saturation_in_stereo(rounding):
    ch = 23
    spec = spec_of("cfg3", ch, rc.ARITH_CMSIS, q15_rounding=rounding)        # AGC on: audio peaks at 0.5; taps of gain 6: well over full scale
    h = taps(4, 8, gain=6.0)
    rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 4, h, oo.OUT_STEREO)
    rx.set_out(4, h, sr.OUT_STEREO)
    hit = set()
    for call in range(3):
        qi = to_q15(rc.synth_iq(0, ch, call * 1024, 1024))
        want = exp.process_q15(qi)
        assert_bits(rx.process_q15(qi), want, "call %d" % call)
        hit |= {int(want.max()), int(want.min())}
    assert {32767, -32768} <= hit


def test_overflow_raises_naninf_and_leaves_clean_channels_alone():
    ch, hot = 20, 11
    spec = spec_of("cfg1", ch, rc.ARITH_CMSIS, agc=False)
    h = taps(2, 8, gain=64.0)
    iq = rc.synth_iq(0, ch, 0, 512)
    iq[hot] *= np.float32(1e37)                                  # the chain's audio stays finite (a few 1e37), the stage's output does not
    plain = sr.Rx(spec.config())
    pre = plain.process(iq)
    assert np.isfinite(pre).all()
    rx = sr.Rx(spec.config())
    rx.set_out(2, h, sr.OUT_MONO)
    d_in, d_out = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(ch * 1024 * 4)
    d_in.upload(iq)
    rx.process_device(d_in.ptr, d_out.ptr, 512)
    with pytest.raises(sr.RxError) as ei:
        rx.sync()
    assert ei.value.code == sr.NANINF
    got = d_out.download((ch, 1024), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        want = oo.OutStage(ch, 2, h).process(pre)
    assert not np.isfinite(got[hot]).all() and not np.isfinite(want[hot]).all()
    clean = [c for c in range(ch) if c != hot]
    assert_bits(got[clean], want[clean])
    rx2 = sr.Rx(spec.config())
    rx2.set_out(2, h, sr.OUT_MONO)
    with pytest.raises(sr.RxError) as ei:                        # the host-pointer call latches it too
        rx2.process(iq)
    assert ei.value.code == sr.NANINF


# ---- at size ---------------------------------------------------------------------------------------------------------------------------
AT_SIZE_CHANNELS = 16384


@pytest.mark.parametrize("q15,frames", [(True, 1), (False, 0)], ids=["int16-stereo", "f32-mono"])
def test_at_size_every_channel_given_own_audio(q15, frames):
    """cfg3 in _AUTO, 16 384 channels x 4096 samples, L = 4, P = 8: the numpy form of the oracle over EVERY channel, from the audio of the
    un-staged instance"""
    ch, bs = AT_SIZE_CHANNELS, 4096
    spec = spec_of("cfg3", ch, rc.ARITH_AUTO)
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    h = sr.design_interp(32, 4, 0.1)
    a.set_out(4, h, frames)
    stage = oo.OutStage(ch, 4, h, frames)
    nout, vals = bs // 4, a.out_values(bs)
    assert vals == nout * 4 * (2 if frames else 1)
    d_iq = sr.DeviceBuffer(ch * bs * 8)
    d_b = sr.DeviceBuffer(ch * nout * 4)
    d_a = sr.DeviceBuffer(ch * vals * (2 if q15 else 4))
    d_q = sr.DeviceBuffer(ch * bs * 4) if q15 else None
    for call in range(2):
        a.synth_device(d_iq.ptr, 0, ch, call * bs, bs, rc.SEED)
        a.sync()                        # (b runs on a stream of its own)
        if q15:
            qi = to_q15(d_iq.download((ch, bs, 2), np.float32))
            d_q.upload(qi)
            d_iq.upload(q15_as_f32(qi))
            a.process_q15_device(d_q.ptr, d_a.ptr, bs)
        else:
            a.process_device(d_iq.ptr, d_a.ptr, bs)
        b.process_device(d_iq.ptr, d_b.ptr, bs)
        a.sync(); b.sync()
        got = d_a.download((ch, vals), np.int16 if q15 else np.float32)
        want = stage.process(d_b.download((ch, nout), np.float32), q15=q15, rounding=False)
        assert_bits(got, want, "call %d" % call)
        assert np.abs(got.astype(np.float64)).max() > 0
    assert_bits(a.out_state(), stage.state)


@pytest.mark.parametrize("q15,frames", [(True, 1), (False, 0)], ids=["int16-stereo", "f32-mono"])
def test_at_size_64_seeded_channels_end_to_end(q15, frames):
    """64 channels drawn from the 16 384 of the full-size shape, in _CMSIS, against the oracle chain + the C form of the stage"""
    rng = np.random.default_rng(0x0A7)
    picks = np.sort(rng.choice(AT_SIZE_CHANNELS, 64, replace=False))
    bs = 4096
    spec = spec_of("cfg3", 64, rc.ARITH_CMSIS)
    h = sr.design_interp(32, 4, 0.1)
    rx, exp = sr.Rx(spec.config()), oo.StagedChain(spec, 4, h, frames)
    rx.set_out(4, h, frames)
    for call in range(2):
        iq = np.concatenate([rc.synth_iq(int(c), 1, call * bs, bs) for c in picks], axis=0)
        if q15:
            assert_bits(rx.process_q15(to_q15(iq)), exp.process_q15(to_q15(iq)), "call %d" % call)
        else:
            assert_bits(rx.process(iq), exp.process(iq), "call %d" % call)
    check_state(rx, exp.stage)


# ---- validation, host example ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,code", [("interp", 0, sr.ARGUMENT_ERROR), ("interp", 3, sr.ARGUMENT_ERROR), ("interp", 16, sr.ARGUMENT_ERROR),
                                              ("ni_taps", 30, sr.LENGTH_ERROR), ("ni_taps", 4 * 65, sr.ARGUMENT_ERROR), ("ni_taps", 0, sr.ARGUMENT_ERROR),
                                              ("frames", 2, sr.ARGUMENT_ERROR), ("struct_size", 16, sr.ARGUMENT_ERROR), ("coeffs", None, sr.ARGUMENT_ERROR)])
def test_bad_field_is_refused_and_instance_stays_as_it_was(field, value, code):
    spec = spec_of("cfg1", 16, rc.ARITH_CMSIS)
    h = taps(2, 13)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_out(2, h, sr.OUT_STEREO)
    iq = rc.synth_iq(0, 16, 0, 512)
    assert_bits(rx.process(iq), ref.process(iq))
    big = np.zeros(4 * 65, np.float32)
    g = sr.OutConfig()
    g.struct_size, g.interp, g.ni_taps, g.frames, g.coeffs = C.sizeof(sr.OutConfig), 4, 32, sr.OUT_MONO, big.ctypes.data_as(sr.f32p)
    setattr(g, field, value)
    assert rx.L.selenite_rx_set_out(rx.h, C.byref(g)) == code
    assert rx.status() == 0 and rx.out_values(512) == 512 * 2 * 2
    iq = rc.synth_iq(0, 16, 512, 512)
    assert_bits(rx.process(iq), ref.process(iq), "after the refused set_out")
    assert_bits(rx.out_state(), ref.out_state())
    with pytest.raises(sr.RxError):
        rx.set_out(4, np.full(32, np.nan, np.float32))
    assert rx.out_values(512) == 512 * 2 * 2                     # (the Python face still knows the old stage)
    assert rx.out_state().shape == (16, 12)


def test_host_example_builds_with_gcc_and_runs():
    src = os.path.join(rc.PKG_DIR, "host", "dsp_if_codec_slot.c")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dsp_if_codec_slot")
        subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(rc.ROOT, "include"), src, "-L" + rc.PKG_DIR, "-lselenite_rx",
                        "-Wl,-rpath," + rc.PKG_DIR, "-lm", "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "96 L/R frames per channel" in r.stdout
