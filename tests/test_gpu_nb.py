"""GPU: the impulse noise blanker (selenite_rx_set_nb, csrc/rx_nb.hip) against the numpy restatement of the stage (tests/nb_oracle.py, pinned to
the reference by tests/test_nb_oracle.py).  The stage's output is observed through the chain: an instance with the blanker, fed X, must give
the same audio bits and the same chain state as an instance without it fed nb_oracle(X); level, blanked and bursts must equal the
restatement's after every call (the level as bits where it is finite, elsewhere as the set of NaN / Inf positions).

The input is rc.synth_iq (scaled by 0.25 for int16 slots, so that full-scale impulses stand clear of it) with, per channel role, impulses of
I = Q = 4.0 (full scale for int16) and the other events of ROLES below.  Channels without an event must end with blanked == 0 and
bursts == 0 at threshold 8, alpha 0.125, clamp 2: over 128 channels x 8192 samples of rc.synth_iq the largest p / level is 2.96 at F = 32,
2.82 at F = 64 and 2.81 at F = 128, about 2.7 times under the threshold."""
import ctypes as C

import numpy as np
import pytest

import nb_oracle as no
import rxcommon as rc
import selenite_rx as sr
import spectrum_oracle as so

pytestmark = pytest.mark.gpu

FRAMES = (32, 64, 128)
ARITHS = (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO)
DEFAULTS = dict(guard=2, max_hits=8, threshold=8.0, alpha=0.125, clamp=2.0)
# what happens in the channels c with c % PERIOD == role (every other channel is left alone)
ROLES = ["clean", "mid_frame", "frame_edges", "run_of_three", "call_edges", "burst", "level_step", "silent", "late_start", "nan", "inf"]
PERIOD = 17


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        u = {4: np.uint32, 2: np.uint16, 8: np.uint64}[got.dtype.itemsize]
        bad = np.argwhere(got.view(u) != want.view(u))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def role_of(c):
    return ROLES[c % PERIOD] if c % PERIOD < len(ROLES) else "clean"


def make_stream(channels, cuts, F, q15=False, nonfinite=False, ch0=0):
    """the whole stream [channels][sum(cuts)][2] with the events of ROLES, in the slot's format; the events sit behind frame 2 (the level is
    primed by then) and in front of the level step's half-way point"""
    total = sum(cuts)
    x = rc.synth_iq(ch0, channels, 0, total) * np.float32(0.25 if q15 else 1.0)
    amp = 1.0 if q15 else 4.0                                     # (to_q15 saturates 1.0 to 32767: full scale)
    for c in range(channels):
        role = role_of(c)
        if role == "mid_frame":
            x[c, 3 * F + F // 2] = amp
        elif role == "frame_edges":
            x[c, 4 * F] = amp
            x[c, 6 * F - 1] = amp
        elif role == "run_of_three":
            x[c, 3 * F + 10:3 * F + 13] = amp
        elif role == "call_edges" and len(cuts) > 1:
            x[c, cuts[0] - 1] = amp                               # the last sample of a call and the first of the next
            x[c, cuts[0]] = amp
        elif role == "burst":
            x[c, 4 * F + 1:4 * F + 1 + 2 * (DEFAULTS["max_hits"] + 1):2] = amp
        elif role == "level_step":
            x[c, total // 2 + 5:] *= np.float32(31.62)            # +30 dB, held to the end (int16 slots clip: still a step)
        elif role == "silent":
            x[c] = 0
        elif role == "late_start":
            x[c, :total // 3] = 0
        elif role == "nan" and nonfinite:
            x[c, 5 * F + 7, 1] = np.nan
        elif role == "inf" and nonfinite:
            x[c, 5 * F + 9, 0] = np.inf
    return to_q15(x) if q15 else x


def run(rx, data, q15=False, device=False, naninf_ok=False):
    """one process call on `data` (f32 or int16 I/Q) through the host-pointer or the device-pointer entry point"""
    if not device:
        assert not naninf_ok
        return rx.process_q15(data) if q15 else rx.process(data)
    ch, bs = data.shape[0], data.shape[1]
    dt = np.int16 if q15 else np.float32
    vals = rx.out_len(bs)
    d_in, d_out = sr.DeviceBuffer(data.nbytes), sr.DeviceBuffer(ch * vals * np.dtype(dt).itemsize)
    d_in.upload(np.ascontiguousarray(data, dt))
    (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
    code = rx.L.selenite_rx_sync(rx.h)
    assert code == 0 or (naninf_ok and code == sr.NANINF), (code, rx.error())      # (a NaN input sample is NaN audio: that status is the chain's)
    out = d_out.download((ch, vals), dt)
    d_in.free(); d_out.free()
    return out


def check(rx, orc, what=""):
    st = rx.nb_state()
    got, want = st["level"], orc.level
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), what + " level: NaN / Inf positions"
    assert_bits(got[fin], want[fin], what + " level")
    assert_bits(st["blanked"], orc.blanked, what + " blanked")
    assert_bits(st["bursts"], orc.bursts, what + " bursts")


def chain_state_equal(a, b, what=""):
    sa, sb = a.state(), b.state()
    for k in sa:
        assert_bits(sa[k], sb[k], what + " chain state." + k)


def clean_channels_untouched(orc, channels, what=""):
    """the condition of this file's docstring (on the restatement, which the instance has just been shown to equal)"""
    clean = np.array([role_of(c) == "clean" for c in range(channels)])
    assert clean.any() and not orc.blanked[clean].any() and not orc.bursts[clean].any(), what


def stream(spec, cuts, F, q15=False, device=False, prepare=None, nonfinite=False, every_call=True, nb=None, x=None):
    """the stream cut into `cuts` through an instance with the blanker fed X, the restatement, and an instance without it fed nb_oracle(X)"""
    par = dict(DEFAULTS, **(nb or {}))
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        if prepare:
            prepare(r)
    rx.set_nb(F, **par)
    orc = no.Blanker(spec.channels, F, **par)
    if x is None:
        x = make_stream(spec.channels, cuts, F, q15, nonfinite)
    at, audio = 0, []
    for i, bs in enumerate(cuts):
        data = np.ascontiguousarray(x[:, at:at + bs])
        dev = device if isinstance(device, bool) else device[i % len(device)]
        got = run(rx, data, q15, dev, nonfinite)
        want = run(ref, orc.process(data), q15, dev, nonfinite)
        assert_bits(got, want, "audio of call %d" % i)
        audio.append(got)
        if every_call or i == len(cuts) - 1:
            check(rx, orc, "call %d at %d" % (i, at))
        at += bs
    chain_state_equal(rx, ref)
    if par == DEFAULTS:
        clean_channels_untouched(orc, spec.channels)
    return rx, orc, ref, np.concatenate(audio, axis=1)


# ---- every chain, every arithmetic, the three frame lengths ---------------------------------------------------------------------------
SHAPES = {"cfg1": [512, 256, 1280], "cfg2": [256, 768, 1024], "cfg3": [1024, 2048, 1024], "cfg4": [512, 256, 1280]}


@pytest.mark.parametrize("arith", ARITHS, ids=["cmsis", "fma", "split16", "auto"])
@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4"])
def test_chains_and_arith_modes(name, arith):
    k = ["cfg1", "cfg2", "cfg3", "cfg4"].index(name) + 4 * ARITHS.index(arith)
    _, orc, _, _ = stream(rc.baseline_spec(name, (37, 70, 65, 100)[k % 4], arith), SHAPES[name], FRAMES[k % 3], q15=(k // 2) % 2 == 1,
                          device=(k // 3) % 2 == 1)
    # the events did what they are there for
    role = {r: ROLES.index(r) for r in ROLES}
    assert orc.blanked[role["mid_frame"]] == 5 and orc.blanked[role["run_of_three"]] == 7 and orc.blanked[role["frame_edges"]] == 6
    assert orc.blanked[role["call_edges"]] == 6 and orc.bursts[role["burst"]] >= 1 and orc.bursts[role["level_step"]] >= 1
    assert orc.level[role["silent"]] == 0 and not orc.blanked[role["silent"]] and orc.level[role["late_start"]] > 0


# ---- call cuts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FRAMES)
def test_call_cuts_give_one_stream(F):
    spec = rc.baseline_spec("cfg3", 33, rc.ARITH_CMSIS)
    x = make_stream(33, [768, 256, 3072], F)                      # (one stream for the three cuts: the call-edge impulses at 767 / 768)
    outs = [stream(spec, cuts, F, device=[True, False], x=x) for cuts in ([4096], [256] * 16, [768, 256, 3072])]
    for _, orc, _, audio in outs[1:]:
        assert_bits(audio, outs[0][3], "audio against the uncut stream")
        for k in ("level", "blanked", "bursts"):
            assert_bits(orc.state()[k], outs[0][1].state()[k], k)


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_forty_firmware_slots_of_96(q15):
    """DSP blocks of 96: frames of 32 divide them, three per slot and a half-filled wave load; frames of 64 do not"""
    spec = rc.ChainSpec(37, 96, 4, 256, 63, 0, sr.MODE_LSB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000)
    rx, _, _, _ = stream(spec, [96] * 40, 32, q15=q15, device=[False, True, True])
    for F in (64, 128):
        with pytest.raises(sr.RxError) as ei:
            rx.set_nb(F)
        assert ei.value.code == sr.LENGTH_ERROR
    assert rx.nb_state()["level"].any()                           # the blanker of 32 is still there, with its state


def test_cfg2_one_second_call():
    """BASELINE cfg2's 48 000 samples per call: 375 frames of 128, 750 of 64 -- many tiles, the last one partial"""
    spec = rc.baseline_spec("cfg2_48k128", 5, rc.ARITH_AUTO)
    for F in (128, 64):
        stream(spec, [48000], F, device=True)


# ---- pointer kinds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,q15", [(128, False), (32, True)])
def test_host_call_cut_into_channel_chunks(F, q15):
    """64 KiB of input per channel: the host-pointer pipeline cuts 1100 channels into chunks of 512 (32 KiB for int16 slots: 1024); level and
    counters follow each chunk's first channel"""
    spec = rc.baseline_spec("cfg1", 1100, rc.ARITH_FMA)
    _, orc, _, _ = stream(spec, [8192, 256, 8192], F, q15=q15, device=False, every_call=False)
    assert orc.blanked[PERIOD * 40 + 1] == 5 and orc.blanked[PERIOD * 62 + 3] == 7      # events in the second and the third chunk


# ---- combinations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FRAMES)
def test_with_the_spectrum_tap_rows_are_of_the_raw_input(F):
    spec = rc.baseline_spec("cfg3", 43, rc.ARITH_AUTO)
    cuts = [1024, 768, 2304]
    x = make_stream(43, cuts, F)
    rx, orc, _, _ = stream(spec, cuts, F, device=[True, False], x=x, prepare=lambda r: r.set_spectrum(64, 1, 1, 0.25))
    tap = so.Spectrum(43, 64, 1, 1, 0.25)
    tap.process(x)
    assert_bits(rx.spectrum()[0], tap.rows, "rows on the raw input")
    blanked = so.Spectrum(43, 64, 1, 1, 0.25)
    blanked.process(no.Blanker(43, F, **DEFAULTS).process(x))
    assert blanked.rows.tobytes() != tap.rows.tobytes()           # (... which the blanked input would not give)


@pytest.mark.parametrize("F", FRAMES)
def test_with_nlms_and_an_output_stage_on_int16_slots(F):
    spec = rc.baseline_spec("cfg3", 43, rc.ARITH_AUTO)
    h = sr.design_interp(32, 4, 0.1)

    def prepare(r):
        r.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.05)
        r.set_out(4, h, sr.OUT_STEREO)
    stream(spec, [1024, 768, 2304], F, q15=True, device=[True, False], prepare=prepare)
    stream(spec, [1024, 768], F, q15=False, device=[False, True], prepare=lambda r: r.set_nr(sr.NR_NOTCH, num_taps=8, delay=4, mu=0.1))


@pytest.mark.parametrize("F", FRAMES)
def test_global_gain_one_call_and_split_calls(F):
    ch, bs = 48, 1024
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS, agc_global=True)
    # the one-call entries: process_f32_device / the host call on an agc_global instance
    stream(spec, [bs, 256, bs], F, device=[True, False])
    # phase 1 + phase 2, and selenite_rx_global_process_f32_device: the blanker runs in phase 1 (phase 2 has no input)
    a, b, ref = sr.Rx(spec.config()), sr.Rx(spec.config()), sr.Rx(spec.config())
    orc = no.Blanker(ch, F, **DEFAULTS)
    for r in (a, b):
        r.set_nb(F, **DEFAULTS)
    nout = bs // 4
    x = make_stream(ch, [bs] * 3, F)
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(4 * (bs // 256))
    a.L.selenite_rx_global_process_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    for call in range(3):
        iq = np.ascontiguousarray(x[:, call * bs:(call + 1) * bs])
        want = ref.process(orc.process(iq))
        d_in.upload(iq)
        a.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
        a.sync()
        check(a, orc, "behind phase 1 of call %d" % call)
        a.global_phase2(d_out.ptr, d_env.ptr, bs)
        a.sync()
        assert_bits(d_out.download((ch, nout), np.float32), want, "split calls, audio %d" % call)
        check(a, orc, "behind phase 2 of call %d" % call)
        assert b.L.selenite_rx_global_process_f32_device(b.h, d_in.ptr, d_out.ptr, bs, None) == 0
        b.sync()
        assert_bits(d_out.download((ch, nout), np.float32), want, "one entry, audio %d" % call)
        check(b, orc, "one entry, call %d" % call)
    assert orc.blanked.any()
    chain_state_equal(a, ref); chain_state_equal(b, ref)
    d_in.free(); d_out.free(); d_env.free()


def test_timing_calls_run_the_blanker():
    ch, bs, F = 16, 1024, 64
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    rx.set_nb(F, **DEFAULTS)
    orc = no.Blanker(ch, F, **DEFAULTS)
    iq = make_stream(ch, [bs], F)
    qi = make_stream(ch, [bs], F, q15=True)
    d_in, d_q, d_out = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(qi.nbytes), sr.DeviceBuffer(ch * bs)
    d_in.upload(iq); d_q.upload(qi)
    rx.time_process(d_in.ptr, d_out.ptr, bs, 3)
    rx.time_process_each(d_in.ptr, d_out.ptr, bs, 2)
    rx.time_process_q15(d_q.ptr, d_out.ptr, bs, 2)
    rx.time_process_each(d_q.ptr, d_out.ptr, bs, 1, q15=True)
    for data in [iq] * 5 + [qi] * 3:
        orc.process(data)
    check(rx, orc)
    assert orc.blanked.any()
    d_in.free(); d_q.free(); d_out.free()


# ---- non-finite input -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FRAMES)
def test_a_nan_sample_and_an_inf_sample(F):
    """each in a channel of its own: the NaN is not a hit and passes (its audio is the chain's business), the Inf is a hit and is blanked;
    the stage raises no status of its own"""
    spec = rc.baseline_spec("cfg1", 2 * PERIOD, rc.ARITH_CMSIS)
    rx, orc, _, _ = stream(spec, [1024, 1024], F, device=True, nonfinite=True)
    nan, inf = ROLES.index("nan"), ROLES.index("inf")
    assert orc.blanked[inf] == 5 and orc.blanked[nan] == 0 and np.isfinite(orc.level).all()
    # ... and without the NaN channel the status stays clean
    x = make_stream(2 * PERIOD, [1024], F, nonfinite=True)
    x[nan::PERIOD] = 0
    rx2 = sr.Rx(spec.config())
    rx2.set_nb(F, **DEFAULTS)
    assert np.isfinite(run(rx2, x, device=True)).all() and rx2.status() == 0
    # an unprimed channel takes an Inf mean as its level, and loses it again as the formulas say: Inf, NaN (Inf - Inf), the next mean
    y = np.zeros((2 * PERIOD, 1024, 2), np.float32)
    y[:, :, 0] = 0.25
    y[3, 5, 0] = np.inf
    rx3, orc3 = sr.Rx(rc.baseline_spec("cfg1", 2 * PERIOD, rc.ARITH_CMSIS, agc=False).config()), no.Blanker(2 * PERIOD, F, **DEFAULTS)
    rx3.set_nb(F, **DEFAULTS)
    for i in range(4):
        part = np.ascontiguousarray(y[:, 256 * i:256 * (i + 1)])
        run(rx3, part, device=True, naninf_ok=True)
        orc3.process(part)
        check(rx3, orc3, "Inf mean, call %d" % i)
    assert orc3.level[3] == np.float32(0.0625) and not orc3.blanked.any()


# ---- life cycle -------------------------------------------------------------------------------------------------------------------
BAD = [("frame", 0, sr.LENGTH_ERROR), ("frame", 48, sr.LENGTH_ERROR), ("frame", 256, sr.LENGTH_ERROR), ("guard", 9, sr.ARGUMENT_ERROR),
       ("max_hits", 0, sr.ARGUMENT_ERROR), ("max_hits", 17, sr.ARGUMENT_ERROR), ("threshold", 0.5, sr.ARGUMENT_ERROR),
       ("threshold", float("nan"), sr.ARGUMENT_ERROR), ("alpha", 0.0, sr.ARGUMENT_ERROR), ("alpha", 1.5, sr.ARGUMENT_ERROR),
       ("clamp", 0.5, sr.ARGUMENT_ERROR), ("clamp", float("inf"), sr.ARGUMENT_ERROR), ("struct_size", 24, sr.ARGUMENT_ERROR)]


@pytest.mark.parametrize("field,value,code", BAD, ids=["%s-%s" % (b[0], b[1]) for b in BAD])
def test_bad_field_leaves_a_working_blanker_as_it_was(field, value, code):
    spec = rc.baseline_spec("cfg1", 20, rc.ARITH_CMSIS)
    cuts = [768, 512]
    x = make_stream(20, cuts, 32)
    rx, orc, ref, _ = stream(spec, cuts[:1], 32, x=x)
    g = sr.NbConfig()
    g.struct_size, g.frame, g.guard, g.max_hits, g.threshold, g.alpha, g.clamp = C.sizeof(sr.NbConfig), 64, 1, 16, 4.0, 0.5, 1.5      # (F / 4 = 16)
    setattr(g, field, value)
    assert rx.L.selenite_rx_set_nb(rx.h, C.byref(g)) == code
    assert rx.status() == 0 and rx.L.selenite_rx_error_string(None)
    check(rx, orc, "behind the refused set_nb")
    iq = np.ascontiguousarray(x[:, 768:])
    assert_bits(rx.process(iq), ref.process(orc.process(iq)))
    check(rx, orc, "the call behind it")
    assert orc.blanked.sum() > 0


def test_python_face_keeps_the_blanker_on_a_refusal():
    rx = sr.Rx(rc.baseline_spec("cfg1", 8, rc.ARITH_CMSIS).config())
    with pytest.raises(sr.RxError):
        rx.nb_state()
    rx.set_nb(64)
    with pytest.raises(sr.RxError) as ei:
        rx.set_nb(64, guard=9)
    assert ei.value.code == sr.ARGUMENT_ERROR
    assert rx.nb_state()["level"].shape == (8,)


@pytest.mark.parametrize("F", FRAMES)
def test_reset_and_removal(F):
    spec = rc.baseline_spec("cfg3", 21, rc.ARITH_CMSIS)
    cuts = [1024, 512]
    rx, orc, ref, first = stream(spec, cuts, F)
    assert orc.level.any() and orc.blanked.any()
    # reset: level and counters back to zero with the chain's state; the same stream gives the same audio again
    rx.reset(); ref.reset(); orc.reset()
    check(rx, orc, "behind reset")
    assert not rx.nb_state()["level"].any()
    x = make_stream(21, cuts, F)
    again = [rx.process(np.ascontiguousarray(x[:, :1024])), rx.process(np.ascontiguousarray(x[:, 1024:]))]
    assert_bits(np.concatenate(again, axis=1), first, "the stream again behind reset")
    for part in (x[:, :1024], x[:, 1024:]):
        ref.process(orc.process(np.ascontiguousarray(part)))
    check(rx, orc, "behind the second run")
    # removal: the next call equals that of the instance that never had a blanker; the state calls refuse
    rx.set_nb(None)
    with pytest.raises(sr.RxError):
        rx.nb_state()
    v = sr.NbStateView(None, None, None)
    assert rx.L.selenite_rx_get_nb_state(rx.h, C.byref(v)) == sr.ARGUMENT_ERROR
    assert rx.L.selenite_rx_set_nb_state(rx.h, C.byref(v)) == sr.ARGUMENT_ERROR
    iq = make_stream(21, [768], F)                                # (impulses and all: nothing blanks them now)
    assert_bits(run(rx, iq, device=True), run(ref, iq, device=True), "behind removal")
    chain_state_equal(rx, ref)
    # set again: state from zero, the chain's state untouched
    rx.set_nb(F, **DEFAULTS)
    orc = no.Blanker(21, F, **DEFAULTS)
    check(rx, orc, "behind the second set_nb")
    assert_bits(rx.process(iq), ref.process(orc.process(iq)))
    check(rx, orc, "second blanker")


def test_an_instance_that_had_the_stage_equals_one_that_never_had():
    for name, q15 in (("cfg3", False), ("cfg4", True)):
        spec = rc.baseline_spec(name, 19, rc.ARITH_AUTO)
        a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
        a.set_nb(128)
        a.set_nb(None)
        cuts, at = [1024, 256, 768], 0
        x = make_stream(19, cuts, 128, q15)                       # (impulses and all: nothing blanks them)
        for i, bs in enumerate(cuts):
            data = np.ascontiguousarray(x[:, at:at + bs])
            at += bs
            assert_bits(run(a, data, q15, i % 2 == 1), run(b, data, q15, i % 2 == 1), "%s call %d" % (name, i))
        chain_state_equal(a, b)


def test_set_mode_set_nr_set_out_set_spectrum_between_calls_leave_the_blanker_alone():
    F = 64
    spec = rc.baseline_spec("cfg3", 23, rc.ARITH_AUTO)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    rx.set_nb(F, **DEFAULTS)
    orc = no.Blanker(23, F, **DEFAULTS)
    h = sr.design_interp(16, 2, 0.2)
    steps = [lambda r: None, lambda r: r.set_mode(sr.MODE_LSB), lambda r: r.set_nr(sr.NR_NOTCH, num_taps=8, delay=4, mu=0.1),
             lambda r: r.set_spectrum(64), lambda r: r.set_mode(sr.MODE_AM), lambda r: r.set_out(2, h, sr.OUT_MONO), lambda r: r.set_mode(sr.MODE_FM)]
    x = make_stream(23, [768] * len(steps), F)
    for i, step in enumerate(steps):
        step(rx); step(ref)
        iq = np.ascontiguousarray(x[:, 768 * i:768 * (i + 1)])
        assert_bits(run(rx, iq, device=i % 2 == 1), run(ref, orc.process(iq), device=i % 2 == 1), "audio %d" % i)
        check(rx, orc, "step %d" % i)
    chain_state_equal(rx, ref)
    assert orc.blanked.any()


@pytest.mark.parametrize("F", FRAMES)
def test_state_round_trip_continues_the_stream(F):
    spec = rc.baseline_spec("cfg3", 29, rc.ARITH_CMSIS)
    cuts = [1024, 512, 768, 256]
    x = make_stream(29, cuts, F)
    a, orc, _, _ = stream(spec, cuts[:2], F, x=x)
    st = a.nb_state()
    assert st["level"].any() and st["blanked"].any()
    b = sr.Rx(spec.config())
    b.set_nb(F, **DEFAULTS)
    b.set_nb_state(st)
    b.set_state(a.state())
    for at, bs in ((1536, 768), (2304, 256)):
        iq = np.ascontiguousarray(x[:, at:at + bs])
        assert_bits(b.process(iq), a.process(iq)); orc.process(iq)
        check(a, orc, "a at %d" % at); check(b, orc, "b at %d" % at)
    # a partial view: the level alone
    lv = np.full(29, 3.0, np.float32)
    b.set_nb_state(dict(level=lv))
    st2 = b.nb_state()
    assert_bits(st2["level"], lv); assert_bits(st2["blanked"], orc.blanked); assert_bits(st2["bursts"], orc.bursts)


# ---- the decisions on hand-built frames (the cases of tests/test_nb_oracle.py, through the kernel) ---------------------------------------
@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_power_equal_to_the_threshold_is_not_a_hit_and_max_hits_is_not_a_burst(F, q15):
    """a given level of 2^-4 (2^-12 for int16 slots) and threshold 8: thr = 0.5 (2^-9).  Channel 0: a sample whose power IS thr, and one a float
    (a count) above it; channel 1: max_hits hits; channel 2: max_hits + 1; channel 3: the level given is -1, NaN in channel 4: not primed"""
    ch = 6
    spec = rc.baseline_spec("cfg1", ch, rc.ARITH_CMSIS, agc=False)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    rx.set_nb(F, **DEFAULTS)
    orc = no.Blanker(ch, F, **DEFAULTS)
    level = np.full(ch, 2.0 ** -12 if q15 else 0.0625, np.float32)
    level[3], level[4] = -1.0, np.nan
    if q15:
        x = np.zeros((ch, 256, 2), np.int16)
        x[:, :, 0] = 512                                          # power 2^-12
        x[0, 7] = (1024, 1024)                                    # 2^-10 + 2^-10 = 2^-9 = thr
        x[0, 20] = (1025, 1024)
        big = (32767, 32767)
    else:
        x = np.zeros((ch, 256, 2), np.float32)
        x[:, :, 0] = 0.25
        x[0, 7] = 0.5                                             # 0.25 + 0.25 = thr
        x[0, 20] = (np.nextafter(np.float32(0.5), np.float32(1)), 0.5)
        big = (4.0, 4.0)
    x[1, F + 1:F + 1 + 2 * 8:2] = big
    x[2, F + 1:F + 1 + 2 * 9:2] = big
    x[3, 5], x[4, 5], x[5, F - 1], x[5, F] = big, big, big, big
    rx.set_nb_state(dict(level=level))
    orc.level = level.copy()
    got = run(rx, x, q15, device=True)
    y = orc.process(x)
    assert_bits(got, run(ref, y, q15, device=True), "audio")
    check(rx, orc)
    chain_state_equal(rx, ref)
    # (channel 1: hits at n = 1, 3 .. 15 of frame 1 and guard 2: n = 0 .. 17, the sample in front of the frame is not reached)
    assert y[0, 7].any() and not y[0, 20].any() and list(orc.blanked) == [5, 18, 0, 0, 0, 6] and list(orc.bursts) == [0, 0, 1, 0, 0, 0]


# ---- the parameters away from their defaults --------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("guard", [0, 8])
def test_guard_extremes_and_other_parameters(F, guard):
    """guard 0 and 8 with the impulses at n = 0 and n = F - 1 (the clipping), max_hits at its largest, a low threshold that the signal
    itself crosses, and a quick level"""
    spec = rc.baseline_spec("cfg1", 2 * PERIOD, rc.ARITH_CMSIS)
    _, orc, _, _ = stream(spec, [512, 1536], F, q15=guard == 8, device=[True, False],
                          nb=dict(guard=guard, max_hits=F // 4, threshold=1.5, alpha=0.5, clamp=1.25))
    assert orc.blanked[ROLES.index("frame_edges")] > 0
    assert orc.blanked[0] + orc.bursts[0] > 0                     # (threshold 1.5 is under the signal's own crest: the compare itself is exercised)
