"""GPU: the spectrum tap (selenite_rx_set_spectrum, csrc/rx_spectrum.hip) against the numpy restatement of the stage (tests/spectrum_oracle.py,
pinned to the reference by tests/test_spectrum_oracle.py).  The tap reads the call's own input, so rows and state are compared bit for bit in
every arith mode; where the input is non-finite the comparison is the set of NaN / Inf bins.  Every stream also runs through a second instance
of the same configuration without the tap: audio and chain state of the two are the same bits."""
import ctypes as C

import numpy as np
import pytest

import rxcommon as rc
import selenite_rx as sr
import spectrum_oracle as so

pytestmark = pytest.mark.gpu

LENS = (64, 512)
ARITHS = (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO)


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


def window(n, seed=0):
    """a designed window with a little of everything on top: nothing a symmetric window would hide"""
    rng = np.random.default_rng(n + seed)
    return (sr.design_window(n, sr.WINDOW_BLACKMAN_HARRIS) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        u = {4: np.uint32, 2: np.uint16, 8: np.uint64}[got.dtype.itemsize]
        bad = np.argwhere(got.view(u) != want.view(u))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def run(rx, data, q15=False, device=False):
    """one process call on `data` (f32 or int16 I/Q) through the host-pointer or the device-pointer entry point"""
    if not device:
        return rx.process_q15(data) if q15 else rx.process(data)
    ch, bs = data.shape[0], data.shape[1]
    dt = np.int16 if q15 else np.float32
    vals = rx.out_len(bs)
    d_in, d_out = sr.DeviceBuffer(data.nbytes), sr.DeviceBuffer(ch * vals * np.dtype(dt).itemsize)
    d_in.upload(np.ascontiguousarray(data, dt))
    (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
    rx.sync()
    out = d_out.download((ch, vals), dt)
    d_in.free(); d_out.free()
    return out


def check(rx, orc, what=""):
    rows, frames = rx.spectrum()
    assert_bits(rows, orc.rows, what + " rows")
    assert frames == orc.frames, (what, frames, orc.frames)
    st, want = rx.spectrum_state(), orc.state()
    for k in ("rows", "pending", "position"):
        assert_bits(st[k], want[k], what + " state." + k)


def chain_state_equal(a, b, what=""):
    sa, sb = a.state(), b.state()
    for k in sa:
        assert_bits(sa[k], sb[k], what + " chain state." + k)


def stream(spec, cuts, n, stride=1, average=0, alpha=0.25, win=None, q15=False, device=False, prepare=None, level=1.0, every_call=True, ch0=0):
    """the stream cut into `cuts` through an instance with the tap, the restatement, and an instance without the tap"""
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        if prepare:
            prepare(r)
    rx.set_spectrum(n, stride, average, alpha, win)
    orc = so.Spectrum(spec.channels, n, stride, average, alpha, win)
    at = 0
    for i, bs in enumerate(cuts):
        iq = rc.synth_iq(ch0, spec.channels, at, bs) * np.float32(level)
        data = to_q15(iq) if q15 else iq
        dev = device if isinstance(device, bool) else device[i % len(device)]
        got, want = run(rx, data, q15, dev), run(ref, data, q15, dev)
        assert_bits(got, want, "audio of call %d" % i)
        orc.process(data)
        if every_call or i == len(cuts) - 1:
            check(rx, orc, "call %d at %d" % (i, at))
        at += bs
    chain_state_equal(rx, ref)
    return rx, orc, ref


# ---- every chain, every arithmetic, both lengths ----------------------------------------------------------------------------------
SHAPES = {"cfg1": [512, 256, 1280], "cfg2": [256, 768, 1024], "cfg3": [1024, 2048, 1024], "cfg4": [512, 256, 1280]}


@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("arith", ARITHS, ids=["cmsis", "fma", "split16", "auto"])
@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4"])
def test_chains_and_arith_modes(name, arith, n):
    k = ["cfg1", "cfg2", "cfg3", "cfg4"].index(name) + 4 * ARITHS.index(arith) + 16 * LENS.index(n)
    stream(rc.baseline_spec(name, (37, 70, 65, 100)[k % 4], arith), SHAPES[name], n, stride=(1, 2, 1, 3)[(k // 4) % 4], average=k % 2,
           win=window(n) if k % 3 else None, q15=(k // 2) % 2 == 1, device=(k // 3) % 2 == 1)


# ---- call cuts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("average", [0, 1])
@pytest.mark.parametrize("cuts", [[4096], [256] * 16, [768, 256, 3072]], ids=["one", "sixteen", "three"])
def test_call_cuts_give_one_stream(cuts, average, n):
    rx, orc, _ = stream(rc.baseline_spec("cfg3", 33, rc.ARITH_AUTO), cuts, n, average=average, win=window(n), device=[True, False])
    whole = so.Spectrum(33, n, 1, average, 0.25, window(n))
    whole.process(rc.synth_iq(0, 33, 0, 4096))
    assert_bits(rx.spectrum()[0], whole.rows, "against the uncut stream")


@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_forty_firmware_slots_of_96(n, q15):
    """96 samples per call under frames of 512: five or six calls per frame, the pending frame completed again and again"""
    spec = rc.ChainSpec(37, 96, 4, 256, 63, 0, sr.MODE_LSB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000)
    stream(spec, [96] * 40, n, average=1, win=window(n), q15=q15, device=[False, True, True])


@pytest.mark.parametrize("n", LENS)
def test_cfg2_one_second_call(n):
    """BASELINE cfg2's 48 000 samples per call: 93.75 frames of 512, the last quarter waits; the second call completes it"""
    spec = rc.baseline_spec("cfg2_48k128", 5, rc.ARITH_AUTO)
    rx, orc, _ = stream(spec, [48000, 48000], n, average=1, alpha=0.125, device=True)
    assert orc.position == 96000 and rx.spectrum()[1] == 96000 // n


# ---- strides ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("stride", [1, 3, 8])
def test_strides(stride, q15, n):
    stream(rc.baseline_spec("cfg1", 41, rc.ARITH_CMSIS), [768, 256, 3072, 256, 1280], n, stride=stride, average=1, q15=q15, device=[False, True])


@pytest.mark.parametrize("n", LENS)
def test_stride_larger_than_the_calls_leaves_the_row_alone(n):
    """frame 0 is the only multiple of the stride the stream reaches: the calls behind it change nothing and launch nothing"""
    spec = rc.baseline_spec("cfg1", 19, rc.ARITH_CMSIS)
    rx = sr.Rx(spec.config())
    rx.set_spectrum(n, 60000, 1, 0.5, None)
    orc = so.Spectrum(19, n, 60000, 1, 0.5)
    iq = rc.synth_iq(0, 19, 0, 1024)
    rx.process(iq); orc.process(iq)
    check(rx, orc, "frame 0")
    row, frames = rx.spectrum()
    assert frames == 1 and row.any()
    for call in range(1, 4):
        iq = rc.synth_iq(0, 19, 1024 * call, 1024)
        run(rx, iq, device=call % 2 == 1); orc.process(iq)
        got, f = rx.spectrum()
        assert f == 1
        assert_bits(got, row, "row behind call %d" % call)
        check(rx, orc, "call %d" % call)


# ---- pointer kinds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q15", [(512, False), (64, True)])
def test_host_call_cut_into_channel_chunks(n, q15):
    """64 KiB of input per channel: the host-pointer pipeline cuts 1100 channels into chunks of 512 (32 KiB for int16 slots: 1024); the
    tap's state follows each chunk's first channel and every chunk starts from the same stream position"""
    spec = rc.baseline_spec("cfg1", 1100, rc.ARITH_FMA)
    stream(spec, [8192, 256, 8192], n, stride=2, average=1, win=window(n), q15=q15, device=False, every_call=False)


# ---- combinations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_with_nlms_and_with_an_output_stage(n, q15):
    spec = rc.baseline_spec("cfg3", 43, rc.ARITH_AUTO)
    stream(spec, [1024, 768, 2304], n, average=1, q15=q15, device=[True, False],
           prepare=lambda r: r.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.05))
    h = sr.design_interp(32, 4, 0.1)
    stream(spec, [1024, 768, 2304], n, average=1, q15=q15, device=[False, True], prepare=lambda r: r.set_out(4, h, sr.OUT_STEREO))


@pytest.mark.parametrize("n", LENS)
def test_global_gain_one_call_and_split_calls(n):
    ch, bs = 48, 1024
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS, agc_global=True)
    # the one-call entries: process_f32_device / the host call on an agc_global instance
    stream(spec, [bs, 256, bs], n, average=1, win=window(n), device=[True, False])
    # phase 1 + phase 2, and selenite_rx_global_process_f32_device: the tap runs in phase 1 (phase 2 has no input)
    a, b, ref = sr.Rx(spec.config()), sr.Rx(spec.config()), sr.Rx(spec.config())
    orc = so.Spectrum(ch, n, 1, 1, 0.25, window(n))
    for r in (a, b):
        r.set_spectrum(n, 1, 1, 0.25, window(n))
    nout = bs // 4
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(4 * (bs // 256))
    a.L.selenite_rx_global_process_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    for call in range(3):
        iq = rc.synth_iq(0, ch, call * bs, bs)
        want = ref.process(iq)
        orc.process(iq)
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
    d_in.free(); d_out.free(); d_env.free()


def test_timing_calls_run_the_tap():
    ch, bs, n = 16, 1024, 512
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    rx.set_spectrum(n, 1, 1, 0.5, None)
    orc = so.Spectrum(ch, n, 1, 1, 0.5)
    iq = rc.synth_iq(0, ch, 0, bs)
    qi = to_q15(iq)
    d_in, d_q, d_out = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(qi.nbytes), sr.DeviceBuffer(ch * bs)
    d_in.upload(iq); d_q.upload(qi)
    rx.time_process(d_in.ptr, d_out.ptr, bs, 3)
    rx.time_process_each(d_in.ptr, d_out.ptr, bs, 2)
    rx.time_process_q15(d_q.ptr, d_out.ptr, bs, 2)
    rx.time_process_each(d_q.ptr, d_out.ptr, bs, 1, q15=True)
    for data in [iq] * 5 + [qi] * 3:
        orc.process(data)
    check(rx, orc)
    d_in.free(); d_q.free(); d_out.free()


# ---- life cycle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENS)
def test_reset_removal_and_reset_again(n):
    spec = rc.baseline_spec("cfg3", 21, rc.ARITH_CMSIS)
    rx, orc, ref = stream(spec, [768, 256], n, average=1, win=window(n))
    assert rx.spectrum_device()
    # reset: rows, pending and position cleared with the chain's state
    rx.reset(); ref.reset(); orc.reset()
    check(rx, orc, "behind reset")
    for at in (0, 1280):
        iq = rc.synth_iq(0, 21, at, 1280)
        assert_bits(rx.process(iq), ref.process(iq)); orc.process(iq)
        check(rx, orc, "behind reset, at %d" % at)
    # removal: the calls go on without the tap; the getters refuse
    rx.set_spectrum(None)
    assert rx.spectrum_device() is None
    with pytest.raises(sr.RxError):
        rx.spectrum()
    with pytest.raises(sr.RxError):
        rx.spectrum_state()
    assert rx.L.selenite_rx_get_spectrum(rx.h, None, None) == sr.ARGUMENT_ERROR
    iq = rc.synth_iq(0, 21, 2560, 768)
    assert_bits(rx.process(iq), ref.process(iq))
    # set again, another length and no window: state from zero, the chain's state untouched
    m = 576 - n
    rx.set_spectrum(m, 2, 0)
    orc = so.Spectrum(21, m, 2, 0)
    check(rx, orc, "behind the second set_spectrum")
    for at in (3328, 3584):
        iq = rc.synth_iq(0, 21, at, 256)
        assert_bits(rx.process(iq), ref.process(iq)); orc.process(iq)
        check(rx, orc, "second tap, at %d" % at)
    chain_state_equal(rx, ref)


@pytest.mark.parametrize("n", LENS)
def test_state_round_trip_in_mid_frame(n):
    """eleven firmware slots: position 1056, 32 samples into a frame of either length; a fresh instance given the tap's and the chain's state
    goes on as the first one does"""
    spec = rc.ChainSpec(29, 96, 4, 256, 63, 0, sr.MODE_LSB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000)
    a, orc, _ = stream(spec, [96 * 11], n, average=1, win=window(n))
    st = a.spectrum_state()
    assert int(st["position"][0]) == 1056 and st["pending"][:, :32].any()
    b = sr.Rx(spec.config())
    b.set_spectrum(n, 1, 1, 0.25, window(n))
    b.set_spectrum_state(st)
    b.set_state(a.state())
    for at in (1056, 1536):
        iq = rc.synth_iq(0, 29, at, 480)
        assert_bits(b.process(iq), a.process(iq)); orc.process(iq)
        check(a, orc, "a at %d" % at); check(b, orc, "b at %d" % at)


def test_state_round_trip_inside_a_512_frame():
    """position 768: half of frame 1 waits in pending; a fresh instance given that state completes the frame"""
    spec = rc.baseline_spec("cfg1", 11, rc.ARITH_CMSIS)
    a, orc, _ = stream(spec, [768], 512, average=1)
    st = a.spectrum_state()
    assert int(st["position"][0]) == 768 and st["pending"][:, :256].any()
    b = sr.Rx(spec.config())
    b.set_spectrum(512, 1, 1, 0.25)
    b.set_spectrum_state(st)
    iq = rc.synth_iq(0, 11, 768, 256)
    b.process(iq); orc.process(iq)
    check(b, orc, "the completed frame")
    assert b.spectrum()[1] == 2
    # a partial view: rows alone
    rows = np.full((11, 512), 3.0, np.float32)
    b.set_spectrum_state(dict(rows=rows))
    st2 = b.spectrum_state()
    assert_bits(st2["rows"], rows); assert_bits(st2["pending"], orc.state()["pending"]); assert int(st2["position"][0]) == 1024


BAD = [("fft_len", 128, sr.LENGTH_ERROR), ("fft_len", 256, sr.LENGTH_ERROR), ("fft_len", 4096, sr.LENGTH_ERROR), ("fft_len", 0, sr.LENGTH_ERROR),
       ("fft_len", 100, sr.LENGTH_ERROR), ("stride", 0, sr.ARGUMENT_ERROR), ("stride", 65536, sr.ARGUMENT_ERROR), ("average", 2, sr.ARGUMENT_ERROR),
       ("alpha", 0.0, sr.ARGUMENT_ERROR), ("alpha", 1.5, sr.ARGUMENT_ERROR), ("alpha", -0.25, sr.ARGUMENT_ERROR),
       ("alpha", float("nan"), sr.ARGUMENT_ERROR), ("alpha", float("inf"), sr.ARGUMENT_ERROR), ("struct_size", 16, sr.ARGUMENT_ERROR),
       ("window", "inf", sr.ARGUMENT_ERROR), ("window", "nan", sr.ARGUMENT_ERROR)]


@pytest.mark.parametrize("field,value,code", BAD, ids=["%s-%s" % (b[0], b[1]) for b in BAD])
def test_bad_field_leaves_a_working_tap_as_it_was(field, value, code):
    spec = rc.baseline_spec("cfg1", 16, rc.ARITH_CMSIS)
    rx, orc, ref = stream(spec, [768], 512, average=1, win=window(512))
    g = sr.SpecConfig()
    g.struct_size, g.fft_len, g.stride, g.average, g.alpha = C.sizeof(sr.SpecConfig), 64, 2, 0, 0.5
    w = np.ones(512, np.float32)
    if field == "window":
        w[40] = float(value)
        g.window = w.ctypes.data_as(sr.f32p)
    else:
        setattr(g, field, value)
    assert rx.L.selenite_rx_set_spectrum(rx.h, C.byref(g)) == code
    assert rx.status() == 0
    check(rx, orc, "behind the refused set_spectrum")
    iq = rc.synth_iq(0, 16, 768, 512)
    assert_bits(rx.process(iq), ref.process(iq)); orc.process(iq)
    check(rx, orc, "the call behind it")


def test_python_face_keeps_the_tap_on_a_refusal():
    spec = rc.baseline_spec("cfg1", 8, rc.ARITH_CMSIS)
    rx = sr.Rx(spec.config())
    rx.set_spectrum(64)
    with pytest.raises(sr.RxError) as ei:
        rx.set_spectrum(1024)
    assert ei.value.code == sr.LENGTH_ERROR
    assert rx.spectrum()[0].shape == (8, 64)


@pytest.mark.parametrize("n", LENS)
def test_set_mode_set_nr_set_out_between_calls_leave_the_tap_alone(n):
    spec = rc.baseline_spec("cfg3", 23, rc.ARITH_AUTO)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    rx.set_spectrum(n, 1, 1, 0.25, window(n))
    orc = so.Spectrum(23, n, 1, 1, 0.25, window(n))
    h = sr.design_interp(16, 2, 0.2)
    steps = [lambda r: None, lambda r: r.set_mode(sr.MODE_LSB), lambda r: r.set_nr(sr.NR_NOTCH, num_taps=8, delay=4, mu=0.1),
             lambda r: r.set_mode(sr.MODE_AM), lambda r: r.set_out(2, h, sr.OUT_MONO), lambda r: r.set_mode(sr.MODE_FM)]
    at = 0
    for i, step in enumerate(steps):
        step(rx); step(ref)
        iq = rc.synth_iq(0, 23, at, 768)
        assert_bits(run(rx, iq, device=i % 2 == 1), run(ref, iq, device=i % 2 == 1), "audio %d" % i)
        orc.process(iq)
        check(rx, orc, "step %d" % i)
        at += 768
    chain_state_equal(rx, ref)


# ---- the edges of the arithmetic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("average", [0, 1])
def test_tiny_input_products_are_denormals(n, average):
    """level 1e-22: re * re, im * im and their sum are denormals, so are alpha * (p - row) and the row"""
    spec = rc.baseline_spec("cfg1", 13, rc.ARITH_CMSIS, agc=False)
    rx, orc, _ = stream(spec, [1024, 1024], n, average=average, alpha=0.25, win=window(n), level=1e-22)
    rows = rx.spectrum()[0]
    assert rows.any() and (rows < np.finfo(np.float32).tiny).all()


@pytest.mark.parametrize("n", LENS)
def test_overflowing_power_is_stored_and_raises_nothing(n):
    """level 1e19: the audio stays finite, the power does not -- stored as it comes (+Inf; with averaging Inf - Inf = NaN follows), and the
    status keeps meaning audio"""
    spec = rc.baseline_spec("cfg1", 9, rc.ARITH_CMSIS, agc=False)
    rx = sr.Rx(spec.config())
    rx.set_spectrum(n, 1, 0)
    orc = so.Spectrum(9, n, 1, 0)
    iq = rc.synth_iq(0, 9, 0, 1024) * np.float32(1e19)
    audio = rx.process(iq)                                        # (raises on SELENITE_RX_NANINF)
    orc.process(iq)
    assert np.isfinite(audio).all() and rx.status() == 0
    rows = rx.spectrum()[0]
    assert np.isinf(rows).any() and not np.isnan(rows).any()
    assert_bits(rows, orc.rows)


@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("average", [0, 1])
def test_non_finite_input_same_set_of_nan_and_inf_bins(n, average):
    ch = 6
    spec = rc.baseline_spec("cfg1", ch, rc.ARITH_CMSIS, agc=False)
    rx = sr.Rx(spec.config())
    rx.set_spectrum(n, 1, average, 0.5, window(n))
    orc = so.Spectrum(ch, n, 1, average, 0.5, window(n))
    iq = rc.synth_iq(0, ch, 0, 1024)
    # all in the last frame of either length; sample 960 is element 0 of a frame of 64 and element 448 of one of 512: column 0 of the first
    # pass, whose butterflies store their sums without a twiddle multiply (0 * Inf would be NaN there)
    iq[1, 1003, 0] = np.inf
    iq[2, 961, 1] = -np.inf
    iq[3, 1023, 1] = np.nan
    iq[4, 960, 0] = np.inf
    d_in, d_out = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(ch * 1024 * 4)
    d_in.upload(iq)
    rx.process_device(d_in.ptr, d_out.ptr, 1024)                 # (selenite_rx_sync would report the audio: SELENITE_RX_NANINF)
    orc.process(iq)
    rows = rx.spectrum()[0]
    d_in.free(); d_out.free()
    assert np.array_equal(np.isnan(rows), np.isnan(orc.rows)) and np.array_equal(np.isinf(rows), np.isinf(orc.rows))
    ok = np.isfinite(orc.rows)
    assert all(not ok[c].all() for c in (1, 2, 3, 4)) and ok[0].all() and ok[5].all()
    assert np.isinf(orc.rows[4]).any()                           # (Inf survives where the reference keeps it apart from NaN)
    assert np.array_equal(rows.view(np.uint32)[ok], orc.rows.view(np.uint32)[ok])


def test_minus_zero_and_silence():
    """a silent stream and one of -0.0 samples: the transform's zeros keep the reference's signs, the power is +0.0"""
    ch, n = 4, 512
    spec = rc.baseline_spec("cfg1", ch, rc.ARITH_CMSIS, agc=False)
    rx = sr.Rx(spec.config())
    rx.set_spectrum(n, 1, 1, 0.5, -window(n))
    orc = so.Spectrum(ch, n, 1, 1, 0.5, -window(n))
    iq = np.zeros((ch, 1024, 2), np.float32)
    iq[1] = -0.0
    iq[2, ::3, 0] = -0.0
    iq[3, 100:, 1] = -0.0
    rx.process(iq); orc.process(iq)
    check(rx, orc)
    assert not rx.spectrum()[0].any()
